"""The Python surface of the window queries stays as it is: the 24 callables (six queries on four surfaces) keep their
signatures and docstrings, and the two command lines share one copy of their bucket-query code."""
import inspect
import os
import re

import pytest

import atsc_amd
from atsc_amd import engine, stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OWNERS = {"Context": engine.Context, "DPlan": engine.DPlan, "CompressedStream": stream.CompressedStream, "stream": stream}

SIGNATURES = {
    ("Context", "aggregate_windows_host"): "(self, records, begins, counts, has_count=False)",
    ("DPlan", "aggregate_windows"): "(self, d_body, begins, counts, d_stats, stream=0)",
    ("CompressedStream", "aggregate_windows"): "(self, begins, counts)",
    ("stream", "aggregate_data_windows"): "(ctx, bro, begins, counts)",
    ("Context", "moments_windows_host"): "(self, records, begins, counts, has_count=False)",
    ("DPlan", "moments_windows"): "(self, d_body, begins, counts, d_out, stream=0)",
    ("CompressedStream", "moments_windows"): "(self, begins, counts)",
    ("stream", "moments_data_windows"): "(ctx, bro, begins, counts)",
    ("Context", "delta_windows_host"): "(self, records, begins, counts, has_count=False)",
    ("DPlan", "delta_windows"): "(self, d_body, begins, counts, d_out, stream=0)",
    ("CompressedStream", "delta_windows"): "(self, begins, counts)",
    ("stream", "delta_data_windows"): "(ctx, bro, begins, counts)",
    ("Context", "runs_windows_host"): "(self, records, begins, counts, op, limit, has_count=False)",
    ("DPlan", "runs_windows"): "(self, d_body, begins, counts, op, limit, d_out, stream=0)",
    ("CompressedStream", "runs_windows"): "(self, begins, counts, op, limit)",
    ("stream", "runs_data_windows"): "(ctx, bro, begins, counts, op, limit)",
    ("Context", "quantile_windows_host"): "(self, records, begins, counts, levels, method=0, has_count=False)",
    ("DPlan", "quantile_windows"): "(self, d_body, begins, counts, levels, d_out, method=0, stream=0)",
    ("CompressedStream", "quantile_windows"): "(self, begins, counts, levels, method=0)",
    ("stream", "quantile_data_windows"): "(ctx, bro, begins, counts, levels, method=0)",
    ("Context", "histogram_windows_host"): "(self, records, begins, counts, edges, closed=0, has_count=False)",
    ("DPlan", "histogram_windows"): "(self, d_body, begins, counts, edges, d_out, closed=0, stream=0)",
    ("CompressedStream", "histogram_windows"): "(self, begins, counts, edges, closed=0)",
    ("stream", "histogram_data_windows"): "(ctx, bro, begins, counts, edges, closed=0)",
}


@pytest.mark.parametrize("owner,name", sorted(SIGNATURES))
def test_signature_and_docstring(owner, name):
    f = getattr(OWNERS[owner], name)
    assert str(inspect.signature(f)) == SIGNATURES[(owner, name)]
    assert f.__doc__ and f.__doc__.strip()
    # written out as a def where a reader looks for it
    src = inspect.getsource(inspect.getmodule(f))
    assert re.search(r"^\s*def %s\(" % name, src, re.M)


def test_data_windows_are_package_names():
    for (owner, name) in SIGNATURES:
        if owner == "stream":
            assert getattr(atsc_amd, name) is getattr(stream, name)


def test_parse_runs_is_defined_once():
    """atsc_cli_buckets.h is the only place that defines parse_runs (and with it the other bucket-query parsers)"""
    csrc = os.path.join(ROOT, "atsc_amd", "csrc")
    for fn in ("parse_runs", "parse_levels", "parse_method", "parse_histogram"):
        definition = re.compile(r"^\w[\w \*&:<>]*\b%s\(.*\)\s*$" % fn, re.M)
        where = [f for f in sorted(os.listdir(csrc)) if definition.search(open(os.path.join(csrc, f)).read())]
        assert where == ["atsc_cli_buckets.h"], (fn, where)
