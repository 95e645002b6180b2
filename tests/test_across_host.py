"""The windowed across without a GPU: the NumPy model of the contract (tests/across_model.py) on hand-written columns,
and the host-only parts of the library: atsc_across_outputs, the record's layout, the new symbols and the four public
surfaces."""
import inspect

import numpy as np
import pytest

from tests import across_model as M


@pytest.fixture(scope="module")
def A():
    import __graft_entry__ as G

    G.build()
    import atsc_amd

    return atsc_amd


def _bits(v):
    return np.asarray(v, dtype=np.float64).view(np.uint64).tolist()


def test_across_outputs_against_the_model(A):
    values = (0, 1, 2, 7, 2 ** 40)
    for count in values:
        for stride in values:
            want = (count - 1) // stride + 1 if count and stride else 0
            assert A.across_outputs(count, stride) == M.outputs(count, stride) == want, (count, stride)
            assert A.capi.lib().atsc_across_outputs(count, stride) == want
    assert A.across_outputs(2 ** 64 - 1, 1) == 2 ** 64 - 1
    assert A.across_offsets([10, 0, 1, 7], 3).tolist() == M.offsets([10, 0, 1, 7], 3).tolist() == [0, 4, 4, 5, 8]
    assert A.across_offsets([5], 1).dtype == np.uint64


def test_record_layout(A):
    r = A.ACROSS_RECORD
    assert r.itemsize == 32 and r.names == ("count", "min_at", "max_at", "min", "max", "sum")
    assert [r.fields[n][1] for n in r.names] == [0, 4, 6, 8, 16, 24]
    assert [r.fields[n][0].str for n in r.names] == ["<u4", "<u2", "<u2", "<f8", "<f8", "<f8"]
    assert r == M.RECORD
    assert A.ACROSS_MAX_STREAMS == M.MAX_STREAMS == 64


def test_model_on_columns_of_nan():
    nan = np.nan
    r = M.fold([[nan, 1.0], [nan, nan], [nan, 3.0]])
    assert r["count"].tolist() == [0, 2]
    assert r["min_at"].tolist() == [0xFFFF, 0] and r["max_at"].tolist() == [0xFFFF, 2]
    assert np.isnan(r["min"][0]) and np.isnan(r["max"][0])
    assert _bits(r["sum"]) == _bits([0.0, 4.0])  # +0.0, not -0.0, where every sample is NaN
    assert (r["min"][1], r["max"][1]) == (1.0, 3.0)
    one = M.fold([[nan, -0.0, 2.5]])
    assert one["count"].tolist() == [0, 1, 1] and _bits(one["sum"]) == _bits([0.0, -0.0, 2.5])
    assert _bits(one["min"][1:]) == _bits(one["max"][1:]) == _bits([-0.0, 2.5])


def test_model_keeps_the_first_zero_of_either_sign():
    a = M.fold([[-0.0, 0.0], [0.0, -0.0]])  # -0.0 then +0.0, and the reverse
    assert _bits(a["min"]) == _bits(a["max"]) == _bits([-0.0, 0.0])
    assert a["min_at"].tolist() == a["max_at"].tolist() == [0, 0]
    assert _bits(a["sum"]) == _bits([0.0, 0.0])  # (-0.0) + (+0.0) is +0.0 in either order
    b = M.fold([[np.nan, np.nan], [-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0]])
    assert _bits(b["min"]) == _bits(b["max"]) == _bits([-0.0, 0.0]) and b["min_at"].tolist() == b["max_at"].tolist() == [1, 1]
    c = M.fold([[-0.0], [np.nan], [-0.0]])
    assert _bits(c["sum"]) == _bits([-0.0]) and c["count"].tolist() == [2]


def test_model_infinities_and_ties():
    r = M.fold([[np.inf, 1.0, 5.0], [-np.inf, 1.0, 7.0], [3.0, 1.0, 5.0], [np.inf, 0.5, 7.0]])
    assert np.isnan(r["sum"][0]) and r["count"].tolist() == [4, 4, 4]
    assert (r["min"][0], r["max"][0]) == (-np.inf, np.inf) and (r["min_at"][0], r["max_at"][0]) == (1, 0)
    assert (r["min"][1], r["min_at"][1], r["max"][1], r["max_at"][1]) == (0.5, 3, 1.0, 0)  # ties: the lowest index
    assert (r["min"][2], r["min_at"][2], r["max"][2], r["max_at"][2]) == (5.0, 0, 7.0, 1)
    assert r["sum"][1:].tolist() == [3.5, 24.0]
    # list order: ((1e16 + 1) + -1e16) + 1 is 1, another order gives 2 or 0
    assert M.fold([[1e16], [1.0], [-1e16], [1.0]])["sum"].tolist() == [1.0]
    assert M.fold([[1.0], [1.0], [1e16], [-1e16]])["sum"].tolist() == [2.0]
    assert M.fold([[1e16], [1.0], [1.0], [-1e16]])["sum"].tolist() == [0.0]


def test_model_ranges_and_offsets():
    x = [np.arange(20.0), np.arange(20.0)[::-1].copy()]
    rec, off = M.across(x, [3, 0, 19, 5], [10, 0, 1, 15], 4)
    assert off.tolist() == [0, 3, 3, 4, 8] and len(rec) == 8
    assert rec["min"].tolist() == [3.0, 7.0, 8.0, 0.0, 5.0, 9.0, 6.0, 2.0]
    assert rec["max_at"].tolist() == [1, 1, 0, 0, 1, 1, 0, 0]
    assert rec["sum"].tolist() == [19.0] * 8


def test_symbols_are_bound(A):
    lib = A.capi.lib()
    for name in ("atsc_across_outputs", "atsc_across_windows_dev", "atsc_across_windows", "atsc_stream_across_windows"):
        assert hasattr(lib, name) and name in A.capi.SIGNATURES, name


def test_public_surfaces(A):
    want = {(A.Context, "across_windows_host"): "(self, records_list, begins, counts, stride=1, has_count=False)",
            (A.DPlan, "across_windows"): "(self, d_body, others, other_bodies, begins, counts, d_out, stride=1, stream=0)",
            (A.CompressedStream, "across_windows"): "(self, others, begins, counts, stride=1)",
            (A.stream, "across_data_windows"): "(ctx, bros, begins, counts, stride=1)"}
    for (owner, name), sig in want.items():
        f = getattr(owner, name)
        assert str(inspect.signature(f)) == sig, name
        assert f.__doc__ and f.__doc__.strip()
    assert A.across_data_windows is A.stream.across_data_windows
    assert A.across_outputs is A.engine.across_outputs and A.across_offsets is A.engine.across_offsets
