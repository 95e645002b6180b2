"""NumPy model of the windowed across (include/atsc_hip.h, DESIGN.md "Windowed across"): count, min, max and sum over N
streams at every position of ranges of the decoded streams.  The fold walks the streams in list order; min and max keep
the first of equal values (and of zeros of either sign), the sum is ((t_0 + t_1) + t_2) + .. with t_k the sample, or
-0.0 where it is NaN, and +0.0 where every sample is NaN.  NumPy's float64 add is one correctly rounded IEEE add, so
every field is the contract's bit for bit."""
import numpy as np

RECORD = np.dtype([("count", "<u4"), ("min_at", "<u2"), ("max_at", "<u2"), ("min", "<f8"), ("max", "<f8"), ("sum", "<f8")])
MAX_STREAMS = 64
NONE = 0xFFFF


def outputs(count, stride):
    """positions of a range of `count` samples taken every `stride` samples"""
    return (int(count) - 1) // int(stride) + 1 if count and stride else 0


def offsets(counts, stride):
    """-> len(counts) + 1 offsets: the records of range i are [off[i], off[i + 1])"""
    return np.concatenate([[0], np.cumsum([outputs(c, stride) for c in counts])]).astype(np.uint64)


def fold(columns):
    """columns: N arrays of M samples each, stream k's samples at the M positions -> RECORD array of M records"""
    columns = [np.asarray(c, dtype=np.float64) for c in columns]
    assert 1 <= len(columns) <= MAX_STREAMS
    m = len(columns[0])
    cnt = np.zeros(m, dtype=np.uint32)
    mn, mx = np.full(m, np.nan), np.full(m, np.nan)
    mn_at, mx_at = np.full(m, NONE, dtype=np.uint16), np.full(m, NONE, dtype=np.uint16)
    total = np.full(m, -0.0)
    for k, x in enumerate(columns):
        assert len(x) == m
        ok = ~np.isnan(x)
        with np.errstate(invalid="ignore"):
            total = total + np.where(ok, x, -0.0)
            first = ok & (cnt == 0)
            lt = first | (ok & (x < mn))
            gt = first | (ok & (x > mx))
        mn, mn_at = np.where(lt, x, mn), np.where(lt, np.uint16(k), mn_at)
        mx, mx_at = np.where(gt, x, mx), np.where(gt, np.uint16(k), mx_at)
        cnt = cnt + ok.astype(np.uint32)
    out = np.zeros(m, dtype=RECORD)
    out["count"], out["min_at"], out["max_at"] = cnt, mn_at, mx_at
    out["min"], out["max"] = mn, mx
    out["sum"] = np.where(cnt == 0, 0.0, total)
    return out


def across(fulls, begins, counts, stride):
    """fulls: the full decode of every stream, in list order -> (records, off) of an across call over the ranges"""
    off = offsets(counts, stride)
    parts = []
    for b, c in zip(begins, counts):
        idx = int(b) + int(stride) * np.arange(outputs(c, stride), dtype=np.int64)
        assert len(idx) == 0 or all(idx[-1] < len(f) for f in fulls)
        parts.append(fold([np.asarray(f)[idx] for f in fulls]))
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=RECORD)), off
