"""Thin Python plumbing over the C ABI: device memory and streams come from PyTorch-ROCm,
everything else happens inside libatsc_hip.so.  No compression logic lives here."""
import collections
import ctypes as C
import weakref

import numpy as np

from . import capi


def _u64(arr):
    a = np.ascontiguousarray(np.asarray(arr, dtype=np.uint64))
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


# atsc_window_stats (include/atsc_hip.h): the summary record of one window, 48 bytes
WINDOW_STATS = np.dtype([("count", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sum", "<f8"), ("first", "<f8"),
                         ("last", "<f8")])
# atsc_window_moments (include/atsc_hip.h): the centred moments of one window, 48 bytes
WINDOW_MOMENTS = np.dtype([("count", "<u8"), ("mean", "<f8"), ("m2", "<f8"), ("t_mean", "<f8"), ("t_m2", "<f8"),
                           ("c_tx", "<f8")])
# atsc_window_fit: what atsc_moments_fit reads off them, 56 bytes; slope is in value units per sample
WINDOW_FIT = np.dtype([("mean", "<f8"), ("variance", "<f8"), ("stddev", "<f8"), ("sample_variance", "<f8"),
                       ("sample_stddev", "<f8"), ("slope", "<f8"), ("intercept", "<f8")])
# atsc_window_pair (include/atsc_hip.h): the centred moments and co-moment of two streams over one window, 48 bytes
WINDOW_PAIR = np.dtype([("count", "<u8"), ("mean_x", "<f8"), ("m2_x", "<f8"), ("mean_y", "<f8"), ("m2_y", "<f8"),
                        ("c_xy", "<f8")])
# atsc_window_pair_fit: what atsc_pair_fit reads off them, 56 bytes; slope and intercept are of y on x
WINDOW_PAIR_FIT = np.dtype([("covariance", "<f8"), ("sample_covariance", "<f8"), ("correlation", "<f8"), ("slope", "<f8"),
                            ("intercept", "<f8"), ("r2", "<f8"), ("mean_diff", "<f8")])
# atsc_window_delta (include/atsc_hip.h): what the samples of one window do from one to the next, 64 bytes
WINDOW_DELTA = np.dtype([("pairs", "<u8"), ("rises", "<u8"), ("falls", "<u8"), ("up", "<f8"), ("down", "<f8"),
                         ("after_falls", "<f8"), ("max_rise", "<f8"), ("max_fall", "<f8")])
# atsc_window_delta_fit: what atsc_delta_derive reads off them, 40 bytes
WINDOW_DELTA_FIT = np.dtype([("changes", "<u8"), ("variation", "<f8"), ("net", "<f8"), ("increase", "<f8"),
                             ("mean_step", "<f8")])

# atsc_window_runs (include/atsc_hip.h): the samples of one window that meet a condition and their runs, 80 bytes
WINDOW_RUNS = np.dtype([("samples", "<u8"), ("inside", "<u8"), ("runs", "<u8"), ("longest", "<u8"),
                        ("longest_at", "<u8"), ("first_at", "<u8"), ("last_at", "<u8"), ("head", "<u8"), ("tail", "<u8"),
                        ("excess", "<f8")])
# the condition's operators, and the position of a record that has none (ATSC_RUNS_*)
RUNS_GT, RUNS_GE, RUNS_LT, RUNS_LE, RUNS_EQ, RUNS_NE = (capi.RUNS_GT, capi.RUNS_GE, capi.RUNS_LT, capi.RUNS_LE,
                                                        capi.RUNS_EQ, capi.RUNS_NE)
RUNS_NONE = capi.RUNS_NONE

# one entry of a window's extremes (atsc_extreme): the sample's own bits and its offset from the window's begin
EXTREME = np.dtype([("value", "<f8"), ("at", "<u8")])
EXTREMES_MAX_K, EXTREMES_NONE = capi.EXTREMES_MAX_K, capi.EXTREMES_NONE

# one entry of a window's value counts (atsc_value_count): a distinct value and the window's samples equal to it
VALUE_COUNT = np.dtype([("value", "<f8"), ("n", "<u8")])
VALUES_MAX_K = capi.VALUES_MAX_K
# atsc_value_mode: what atsc_values_mode reads off a record, 24 bytes
VALUE_MODE = np.dtype([("value", "<f8"), ("n", "<u8"), ("exact", "<u4"), ("pad", "<u4")])


# one entry of a select call's block (atsc_selected): the sample's own bits and its offset from the window's begin
SELECTED = np.dtype([("value", "<f8"), ("at", "<u8")])


# atsc_window_rolling (include/atsc_hip.h): the record of one position of a rolling call, 32 bytes
WINDOW_ROLLING = np.dtype([("count", "<u8"), ("min", "<f8"), ("max", "<f8"), ("sum", "<f8")])
ROLLING_MAX_WIDTH = capi.ROLLING_MAX_WIDTH


def rolling_outputs(count, width, stride=1):
    """-> the positions of a range of `count` samples under a window of `width` samples moved by `stride`
    (atsc_rolling_outputs; no GPU): (count - width) // stride + 1, or 0 where the range is shorter than the window or
    width or stride is 0"""
    return int(capi.lib().atsc_rolling_outputs(int(count), int(width), int(stride)))


def rolling_offsets(counts, width, stride=1):
    """-> uint64 array of len(counts) + 1 offsets: the records of range i of a rolling call are [off[i], off[i + 1])"""
    c = np.atleast_1d(np.asarray(counts, dtype=np.uint64))
    return np.concatenate([[0], np.cumsum([rolling_outputs(v, width, stride) for v in c], dtype=np.uint64)]).astype(np.uint64)


# atsc_across_record (include/atsc_hip.h): the record of one position of an across call, 32 bytes
ACROSS_RECORD = np.dtype([("count", "<u4"), ("min_at", "<u2"), ("max_at", "<u2"), ("min", "<f8"), ("max", "<f8"), ("sum", "<f8")])
ACROSS_MAX_STREAMS = capi.ACROSS_MAX_STREAMS


# atsc_across_moments (include/atsc_hip.h): the record of one position of an across moments call, 24 bytes
ACROSS_MOMENTS = np.dtype([("count", "<u4"), ("nans", "<u4"), ("mean", "<f8"), ("m2", "<f8")])
# atsc_across_fit: what atsc_across_moments_fit reads off them, 40 bytes
ACROSS_FIT = np.dtype([("mean", "<f8"), ("variance", "<f8"), ("stddev", "<f8"), ("sample_variance", "<f8"),
                       ("sample_stddev", "<f8")])


def across_outputs(count, stride=1):
    """-> the positions of a range of `count` samples taken every `stride` samples (atsc_across_outputs; no GPU):
    (count - 1) // stride + 1, or 0 where count or stride is 0"""
    return int(capi.lib().atsc_across_outputs(int(count), int(stride)))


def across_offsets(counts, stride=1):
    """-> uint64 array of len(counts) + 1 offsets: the records of range i of an across call are [off[i], off[i + 1])"""
    c = np.atleast_1d(np.asarray(counts, dtype=np.uint64))
    return np.concatenate([[0], np.cumsum([across_outputs(v, stride) for v in c], dtype=np.uint64)]).astype(np.uint64)


def select_bytes(n_windows, cap):
    """-> bytes of the block of a select call (ATSC_SELECT_BYTES): n_windows + 1 offsets, then cap entries"""
    return 8 * (int(n_windows) + 1) + 16 * int(cap)


def window_extremes_dtype(k):
    """-> the record of one window of an extremes call with k entries per list (include/atsc_hip.h), 16 + 32 k bytes:
    count, nans, largest[k] and smallest[k], the last two of (value, at); an empty entry is (NaN, EXTREMES_NONE)"""
    k = int(k)
    if not 1 <= k <= EXTREMES_MAX_K:
        raise ValueError("k outside 1..%d" % EXTREMES_MAX_K)
    return np.dtype([("count", "<u8"), ("nans", "<u8"), ("largest", EXTREME, (k,)), ("smallest", EXTREME, (k,))])


def window_values_dtype(k):
    """-> the record of one window of a value-count call with k entries (include/atsc_hip.h), 32 + 16 k bytes: count,
    nans, below, distinct, more and entry[k] of (value, n); an unused entry is (NaN, 0)"""
    k = int(k)
    if not 1 <= k <= VALUES_MAX_K:
        raise ValueError("k outside 1..%d" % VALUES_MAX_K)
    return np.dtype([("count", "<u8"), ("nans", "<u8"), ("below", "<u8"), ("distinct", "<u4"), ("more", "<u4"),
                     ("entry", VALUE_COUNT, (k,))])


def _windows(begins, counts):
    b, pb = _u64(np.atleast_1d(begins))
    c, pc = _u64(np.atleast_1d(counts))
    if len(b) != len(c):
        raise ValueError("begins and counts differ in length")
    return b, pb, c, pc


def _levels(levels):
    q = np.ascontiguousarray(np.atleast_1d(np.asarray(levels, dtype=np.float64)))
    return q, q.ctypes.data_as(C.POINTER(C.c_double))


# One window query, as its four surfaces (Context.*_windows_host, DPlan.*_windows, CompressedStream.*_windows and
# *_data_windows) need it:
#   stem    the C calls are atsc_<stem>, atsc_<stem>_dev and atsc_stream_<stem>
#   dtype   of the result: one record per window (extra is None), or per window a row of `extra` cells more than the
#           call's levels or edges; the device tensor holds at least that many bytes per window.  A function of the
#           call's own arguments where the record depends on them (the extremes' k)
#   params  the call's own arguments -> their C arguments, which stand between the windows and the result
#   block   None, or for a result that is one block whose size is not a number of records (the select's offsets and
#           entries): (n_windows, cargs) -> its bytes; the result is then that many bytes as uint64 words, whole
#   inputs  the streams the query reads, 1 or 2: each surface takes that many records, (plan, device bytes) or streams,
#           the first as its own and the others through `others`, in front of the windows in the C call.  None: the
#           number is the call's own (the across), and the C call takes it and the streams as lists (_across_*)
_Query = collections.namedtuple("_Query", "stem dtype extra params block inputs", defaults=(None, 1))


def _no_params():
    return ()


def _runs_params(op, limit):
    return int(op), float(limit)


def _extremes_params(k):
    return (C.c_uint32(_extremes_k(k)),)


def _extremes_k(k):
    k = int(k)
    if not 0 <= k < 2 ** 32:
        raise ValueError("k outside uint32")
    return k


def _extremes_dtype(k):
    """the record of a call with k; a k that the library refuses still gets a result to leave untouched"""
    return window_extremes_dtype(min(max(_extremes_k(k), 1), EXTREMES_MAX_K))


def _values_params(k, above):
    return C.c_uint32(_extremes_k(k)), C.c_double(float(above))


def _values_dtype(k, above):
    """the record of a call with k; a k that the library refuses still gets a result to leave untouched"""
    return window_values_dtype(min(max(_extremes_k(k), 1), VALUES_MAX_K))


def _select_params(op, limit, cap):
    cap = int(cap)
    if not 0 <= cap < 2 ** 64:
        raise ValueError("cap outside uint64")
    return int(op), float(limit), C.c_uint64(cap)


def _select_block(n, cargs):
    return select_bytes(n, cargs[2].value)


def _select_result(run, n, cap):
    """run(cap) -> the block of a select call over n windows as uint64 words.  -> (off, entries): the n + 1 offsets and
    the SELECTED entries written, min(off[-1], cap) of them; cap None: the sizing call, then the exact one"""
    if cap is None:
        cap = int(run(0)[n])
    blk = run(int(cap))
    off = blk[: n + 1].copy()
    m = min(int(off[n]), int(cap))
    return off, blk[n + 1: n + 1 + 2 * m].copy().view(SELECTED)


class _RollArgs(tuple):
    """the C arguments of a rolling or an across call, and the records of its ranges"""
    records = 0


def _rolling_params(width, stride, records):
    width, stride = int(width), int(stride)
    if not (0 <= width < 2 ** 64 and 0 <= stride < 2 ** 64):
        raise ValueError("width or stride outside uint64")
    a = _RollArgs((C.c_uint64(width), C.c_uint64(stride)))
    a.records = int(records)
    return a


def _rolling_block(n, cargs):
    return WINDOW_ROLLING.itemsize * cargs.records


def _rolling_delta_block(n, cargs):
    return WINDOW_DELTA.itemsize * cargs.records


def _rolling_moments_block(n, cargs):
    return WINDOW_MOMENTS.itemsize * cargs.records


def _rolling_pair_block(n, cargs):
    return WINDOW_PAIR.itemsize * cargs.records


def _rolling_runs_params(width, stride, records, op, limit):
    """the rolling's arguments, then the runs' condition"""
    a = _RollArgs(tuple(_rolling_params(width, stride, records)) + _runs_params(op, limit))
    a.records = int(records)
    return a


def _rolling_runs_block(n, cargs):
    return WINDOW_RUNS.itemsize * cargs.records


def _rolling_result(run, counts, width, stride, record=WINDOW_ROLLING):
    """run(records) -> the block of a rolling call as uint64 words.  -> (records, off): the `record` records
    (WINDOW_ROLLING; the rolling deltas': WINDOW_DELTA; the rolling moments': WINDOW_MOMENTS; the rolling pair moments': WINDOW_PAIR; the rolling runs': WINDOW_RUNS) of every position, range after range, and the ranges' record
    offsets (rolling_offsets)"""
    off = rolling_offsets(counts, width, stride)
    return run(int(off[-1])).view(record), off


def _rolling_quantile_params(width, stride, records, levels, method):
    """the rolling's arguments, then the levels and the method"""
    a = _RollArgs(tuple(_rolling_params(width, stride, records)) + _array_params(levels, method))
    a.records = int(records)
    return a


def _rolling_quantile_block(n, cargs):
    return 8 * cargs[2] * cargs.records


def _rolling_quantile_result(run, counts, width, stride, levels):
    """run(records) -> the block of a rolling quantile call as uint64 words.  -> (rows, off): a (records, n_q) float64
    array, a row per position, range after range, and the ranges' record offsets (rolling_offsets)"""
    off = rolling_offsets(counts, width, stride)
    return run(int(off[-1])).view(np.float64).reshape(int(off[-1]), len(_levels(levels)[0])), off


def _rolling_histogram_params(width, stride, records, edges, closed):
    """the rolling's arguments, then the edges and the closed side"""
    a = _RollArgs(tuple(_rolling_params(width, stride, records)) + _array_params(edges, closed))
    a.records = int(records)
    return a


def _rolling_histogram_block(n, cargs):
    return 8 * (cargs[2] + 2) * cargs.records


def _rolling_histogram_result(run, counts, width, stride, edges):
    """run(records) -> the block of a rolling histogram call as uint64 words.  -> (rows, off): a (records, n_edges + 2)
    uint64 array, a row per position, range after range, and the ranges' record offsets (rolling_offsets)"""
    off = rolling_offsets(counts, width, stride)
    return run(int(off[-1])).reshape(int(off[-1]), len(_levels(edges)[0]) + 2), off


def _across_params(stride, records):
    stride = int(stride)
    if not 0 <= stride < 2 ** 64:
        raise ValueError("stride outside uint64")
    a = _RollArgs((C.c_uint64(stride),))
    a.records = int(records)
    return a


def _across_block(n, cargs):
    return ACROSS_RECORD.itemsize * cargs.records


def _pair_matrix_params(stride, records):
    """no C argument of its own, and the records of the call"""
    a = _RollArgs(())
    a.records = int(records)
    return a


def pair_matrix_records(n):
    """-> P = n (n + 1) / 2, the records per window of a pair matrix call over n streams (atsc_pair_matrix_records; no GPU)"""
    return int(capi.lib().atsc_pair_matrix_records(int(n)))


def pair_matrix_index(n, i, j):
    """-> p, the place of pair (i, j), i <= j < n, among a window's records of a pair matrix call over n streams
    (atsc_pair_matrix_index; no GPU); ValueError for i > j or j >= n"""
    p = int(capi.lib().atsc_pair_matrix_index(int(n), int(i), int(j)))
    if p == 2 ** 64 - 1:
        raise ValueError("no pair (%d, %d) among %d streams" % (i, j, n))
    return p


def _pair_matrix_result(run, n_streams, n_windows):
    """run(records) -> the block of a pair matrix call as uint64 words.  -> the (n_windows, P) WINDOW_PAIR array"""
    p = pair_matrix_records(n_streams)
    return run(n_windows * p).view(WINDOW_PAIR).reshape(n_windows, p)


def pair_matrix_correlation(records, n):
    """-> the (W, n, n) float64 array of the correlations of every pair of the n streams, symmetric, from the (W, P)
    WINDOW_PAIR records of a pair matrix call, read through pair_fit: NaN where pair_fit gives NaN (a pair without a
    counted sample, or a stream that is constant over them).  NumPy only"""
    n = int(n)
    rec = np.asarray(records, dtype=WINDOW_PAIR).reshape(-1, pair_matrix_records(n))
    corr = pair_fit(rec.reshape(-1))["correlation"].reshape(rec.shape)
    out = np.empty((rec.shape[0], n, n), dtype=np.float64)
    i, j = np.triu_indices(n)  # row-major over i <= j: the records' order
    out[:, i, j] = corr
    out[:, j, i] = corr
    return out


def _across_result(run, counts, stride):
    """run(records) -> the block of an across call as uint64 words.  -> (records, off): the ACROSS_RECORD records of
    every position, range after range, and the ranges' record offsets (across_offsets)"""
    off = across_offsets(counts, stride)
    return run(int(off[-1])).view(ACROSS_RECORD), off


def _across_quantile_params(stride, records, levels, method):
    """the across' arguments, then the levels and the method"""
    a = _RollArgs(tuple(_across_params(stride, records)) + _array_params(levels, method))
    a.records = int(records)
    return a


def _across_quantile_block(n, cargs):
    return 8 * cargs[1] * cargs.records


def _across_quantile_result(run, counts, stride, levels):
    """run(records) -> the block of an across quantile call as uint64 words.  -> (rows, off): a (records, n_q) float64
    array, a row per position, range after range, and the ranges' record offsets (across_offsets)"""
    off = across_offsets(counts, stride)
    return run(int(off[-1])).view(np.float64).reshape(int(off[-1]), len(_levels(levels)[0])), off


def _across_extremes_params(stride, records, k):
    """the across' arguments, then k"""
    a = _RollArgs(tuple(_across_params(stride, records)) + _extremes_params(k))
    a.records = int(records)
    return a


def _across_extremes_block(n, cargs):
    """(a k that the library refuses still gets a result to leave untouched)"""
    return _extremes_dtype(cargs[1].value).itemsize * cargs.records


def _across_extremes_result(run, counts, stride, k):
    """run(records) -> the block of an across extremes call as uint64 words.  -> (records, off): the
    window_extremes_dtype(k) records of every position, range after range, and the ranges' record offsets
    (across_offsets)"""
    off = across_offsets(counts, stride)
    return run(int(off[-1])).view(_extremes_dtype(k)), off


def _across_moments_block(n, cargs):
    return ACROSS_MOMENTS.itemsize * cargs.records


def _across_moments_result(run, counts, stride):
    """run(records) -> the block of an across moments call as uint64 words.  -> (records, off): the ACROSS_MOMENTS
    records of every position, range after range, and the ranges' record offsets (across_offsets)"""
    off = across_offsets(counts, stride)
    return run(int(off[-1])).view(ACROSS_MOMENTS), off


def _across_histogram_block(n, cargs):
    return 8 * (cargs[1] + 2) * cargs.records


def _across_histogram_result(run, counts, stride, edges):
    """run(records) -> the block of an across histogram call as uint64 words.  -> (rows, off): a (records, n_edges + 2)
    uint64 array, a row per position, range after range, and the ranges' record offsets (across_offsets)"""
    off = across_offsets(counts, stride)
    return run(int(off[-1])).reshape(int(off[-1]), len(_levels(edges)[0]) + 2), off


def _across_values_params(stride, records, k, above):
    """the across' arguments, then k and above"""
    a = _RollArgs(tuple(_across_params(stride, records)) + _values_params(k, above))
    a.records = int(records)
    return a


def _across_values_block(n, cargs):
    """(a k that the library refuses still gets a result to leave untouched)"""
    return _values_dtype(cargs[1].value, None).itemsize * cargs.records


def _across_values_result(run, counts, stride, k):
    """run(records) -> the block of an across value-count call as uint64 words.  -> (records, off): the
    window_values_dtype(k) records of every position, range after range, and the ranges' record offsets
    (across_offsets)"""
    off = across_offsets(counts, stride)
    return run(int(off[-1])).view(_values_dtype(k, None)), off


def _array_params(values, flag):
    """levels and method, or edges and closed"""
    a, pa = _levels(values)
    return len(a), pa, int(flag)


_AGGREGATE = _Query("aggregate_windows", WINDOW_STATS, None, _no_params)
_MOMENTS = _Query("moments_windows", WINDOW_MOMENTS, None, _no_params)
_DELTA = _Query("delta_windows", WINDOW_DELTA, None, _no_params)
_PAIR = _Query("pair_windows", WINDOW_PAIR, None, _no_params, inputs=2)
_RUNS = _Query("runs_windows", WINDOW_RUNS, None, _runs_params)
_EXTREMES = _Query("extremes_windows", _extremes_dtype, None, _extremes_params)
_VALUES = _Query("values_windows", _values_dtype, None, _values_params)
_SELECT = _Query("select_windows", np.dtype(np.uint64), None, _select_params, _select_block)
_ROLLING = _Query("rolling_windows", np.dtype(np.uint64), None, _rolling_params, _rolling_block)
_ROLLING_DELTA = _Query("rolling_delta_windows", np.dtype(np.uint64), None, _rolling_params, _rolling_delta_block)
_ROLLING_MOMENTS = _Query("rolling_moments_windows", np.dtype(np.uint64), None, _rolling_params, _rolling_moments_block)
_ROLLING_RUNS = _Query("rolling_runs_windows", np.dtype(np.uint64), None, _rolling_runs_params, _rolling_runs_block)
_ROLLING_PAIR = _Query("rolling_pair_windows", np.dtype(np.uint64), None, _rolling_params, _rolling_pair_block, inputs=2)
_ROLLING_QUANTILE = _Query("rolling_quantile_windows", np.dtype(np.uint64), None, _rolling_quantile_params, _rolling_quantile_block)
_ROLLING_HISTOGRAM = _Query("rolling_histogram_windows", np.dtype(np.uint64), None, _rolling_histogram_params,
                           _rolling_histogram_block)
_ACROSS = _Query("across_windows", np.dtype(np.uint64), None, _across_params, _across_block, inputs=None)
_ACROSS_QUANTILE = _Query("across_quantile_windows", np.dtype(np.uint64), None, _across_quantile_params, _across_quantile_block,
                          inputs=None)
_ACROSS_EXTREMES = _Query("across_extremes_windows", np.dtype(np.uint64), None, _across_extremes_params, _across_extremes_block,
                          inputs=None)
_ACROSS_MOMENTS = _Query("across_moments_windows", np.dtype(np.uint64), None, _across_params, _across_moments_block, inputs=None)
# (the across quantiles' arguments serve: the stride, then the edges and the closed side in the levels' and the method's place)
_ACROSS_HISTOGRAM = _Query("across_histogram_windows", np.dtype(np.uint64), None, _across_quantile_params, _across_histogram_block,
                           inputs=None)
_ACROSS_VALUES = _Query("across_values_windows", np.dtype(np.uint64), None, _across_values_params, _across_values_block,
                        inputs=None)
# (the pair matrix takes its streams as lists, as the across calls do, and nothing of its own: `stride` is not passed on)
_PAIR_MATRIX = _Query("pair_matrix_windows", np.dtype(np.uint64), None, _pair_matrix_params, _rolling_pair_block, inputs=None)
_QUANTILE = _Query("quantile_windows", np.dtype(np.float64), 0, _array_params)
_HISTOGRAM = _Query("histogram_windows", np.dtype(np.uint64), 2, _array_params)


def _query_width(q, cargs):
    """elements of q.dtype per window"""
    return 1 if q.extra is None else cargs[0] + q.extra


def _query_dtype(q, params):
    return q.dtype(*params) if callable(q.dtype) else q.dtype


def _query_bytes(q, n, cargs, params):
    """bytes of the result of n windows"""
    return q.block(n, cargs) if q.block else _query_dtype(q, params).itemsize * _query_width(q, cargs) * n


def _query_result(q, n, cargs, fn, params=()):
    """-> (the zeroed host result of n windows, at least one, and its pointer as fn's last argument)"""
    rows = max(n, 1)
    if q.block:
        out = np.zeros(q.block(n, cargs) // 8, dtype=np.uint64)
    else:
        out = np.zeros(rows if q.extra is None else (rows, _query_width(q, cargs)), dtype=_query_dtype(q, params))
    return out, out.ctypes.data_as(fn.argtypes[-1])


def _query_rows(q, out, n):
    """the result of n windows: its records, or the block whole"""
    return out if q.block else out[:n]


def _query_others(q, others):
    if len(others) != q.inputs - 1:
        raise ValueError("%s reads %d streams" % (q.stem, q.inputs))
    return others


def _query_host(q, ctx, records, begins, counts, has_count, *params, others=()):
    """Context.*_windows_host: atsc_<stem> over the records (others: the further streams' records)"""
    arrays = [np.frombuffer(bytes(r), dtype=np.uint8) for r in (records,) + tuple(_query_others(q, others))]
    bodies = []
    for b in arrays:
        bodies += [b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), int(has_count)]
    wb, pb, wc, pc = _windows(begins, counts)
    cargs = q.params(*params)
    fn = getattr(capi.lib(), "atsc_" + q.stem)
    out, po = _query_result(q, len(wb), cargs, fn, params)
    rc = fn(ctx._h, *bodies, len(wb), pb, pc, *cargs, po)
    capi.check(rc, ctx._h)
    return _query_rows(q, out, len(wb))


def _query_dev(q, dplan, d_body, begins, counts, d_out, stream, *params, others=()):
    """DPlan.*_windows: atsc_<stem>_dev into the device tensor d_out (others: the further streams' (plan, device bytes))"""
    b, pb, c, pc = _windows(begins, counts)
    cargs = q.params(*params)
    assert q.extra is None or d_out.element_size() == 8
    assert d_out.is_contiguous()
    assert d_out.numel() * d_out.element_size() >= _query_bytes(q, len(b), cargs, params)
    plans = [dplan._h, C.c_void_p(d_body.data_ptr())]
    for dp, body in _query_others(q, others):
        plans += [dp._h, C.c_void_p(body.data_ptr())]
    rc = getattr(capi.lib(), "atsc_%s_dev" % q.stem)(dplan.ctx._h, *plans, len(b), pb, pc,
                                                     *cargs, C.c_void_p(d_out.data_ptr()), C.c_void_p(stream))
    capi.check(rc, dplan.ctx._h)


def _across_list(pointers):
    """a C array of pointers, as the across calls take their streams"""
    return (C.c_void_p * max(len(pointers), 1))(*pointers)


def _across_host(ctx, records_list, begins, counts, has_count, stride, records, *params, q=_ACROSS):
    """atsc_across_windows (q: or the across call that takes `params` more) over the records of every stream of the list
    (has_count: one flag for all of them)"""
    arrays = [np.frombuffer(bytes(r), dtype=np.uint8) for r in records_list]
    lens, plens = _u64(np.array([len(b) for b in arrays], dtype=np.uint64))
    flags = np.full(max(len(arrays), 1), int(has_count), dtype=np.int32)
    wb, pb, wc, pc = _windows(begins, counts)
    cargs = q.params(stride, records, *params)
    fn = getattr(capi.lib(), "atsc_" + q.stem)
    out, po = _query_result(q, len(wb), cargs, fn)
    rc = fn(ctx._h, len(arrays), _across_list([b.ctypes.data for b in arrays]), plens,
            flags.ctypes.data_as(C.POINTER(C.c_int32)), len(wb), pb, pc, *cargs, po)
    capi.check(rc, ctx._h)
    return _query_rows(q, out, len(wb))


def _across_dev(plans, bodies, begins, counts, d_out, stream, stride, records, *params, q=_ACROSS):
    """atsc_across_windows_dev (q: or the across call that takes `params` more) over the plans and their device bytes
    into the device tensor d_out"""
    b, pb, c, pc = _windows(begins, counts)
    cargs = q.params(stride, records, *params)
    assert len(plans) == len(bodies) and d_out.is_contiguous()
    assert d_out.numel() * d_out.element_size() >= _query_bytes(q, len(b), cargs, ())
    ctx = plans[0].ctx
    rc = getattr(capi.lib(), "atsc_%s_dev" % q.stem)(ctx._h, len(plans), _across_list([p._h.value for p in plans]),
                                                     _across_list([t.data_ptr() for t in bodies]), len(b), pb, pc, *cargs,
                                                     C.c_void_p(d_out.data_ptr()), C.c_void_p(stream))
    capi.check(rc, ctx._h)


def histogram_edges_uniform(lo, hi, n_bins):
    """-> the n_bins + 1 edges of n_bins equal bins over [lo, hi]: numpy.linspace(lo, hi, n_bins + 1) bit for bit, or
    AtscError(E_INVALID) where that is no strictly ascending edge set (atsc_histogram_edges_uniform; no GPU)"""
    n_bins = int(n_bins)
    if not 0 <= n_bins < 2 ** 32:
        raise ValueError("n_bins outside uint32")
    out = np.zeros(min(n_bins, capi.HIST_MAX_EDGES) + 1, dtype=np.float64)
    capi.check(capi.lib().atsc_histogram_edges_uniform(float(lo), float(hi), n_bins,
                                                       out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


def moments_fit(moments):
    """-> WINDOW_FIT array: mean, population and sample variance / stddev, and the least-squares slope (per sample) and
    intercept (at the window's first sample) of every WINDOW_MOMENTS record (atsc_moments_fit; no GPU)"""
    m = np.ascontiguousarray(np.atleast_1d(np.asarray(moments, dtype=WINDOW_MOMENTS)))
    out = np.zeros(max(len(m), 1), dtype=WINDOW_FIT)
    capi.check(capi.lib().atsc_moments_fit(C.c_void_p(m.ctypes.data), len(m), C.c_void_p(out.ctypes.data)))
    return out[: len(m)]


def across_moments_fit(moments):
    """-> ACROSS_FIT array: mean, population and sample variance / stddev of every ACROSS_MOMENTS record
    (atsc_across_moments_fit; no GPU)"""
    m = np.ascontiguousarray(np.atleast_1d(np.asarray(moments, dtype=ACROSS_MOMENTS)))
    out = np.zeros(max(len(m), 1), dtype=ACROSS_FIT)
    capi.check(capi.lib().atsc_across_moments_fit(C.c_void_p(m.ctypes.data), len(m), C.c_void_p(out.ctypes.data)))
    return out[: len(m)]


def across_moments_merge(records):
    """-> one ACROSS_MOMENTS record (a 0-d array): the records of one position from calls over consecutive sub-lists of a
    list, left to right, folded by the moments' Merge into the record of the whole list (atsc_across_moments_merge; no
    GPU) -- how more than ACROSS_MAX_STREAMS streams are queried"""
    r = np.ascontiguousarray(np.atleast_1d(np.asarray(records, dtype=ACROSS_MOMENTS)))
    out = np.zeros(1, dtype=ACROSS_MOMENTS)
    capi.check(capi.lib().atsc_across_moments_merge(C.c_void_p(r.ctypes.data if len(r) else None), len(r),
                                                    C.c_void_p(out.ctypes.data)))
    return out[0]


def pair_fit(pairs):
    """-> WINDOW_PAIR_FIT array: population and sample covariance, correlation (clamped to [-1, 1]), the least-squares
    slope and intercept of y on x, r2 and the difference of the means of every WINDOW_PAIR record (atsc_pair_fit; no GPU)"""
    m = np.ascontiguousarray(np.atleast_1d(np.asarray(pairs, dtype=WINDOW_PAIR)))
    out = np.zeros(max(len(m), 1), dtype=WINDOW_PAIR_FIT)
    capi.check(capi.lib().atsc_pair_fit(C.c_void_p(m.ctypes.data), len(m), C.c_void_p(out.ctypes.data)))
    return out[: len(m)]


def delta_derive(deltas):
    """-> WINDOW_DELTA_FIT array: changes, total variation, net change, counter increase and mean step of every
    WINDOW_DELTA record (atsc_delta_derive; no GPU)"""
    d = np.ascontiguousarray(np.atleast_1d(np.asarray(deltas, dtype=WINDOW_DELTA)))
    out = np.zeros(max(len(d), 1), dtype=WINDOW_DELTA_FIT)
    capi.check(capi.lib().atsc_delta_derive(C.c_void_p(d.ctypes.data), len(d), C.c_void_p(out.ctypes.data)))
    return out[: len(d)]


def runs_merge(records):
    """-> one WINDOW_RUNS record (a 0-d array): the records of adjacent windows, left to right, folded into the record of
    their union (atsc_runs_merge; no GPU).  The nine integers are the union window's; excess is the records' sum, one add
    per record"""
    r = np.ascontiguousarray(np.atleast_1d(np.asarray(records, dtype=WINDOW_RUNS)))
    out = np.zeros(1, dtype=WINDOW_RUNS)
    capi.check(capi.lib().atsc_runs_merge(C.c_void_p(r.ctypes.data if len(r) else None), len(r),
                                          C.c_void_p(out.ctypes.data)))
    return out[0]


def extremes_merge(records, k):
    """-> one record of window_extremes_dtype(k) (a 0-d array): the records of adjacent windows, left to right, folded
    into the record of their union, which it equals bit for bit (atsc_extremes_merge; no GPU)"""
    dt = window_extremes_dtype(k)
    r = np.ascontiguousarray(np.atleast_1d(np.asarray(records, dtype=dt)))
    out = np.zeros(1, dtype=dt)
    capi.check(capi.lib().atsc_extremes_merge(C.c_void_p(r.ctypes.data if len(r) else None), len(r), int(k),
                                              C.c_void_p(out.ctypes.data)))
    return out[0]


def values_merge(records, k):
    """-> one record of window_values_dtype(k) (a 0-d array): the records of pairwise disjoint windows (one k, one
    above; any order, any streams) folded into the record of their union, which it equals bit for bit
    (atsc_values_merge; no GPU)"""
    dt = window_values_dtype(k)
    r = np.ascontiguousarray(np.atleast_1d(np.asarray(records, dtype=dt)))
    out = np.zeros(1, dtype=dt)
    capi.check(capi.lib().atsc_values_merge(C.c_void_p(r.ctypes.data if len(r) else None), len(r), int(k),
                                            C.c_void_p(out.ctypes.data)))
    return out[0]


def values_mode(records, k):
    """-> VALUE_MODE array: of every record of window_values_dtype(k) the listed value with the largest n (of equal n
    the smallest value), that n, and exact = (more == 0); (NaN, 0) where nothing is listed (atsc_values_mode; no GPU)"""
    dt = window_values_dtype(k)
    r = np.ascontiguousarray(np.atleast_1d(np.asarray(records, dtype=dt)))
    out = np.zeros(max(len(r), 1), dtype=VALUE_MODE)
    capi.check(capi.lib().atsc_values_mode(C.c_void_p(r.ctypes.data if len(r) else None), len(r), int(k),
                                           C.c_void_p(out.ctypes.data)))
    return out[: len(r)]


def bucket_windows(begin, count, bucket):
    """-> (begins, counts): [begin, begin + count) cut into windows of `bucket` samples, the last one shorter"""
    begin, count, bucket = int(begin), int(count), int(bucket)
    if bucket < 1:
        raise ValueError("bucket must be >= 1")
    b = np.arange(begin, begin + count, bucket, dtype=np.uint64)
    c = np.minimum(np.uint64(bucket), np.uint64(begin + count) - b).astype(np.uint64)
    return b, c


class Context:
    """One atsc_ctx (one per host thread / per GPU rank)."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        capi.check(capi.lib().atsc_ctx_create(C.byref(self._h), int(device)))
        self.device = int(device)
        self._children = weakref.WeakSet()  # plans own device blocks of this context's pool

    def close(self):
        if self._h:
            for ch in list(self._children):  # plans go first: atsc_ctx_destroy releases the pool
                ch.close()
            capi.lib().atsc_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- diagnostics -----------------------------------------------------------------------
    def enable_diag(self, on=True):
        capi.check(capi.lib().atsc_ctx_enable_diag(self._h, int(on)), self._h)

    def last_diag(self, n_frames):
        arr = (capi.FrameDiag * n_frames)()
        capi.check(capi.lib().atsc_ctx_last_diag(self._h, arr, n_frames), self._h)
        return arr

    def set_adaptive_order(self, on=True):
        """Pipelined calls start a class's costliest frames (previous batch's clocks) first."""
        capi.check(capi.lib().atsc_ctx_set_adaptive_order(self._h, int(on)), self._h)

    def set_chains(self, n):
        """Chains (context streams + scratch sets) the pipelined calls rotate over: 1..4."""
        capi.check(capi.lib().atsc_ctx_set_chains(self._h, int(n)), self._h)

    def set_profiling(self, on=True):
        capi.check(capi.lib().atsc_ctx_set_profiling(self._h, int(on)), self._h)

    def profile_read(self):
        """-> (summed ms of the dominant k_compress launches, number of launches)"""
        ms = C.c_double()
        cnt = C.c_uint64()
        capi.check(capi.lib().atsc_ctx_profile_read(self._h, C.byref(ms), C.byref(cnt)), self._h)
        return ms.value, cnt.value

    # ---- host-pointer convenience ----------------------------------------------------------
    def compress_host(self, samples, frame_off, compressor=capi.AUTO, bounded=True, max_error=0.03,
                      level=0):
        """-> (records bytes, rec_off uint64[n+1], chosen uint8[n], err float64[n])"""
        x = np.ascontiguousarray(np.asarray(samples, dtype=np.float64))
        off, poff = _u64(frame_off)
        nf = len(off) - 1
        lens = np.diff(off.astype(np.int64))
        cap = int(np.sum(48 + np.where(lens > 65535, 17, 14) * lens))  # sum of atsc_payload_bound_bytes + 16
        body = np.empty(max(cap, 16), dtype=np.uint8)
        blen = C.c_uint64()
        rec = np.zeros(nf + 1, dtype=np.uint64)
        chosen = np.zeros(nf, dtype=np.uint8)
        err = np.zeros(nf, dtype=np.float64)
        rc = capi.lib().atsc_compress_frames(
            self._h, x.ctypes.data_as(C.POINTER(C.c_double)), poff, nf, int(compressor),
            int(bool(bounded)), C.c_float(np.float32(max_error)), int(level),
            body.ctypes.data_as(C.POINTER(C.c_uint8)), body.size, C.byref(blen),
            rec.ctypes.data_as(C.POINTER(C.c_uint64)), chosen.ctypes.data_as(C.POINTER(C.c_uint8)),
            err.ctypes.data_as(C.POINTER(C.c_double)))
        capi.check(rc, self._h)
        return bytes(body[: blen.value]), rec, chosen, err

    def decompress_host(self, records, has_count=False):
        b = np.frombuffer(bytes(records), dtype=np.uint8)
        dp = DPlan(self, records, has_count)
        n = dp.n_samples
        dp.close()
        out = np.empty(max(n, 1), dtype=np.float64)
        on = C.c_uint64()
        rc = capi.lib().atsc_decompress_frames(
            self._h, b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), int(has_count),
            out.ctypes.data_as(C.POINTER(C.c_double)), out.size, C.byref(on))
        capi.check(rc, self._h)
        return out[: on.value]

    def decompress_window_host(self, records, begin, count, has_count=False):
        """Samples [begin, begin + count) of the decoded records (atsc_decompress_window): only the touched records
        are planned and uploaded."""
        b = np.frombuffer(bytes(records), dtype=np.uint8)
        out = np.empty(max(int(count), 1), dtype=np.float64)
        on = C.c_uint64()
        rc = capi.lib().atsc_decompress_window(
            self._h, b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), int(has_count), int(begin), int(count),
            out.ctypes.data_as(C.POINTER(C.c_double)), int(count), C.byref(on))
        capi.check(rc, self._h)
        return out[: on.value]

    def aggregate_windows_host(self, records, begins, counts, has_count=False):
        """-> WINDOW_STATS array: count / min / max / sum / first / last of every window [begins[i], begins[i] +
        counts[i]) of the decoded records (atsc_aggregate_windows)"""
        return _query_host(_AGGREGATE, self, records, begins, counts, has_count)

    def moments_windows_host(self, records, begins, counts, has_count=False):
        """-> WINDOW_MOMENTS array: count, mean and the centred moments of value and position of every window
        [begins[i], begins[i] + counts[i]) of the decoded records (atsc_moments_windows)"""
        return _query_host(_MOMENTS, self, records, begins, counts, has_count)

    def pair_windows_host(self, records_x, records_y, begins, counts, has_count=False):
        """-> WINDOW_PAIR array: count, the means and centred moments of x and y and their co-moment over every window
        [begins[i], begins[i] + counts[i]) of the two decoded record streams (atsc_pair_windows)"""
        return _query_host(_PAIR, self, records_x, begins, counts, has_count, others=(records_y,))

    def delta_windows_host(self, records, begins, counts, has_count=False):
        """-> WINDOW_DELTA array: the counted pairs of adjacent samples, the rises and falls among them, their sums and
        largest steps of every window [begins[i], begins[i] + counts[i]) of the decoded records (atsc_delta_windows)"""
        return _query_host(_DELTA, self, records, begins, counts, has_count)

    def runs_windows_host(self, records, begins, counts, op, limit, has_count=False):
        """-> WINDOW_RUNS array: the samples with x OP limit (op: RUNS_GT .. RUNS_NE), their maximal runs, the longest
        run, the first and last such sample, the runs at the two ends and the sum of |x - limit| of every window
        [begins[i], begins[i] + counts[i]) of the decoded records (atsc_runs_windows)"""
        return _query_host(_RUNS, self, records, begins, counts, has_count, op, limit)

    def select_windows_host(self, records, begins, counts, op, limit, cap=None, has_count=False):
        """-> (off, entries): the samples with x OP limit (op: RUNS_GT .. RUNS_NE) of every window and where they are
        (atsc_select_windows).  off: n_windows + 1 offsets, off[i + 1] - off[i] the selected samples of window i, always the
        true numbers; entries: SELECTED records (value, at) in window order and ascending position, the first
        min(off[-1], cap) of them.  cap None: a sizing call (cap 0), then the exact one"""
        n = len(np.atleast_1d(begins))
        return _select_result(lambda c: _query_host(_SELECT, self, records, begins, counts, has_count, op, limit, c), n, cap)

    def rolling_windows_host(self, records, begins, counts, width, stride=1, has_count=False):
        """-> (records, off): count / min / max / sum of the window of `width` samples at every `stride`-th position of
        every range [begins[i], begins[i] + counts[i]) of the decoded records (atsc_rolling_windows).  records: a
        WINDOW_ROLLING array, range after range; off: len(begins) + 1 offsets, range i's records being
        records[off[i]:off[i + 1]] (a range shorter than the window has none)"""
        return _rolling_result(lambda m: _query_host(_ROLLING, self, records, begins, counts, has_count, width, stride, m),
                               counts, width, stride)

    def rolling_delta_windows_host(self, records, begins, counts, width, stride=1, has_count=False):
        """-> (records, off): the deltas' record (pairs, rises, falls, their sums and largest steps) of the window of
        `width` samples at every `stride`-th position of every range [begins[i], begins[i] + counts[i]) of the decoded
        records (atsc_rolling_delta_windows).  records: a WINDOW_DELTA array, range after range, which delta_derive
        takes; off: as rolling_windows_host's"""
        return _rolling_result(lambda m: _query_host(_ROLLING_DELTA, self, records, begins, counts, has_count, width, stride, m),
                               counts, width, stride, WINDOW_DELTA)

    def rolling_runs_windows_host(self, records, begins, counts, width, op, limit, stride=1, has_count=False):
        """-> (records, off): the runs' record (samples, inside, runs, the longest run and where, the first and last
        inside sample, head, tail, excess) under the condition x OP limit (op: RUNS_GT .. RUNS_NE) of the window of
        `width` samples at every `stride`-th position of every range [begins[i], begins[i] + counts[i]) of the decoded
        records (atsc_rolling_runs_windows).  records: a WINDOW_RUNS array, range after range, positions counted from
        each window's first sample; runs_merge folds the records of adjacent disjoint positions (stride == width); off:
        as rolling_windows_host's"""
        return _rolling_result(
            lambda m: _query_host(_ROLLING_RUNS, self, records, begins, counts, has_count, width, stride, m, op, limit),
            counts, width, stride, WINDOW_RUNS)

    def rolling_moments_windows_host(self, records, begins, counts, width, stride=1, has_count=False):
        """-> (records, off): the moments' record (count, mean, m2, t_mean, t_m2, c_tx) of the window of `width` samples
        at every `stride`-th position of every range [begins[i], begins[i] + counts[i]) of the decoded records
        (atsc_rolling_moments_windows).  records: a WINDOW_MOMENTS array, range after range, which moments_fit takes
        (the slope per sample, t_mean from the window's first sample); off: as rolling_windows_host's"""
        return _rolling_result(lambda m: _query_host(_ROLLING_MOMENTS, self, records, begins, counts, has_count, width, stride, m),
                               counts, width, stride, WINDOW_MOMENTS)

    def rolling_quantile_windows_host(self, records, begins, counts, width, levels, stride=1, method=capi.QUANTILE_LINEAR,
                                      has_count=False):
        """-> (rows, off): the levels (quantile_windows_host's rule and methods) of the window of `width` samples, at most
        ROLLING_QUANTILE_MAX_WIDTH, at every `stride`-th position of every range [begins[i], begins[i] + counts[i]) of
        the decoded records (atsc_rolling_quantile_windows).  rows: a (records, n_levels) float64 array, a row per
        position, range after range: the row quantile_windows_host gives for the listed window; NaN where the window
        holds no sample; off: as rolling_windows_host's"""
        return _rolling_quantile_result(
            lambda m: _query_host(_ROLLING_QUANTILE, self, records, begins, counts, has_count, width, stride, m, levels, method),
            counts, width, stride, levels)

    def rolling_histogram_windows_host(self, records, begins, counts, width, edges, stride=1, closed=capi.HIST_LEFT_CLOSED,
                                       has_count=False):
        """-> (rows, off): the value-bin counts (histogram_windows_host's edges, closed side and layout) of the window of
        `width` samples at every `stride`-th position of every range [begins[i], begins[i] + counts[i]) of the decoded
        records (atsc_rolling_histogram_windows).  rows: a (records, n_edges + 2) uint64 array, a row per position, range
        after range: the row histogram_windows_host gives for the listed window, its counters summing to `width`; off: as
        rolling_windows_host's"""
        return _rolling_histogram_result(
            lambda m: _query_host(_ROLLING_HISTOGRAM, self, records, begins, counts, has_count, width, stride, m, edges, closed),
            counts, width, stride, edges)

    def rolling_pair_windows_host(self, records_x, records_y, begins, counts, width, stride=1, has_count=False):
        """-> (records, off): the pair moments' record (count, mean_x, m2_x, mean_y, m2_y, c_xy) of the window of `width`
        samples at every `stride`-th position of every range [begins[i], begins[i] + counts[i]) of the two decoded
        record streams (atsc_rolling_pair_windows): sample j of x goes with sample j of y, and a position's window must
        lie inside both.  records: a WINDOW_PAIR array, range after range, which pair_fit takes (covariance,
        correlation, the slope and intercept of y on x); off: as rolling_windows_host's"""
        return _rolling_result(lambda m: _query_host(_ROLLING_PAIR, self, records_x, begins, counts, has_count, width, stride, m,
                                                     others=(records_y,)),
                               counts, width, stride, WINDOW_PAIR)

    def pair_matrix_windows_host(self, records_list, begins, counts, has_count=False):
        """-> (W, P) WINDOW_PAIR array: per window [begins[i], begins[i] + counts[i]) the pair moments of every pair
        (i, j), i <= j, of the decoded record streams of records_list (at most ACROSS_MAX_STREAMS; has_count holds for
        every one of them), at column pair_matrix_index(n, i, j): bit for bit what pair_windows_host gives for streams i
        and j (atsc_pair_matrix_windows).  pair_fit and pair_matrix_correlation read covariance and correlation off it"""
        return _pair_matrix_result(lambda m: _across_host(self, records_list, begins, counts, has_count, 0, m, q=_PAIR_MATRIX),
                                   len(records_list), len(np.atleast_1d(begins)))

    def across_windows_host(self, records_list, begins, counts, stride=1, has_count=False):
        """-> (records, off): count / min / max / sum over the streams of records_list (at most ACROSS_MAX_STREAMS
        decoded record streams, sample j of one going with sample j of every other) at every `stride`-th position of
        every range [begins[i], begins[i] + counts[i]) (atsc_across_windows).  records: an ACROSS_RECORD array, range
        after range, min_at / max_at the index in records_list of the stream that holds the extreme; off: len(begins)
        + 1 offsets, range i's records being records[off[i]:off[i + 1]].  has_count holds for every stream"""
        return _across_result(lambda m: _across_host(self, records_list, begins, counts, has_count, stride, m), counts, stride)

    def across_quantile_windows_host(self, records_list, begins, counts, levels, stride=1, method=capi.QUANTILE_LINEAR,
                                     has_count=False):
        """-> (rows, off): the levels (quantile_windows_host's rule and methods) of the samples that the streams of
        records_list (at most ACROSS_MAX_STREAMS decoded record streams, as across_windows_host takes them) hold at every
        `stride`-th position of every range [begins[i], begins[i] + counts[i]) (atsc_across_quantile_windows).  rows: a
        (records, n_levels) float64 array, a row per position, range after range, NaN where every stream's sample is NaN;
        off: across_offsets(counts, stride), range i's rows being rows[off[i]:off[i + 1]].  has_count holds for every
        stream"""
        return _across_quantile_result(
            lambda m: _across_host(self, records_list, begins, counts, has_count, stride, m, levels, method, q=_ACROSS_QUANTILE),
            counts, stride, levels)

    def across_histogram_windows_host(self, records_list, begins, counts, edges, stride=1, closed=capi.HIST_LEFT_CLOSED,
                                      has_count=False):
        """-> (rows, off): how many of the streams of records_list (at most ACROSS_MAX_STREAMS decoded record streams, as
        across_windows_host takes them) hold a sample in each value bin (histogram_windows_host's edges, `closed` and
        rule) at every `stride`-th position of every range [begins[i], begins[i] + counts[i])
        (atsc_across_histogram_windows).  rows: a (records, n_edges + 2) uint64 array, a row per position, range after
        range: bins 0 .. n_edges, then the streams whose sample is NaN; a row sums to len(records_list), and the rows of
        sub-lists add to the row of the whole list.  off: across_offsets(counts, stride), range i's rows being
        rows[off[i]:off[i + 1]].  has_count holds for every stream"""
        return _across_histogram_result(
            lambda m: _across_host(self, records_list, begins, counts, has_count, stride, m, edges, closed, q=_ACROSS_HISTOGRAM),
            counts, stride, edges)

    def across_extremes_windows_host(self, records_list, begins, counts, k, stride=1, has_count=False):
        """-> (records, off): the k largest and the k smallest of the samples that the streams of records_list (at most
        ACROSS_MAX_STREAMS decoded record streams, as across_windows_host takes them) hold at every `stride`-th position
        of every range [begins[i], begins[i] + counts[i]), and which streams hold them (atsc_across_extremes_windows).
        records: an array of window_extremes_dtype(k), one per position, range after range: the windowed extremes' record
        of the position's column, `at` being the stream's index in records_list; extremes_merge over the records of one
        position from consecutive sub-lists is the record of the whole list.  off: across_offsets(counts, stride), range
        i's records being records[off[i]:off[i + 1]].  has_count holds for every stream"""
        return _across_extremes_result(
            lambda m: _across_host(self, records_list, begins, counts, has_count, stride, m, k, q=_ACROSS_EXTREMES), counts, stride, k)

    def across_values_windows_host(self, records_list, begins, counts, k, stride=1, above=float("nan"), has_count=False):
        """-> (records, off): which values the streams of records_list (at most ACROSS_MAX_STREAMS decoded record streams,
        as across_windows_host takes them) hold at every `stride`-th position of every range
        [begins[i], begins[i] + counts[i]), and how many streams hold each: PromQL's count_values
        (atsc_across_values_windows).  records: an array of window_values_dtype(k), one per position, range after range:
        the windowed value counts' record of the position's column -- count = len(records_list), the k smallest distinct
        values above `above` (NaN: all of them) with the number of streams that hold each; values_merge over the records
        of one position from sub-lists is the record of the whole list, values_mode reads the majority value off it.
        off: across_offsets(counts, stride), range i's records being records[off[i]:off[i + 1]].  has_count holds for
        every stream"""
        return _across_values_result(
            lambda m: _across_host(self, records_list, begins, counts, has_count, stride, m, k, above, q=_ACROSS_VALUES),
            counts, stride, k)

    def across_moments_windows_host(self, records_list, begins, counts, stride=1, has_count=False):
        """-> (records, off): count, mean and m2 = sum (x - mean)^2 of the samples that the streams of records_list (at
        most ACROSS_MAX_STREAMS decoded record streams, as across_windows_host takes them) hold at every `stride`-th
        position of every range [begins[i], begins[i] + counts[i]) (atsc_across_moments_windows).  records: an array of
        ACROSS_MOMENTS, one per position, range after range; across_moments_fit reads mean, variance and stddev off them,
        across_moments_merge folds the records of one position from consecutive sub-lists.  off: across_offsets(counts,
        stride), range i's records being records[off[i]:off[i + 1]].  has_count holds for every stream"""
        return _across_moments_result(
            lambda m: _across_host(self, records_list, begins, counts, has_count, stride, m, q=_ACROSS_MOMENTS), counts, stride)

    def extremes_windows_host(self, records, begins, counts, k, has_count=False):
        """-> array of window_extremes_dtype(k): the k largest and the k smallest non-NaN samples, each with its offset
        in the window, the number of NaN samples and the length of every window [begins[i], begins[i] + counts[i]) of
        the decoded records (atsc_extremes_windows)"""
        return _query_host(_EXTREMES, self, records, begins, counts, has_count, k)

    def values_windows_host(self, records, begins, counts, k, above=float("nan"), has_count=False):
        """-> array of window_values_dtype(k): the k smallest distinct values above `above` (NaN: all of them), each
        with the number of samples equal to it, the NaN samples, the samples not above `above` and the length of every
        window [begins[i], begins[i] + counts[i]) of the decoded records (atsc_values_windows)"""
        return _query_host(_VALUES, self, records, begins, counts, has_count, k, above)

    def quantile_windows_host(self, records, begins, counts, levels, method=capi.QUANTILE_LINEAR, has_count=False):
        """-> (n_windows, n_levels) float64 array: the levels of every window [begins[i], begins[i] + counts[i]) of the
        decoded records (atsc_quantile_windows)"""
        return _query_host(_QUANTILE, self, records, begins, counts, has_count, levels, method)

    def histogram_windows_host(self, records, begins, counts, edges, closed=capi.HIST_LEFT_CLOSED, has_count=False):
        """-> (n_windows, n_edges + 2) uint64 array: per window [begins[i], begins[i] + counts[i]) of the decoded
        records, the samples in each of the n_edges + 1 bins the ascending edges cut, then the NaN samples
        (atsc_histogram_windows)"""
        return _query_host(_HISTOGRAM, self, records, begins, counts, has_count, edges, closed)

    def set_aggregate_scratch(self, nbytes):
        """Upper bound on the decoded-sample scratch of the aggregate calls (0: the default; raised to one piece)"""
        capi.check(capi.lib().atsc_ctx_set_aggregate_scratch(self._h, int(nbytes)), self._h)

    # ---- device-resident path --------------------------------------------------------------
    def plan(self, frame_off):
        return Plan(self, frame_off)


class Plan:
    """Frame layout of one batch, uploaded once (atsc_plan)."""

    def __init__(self, ctx, frame_off):
        self.ctx = ctx
        off, poff = _u64(frame_off)
        self._h = C.c_void_p()
        capi.check(capi.lib().atsc_plan_create(ctx._h, poff, len(off) - 1, C.byref(self._h)), ctx._h)
        self.n_frames = int(capi.lib().atsc_plan_n_frames(self._h))
        self.n_samples = int(capi.lib().atsc_plan_n_samples(self._h))
        self.body_bound = int(capi.lib().atsc_plan_body_bound(self._h))
        ctx._children.add(self)

    def close(self):
        if self._h:
            capi.lib().atsc_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def alloc_outputs(self, torch, device):
        """Device buffers for one compress call (torch tensors own the memory)."""
        return {
            "body": torch.empty(max(self.body_bound, 16), dtype=torch.uint8, device=device),
            "rec_off": torch.empty(self.n_frames + 1, dtype=torch.int64, device=device),
            "chosen": torch.empty(self.n_frames, dtype=torch.uint8, device=device),
            "err": torch.empty(self.n_frames, dtype=torch.float64, device=device),
        }

    def compress(self, d_samples, outs, compressor=capi.AUTO, bounded=True, max_error=0.03, level=0,
                 stream=0, pipelined=False):
        """Enqueues the compression of every frame on `stream` (a raw hipStream_t or 0).
        pipelined=True: atsc_compress_plan_dev_pipelined -- consecutive calls rotate over the plan's chains
        (streams of the context's own); `join(stream)` orders a stream after their records,
        `input_release(stream)` after their last read of d_samples."""
        assert d_samples.dtype.is_floating_point and d_samples.element_size() == 8
        assert d_samples.is_contiguous() and d_samples.numel() >= self.n_samples
        fn = capi.lib().atsc_compress_plan_dev_pipelined if pipelined else capi.lib().atsc_compress_plan_dev
        rc = fn(
            self.ctx._h, self._h, C.c_void_p(d_samples.data_ptr()), int(compressor),
            int(bool(bounded)), C.c_float(np.float32(max_error)), int(level),
            C.c_void_p(outs["body"].data_ptr()), outs["body"].numel(),
            C.c_void_p(outs["rec_off"].data_ptr()), C.c_void_p(outs["chosen"].data_ptr()),
            C.c_void_p(outs["err"].data_ptr()), C.c_void_p(stream))
        capi.check(rc, self.ctx._h)

    def join(self, stream=0):
        """`stream` waits on the device for every pipelined batch enqueued so far (records packed)."""
        capi.check(capi.lib().atsc_plan_join(self.ctx._h, self._h, C.c_void_p(stream)), self.ctx._h)

    def input_release(self, stream=0):
        """`stream` waits on the device until the pipelined calls enqueued so far have read their inputs."""
        capi.check(capi.lib().atsc_plan_input_release(self.ctx._h, self._h, C.c_void_p(stream)), self.ctx._h)


class DPlan:
    """Parsed frame table of encoded records (atsc_dplan)."""

    def __init__(self, ctx, records, has_count=False):
        self.ctx = ctx
        self._bytes = np.frombuffer(bytes(records), dtype=np.uint8)
        self._h = C.c_void_p()
        capi.check(capi.lib().atsc_dplan_create(
            ctx._h, self._bytes.ctypes.data_as(C.POINTER(C.c_uint8)), len(self._bytes),
            int(has_count), C.byref(self._h)), ctx._h)
        self.n_frames = int(capi.lib().atsc_dplan_n_frames(self._h))
        self.n_samples = int(capi.lib().atsc_dplan_n_samples(self._h))
        ctx._children.add(self)

    def close(self):
        if self._h:
            capi.lib().atsc_dplan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decompress(self, d_body, d_out, stream=0):
        rc = capi.lib().atsc_decompress_plan_dev(
            self.ctx._h, self._h, C.c_void_p(d_body.data_ptr()), C.c_void_p(d_out.data_ptr()),
            C.c_void_p(stream))
        capi.check(rc, self.ctx._h)

    def find_frames(self, begin, count):
        """-> (frame_begin, frame_end): the frames the window [begin, begin + count) touches"""
        fb, fe = C.c_uint64(), C.c_uint64()
        capi.check(capi.lib().atsc_dplan_find_frames(self._h, int(begin), int(count), C.byref(fb), C.byref(fe)),
                   self.ctx._h)
        return fb.value, fe.value

    def decompress_windows(self, d_body, begins, counts, d_out, out_off, stream=0):
        """Enqueues the windows [begins[i], begins[i] + counts[i]) into d_out at out_off[i] (atsc_decompress_windows_dev)"""
        b, pb = _u64(begins)
        c, pc = _u64(counts)
        o, po = _u64(out_off)
        assert len(b) == len(c) == len(o)
        assert d_out.element_size() == 8 and d_out.is_contiguous()
        rc = capi.lib().atsc_decompress_windows_dev(
            self.ctx._h, self._h, C.c_void_p(d_body.data_ptr()), len(b), pb, pc, po, C.c_void_p(d_out.data_ptr()),
            C.c_void_p(stream))
        capi.check(rc, self.ctx._h)

    def aggregate_windows(self, d_body, begins, counts, d_stats, stream=0):
        """Enqueues the summaries of the windows [begins[i], begins[i] + counts[i]) into d_stats, a device tensor of at
        least 48 bytes per window (atsc_aggregate_windows_dev; WINDOW_STATS records)"""
        _query_dev(_AGGREGATE, self, d_body, begins, counts, d_stats, stream)

    def moments_windows(self, d_body, begins, counts, d_out, stream=0):
        """Enqueues the moments of the windows [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least
        48 bytes per window (atsc_moments_windows_dev; WINDOW_MOMENTS records)"""
        _query_dev(_MOMENTS, self, d_body, begins, counts, d_out, stream)

    def pair_windows(self, d_body, other, other_body, begins, counts, d_out, stream=0):
        """Enqueues the pair moments of this plan's stream (x) and the plan `other`'s (y, its device bytes other_body)
        over the windows [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least 48 bytes per window
        (atsc_pair_windows_dev; WINDOW_PAIR records).  other may be this plan"""
        _query_dev(_PAIR, self, d_body, begins, counts, d_out, stream, others=((other, other_body),))

    def pair_matrix_windows(self, d_body, others, other_bodies, begins, counts, d_out, stream=0):
        """Enqueues the pair moments of every pair (i, j), i <= j, of this plan's stream (stream 0) and the plans `others`'
        (stream 1 and on, their device bytes other_bodies; at most ACROSS_MAX_STREAMS in all) over the windows
        [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least 48 P bytes per window
        (atsc_pair_matrix_windows_dev).  A plan may appear more than once.  -> the view of d_out's front as (W, P)
        WINDOW_PAIR records (a uint8 tensor of shape (W, P, 48); .cpu().numpy().view(WINDOW_PAIR)[..., 0] gives the
        fields), filled once `stream` has run"""
        import torch  # (d_out is a torch tensor: the module is loaded)
        plans = [self] + list(others)
        n, p, size = len(np.atleast_1d(begins)), pair_matrix_records(len(plans)), WINDOW_PAIR.itemsize
        _across_dev(plans, [d_body] + list(other_bodies), begins, counts, d_out, stream, 0, n * p, q=_PAIR_MATRIX)
        return d_out.reshape(-1).view(torch.uint8)[: n * p * size].reshape(n, p, size)

    def delta_windows(self, d_body, begins, counts, d_out, stream=0):
        """Enqueues the deltas of the windows [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least
        64 bytes per window (atsc_delta_windows_dev; WINDOW_DELTA records)"""
        _query_dev(_DELTA, self, d_body, begins, counts, d_out, stream)

    def runs_windows(self, d_body, begins, counts, op, limit, d_out, stream=0):
        """Enqueues the runs of the samples with x OP limit of the windows [begins[i], begins[i] + counts[i]) into d_out,
        a device tensor of at least 80 bytes per window (atsc_runs_windows_dev; WINDOW_RUNS records)"""
        _query_dev(_RUNS, self, d_body, begins, counts, d_out, stream, op, limit)

    def select_windows(self, d_body, begins, counts, op, limit, cap, d_out, stream=0):
        """the samples with x OP limit of the windows and where they are, enqueued on `stream`, into d_out, a device
        tensor of at least select_bytes(len(begins), cap) bytes: the offsets, then the entries below cap
        (atsc_select_windows_dev)"""
        _query_dev(_SELECT, self, d_body, begins, counts, d_out, stream, op, limit, cap)

    def rolling_windows(self, d_body, begins, counts, width, stride, d_out, stream=0):
        """Enqueues count / min / max / sum of the window of `width` samples at every `stride`-th position of the ranges
        [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least 32 bytes per position
        (atsc_rolling_windows_dev; WINDOW_ROLLING records, range after range).  -> the ranges' record offsets
        (rolling_offsets)"""
        off = rolling_offsets(counts, width, stride)
        _query_dev(_ROLLING, self, d_body, begins, counts, d_out, stream, width, stride, int(off[-1]))
        return off

    def rolling_delta_windows(self, d_body, begins, counts, width, stride, d_out, stream=0):
        """Enqueues the deltas' record of the window of `width` samples at every `stride`-th position of the ranges
        [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least 64 bytes per position
        (atsc_rolling_delta_windows_dev; WINDOW_DELTA records, range after range).  -> the ranges' record offsets
        (rolling_offsets)"""
        off = rolling_offsets(counts, width, stride)
        _query_dev(_ROLLING_DELTA, self, d_body, begins, counts, d_out, stream, width, stride, int(off[-1]))
        return off

    def rolling_runs_windows(self, d_body, begins, counts, width, stride, op, limit, d_out, stream=0):
        """Enqueues the runs' record under the condition x OP limit of the window of `width` samples at every
        `stride`-th position of the ranges [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least
        80 bytes per position (atsc_rolling_runs_windows_dev; WINDOW_RUNS records, range after range).  -> the ranges'
        record offsets (rolling_offsets)"""
        off = rolling_offsets(counts, width, stride)
        _query_dev(_ROLLING_RUNS, self, d_body, begins, counts, d_out, stream, width, stride, int(off[-1]), op, limit)
        return off

    def rolling_moments_windows(self, d_body, begins, counts, width, stride, d_out, stream=0):
        """Enqueues the moments' record of the window of `width` samples at every `stride`-th position of the ranges
        [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least 48 bytes per position
        (atsc_rolling_moments_windows_dev; WINDOW_MOMENTS records, range after range).  -> the ranges' record offsets
        (rolling_offsets)"""
        off = rolling_offsets(counts, width, stride)
        _query_dev(_ROLLING_MOMENTS, self, d_body, begins, counts, d_out, stream, width, stride, int(off[-1]))
        return off

    def rolling_quantile_windows(self, d_body, begins, counts, width, stride, levels, d_out, method=capi.QUANTILE_LINEAR,
                                 stream=0):
        """Enqueues the levels of the window of `width` samples at every `stride`-th position of the ranges [begins[i],
        begins[i] + counts[i]) into d_out, a float64 device tensor of at least n_levels elements per position,
        position-major (atsc_rolling_quantile_windows_dev).  -> (rows, off): the (records, n_levels) view of d_out and
        the ranges' record offsets (rolling_offsets)"""
        off = rolling_offsets(counts, width, stride)
        m, n_q = int(off[-1]), len(_levels(levels)[0])
        _query_dev(_ROLLING_QUANTILE, self, d_body, begins, counts, d_out, stream, width, stride, m, levels, method)
        return d_out.view(-1)[: m * n_q].view(m, n_q), off

    def rolling_histogram_windows(self, d_body, begins, counts, width, stride, edges, d_out, closed=capi.HIST_LEFT_CLOSED,
                                  stream=0):
        """Enqueues the value-bin counts of the window of `width` samples at every `stride`-th position of the ranges
        [begins[i], begins[i] + counts[i]) into d_out, a 64-bit integer device tensor of at least n_edges + 2 elements per
        position, position-major (atsc_rolling_histogram_windows_dev).  -> (rows, off): the (records, n_edges + 2) view
        of d_out and the ranges' record offsets (rolling_offsets)"""
        off = rolling_offsets(counts, width, stride)
        m, rows = int(off[-1]), len(_levels(edges)[0]) + 2
        _query_dev(_ROLLING_HISTOGRAM, self, d_body, begins, counts, d_out, stream, width, stride, m, edges, closed)
        return d_out.view(-1)[: m * rows].view(m, rows), off

    def rolling_pair_windows(self, d_body, other, other_body, begins, counts, width, stride, d_out, stream=0):
        """Enqueues the pair moments' record of this plan's stream (x) and the plan `other`'s (y; its device bytes
        other_body) over the window of `width` samples at every `stride`-th position of the ranges [begins[i],
        begins[i] + counts[i]) into d_out, a device tensor of at least 48 bytes per position
        (atsc_rolling_pair_windows_dev; WINDOW_PAIR records, range after range).  other may be this plan.  -> the
        ranges' record offsets (rolling_offsets)"""
        off = rolling_offsets(counts, width, stride)
        _query_dev(_ROLLING_PAIR, self, d_body, begins, counts, d_out, stream, width, stride, int(off[-1]),
                   others=((other, other_body),))
        return off

    def across_windows(self, d_body, others, other_bodies, begins, counts, d_out, stride=1, stream=0):
        """Enqueues count / min / max / sum over this plan's stream (stream 0) and the plans `others` (their device
        bytes other_bodies; stream 1 and on, in that order) at every `stride`-th position of the ranges [begins[i],
        begins[i] + counts[i]) into d_out, a device tensor of at least 32 bytes per position
        (atsc_across_windows_dev; ACROSS_RECORD records, range after range).  A plan may appear more than once.  -> the
        ranges' record offsets (across_offsets)"""
        off = across_offsets(counts, stride)
        _across_dev([self] + list(others), [d_body] + list(other_bodies), begins, counts, d_out, stream, stride, int(off[-1]))
        return off

    def across_quantile_windows(self, d_body, others, other_bodies, begins, counts, levels, d_out, stride=1,
                                method=capi.QUANTILE_LINEAR, stream=0):
        """Enqueues the levels of the samples that this plan's stream and the plans `others` (their device bytes
        other_bodies) hold at every `stride`-th position of the ranges [begins[i], begins[i] + counts[i]) into d_out, a
        float64 device tensor of at least n_levels elements per position, position-major
        (atsc_across_quantile_windows_dev).  A plan may appear more than once.  -> (rows, off): the (records, n_levels)
        view of d_out's front, filled once `stream` has run, and the ranges' record offsets (across_offsets)"""
        off = across_offsets(counts, stride)
        m, n_q = int(off[-1]), len(_levels(levels)[0])
        assert d_out.element_size() == 8
        _across_dev([self] + list(others), [d_body] + list(other_bodies), begins, counts, d_out, stream, stride, m, levels, method,
                    q=_ACROSS_QUANTILE)
        return d_out.reshape(-1)[: m * n_q].reshape(m, n_q), off

    def across_histogram_windows(self, d_body, others, other_bodies, begins, counts, edges, d_out, stride=1,
                                 closed=capi.HIST_LEFT_CLOSED, stream=0):
        """Enqueues, for every `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), how many of this
        plan's stream and the plans `others` (their device bytes other_bodies) hold a sample in each value bin into
        d_out, a uint64 (or int64) device tensor of at least n_edges + 2 elements per position, position-major
        (atsc_across_histogram_windows_dev).  A plan may appear more than once.  -> (rows, off): the
        (records, n_edges + 2) view of d_out's front, filled once `stream` has run, and the ranges' record offsets
        (across_offsets)"""
        off = across_offsets(counts, stride)
        m, rows = int(off[-1]), len(_levels(edges)[0]) + 2
        assert d_out.element_size() == 8
        _across_dev([self] + list(others), [d_body] + list(other_bodies), begins, counts, d_out, stream, stride, m, edges, closed,
                    q=_ACROSS_HISTOGRAM)
        return d_out.reshape(-1)[: m * rows].reshape(m, rows), off

    def across_extremes_windows(self, d_body, others, other_bodies, begins, counts, k, d_out, stride=1, stream=0):
        """Enqueues the k largest and the k smallest of the samples that this plan's stream (stream 0) and the plans
        `others` (their device bytes other_bodies; stream 1 and on, in that order) hold at every `stride`-th position of
        the ranges [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least 16 + 32 k bytes per
        position (atsc_across_extremes_windows_dev).  A plan may appear more than once.  -> (records, off): the view of
        d_out's front as window_extremes_dtype(k) records, one per position (a uint8 tensor of 16 + 32 k bytes a row;
        .cpu().numpy().view(window_extremes_dtype(k)) gives the fields), filled once `stream` has run, and the ranges'
        record offsets (across_offsets)"""
        import torch  # (d_out is a torch tensor: the module is loaded)
        off = across_offsets(counts, stride)
        m, size = int(off[-1]), _extremes_dtype(k).itemsize
        _across_dev([self] + list(others), [d_body] + list(other_bodies), begins, counts, d_out, stream, stride, m, k,
                    q=_ACROSS_EXTREMES)
        return d_out.reshape(-1).view(torch.uint8)[: m * size].reshape(m, size), off

    def across_values_windows(self, d_body, others, other_bodies, begins, counts, k, d_out, stride=1, above=float("nan"), stream=0):
        """Enqueues which values this plan's stream and the plans `others` (their device bytes other_bodies) hold at every
        `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), and how many streams hold each, into
        d_out, a device tensor of at least 32 + 16 k bytes per position (atsc_across_values_windows_dev): the k smallest
        distinct values above `above` (NaN: all of them).  A plan may appear more than once.  -> (records, off): the view
        of d_out's front as window_values_dtype(k) records, one per position (a uint8 tensor of 32 + 16 k bytes a row;
        .cpu().numpy().view(window_values_dtype(k)) gives the fields), filled once `stream` has run, and the ranges'
        record offsets (across_offsets)"""
        import torch  # (d_out is a torch tensor: the module is loaded)
        off = across_offsets(counts, stride)
        m, size = int(off[-1]), _values_dtype(k, None).itemsize
        _across_dev([self] + list(others), [d_body] + list(other_bodies), begins, counts, d_out, stream, stride, m, k, above,
                    q=_ACROSS_VALUES)
        return d_out.reshape(-1).view(torch.uint8)[: m * size].reshape(m, size), off

    def across_moments_windows(self, d_body, others, other_bodies, begins, counts, d_out, stride=1, stream=0):
        """Enqueues count, mean and m2 of the samples that this plan's stream (stream 0) and the plans `others` (their
        device bytes other_bodies; stream 1 and on, in that order) hold at every `stride`-th position of the ranges
        [begins[i], begins[i] + counts[i]) into d_out, a device tensor of at least 24 bytes per position
        (atsc_across_moments_windows_dev).  A plan may appear more than once.  -> (records, off): the view of d_out's front
        as ACROSS_MOMENTS records, one per position (a uint8 tensor of 24 bytes a row; .cpu().numpy().view(ACROSS_MOMENTS)
        gives the fields), filled once `stream` has run, and the ranges' record offsets (across_offsets)"""
        import torch  # (d_out is a torch tensor: the module is loaded)
        off = across_offsets(counts, stride)
        m, size = int(off[-1]), ACROSS_MOMENTS.itemsize
        _across_dev([self] + list(others), [d_body] + list(other_bodies), begins, counts, d_out, stream, stride, m,
                    q=_ACROSS_MOMENTS)
        return d_out.reshape(-1).view(torch.uint8)[: m * size].reshape(m, size), off

    def extremes_windows(self, d_body, begins, counts, k, d_out, stream=0):
        """Enqueues the k largest and the k smallest samples of the windows [begins[i], begins[i] + counts[i]) into
        d_out, a device tensor of at least 16 + 32 k bytes per window (atsc_extremes_windows_dev; records of
        window_extremes_dtype(k))"""
        _query_dev(_EXTREMES, self, d_body, begins, counts, d_out, stream, k)

    def values_windows(self, d_body, begins, counts, k, d_out, above=float("nan"), stream=0):
        """Enqueues the k smallest distinct values above `above` (NaN: all of them) of the windows [begins[i],
        begins[i] + counts[i]) and how often each occurs into d_out, a device tensor of at least 32 + 16 k bytes per
        window (atsc_values_windows_dev; records of window_values_dtype(k))"""
        _query_dev(_VALUES, self, d_body, begins, counts, d_out, stream, k, above)

    def quantile_windows(self, d_body, begins, counts, levels, d_out, method=capi.QUANTILE_LINEAR, stream=0):
        """Enqueues the levels of the windows [begins[i], begins[i] + counts[i]) into d_out, a float64 device tensor of
        at least n_windows * n_levels elements, window-major (atsc_quantile_windows_dev)"""
        _query_dev(_QUANTILE, self, d_body, begins, counts, d_out, stream, levels, method)

    def histogram_windows(self, d_body, begins, counts, edges, d_out, closed=capi.HIST_LEFT_CLOSED, stream=0):
        """Enqueues the bin counts of the windows [begins[i], begins[i] + counts[i]) into d_out, a 64-bit integer
        device tensor of at least n_windows * (n_edges + 2) elements, window-major (atsc_histogram_windows_dev)"""
        _query_dev(_HISTOGRAM, self, d_body, begins, counts, d_out, stream, edges, closed)


# ---- host-only helpers (no GPU) ------------------------------------------------------------
def chunk_sizes(n):
    cnt = capi.lib().atsc_chunk_sizes(n, None, 0)
    out = np.zeros(max(cnt, 1), dtype=np.uint64)
    capi.lib().atsc_chunk_sizes(n, out.ctypes.data_as(C.POINTER(C.c_uint64)), cnt)
    return [int(v) for v in out[:cnt]]


def clean_data(x):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    out = np.empty(max(len(a), 1), dtype=np.float64)
    k = capi.lib().atsc_clean_data(a.ctypes.data_as(C.POINTER(C.c_double)), len(a),
                                   out.ctypes.data_as(C.POINTER(C.c_double)))
    return out[:k].copy()


def bro_prefix(n_frames):
    buf = (C.c_uint8 * 32)()
    k = capi.lib().atsc_bro_prefix(n_frames, buf)
    return bytes(buf[:k])


def bro_find_window(bro, begin, count):
    """-> dict(byte_begin, byte_end, frame_begin, frame_end, sample_begin): the records of a .bro image that the window
    [begin, begin + count) touches (atsc_bro_find_window; host only)"""
    b = np.frombuffer(bytes(bro), dtype=np.uint8)
    v = [C.c_uint64() for _ in range(5)]
    rc = capi.lib().atsc_bro_find_window(b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), int(begin), int(count),
                                         *[C.byref(x) for x in v])
    capi.check(rc)
    return dict(zip(("byte_begin", "byte_end", "frame_begin", "frame_end", "sample_begin"), (x.value for x in v)))


def bro_open(bro):
    b = np.frombuffer(bytes(bro), dtype=np.uint8)
    off = C.c_uint64()
    nf = C.c_uint64()
    rc = capi.lib().atsc_bro_open(b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), C.byref(off),
                                  C.byref(nf))
    capi.check(rc)
    return off.value, nf.value
