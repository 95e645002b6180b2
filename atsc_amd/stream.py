"""Python face of the host-side mirror in libatsc_hip.so (atsc_stream.cpp): same names and argument
meaning as the reference's CompressedStream (atsc/src/data.rs) and the helpers of atsc/src/main.rs,
wavbrro/ and atsc/src/csv.rs.  Pure ctypes plumbing."""
import ctypes as C

import numpy as np

from . import capi
from .engine import WINDOW_DELTA, WINDOW_MOMENTS, WINDOW_PAIR, WINDOW_ROLLING, WINDOW_RUNS, WINDOW_STATS, _levels, _windows, delta_derive, moments_fit, pair_fit  # noqa: F401
from .engine import _AGGREGATE, _DELTA, _EXTREMES, _HISTOGRAM, _MOMENTS, _PAIR, _QUANTILE, _ROLLING, _ROLLING_DELTA, _ROLLING_MOMENTS, _ROLLING_PAIR, _ROLLING_RUNS, _RUNS, _SELECT, _VALUES, _query_others, _query_result, _query_rows, _rolling_result, _select_result
from .engine import ACROSS_RECORD, _ACROSS, _across_host, _across_list, _across_result  # noqa: F401
from .engine import _ACROSS_QUANTILE, _across_quantile_result
from .engine import _ROLLING_QUANTILE, _rolling_quantile_result
from .engine import _ROLLING_HISTOGRAM, _rolling_histogram_result
from .engine import _ACROSS_EXTREMES, _across_extremes_result
from .engine import _ACROSS_MOMENTS, _across_moments_result
from .engine import _ACROSS_HISTOGRAM, _across_histogram_result
from .engine import _ACROSS_VALUES, _across_values_result
from .engine import _PAIR_MATRIX, _pair_matrix_result


def _f64(x):
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _take_bytes(p, n):
    out = bytes(C.string_at(p, n.value)) if n.value else b""
    capi.lib().atsc_free(p)
    return out


def _take_f64(p, n):
    out = np.ctypeslib.as_array(p, shape=(max(n.value, 1),))[: n.value].copy()
    capi.lib().atsc_free(p)
    return out


def _query_stream(q, stream, begins, counts, *params, others=()):
    """CompressedStream.*_windows: atsc_stream_<stem> (q: the query's description, engine._Query; others: the further
    streams)"""
    wb, pb, wc, pc = _windows(begins, counts)
    cargs = q.params(*params)
    fn = getattr(capi.lib(), "atsc_stream_" + q.stem)
    out, po = _query_result(q, len(wb), cargs, fn, params)
    handles = [stream._h] + [o._h for o in _query_others(q, others)]
    capi.check(fn(*handles, len(wb), pb, pc, *cargs, po), stream.ctx._h)
    return _query_rows(q, out, len(wb))


def _query_image(q, ctx, bro, begins, counts, *params):
    """*_data_windows: atsc_bro_open, then atsc_<stem> over the records of the .bro image"""
    b = np.frombuffer(bytes(bro), dtype=np.uint8)
    capi.check(capi.lib().atsc_bro_open(b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), None, None))
    wb, pb, wc, pc = _windows(begins, counts)
    cargs = q.params(*params)
    fn = getattr(capi.lib(), "atsc_" + q.stem)
    out, po = _query_result(q, len(wb), cargs, fn, params)
    r = b[9:]  # the records from the frame-count varint on, as atsc_decompress_data reads them
    rc = fn(ctx._h, r.ctypes.data_as(C.POINTER(C.c_uint8)), len(r), 1, len(wb), pb, pc, *cargs, po)
    capi.check(rc, ctx._h)
    return _query_rows(q, out, len(wb))


class CompressedStream:
    """atsc/src/data.rs:29-110"""

    def __init__(self, ctx, _handle=None):
        self.ctx = ctx
        self._h = C.c_void_p()
        if _handle is None:
            capi.check(capi.lib().atsc_stream_new(ctx._h, C.byref(self._h)), ctx._h)
        else:
            self._h = _handle

    def __del__(self):
        try:
            if self._h:
                capi.lib().atsc_stream_free(self._h)
                self._h = C.c_void_p()
        except Exception:
            pass

    def compress_chunk(self, chunk):
        a, p = _f64(chunk)
        capi.check(capi.lib().atsc_stream_compress_chunk(self._h, p, len(a)), self.ctx._h)

    def compress_chunk_with(self, chunk, compressor):
        a, p = _f64(chunk)
        capi.check(capi.lib().atsc_stream_compress_chunk_with(self._h, p, len(a), int(compressor)), self.ctx._h)

    def compress_chunk_bounded_with(self, chunk, compressor, max_error, compression_speed=0):
        a, p = _f64(chunk)
        capi.check(capi.lib().atsc_stream_compress_chunk_bounded_with(
            self._h, p, len(a), int(compressor), C.c_float(np.float32(max_error)), int(compression_speed)),
            self.ctx._h)

    @property
    def frame_count(self):
        return int(capi.lib().atsc_stream_frame_count(self._h))

    def to_bytes(self):
        p = C.POINTER(C.c_uint8)()
        n = C.c_uint64()
        capi.check(capi.lib().atsc_stream_to_bytes(self._h, C.byref(p), C.byref(n)), self.ctx._h)
        return _take_bytes(p, n)

    @classmethod
    def from_bytes(cls, ctx, data):
        b = np.frombuffer(bytes(data), dtype=np.uint8)
        h = C.c_void_p()
        capi.check(capi.lib().atsc_stream_from_bytes(
            ctx._h, b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), C.byref(h)), ctx._h)
        return cls(ctx, h)

    def decompress(self):
        p = C.POINTER(C.c_double)()
        n = C.c_uint64()
        capi.check(capi.lib().atsc_stream_decompress(self._h, C.byref(p), C.byref(n)), self.ctx._h)
        return _take_f64(p, n)

    def decompress_window(self, begin, count):
        """decompress()[begin:begin + count] without decoding the frames outside it"""
        p = C.POINTER(C.c_double)()
        n = C.c_uint64()
        capi.check(capi.lib().atsc_stream_decompress_window(self._h, int(begin), int(count), C.byref(p), C.byref(n)),
                   self.ctx._h)
        return _take_f64(p, n)

    def aggregate_windows(self, begins, counts):
        """-> WINDOW_STATS array of the windows [begins[i], begins[i] + counts[i]) (atsc_stream_aggregate_windows)"""
        return _query_stream(_AGGREGATE, self, begins, counts)

    def moments_windows(self, begins, counts):
        """-> WINDOW_MOMENTS array of the windows [begins[i], begins[i] + counts[i]) (atsc_stream_moments_windows)"""
        return _query_stream(_MOMENTS, self, begins, counts)

    def pair_windows(self, other, begins, counts):
        """-> WINDOW_PAIR array of the windows [begins[i], begins[i] + counts[i]) of this stream (x) and `other` (y)
        (atsc_stream_pair_windows)"""
        return _query_stream(_PAIR, self, begins, counts, others=(other,))

    def delta_windows(self, begins, counts):
        """-> WINDOW_DELTA array of the windows [begins[i], begins[i] + counts[i]) (atsc_stream_delta_windows)"""
        return _query_stream(_DELTA, self, begins, counts)

    def runs_windows(self, begins, counts, op, limit):
        """-> WINDOW_RUNS array of the windows [begins[i], begins[i] + counts[i]) under the condition x OP limit
        (atsc_stream_runs_windows)"""
        return _query_stream(_RUNS, self, begins, counts, op, limit)

    def select_windows(self, begins, counts, op, limit, cap=None):
        """-> (off, entries) of the windows [begins[i], begins[i] + counts[i]) under the condition x OP limit, as
        Context.select_windows_host gives them (atsc_stream_select_windows)"""
        n = len(np.atleast_1d(begins))
        return _select_result(lambda c: _query_stream(_SELECT, self, begins, counts, op, limit, c), n, cap)

    def rolling_windows(self, begins, counts, width, stride=1):
        """-> (records, off) of the window of `width` samples at every `stride`-th position of the ranges [begins[i],
        begins[i] + counts[i]), as Context.rolling_windows_host gives them (atsc_stream_rolling_windows)"""
        return _rolling_result(lambda m: _query_stream(_ROLLING, self, begins, counts, width, stride, m), counts, width, stride)

    def rolling_delta_windows(self, begins, counts, width, stride=1):
        """-> (records, off): the deltas' record of the window of `width` samples at every `stride`-th position of the
        ranges [begins[i], begins[i] + counts[i]), as Context.rolling_delta_windows_host gives them
        (atsc_stream_rolling_delta_windows)"""
        return _rolling_result(lambda m: _query_stream(_ROLLING_DELTA, self, begins, counts, width, stride, m), counts, width,
                               stride, WINDOW_DELTA)

    def rolling_runs_windows(self, begins, counts, width, op, limit, stride=1):
        """-> (records, off): the runs' record under the condition x OP limit of the window of `width` samples at every
        `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), as Context.rolling_runs_windows_host
        gives them (atsc_stream_rolling_runs_windows)"""
        return _rolling_result(lambda m: _query_stream(_ROLLING_RUNS, self, begins, counts, width, stride, m, op, limit),
                               counts, width, stride, WINDOW_RUNS)

    def rolling_moments_windows(self, begins, counts, width, stride=1):
        """-> (records, off): the moments' record of the window of `width` samples at every `stride`-th position of the
        ranges [begins[i], begins[i] + counts[i]), as Context.rolling_moments_windows_host gives them
        (atsc_stream_rolling_moments_windows)"""
        return _rolling_result(lambda m: _query_stream(_ROLLING_MOMENTS, self, begins, counts, width, stride, m), counts, width,
                               stride, WINDOW_MOMENTS)

    def rolling_quantile_windows(self, begins, counts, width, levels, stride=1, method=capi.QUANTILE_LINEAR):
        """-> (rows, off): the levels of the window of `width` samples at every `stride`-th position of the ranges
        [begins[i], begins[i] + counts[i]), as Context.rolling_quantile_windows_host gives them
        (atsc_stream_rolling_quantile_windows)"""
        return _rolling_quantile_result(
            lambda m: _query_stream(_ROLLING_QUANTILE, self, begins, counts, width, stride, m, levels, method), counts, width,
            stride, levels)

    def rolling_histogram_windows(self, begins, counts, width, edges, stride=1, closed=capi.HIST_LEFT_CLOSED):
        """-> (rows, off): the value-bin counts of the window of `width` samples at every `stride`-th position of the
        ranges [begins[i], begins[i] + counts[i]), as Context.rolling_histogram_windows_host gives them
        (atsc_stream_rolling_histogram_windows)"""
        return _rolling_histogram_result(
            lambda m: _query_stream(_ROLLING_HISTOGRAM, self, begins, counts, width, stride, m, edges, closed), counts, width,
            stride, edges)

    def rolling_pair_windows(self, other, begins, counts, width, stride=1):
        """-> (records, off): the pair moments' record of this stream (x) and `other` (y) over the window of `width`
        samples at every `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), as
        Context.rolling_pair_windows_host gives them (atsc_stream_rolling_pair_windows)"""
        return _rolling_result(lambda m: _query_stream(_ROLLING_PAIR, self, begins, counts, width, stride, m, others=(other,)),
                               counts, width, stride, WINDOW_PAIR)

    def across_windows(self, others, begins, counts, stride=1):
        """-> (records, off) over this stream (stream 0) and the streams `others` (stream 1 and on) at every
        `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), as Context.across_windows_host gives
        them (atsc_stream_across_windows)"""
        return _across_result(lambda m: self._across_stream(_ACROSS, others, begins, counts, stride, m), counts, stride)

    def pair_matrix_windows(self, others, begins, counts):
        """-> (W, P) WINDOW_PAIR array: the pair moments of every pair of this stream (stream 0) and the streams `others`
        (stream 1 and on) over the windows [begins[i], begins[i] + counts[i]), as Context.pair_matrix_windows_host gives
        them (atsc_stream_pair_matrix_windows)"""
        return _pair_matrix_result(lambda m: self._across_stream(_PAIR_MATRIX, others, begins, counts, 0, m),
                                   1 + len(others), len(np.atleast_1d(begins)))

    def _across_stream(self, q, others, begins, counts, *params):
        """atsc_stream_<q.stem> over this stream and the streams `others`"""
        streams = [self] + list(others)
        wb, pb, wc, pc = _windows(begins, counts)
        cargs = q.params(*params)
        fn = getattr(capi.lib(), "atsc_stream_" + q.stem)
        out, po = _query_result(q, len(wb), cargs, fn)
        capi.check(fn(_across_list([s._h.value for s in streams]), len(streams), len(wb), pb, pc, *cargs, po), self.ctx._h)
        return _query_rows(q, out, len(wb))

    def across_quantile_windows(self, others, begins, counts, levels, stride=1, method=capi.QUANTILE_LINEAR):
        """-> (rows, off): the levels of the samples that this stream and the streams `others` hold at every
        `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), as Context.across_quantile_windows_host
        gives them (atsc_stream_across_quantile_windows)"""
        return _across_quantile_result(
            lambda m: self._across_stream(_ACROSS_QUANTILE, others, begins, counts, stride, m, levels, method), counts, stride, levels)

    def across_histogram_windows(self, others, begins, counts, edges, stride=1, closed=capi.HIST_LEFT_CLOSED):
        """-> (rows, off): how many of this stream and the streams `others` hold a sample in each value bin at every
        `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), as
        Context.across_histogram_windows_host gives them (atsc_stream_across_histogram_windows)"""
        return _across_histogram_result(
            lambda m: self._across_stream(_ACROSS_HISTOGRAM, others, begins, counts, stride, m, edges, closed), counts, stride, edges)

    def across_values_windows(self, others, begins, counts, k, stride=1, above=float("nan")):
        """-> (records, off): which values this stream and the streams `others` hold at every `stride`-th position of the
        ranges [begins[i], begins[i] + counts[i]), and how many streams hold each, as
        Context.across_values_windows_host gives them (atsc_stream_across_values_windows)"""
        return _across_values_result(
            lambda m: self._across_stream(_ACROSS_VALUES, others, begins, counts, stride, m, k, above), counts, stride, k)

    def across_extremes_windows(self, others, begins, counts, k, stride=1):
        """-> (records, off): the k largest and the k smallest of the samples that this stream (stream 0) and the streams
        `others` (stream 1 and on) hold at every `stride`-th position of the ranges [begins[i], begins[i] + counts[i]),
        and which streams hold them, as Context.across_extremes_windows_host gives them
        (atsc_stream_across_extremes_windows)"""
        return _across_extremes_result(
            lambda m: self._across_stream(_ACROSS_EXTREMES, others, begins, counts, stride, m, k), counts, stride, k)

    def across_moments_windows(self, others, begins, counts, stride=1):
        """-> (records, off): count, mean and m2 of the samples that this stream (stream 0) and the streams `others`
        (stream 1 and on) hold at every `stride`-th position of the ranges [begins[i], begins[i] + counts[i]), as
        Context.across_moments_windows_host gives them (atsc_stream_across_moments_windows)"""
        return _across_moments_result(
            lambda m: self._across_stream(_ACROSS_MOMENTS, others, begins, counts, stride, m), counts, stride)

    def extremes_windows(self, begins, counts, k):
        """-> array of window_extremes_dtype(k) of the windows [begins[i], begins[i] + counts[i]): their k largest and k
        smallest samples and where they are (atsc_stream_extremes_windows)"""
        return _query_stream(_EXTREMES, self, begins, counts, k)

    def values_windows(self, begins, counts, k, above=float("nan")):
        """-> array of window_values_dtype(k) of the windows [begins[i], begins[i] + counts[i]): their k smallest
        distinct values above `above` (NaN: all of them) and how often each occurs (atsc_stream_values_windows)"""
        return _query_stream(_VALUES, self, begins, counts, k, above)

    def quantile_windows(self, begins, counts, levels, method=capi.QUANTILE_LINEAR):
        """-> (n_windows, n_levels) float64 array of the windows' levels (atsc_stream_quantile_windows)"""
        return _query_stream(_QUANTILE, self, begins, counts, levels, method)

    def histogram_windows(self, begins, counts, edges, closed=capi.HIST_LEFT_CLOSED):
        """-> (n_windows, n_edges + 2) uint64 array of the windows' bin counts (atsc_stream_histogram_windows)"""
        return _query_stream(_HISTOGRAM, self, begins, counts, edges, closed)


def compress_data(ctx, vec, compressor=capi.AUTO, error=3, sample_level=0):
    """atsc/src/main.rs:130-165"""
    a, pa = _f64(vec)
    p = C.POINTER(C.c_uint8)()
    n = C.c_uint64()
    capi.check(capi.lib().atsc_compress_data(ctx._h, pa, len(a), int(compressor), int(error), int(sample_level),
                                             C.byref(p), C.byref(n)), ctx._h)
    return _take_bytes(p, n)


def decompress_data(ctx, bro):
    """atsc/src/main.rs:168-172"""
    b = np.frombuffer(bytes(bro), dtype=np.uint8)
    p = C.POINTER(C.c_double)()
    n = C.c_uint64()
    capi.check(capi.lib().atsc_decompress_data(ctx._h, b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b),
                                               C.byref(p), C.byref(n)), ctx._h)
    return _take_f64(p, n)


def decompress_data_window(ctx, bro, begin, count):
    """decompress_data(ctx, bro)[begin:begin + count]: atsc_bro_open, then atsc_decompress_window over the records"""
    b = np.frombuffer(bytes(bro), dtype=np.uint8)
    pb = b.ctypes.data_as(C.POINTER(C.c_uint8))
    capi.check(capi.lib().atsc_bro_open(pb, len(b), None, None))
    out = np.empty(max(int(count), 1), dtype=np.float64)
    on = C.c_uint64()
    # the records from the frame-count varint (offset 9) on, as atsc_decompress_data reads them
    r = b[9:]
    rc = capi.lib().atsc_decompress_window(ctx._h, r.ctypes.data_as(C.POINTER(C.c_uint8)), len(r), 1, int(begin), int(count),
                                           out.ctypes.data_as(C.POINTER(C.c_double)), int(count), C.byref(on))
    capi.check(rc, ctx._h)
    return out[: on.value]


def aggregate_data_windows(ctx, bro, begins, counts):
    """-> WINDOW_STATS array of windows of decompress_data(ctx, bro): atsc_bro_open, then atsc_aggregate_windows over
    the records"""
    return _query_image(_AGGREGATE, ctx, bro, begins, counts)


def moments_data_windows(ctx, bro, begins, counts):
    """-> WINDOW_MOMENTS array of windows of decompress_data(ctx, bro): atsc_bro_open, then atsc_moments_windows over
    the records"""
    return _query_image(_MOMENTS, ctx, bro, begins, counts)


def delta_data_windows(ctx, bro, begins, counts):
    """-> WINDOW_DELTA array of windows of decompress_data(ctx, bro): atsc_bro_open, then atsc_delta_windows over the
    records"""
    return _query_image(_DELTA, ctx, bro, begins, counts)


def runs_data_windows(ctx, bro, begins, counts, op, limit):
    """-> WINDOW_RUNS array of windows of decompress_data(ctx, bro) under the condition x OP limit: atsc_bro_open, then
    atsc_runs_windows over the records"""
    return _query_image(_RUNS, ctx, bro, begins, counts, op, limit)


def select_data_windows(ctx, bro, begins, counts, op, limit, cap=None):
    """-> (off, entries) of windows of decompress_data(ctx, bro) under the condition x OP limit, as
    Context.select_windows_host gives them: atsc_bro_open, then atsc_select_windows over the records"""
    n = len(np.atleast_1d(begins))
    return _select_result(lambda c: _query_image(_SELECT, ctx, bro, begins, counts, op, limit, c), n, cap)


def rolling_data_windows(ctx, bro, begins, counts, width, stride=1):
    """-> (records, off) of the window of `width` samples at every `stride`-th position of ranges of
    decompress_data(ctx, bro), as Context.rolling_windows_host gives them: atsc_bro_open, then atsc_rolling_windows over
    the records"""
    return _rolling_result(lambda m: _query_image(_ROLLING, ctx, bro, begins, counts, width, stride, m), counts, width, stride)


def rolling_delta_data_windows(ctx, bro, begins, counts, width, stride=1):
    """-> (records, off): the deltas' record of the window of `width` samples at every `stride`-th position of ranges of
    decompress_data(ctx, bro), as Context.rolling_delta_windows_host gives them: atsc_bro_open, then
    atsc_rolling_delta_windows over the records"""
    return _rolling_result(lambda m: _query_image(_ROLLING_DELTA, ctx, bro, begins, counts, width, stride, m), counts, width,
                           stride, WINDOW_DELTA)


def rolling_runs_data_windows(ctx, bro, begins, counts, width, op, limit, stride=1):
    """-> (records, off): the runs' record under the condition x OP limit of the window of `width` samples at every
    `stride`-th position of ranges of decompress_data(ctx, bro), as Context.rolling_runs_windows_host gives them:
    atsc_bro_open, then atsc_rolling_runs_windows over the records"""
    return _rolling_result(lambda m: _query_image(_ROLLING_RUNS, ctx, bro, begins, counts, width, stride, m, op, limit),
                           counts, width, stride, WINDOW_RUNS)


def rolling_moments_data_windows(ctx, bro, begins, counts, width, stride=1):
    """-> (records, off): the moments' record of the window of `width` samples at every `stride`-th position of ranges
    of decompress_data(ctx, bro), as Context.rolling_moments_windows_host gives them: atsc_bro_open, then
    atsc_rolling_moments_windows over the records"""
    return _rolling_result(lambda m: _query_image(_ROLLING_MOMENTS, ctx, bro, begins, counts, width, stride, m), counts, width,
                           stride, WINDOW_MOMENTS)


def rolling_quantile_data_windows(ctx, bro, begins, counts, width, levels, stride=1, method=capi.QUANTILE_LINEAR):
    """-> (rows, off): the levels of the window of `width` samples at every `stride`-th position of ranges of
    decompress_data(ctx, bro), as Context.rolling_quantile_windows_host gives them: atsc_bro_open, then
    atsc_rolling_quantile_windows over the records"""
    return _rolling_quantile_result(
        lambda m: _query_image(_ROLLING_QUANTILE, ctx, bro, begins, counts, width, stride, m, levels, method), counts, width,
        stride, levels)


def rolling_histogram_data_windows(ctx, bro, begins, counts, width, edges, stride=1, closed=capi.HIST_LEFT_CLOSED):
    """-> (rows, off): the value-bin counts of the window of `width` samples at every `stride`-th position of ranges of
    decompress_data(ctx, bro), as Context.rolling_histogram_windows_host gives them: atsc_bro_open, then
    atsc_rolling_histogram_windows over the records"""
    return _rolling_histogram_result(
        lambda m: _query_image(_ROLLING_HISTOGRAM, ctx, bro, begins, counts, width, stride, m, edges, closed), counts, width,
        stride, edges)


def rolling_pair_data_windows(ctx, bro_x, bro_y, begins, counts, width, stride=1):
    """-> (records, off): the pair moments' record of the window of `width` samples at every `stride`-th position of
    ranges of decompress_data(ctx, bro_x) (x) and decompress_data(ctx, bro_y) (y), as
    Context.rolling_pair_windows_host gives them: atsc_bro_open of each image, then atsc_rolling_pair_windows over the
    records of both"""
    bodies = []
    for bro in (bro_x, bro_y):
        b = np.frombuffer(bytes(bro), dtype=np.uint8)
        capi.check(capi.lib().atsc_bro_open(b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), None, None))
        bodies.append(b[9:].tobytes())  # the records from the frame-count varint on, as atsc_decompress_data reads them
    return ctx.rolling_pair_windows_host(bodies[0], bodies[1], begins, counts, width, stride, has_count=True)


def across_data_windows(ctx, bros, begins, counts, stride=1):
    """-> (records, off) over the streams decompress_data(ctx, bro) of every .bro image of the list `bros` at every
    `stride`-th position of the ranges, as Context.across_windows_host gives them: atsc_bro_open of each image, then
    atsc_across_windows over their records"""
    records = _across_images(bros)
    return _across_result(lambda m: _across_host(ctx, records, begins, counts, True, stride, m), counts, stride)


def pair_matrix_data_windows(ctx, bros, begins, counts):
    """-> (W, P) WINDOW_PAIR array: the pair moments of every pair of the BRO images of the list `bros` over the windows,
    as Context.pair_matrix_windows_host gives them: atsc_bro_open of each image, then atsc_pair_matrix_windows over their
    records"""
    return ctx.pair_matrix_windows_host(_across_images(bros), begins, counts, has_count=True)


def _across_images(bros):
    """-> the records of every .bro image of the list, each checked by atsc_bro_open"""
    images = [np.frombuffer(bytes(b), dtype=np.uint8) for b in bros]
    for b in images:
        capi.check(capi.lib().atsc_bro_open(b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), None, None))
    # the records from the frame-count varint (offset 9) on, as atsc_decompress_data reads them
    return [b[9:] for b in images]


def across_quantile_data_windows(ctx, bros, begins, counts, levels, stride=1, method=capi.QUANTILE_LINEAR):
    """-> (rows, off): the levels of the samples that the streams decompress_data(ctx, bro) of every .bro image of the
    list `bros` hold at every `stride`-th position of the ranges, as Context.across_quantile_windows_host gives them:
    atsc_bro_open of each image, then atsc_across_quantile_windows over their records"""
    records = _across_images(bros)
    return _across_quantile_result(
        lambda m: _across_host(ctx, records, begins, counts, True, stride, m, levels, method, q=_ACROSS_QUANTILE), counts, stride,
        levels)


def across_histogram_data_windows(ctx, bros, begins, counts, edges, stride=1, closed=capi.HIST_LEFT_CLOSED):
    """-> (rows, off): how many of the streams decompress_data(ctx, bro) of every .bro image of the list `bros` hold a
    sample in each value bin at every `stride`-th position of the ranges, as Context.across_histogram_windows_host gives
    them: atsc_bro_open of each image, then atsc_across_histogram_windows over their records"""
    records = _across_images(bros)
    return _across_histogram_result(
        lambda m: _across_host(ctx, records, begins, counts, True, stride, m, edges, closed, q=_ACROSS_HISTOGRAM), counts, stride,
        edges)


def across_values_data_windows(ctx, bros, begins, counts, k, stride=1, above=float("nan")):
    """-> (records, off): which values the streams decompress_data(ctx, bro) of every .bro image of the list `bros` hold
    at every `stride`-th position of the ranges, and how many streams hold each, as Context.across_values_windows_host
    gives them: atsc_bro_open of each image, then atsc_across_values_windows over their records"""
    records = _across_images(bros)
    return _across_values_result(
        lambda m: _across_host(ctx, records, begins, counts, True, stride, m, k, above, q=_ACROSS_VALUES), counts, stride, k)


def across_extremes_data_windows(ctx, bros, begins, counts, k, stride=1):
    """-> (records, off): the k largest and the k smallest of the samples that the streams decompress_data(ctx, bro) of
    every .bro image of the list `bros` hold at every `stride`-th position of the ranges, and which streams hold them, as
    Context.across_extremes_windows_host gives them: atsc_bro_open of each image, then atsc_across_extremes_windows over
    their records"""
    records = _across_images(bros)
    return _across_extremes_result(
        lambda m: _across_host(ctx, records, begins, counts, True, stride, m, k, q=_ACROSS_EXTREMES), counts, stride, k)


def across_moments_data_windows(ctx, bros, begins, counts, stride=1):
    """-> (records, off): count, mean and m2 of the samples that the streams decompress_data(ctx, bro) of every .bro
    image of the list `bros` hold at every `stride`-th position of the ranges, as Context.across_moments_windows_host
    gives them: atsc_bro_open of each image, then atsc_across_moments_windows over their records"""
    records = _across_images(bros)
    return _across_moments_result(
        lambda m: _across_host(ctx, records, begins, counts, True, stride, m, q=_ACROSS_MOMENTS), counts, stride)


def extremes_data_windows(ctx, bro, begins, counts, k):
    """-> array of window_extremes_dtype(k) of windows of decompress_data(ctx, bro): their k largest and k smallest
    samples and where they are: atsc_bro_open, then atsc_extremes_windows over the records"""
    return _query_image(_EXTREMES, ctx, bro, begins, counts, k)


def values_data_windows(ctx, bro, begins, counts, k, above=float("nan")):
    """-> array of window_values_dtype(k) of windows of decompress_data(ctx, bro): their k smallest distinct values
    above `above` (NaN: all of them) and how often each occurs: atsc_bro_open, then atsc_values_windows over the
    records"""
    return _query_image(_VALUES, ctx, bro, begins, counts, k, above)


def quantile_data_windows(ctx, bro, begins, counts, levels, method=capi.QUANTILE_LINEAR):
    """-> (n_windows, n_levels) float64 array: levels of windows of decompress_data(ctx, bro): atsc_bro_open, then
    atsc_quantile_windows over the records"""
    return _query_image(_QUANTILE, ctx, bro, begins, counts, levels, method)


def histogram_data_windows(ctx, bro, begins, counts, edges, closed=capi.HIST_LEFT_CLOSED):
    """-> (n_windows, n_edges + 2) uint64 array: bin counts of windows of decompress_data(ctx, bro): atsc_bro_open, then
    atsc_histogram_windows over the records"""
    return _query_image(_HISTOGRAM, ctx, bro, begins, counts, edges, closed)


def wbro_from_bytes(data):
    b = np.frombuffer(bytes(data), dtype=np.uint8)
    p = C.POINTER(C.c_double)()
    n = C.c_uint64()
    capi.check(capi.lib().atsc_wbro_from_bytes(b.ctypes.data_as(C.POINTER(C.c_uint8)), len(b), C.byref(p), C.byref(n)))
    return _take_f64(p, n)


def wbro_to_bytes(samples):
    a, pa = _f64(samples)
    p = C.POINTER(C.c_uint8)()
    n = C.c_uint64()
    capi.check(capi.lib().atsc_wbro_to_bytes(pa, len(a), C.byref(p), C.byref(n)))
    return _take_bytes(p, n)


def wbro_read(path):
    p = C.POINTER(C.c_double)()
    n = C.c_uint64()
    capi.check(capi.lib().atsc_wbro_read(str(path).encode(), C.byref(p), C.byref(n)))
    return _take_f64(p, n)


def wbro_write(path, samples):
    a, pa = _f64(samples)
    capi.check(capi.lib().atsc_wbro_write(str(path).encode(), pa, len(a)))


def bro_read_file(path):
    """-> bytes, or None when the file does not start with "BRRO" (bro_reader.rs:31-38)"""
    p = C.POINTER(C.c_uint8)()
    n = C.c_uint64()
    capi.check(capi.lib().atsc_bro_read_file(str(path).encode(), C.byref(p), C.byref(n)))
    if not p:
        return None
    return _take_bytes(p, n)


def csv_read(path, header=True, time_field="time", value_field="value"):
    p = C.POINTER(C.c_double)()
    n = C.c_uint64()
    capi.check(capi.lib().atsc_csv_read(str(path).encode(), int(bool(header)), time_field.encode(),
                                        value_field.encode(), C.byref(p), C.byref(n)))
    return _take_f64(p, n)
