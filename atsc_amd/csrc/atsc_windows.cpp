// atsc_windows.cpp -- the window queries of libatsc_hip.so: samples, aggregates, moments, deltas, runs, extremes, value counts, quantiles, histograms,
// rolling windows, rolling deltas, rolling runs, rolling quantiles, rolling histograms and selected samples of ranges of the decoded stream without decoding the rest, the pair moments of the same ranges of two streams and of every pair of up to 64,
// and count, min, max, sum, quantiles, extremes, moments, histograms and value counts across up to 64 streams at every position of such ranges.  Each query has a device call (host tables, one upload, launches on the caller's
// stream) and a host call (the touched records only: walk, range plan, upload, device call, result back).  What the
// queries have in common comes first: the record walk, the per-plan resources, the upload, the decode of pieces into
// scratch, the argument checks and the host call.  Last, the same queries on a stream under construction.  Context, plans
// and the pool are atsc_host.cpp's (atsc_host_private.h); nothing in atsc_host.cpp or atsc_stream.cpp calls into this file.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <numeric>
#include <type_traits>

#include "atsc_host_private.h"
#include "atsc_moment_rule.h"

namespace atsc {
// (weak: the sanitizer build of the host sources, tests/asan, links without the window kernels and never decodes a window)
__attribute__((weak)) hipError_t launch_decompress_window(const DevDFrame *frames, const DevWTask *tasks, int cls,
                                                          uint32_t count, uint32_t lds, const DevPlan *plans,
                                                          const float2 *twpool, const uint8_t *body, double *out,
                                                          int *status, hipStream_t s);
__attribute__((weak)) hipError_t launch_window_gather(const DevWGather *g, uint32_t n, uint32_t max_len,
                                                      const double *scratch, double *out, hipStream_t s);
// the windowed aggregates' reduce kernels (atsc_aggregate.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_agg_tiles(const DevAggTile *tasks, uint32_t n, const double *scratch,
                                                  DevAggPart *part, double *fl, hipStream_t s);
__attribute__((weak)) hipError_t launch_agg_combine(const DevAggComb *tasks, uint32_t n, DevAggPart *part,
                                                    const double *fl, void *stats, hipStream_t s);
// the windowed quantiles' selection kernels (atsc_quantile.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_qnt_short(const DevQTask *tasks, uint32_t n, const double *scratch, const double *q,
                                                  uint32_t n_q, int method, double *out, hipStream_t s);
__attribute__((weak)) hipError_t launch_qnt_medium(const DevQTask *tasks, uint32_t n, uint32_t P, const double *scratch,
                                                   const double *q, uint32_t n_q, int method, double *out, hipStream_t s);
__attribute__((weak)) hipError_t launch_qnt_hist(const DevQChunk *chunks, uint32_t n, const double *scratch,
                                                 const DevQState *st, uint32_t *hist, uint32_t rows, uint32_t pass,
                                                 hipStream_t s);
__attribute__((weak)) hipError_t launch_qnt_pick(const DevQTask *tasks, uint32_t n, DevQState *st, uint32_t *hist,
                                                 uint32_t rows, uint32_t pass, const double *q, uint32_t n_q, int method,
                                                 double *out, hipStream_t s);
// the windowed histograms' counting kernels (atsc_histogram.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_hst_short(const DevHistTask *tasks, uint32_t n, const double *scratch,
                                                  const double *edges, uint32_t n_edges, int closed, uint64_t *out,
                                                  hipStream_t s);
__attribute__((weak)) hipError_t launch_hst_chunk(const DevHistTask *tasks, uint32_t n, const double *scratch,
                                                  const double *edges, uint32_t n_edges, int closed, uint64_t *out,
                                                  hipStream_t s);
// the windowed moments' reduce kernels (atsc_moments.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_mom_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch,
                                                  DevMomPart *part, hipStream_t s);
__attribute__((weak)) hipError_t launch_mom_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part,
                                                    const uint64_t *begin, void *out, hipStream_t s);
// the windowed deltas' reduce kernels (atsc_delta.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_dlt_tiles(const DevDltTile *tasks, uint32_t n, const double *scratch,
                                                  const double *carry, DevDltPart *part, hipStream_t s);
__attribute__((weak)) hipError_t launch_dlt_combine(const DevAggComb *tasks, uint32_t n, DevDltPart *part, void *out,
                                                    hipStream_t s);
// the windowed runs' reduce kernels (atsc_runs.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_run_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, int op,
                                                  double limit, DevRunPart *part, hipStream_t s);
__attribute__((weak)) hipError_t launch_run_combine(const DevAggComb *tasks, uint32_t n, DevRunPart *part,
                                                    const uint64_t *begin, void *out, hipStream_t s);
// the windowed extremes' selection kernels (atsc_extremes.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_ext_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, uint32_t k,
                                                  void *part, hipStream_t s);
__attribute__((weak)) hipError_t launch_ext_combine(const DevAggComb *tasks, uint32_t n, uint32_t k, void *part,
                                                    const uint64_t *begin, void *out, hipStream_t s);
// the windowed value counts' kernels (atsc_values.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_val_tiles(const DevAggTile *tasks, uint32_t n, const double *scratch, uint32_t k,
                                                  uint64_t above, void *part, hipStream_t s);
__attribute__((weak)) hipError_t launch_val_combine(const DevAggComb *tasks, uint32_t n, uint32_t k, void *part, void *out,
                                                    hipStream_t s);
// the windowed select's count, scan and write kernels (atsc_select.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_sel_count(const DevSelTask *tasks, uint32_t n, const double *scratch, int op,
                                                  double limit, uint64_t *cnt, hipStream_t s);
__attribute__((weak)) hipError_t launch_sel_scan(uint64_t *cnt, uint64_t n, uint64_t *sums, hipStream_t s);
__attribute__((weak)) hipError_t launch_sel_offsets(const uint64_t *pre, const uint32_t *first, uint64_t n, uint64_t *off,
                                                    hipStream_t s);
__attribute__((weak)) hipError_t launch_sel_write(const DevSelTask *tasks, uint32_t n, const double *scratch, int op,
                                                  double limit, const uint64_t *pre, uint64_t cap, void *entries,
                                                  hipStream_t s);
// the windowed pair moments' reduce kernels (atsc_pair.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_pair_tiles(const DevPosTile *tasks, uint32_t n, const double *sx, const double *sy,
                                                   DevMomPart *part, hipStream_t s);
__attribute__((weak)) hipError_t launch_pair_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part, void *out,
                                                     hipStream_t s);
// the windowed pair matrix' reduce kernels (atsc_pair_matrix.hip; weak for the same reason); reg: where each stream's
// region begins in the scratch; part_n: the nodes of one pair
__attribute__((weak)) hipError_t launch_pmx_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                                  uint32_t n_streams, DevMomPart *part, uint64_t part_n, hipStream_t s);
__attribute__((weak)) hipError_t launch_pmx_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part, uint64_t part_n,
                                                    uint32_t n_streams, void *out, hipStream_t s);
// the windowed rolling's pyramid and position kernels (atsc_rolling.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_roll_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc,
                                                     uint32_t lmax, hipStream_t s);
__attribute__((weak)) hipError_t launch_roll_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax,
                                                   hipStream_t s);
__attribute__((weak)) hipError_t launch_roll_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                       const void *pyr, const DevRollPiece *pc, uint64_t w, uint64_t stride,
                                                       void *out, hipStream_t s);
// the windowed rolling deltas' pyramid and position kernels (atsc_rolling_delta.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_rdl_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc,
                                                    uint32_t lmax, hipStream_t s);
__attribute__((weak)) hipError_t launch_rdl_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax,
                                                  hipStream_t s);
__attribute__((weak)) hipError_t launch_rdl_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                      const void *pyr, const DevRollPiece *pc, uint64_t w, uint64_t stride,
                                                      void *out, hipStream_t s);
// the windowed rolling moments' pyramid and position kernels (atsc_rolling_moments.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_rmo_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc,
                                                    uint32_t lmax, hipStream_t s);
__attribute__((weak)) hipError_t launch_rmo_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax,
                                                  hipStream_t s);
__attribute__((weak)) hipError_t launch_rmo_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                      const void *pyr, const DevRollPiece *pc, uint64_t w, uint64_t stride,
                                                      void *out, hipStream_t s);
// the windowed rolling pair moments' pyramid and position kernels (atsc_rolling_pair.hip; weak for the same reason); the
// levels above 11 are launch_rmo_upper's
__attribute__((weak)) hipError_t launch_rpa_pyramid(const double *sx, const double *sy, uint32_t n_tiles, void *pyr,
                                                    const DevRollPiece *pc, uint32_t lmax, hipStream_t s);
__attribute__((weak)) hipError_t launch_rpa_positions(const DevRollTask *tasks, uint32_t n, const double *sx, const double *sy,
                                                      const void *pyr, const DevRollPiece *pc, uint64_t w, uint64_t stride,
                                                      void *out, hipStream_t s);
// the windowed rolling runs' pyramid and position kernels (atsc_rolling_runs.hip; weak for the same reason); op, limit: the
// call's condition
__attribute__((weak)) hipError_t launch_rru_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc,
                                                    uint32_t lmax, int op, double limit, hipStream_t s);
__attribute__((weak)) hipError_t launch_rru_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax,
                                                  hipStream_t s);
__attribute__((weak)) hipError_t launch_rru_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                      const void *pyr, const DevRollPiece *pc, uint64_t w, uint64_t stride,
                                                      int op, double limit, void *out, hipStream_t s);
// the windowed rolling quantiles' span kernel (atsc_rolling_quantile.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_rq_span(const DevRollTask *tasks, uint32_t n, uint32_t P, uint64_t B,
                                                const double *scratch, uint64_t a0, uint32_t w, uint64_t stride,
                                                const double *q, uint32_t n_q, int method, double *out, hipStream_t s);
// the windowed rolling histograms' sliding kernel (atsc_rolling_histogram.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_rh_slide(const DevRollTask *tasks, uint32_t n, const double *scratch, uint64_t a0,
                                                 uint32_t w, uint64_t stride, const double *edges, uint32_t n_edges,
                                                 int closed, uint64_t *out, hipStream_t s);
// the windowed across' position kernel (atsc_across.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_across_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                         const uint64_t *reg, uint32_t n_streams, uint64_t a0,
                                                         uint64_t stride, void *out, hipStream_t s);
// the windowed across quantiles' position kernel (atsc_across_quantile.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_across_quantile_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                                  const uint64_t *reg, uint32_t n_streams, uint64_t a0,
                                                                  uint64_t stride, const double *q, uint32_t n_q, int method,
                                                                  double *out, hipStream_t s);
// the windowed across extremes' position kernel (atsc_across_extremes.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_across_extremes_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                                  const uint64_t *reg, uint32_t n_streams, uint64_t a0,
                                                                  uint64_t stride, uint32_t k, void *out, hipStream_t s);
// the windowed across moments' position kernel (atsc_across_moments.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_across_moments_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                                 const uint64_t *reg, uint32_t n_streams, uint64_t a0,
                                                                 uint64_t stride, void *out, hipStream_t s);
// the windowed across histograms' position kernel (atsc_across_histogram.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_across_histogram_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                                   const uint64_t *reg, uint32_t n_streams, uint64_t a0,
                                                                   uint64_t stride, const double *edges, uint32_t n_edges,
                                                                   int closed, uint64_t *out, hipStream_t s);
// the windowed across value counts' position kernel (atsc_across_values.hip; weak for the same reason)
__attribute__((weak)) hipError_t launch_across_values_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                                                const uint64_t *reg, uint32_t n_streams, uint64_t a0,
                                                                uint64_t stride, uint32_t k, uint64_t above, void *out,
                                                                hipStream_t s);
}  // namespace atsc

using namespace atsc;

// "<call>: <what>"
static int fail_in(atsc_ctx *ctx, int rc, const char *call, const char *what, hipError_t e = hipSuccess)
{
    return fail(ctx, rc, (std::string(call) + ": " + what).c_str(), e);
}

// ------------------------------------------------------------------------------------------
// the record walk of a window, and where a window lies in a stream or a plan
// ------------------------------------------------------------------------------------------
// The record walk of a window read over untrusted bytes: from `pos`, at most max_frames records, with the header checks
// of atsc_bro_scan, up to the record that holds sample begin + count - 1 (count == 0: the record that holds `begin`).
// A Noop record counts the samples it stores (noop.rs:79-83), as the decoder does.  decode: the frame-length checks of
// dplan_parse as well (a frame the decoders cannot take).  ATSC_E_INVALID when the stream ends in front of the window's end.
struct WindowWalk {
    uint64_t byte_begin = 0, byte_end = 0, frame_begin = 0, frame_end = 0, sample_begin = 0;
};
static int window_walk(const uint8_t *b, uint64_t len, uint64_t pos, uint64_t max_frames, uint64_t begin, uint64_t count,
                       bool decode, WindowWalk &w)
{
    if (begin + count < begin) return ATSC_E_INVALID;
    const uint64_t end = begin + count;
    uint64_t s_off = 0, f = 0;
    bool found = false;
    for (; max_frames == ~0ull ? pos < len : f < max_frames; ++f) {
        HostRecord hr;
        if (!host_next_record(b, len, pos, hr)) return ATSC_E_FORMAT;
        if (hr.tag > 6 || hr.tag == ATSC_AUTO) return ATSC_E_FORMAT;
        uint64_t n = hr.sample_count;
        if (hr.tag == ATSC_NOOP) {
            uint64_t q = hr.payload_off + 1, cnt = 0;
            if (hr.payload_len < 2 || !host_varint(b, hr.payload_off + hr.payload_len, q, cnt) || cnt > hr.payload_len)
                return ATSC_E_FORMAT;
            n = cnt;
        }
        if (decode && n == 0) return ATSC_E_FORMAT;
        if (decode && n > MAX_FRAME) return ATSC_E_UNSUPPORTED;
        if (s_off + n < s_off) return ATSC_E_FORMAT;
        if (!found && s_off + n > begin) {
            found = true;
            w.frame_begin = f;
            w.byte_begin = hr.start;
            w.sample_begin = s_off;
            if (count == 0) {
                w.frame_end = f;
                w.byte_end = hr.start;
                return ATSC_OK;
            }
        }
        s_off += n;
        if (found && s_off >= end) {
            w.frame_end = f + 1;
            w.byte_end = pos;
            return ATSC_OK;
        }
    }
    if (count == 0 && begin == s_off) {  // the empty window at the stream's end
        w.frame_begin = w.frame_end = f;
        w.byte_begin = w.byte_end = pos;
        w.sample_begin = s_off;
        return ATSC_OK;
    }
    return ATSC_E_INVALID;
}

extern "C" int atsc_bro_find_window(const uint8_t *bro, uint64_t len, uint64_t begin, uint64_t count,
                                    uint64_t *byte_begin, uint64_t *byte_end, uint64_t *frame_begin, uint64_t *frame_end,
                                    uint64_t *sample_begin)
{
    ATSC_API_BEGIN
    if (!bro) return ATSC_E_INVALID;
    uint64_t pos = 0, nf = 0;
    int rc = atsc_bro_open(bro, len, &pos, &nf);
    if (rc) return rc;
    if (nf > len / 4) return ATSC_E_FORMAT;
    WindowWalk w;
    rc = window_walk(bro, len, pos, nf, begin, count, false, w);
    if (rc) return rc;
    if (byte_begin) *byte_begin = w.byte_begin;
    if (byte_end) *byte_end = w.byte_end;
    if (frame_begin) *frame_begin = w.frame_begin;
    if (frame_end) *frame_end = w.frame_end;
    if (sample_begin) *sample_begin = w.sample_begin;
    return ATSC_OK;
    ATSC_API_END
}

extern "C" int atsc_dplan_find_frames(const atsc_dplan *dp, uint64_t begin, uint64_t count, uint64_t *frame_begin,
                                      uint64_t *frame_end)
{
    if (!dp || !frame_begin || !frame_end) return ATSC_E_INVALID;
    if (begin > dp->n_samples || count > dp->n_samples - begin) return ATSC_E_INVALID;
    const auto &F = dp->h_frames;
    auto by_off = [](uint64_t v, const DevDFrame &d) { return v < d.out_off; };
    // the frame holding `begin` (every frame holds at least one sample), or n_frames at the stream's end
    const uint64_t fb = (uint64_t)(std::upper_bound(F.begin(), F.end(), begin, by_off) - F.begin()) - 1;
    *frame_begin = begin == dp->n_samples ? F.size() : fb;
    *frame_end = count == 0 ? *frame_begin
                            : (uint64_t)(std::upper_bound(F.begin(), F.end(), begin + count - 1, by_off) - F.begin());
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// what a device call holds on its plan, and its one upload
// ------------------------------------------------------------------------------------------
static size_t upload_align(size_t v) { return (v + 255) & ~(size_t)255; }

// The layout of a device call's tables: each at a multiple of 256 bytes, first the ones that go up in the call's one
// copy (add), behind them the ones that only the kernels write and read (device_only).  Both hand back the table's
// offset.  The tables' memory must stay where it is until stage() has copied it.
struct Upload {
    struct Table {
        size_t off;
        const void *src;
        size_t bytes;
    };
    std::vector<Table> tables;
    size_t up_bytes = 0, bytes = 0;
    Upload() { tables.reserve(16); }
    size_t add(const void *src, size_t n)
    {
        const size_t off = bytes;
        tables.push_back(Table{off, src, n});
        up_bytes = bytes = upload_align(bytes + n);
        return off;
    }
    template <class T>
    size_t add(const std::vector<T> &v)
    {
        return add(v.data(), v.size() * sizeof(T));
    }
    size_t device_only(size_t n)
    {
        const size_t off = bytes;
        bytes = upload_align(bytes + n);
        return off;
    }
    void stage(unsigned char *h) const
    {
        for (const Table &t : tables)
            if (t.bytes) memcpy(h + t.off, t.src, t.bytes);
    }
};

// ------------------------------------------------------------------------------------------
// decode tasks: frames, or parts of frames, decoded to where a query wants them
// ------------------------------------------------------------------------------------------
using Span = std::pair<uint64_t, uint64_t>;

// The interval merge: `last` takes in x, which begins at or behind last's begin, when they overlap or touch.
static bool absorb_span(Span &last, const Span &x)
{
    if (x.first > last.second) return false;
    last.second = std::max(last.second, x.second);
    return true;
}
// sorts the intervals and merges them in place
static void merge_spans(std::vector<Span> &v)
{
    if (!std::is_sorted(v.begin(), v.end())) std::sort(v.begin(), v.end());
    size_t m = 0;
    for (const Span &x : v)
        if (!m || !absorb_span(v[m - 1], x)) v[m++] = x;
    v.resize(m);
}

// Cuts the covering intervals (ascending, disjoint, in samples) into the pieces a call decodes one after the other:
// ascending disjoint spans in units of `unit` samples, a covered range's ends rounded outwards to whole units.  Covered
// ranges closer than `gap` units share a run, so that scattered windows do not each cost a piece of launches; a run is
// cut every `len` units.  Hands back the longest piece, in units.
static uint64_t cut_pieces(const std::vector<Span> &cov, uint64_t unit, uint64_t len, uint64_t gap, std::vector<Span> &pcs)
{
    uint64_t longest = 0;
    for (size_t a = 0; a < cov.size();) {
        const uint64_t k0 = cov[a].first / unit;
        uint64_t k1 = (cov[a].second + unit - 1) / unit;
        size_t z = a + 1;
        while (z < cov.size() && cov[z].first / unit < k1 + gap) k1 = std::max(k1, (cov[z++].second + unit - 1) / unit);
        for (uint64_t k = k0; k < k1; k += len) pcs.emplace_back(k, std::min(k1, k + len));
        longest = std::max(longest, std::min(len, k1 - k0));
        a = z;
    }
    return longest;
}

// A task and the piece it belongs to, as a call makes them in its own order (by window, by range).
template <class T>
struct Placed {
    uint32_t piece;
    T t;
};
// The placed tasks of P pieces, sorted by piece (stably: a piece's keep their order), into `tasks`: piece p's are
// tasks[at[p] .. at[p + 1]), one launch.  Frees the placed list.
template <class T>
static void group_tasks(std::vector<Placed<T>> &tk, size_t P, std::vector<T> &tasks, std::vector<size_t> &at)
{
    auto piece_order = [](const Placed<T> &x, const Placed<T> &y) { return x.piece < y.piece; };
    if (P > 1 && !std::is_sorted(tk.begin(), tk.end(), piece_order)) std::stable_sort(tk.begin(), tk.end(), piece_order);
    tasks.reserve(tk.size());
    at.assign(P + 1, 0);
    for (const Placed<T> &x : tk) { tasks.push_back(x.t); ++at[x.piece + 1]; }
    for (size_t p = 0; p < P; ++p) at[p + 1] += at[p];
    std::vector<Placed<T>>().swap(tk);
}

// Reserves the tables and the scratch of a device call on R, stages the upload and enqueues its one copy; the tables'
// device copy is R.d.  scr_n: the scratch's samples.  The caller has waited for R's previous call (R.wait()).
static int stage_upload(atsc_ctx *ctx, QueryRes &R, const Upload &up, uint64_t scr_n, hipStream_t s)
{
    HIPCHK(ctx, R.reserve(ctx, up.up_bytes, up.bytes, scr_n));
    unsigned char *d = R.d;
    up.stage(R.h);
    HIPCHK(ctx, hipMemcpyAsync(d, R.h, up.up_bytes, hipMemcpyHostToDevice, s));
    return ATSC_OK;
}

// the decode tasks of all pieces of one call, and their place in the call's upload
struct DecodeTasks {
    std::vector<DevWTask> small[CLASS_LARGE];
    std::vector<DevDFrame> big;
    std::vector<DevWGather> gat;
    std::vector<uint32_t> ids;  // 0 .. max_big - 1: every piece's large sub-plan is launched in the order of its frames
    uint32_t max_big = 0, spills_used = 0;
    size_t off_small[CLASS_LARGE] = {}, off_big = 0, off_ids = 0, off_gat = 0;
    // per class the pieces' task lists, the large sub-plans, ids 0.., copies
    void place(Upload &U)
    {
        for (int c = 0; c < CLASS_LARGE; ++c) off_small[c] = U.add(small[c]);
        off_big = U.add(big);
        ids.resize(max_big);
        std::iota(ids.begin(), ids.end(), 0u);
        off_ids = U.add(ids);
        off_gat = U.add(gat);
    }
};
// one piece's run of them
struct PieceDecode {
    size_t small_at[CLASS_LARGE], big_at, gat_at;
    uint32_t small_n[CLASS_LARGE], big_n, gat_n, max_len;
};

// the messages of a failed launch, by caller: the query's word in parentheses behind the kernel's name
struct DecodeCaller {
    const char *small, *large, *gather;
};
#define DECODE_CALLER(word) \
    { "launch k_decompress (" word ")", "launch k_decompress_large (" word ")", "launch k_window_gather (" word ")" }
static const DecodeCaller BY_AGGREGATE = DECODE_CALLER("aggregate"), BY_QUANTILE = DECODE_CALLER("quantile"),
                          BY_HISTOGRAM = DECODE_CALLER("histogram"), BY_MOMENTS = DECODE_CALLER("moments"),
                          BY_DELTA = DECODE_CALLER("delta"), BY_RUNS = DECODE_CALLER("runs"),
                          BY_EXTREMES = DECODE_CALLER("extremes"), BY_SELECT = DECODE_CALLER("select"),
                          BY_PAIR = DECODE_CALLER("pair"), BY_PAIR_MATRIX = DECODE_CALLER("pair matrix"),
                          BY_VALUES = DECODE_CALLER("values"),
                          BY_ROLLING = DECODE_CALLER("rolling"), BY_ROLLING_DELTA = DECODE_CALLER("rolling delta"),
                          BY_ROLLING_MOMENTS = DECODE_CALLER("rolling moments"), BY_ROLLING_PAIR = DECODE_CALLER("rolling pair"),
                          BY_ROLLING_RUNS = DECODE_CALLER("rolling runs"),
                          BY_ROLLING_QUANTILE = DECODE_CALLER("rolling quantile"),
                          BY_ROLLING_HISTOGRAM = DECODE_CALLER("rolling histogram"), BY_ACROSS = DECODE_CALLER("across"),
                          BY_ACROSS_QUANTILE = DECODE_CALLER("across quantile"),
                          BY_ACROSS_EXTREMES = DECODE_CALLER("across extremes"),
                          BY_ACROSS_MOMENTS = DECODE_CALLER("across moments"),
                          BY_ACROSS_HISTOGRAM = DECODE_CALLER("across histogram"),
                          BY_ACROSS_VALUES = DECODE_CALLER("across values");
#undef DECODE_CALLER
// (the window decode's gather message carries no word)
static const DecodeCaller BY_WINDOW = {"launch k_decompress (window)", "launch k_decompress_large (window)",
                                       "launch k_window_gather"};

// Enqueues one piece's decode (d: the device copy of the upload).  out: the base the tasks' destinations count from;
// the copies go from gat_src to gat_dst.
static int launch_piece_decode(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, const unsigned char *d,
                               const DecodeTasks &D, const PieceDecode &pt, double *out, const double *gat_src,
                               double *gat_dst, hipStream_t s, const DecodeCaller &who)
{
    for (int c = 0; c < CLASS_LARGE; ++c) {
        if (!pt.small_n[c]) continue;
        LAUNCHCHK(ctx, who.small,
                  launch_decompress_window(dp->d_frames, (const DevWTask *)(d + D.off_small[c]) + pt.small_at[c], c, pt.small_n[c],
                                           dp->class_lds[c], dp->tabs.d_plans, dp->tabs.d_tw, d_body, out, dp->d_status, s));
    }
    if (pt.big_n)
        LAUNCHCHK(ctx, who.large,
                  launch_decompress_large(
                      pt.big_n, (const DevDFrame *)(d + D.off_big) + pt.big_at, (const uint32_t *)(d + D.off_ids),
                      dp->tabs.d_plans, dp->tabs.d_tw, d_body, out, dp->d_status, dp->d_ws, dp->ws_stride, dp->ws_slots,
                      dp->large_tiled ? 1 : 0, large_sparse() ? 1 : 0, s, dp->large_pre.tiles1 ? &dp->large_pre : nullptr,
                      // the (tile, frame) split of the sparse inverse runs for launches of up to LARGE_SPLIT_MAX frames: a
                      // window launch of fewer frames than its plan's full decode takes the full decode's side of that line
                      dp->large_choice_count <= LARGE_SPLIT_MAX ? dp->large_sp_tiles : 0));
    if (pt.gat_n)
        LAUNCHCHK(ctx, who.gather,
                  launch_window_gather((const DevWGather *)(d + D.off_gat) + pt.gat_at, pt.gat_n, pt.max_len, gat_src, gat_dst, s));
    return ATSC_OK;
}

// What every device call checks of its result pointer and its windows; `call` names the caller in the message.
// max_windows: the most windows the call's tasks can name (~0ull: no limit).  A call over several plans checks each:
// begin counts from sample org0 of the stream, and the plan's first sample is sample org of it.
static int check_windows(atsc_ctx *ctx, const char *call, const atsc_dplan *dp, const void *d_res, const char *res_name,
                         uint64_t n_windows, const uint64_t *begin, const uint64_t *count, uint64_t max_windows,
                         uint64_t org0 = 0, uint64_t org = 0)
{
    if ((uintptr_t)d_res & 7u) return fail_in(ctx, ATSC_E_INVALID, call, (std::string(res_name) + " is not 8-byte aligned").c_str());
    const uint64_t ns = dp->n_samples;
    for (uint64_t i = 0; i < n_windows; ++i) {
        const uint64_t a = org0 + begin[i];
        if (a < begin[i] || a < org || a - org > ns || count[i] > ns - (a - org))
            return fail_in(ctx, ATSC_E_INVALID, call, "window beyond the stream");
    }
    if (n_windows > max_windows) return fail_in(ctx, ATSC_E_INVALID, call, "more than 2^32 - 2 windows");
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// the host call of a query: the touched records only
// ------------------------------------------------------------------------------------------
// Walks the headers from the first non-empty window's first record to the record that holds the last window's end,
// plans those records only and uploads only their bytes; the result comes back once the payloads proved well-formed (a
// malformed one leaves `out` untouched).  A query over several streams (n_in > 1, at most MAX_INPUTS) does the walk, the
// range plan and the upload for each body, over the same windows; every body's status word is read before anything is copied out.
// `call` names the caller in the messages.  The caller's two steps:
//   located(any)  after the walk, which is what rejects a window beyond the stream: the caller's own checks, and its
//                 result when every window is empty (any == false: the call ends there);
//   enqueue(in, begin2, d_res, stream)  its device call on the range plans in[0 .. n_in): in[k].org is the stream index
//                 of plan k's first sample; begin2: the windows' begins counted from in[0].org.
// A result whose size depends on the data comes back in two copies: its first head_bytes, and once those are on the
// host the bytes from there up to used(out) (head_bytes == out_bytes: one copy, and used is not called).
// trace: the ATSC_TRACE_HOST line of the upload.
struct HostBody {
    const uint8_t *body;
    uint64_t len;
    int has_count;
};
// one plan of a device call with its record bytes on the device; org: the stream index of the plan's first sample
struct QueryInput {
    const atsc_dplan *dp;
    const uint8_t *d_body;
    uint64_t org;
};
static const int MAX_INPUTS = ATSC_ACROSS_MAX_STREAMS;  // the most streams a query reads (the across; the pair moments: 2)

template <class Located, class Enqueue, class Used>
static int window_host_call(atsc_ctx *ctx, const char *call, const HostBody *hb, int n_in, uint64_t n_windows,
                            const uint64_t *begin, const uint64_t *count, void *out, size_t out_bytes, size_t head_bytes,
                            bool trace, Located located, Enqueue enqueue, Used used)
{
    uint64_t pos[MAX_INPUTS] = {}, max_frames[MAX_INPUTS];
    for (int k = 0; k < n_in; ++k) {
        max_frames[k] = ~0ull;
        if (!hb[k].has_count) continue;
        if (!host_varint(hb[k].body, hb[k].len, pos[k], max_frames[k])) return fail_in(ctx, ATSC_E_FORMAT, call, "frame count");
        if (max_frames[k] > hb[k].len / 4) return fail_in(ctx, ATSC_E_FORMAT, call, "frame count exceeds the bytes present");
    }
    uint64_t B = ~0ull, E = 0;
    for (uint64_t i = 0; i < n_windows; ++i) {
        if (begin[i] + count[i] < begin[i]) return fail_in(ctx, ATSC_E_INVALID, call, "window beyond the stream");
        E = std::max(E, begin[i] + count[i]);
        if (count[i]) B = std::min(B, begin[i]);
    }
    const bool any = B != ~0ull;
    if (!any) B = E;  // only empty windows: the walk checks that each begins inside the stream
    WindowWalk w[MAX_INPUTS];
    int rc = ATSC_OK;
    for (int k = 0; k < n_in; ++k) {
        rc = window_walk(hb[k].body, hb[k].len, pos[k], max_frames[k], B, E - B, true, w[k]);
        if (rc) return fail_in(ctx, rc, call, rc == ATSC_E_INVALID ? "window beyond the stream" : "record walk");
    }
    rc = located(any);
    if (rc || !any) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->work_stream) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->work_stream, hipStreamNonBlocking));
    hipStream_t ws = ctx->work_stream;
    atsc_dplan *dp[MAX_INPUTS] = {};
    uint8_t *d_body[MAX_INPUTS] = {};
    QueryInput in[MAX_INPUTS];
    int status[MAX_INPUTS] = {};
    void *d_res = nullptr;
    hipError_t e = hipSuccess;
    // an empty window begins where every plan has a sample: at the last of the plans' first samples
    uint64_t first = 0;
    for (int k = 0; k < n_in; ++k) first = std::max(first, w[k].sample_begin);
    std::vector<uint64_t> begin2(n_windows);
    for (uint64_t i = 0; i < n_windows; ++i) begin2[i] = (count[i] ? begin[i] : first) - w[0].sample_begin;
#define WCHK(call_)                                                                 \
    do {                                                                            \
        e = (call_);                                                                \
        if (e != hipSuccess) { rc = fail(ctx, ATSC_E_HIP, #call_, e); goto done; } \
    } while (0)
    for (int k = 0; k < n_in; ++k) {
        const uint64_t slice = w[k].byte_end - w[k].byte_begin;
        rc = dplan_create_range(ctx, hb[k].body + w[k].byte_begin, slice, 0, 0, ~0ull, nullptr, &dp[k]);
        if (rc) goto done;
        if (dp[k]->class_count[CLASS_LARGE]) {
            // The large tier's launch forms depend on every large frame of the stream (large_choices): the rest of the
            // record headers is walked as well, so that the touched large frames decode as the full decode does them.
            DPlanHost Hw;
            const char *why;
            rc = dplan_parse(hb[k].body, hb[k].len, hb[k].has_count, Hw, &why);
            if (rc) { rc = fail(ctx, rc, why); goto done; }
            large_choices(dp[k], Hw.tabs.plans, Hw.frames, Hw.cls);
        }
        WCHK(pool_alloc(ctx, (void **)&d_body[k], std::max<uint64_t>(slice, 16)));
        if (k == 0) WCHK(pool_alloc(ctx, &d_res, out_bytes));
        WCHK(hipMemcpyAsync(d_body[k], hb[k].body + w[k].byte_begin, slice, hipMemcpyHostToDevice, ws));
        if (trace) fprintf(stderr, "[window]     h2d records %llu bytes (frames %llu..%llu)\n", (unsigned long long)slice,
                           (unsigned long long)w[k].frame_begin, (unsigned long long)w[k].frame_end);
        in[k] = QueryInput{dp[k], d_body[k], w[k].sample_begin};
    }
    rc = enqueue(in, begin2.data(), d_res, ws);
    if (rc) goto done;
    for (int k = 0; k < n_in; ++k) WCHK(hipMemcpyAsync(&status[k], dp[k]->d_status, sizeof(int), hipMemcpyDeviceToHost, ws));
    WCHK(hipStreamSynchronize(ws));
    for (int k = 0; k < n_in; ++k)
        if (status[k]) { rc = fail_in(ctx, ATSC_E_FORMAT, call, "malformed payload"); goto done; }
    WCHK(hipMemcpyAsync(out, d_res, head_bytes, hipMemcpyDeviceToHost, ws));
    WCHK(hipStreamSynchronize(ws));
    if (head_bytes < out_bytes) {
        const size_t end = std::min(out_bytes, used(out));
        if (end > head_bytes) {
            WCHK(hipMemcpyAsync((char *)out + head_bytes, (const char *)d_res + head_bytes, end - head_bytes, hipMemcpyDeviceToHost, ws));
            WCHK(hipStreamSynchronize(ws));
        }
    }
#undef WCHK
done:
    if (rc) (void)hipStreamSynchronize(ws);
    for (int k = 0; k < n_in; ++k) pool_free(ctx, d_body[k]);
    pool_free(ctx, d_res);
    for (int k = 0; k < n_in; ++k) atsc_dplan_destroy(dp[k]);
    return rc;
}

// ------------------------------------------------------------------------------------------
// window decode: samples [begin, begin + count) of the decoded stream without decoding the rest
// ------------------------------------------------------------------------------------------
// The window decode.  One task per (window, touched frame); tasks go by frame:
//  * a frame of the LDS-resident classes that one window touches: k_decompress<W, SPL, true> straight into d_out;
//  * one that several windows touch: decoded once, over the union of their ranges, into scratch;
//  * a large frame: the large tier's launch sequence over a sub-plan of the touched large frames -- one that a window
//    holds whole is written straight into d_out (its out_off rebased), the others go to scratch whole;
//  * k_window_gather then copies the scratch parts to their windows.
// A destination in scratch is named by its distance from d_out in doubles, modulo 2^64: one base pointer serves both.
extern "C" int atsc_decompress_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                           const uint64_t *begin, const uint64_t *count, const uint64_t *out_off,
                                           double *d_out, void *stream)
{
    ATSC_API_BEGIN
    if (!ctx || !dp || !d_body || !d_out || (n_windows && (!begin || !count || !out_off)))
        return fail(ctx, ATSC_E_INVALID, "decompress_windows: null argument");
    int rc = check_windows(ctx, "decompress_windows", dp, d_out, "d_out", n_windows, begin, count, ~0ull);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const auto &F = dp->h_frames;
    struct Ent {
        uint64_t dst;
        uint32_t frame, lo, hi;
    };
    std::vector<Ent> ents;
    for (uint64_t i = 0; i < n_windows; ++i) {
        if (!count[i]) continue;
        uint64_t fb, fe;
        (void)atsc_dplan_find_frames(dp, begin[i], count[i], &fb, &fe);
        const uint64_t b = begin[i], e = begin[i] + count[i];
        for (uint64_t f = fb; f < fe; ++f) {
            const uint64_t fo = F[f].out_off, fn = F[f].n;
            const uint64_t lo = std::max(b, fo) - fo, hi = std::min(e, fo + fn) - fo;
            ents.push_back(Ent{out_off[i] + (fo + lo - b), (uint32_t)f, (uint32_t)lo, (uint32_t)hi});
        }
    }
    if (ents.empty()) return ATSC_OK;
    if (!launch_decompress_window || !launch_window_gather) return fail(ctx, ATSC_E_UNSUPPORTED, "decompress_windows: no window kernels");
    auto by_frame = [](const Ent &a, const Ent &b) { return a.frame < b.frame; };
    if (!std::is_sorted(ents.begin(), ents.end(), by_frame)) std::stable_sort(ents.begin(), ents.end(), by_frame);
    QueryRes &R = dp->res[Q_WINDOW];
    HIPCHK(ctx, R.wait());
    // one piece holds every task; destinations in scratch count from the scratch's start until it is known where it lies
    DecodeTasks D;
    std::vector<size_t> small_scr_at[CLASS_LARGE], big_scr;
    uint64_t scr = 0;
    uint32_t max_len = 0;
    for (size_t a = 0; a < ents.size();) {
        size_t z = a + 1;
        while (z < ents.size() && ents[z].frame == ents[a].frame) ++z;
        const uint32_t f = ents[a].frame, n = F[f].n;
        const int c = dp->h_cls[f];
        const bool one = z - a == 1;
        if (c != CLASS_LARGE) {
            if (one) {
                D.small[c].push_back(DevWTask{ents[a].dst, f, ents[a].lo, ents[a].hi, 0});
            } else {
                uint32_t ulo = n, uhi = 0;
                for (size_t k = a; k < z; ++k) { ulo = std::min(ulo, ents[k].lo); uhi = std::max(uhi, ents[k].hi); }
                small_scr_at[c].push_back(D.small[c].size());
                D.small[c].push_back(DevWTask{scr, f, ulo, uhi, 0});
                for (size_t k = a; k < z; ++k) {
                    D.gat.push_back(DevWGather{scr + ents[k].lo - ulo, ents[k].dst, ents[k].hi - ents[k].lo, 0});
                    max_len = std::max(max_len, ents[k].hi - ents[k].lo);
                }
                scr += uhi - ulo;
            }
        } else {
            DevDFrame d = F[f];
            if (one && ents[a].lo == 0 && ents[a].hi == n) {
                d.out_off = ents[a].dst;
            } else {
                big_scr.push_back(D.big.size());
                d.out_off = scr;
                for (size_t k = a; k < z; ++k) {
                    D.gat.push_back(DevWGather{scr + ents[k].lo, ents[k].dst, ents[k].hi - ents[k].lo, 0});
                    max_len = std::max(max_len, ents[k].hi - ents[k].lo);
                }
                scr += n;
            }
            D.big.push_back(d);
        }
        a = z;
    }
    PieceDecode pt;
    for (int c = 0; c < CLASS_LARGE; ++c) { pt.small_at[c] = 0; pt.small_n[c] = (uint32_t)D.small[c].size(); }
    pt.big_at = pt.gat_at = 0;
    pt.big_n = D.max_big = (uint32_t)D.big.size();
    pt.gat_n = (uint32_t)D.gat.size();
    pt.max_len = max_len;
    // one upload: the classes' task lists, the large sub-plan (frames, ids), the copies
    Upload U;
    D.place(U);
    HIPCHK(ctx, R.reserve(ctx, U.up_bytes, U.bytes, scr));
    if (scr) {
        const uint64_t base = ((uint64_t)(uintptr_t)R.scratch - (uint64_t)(uintptr_t)d_out) / sizeof(double);
        for (int c = 0; c < CLASS_LARGE; ++c)
            for (size_t i : small_scr_at[c]) D.small[c][i].dst += base;
        for (size_t i : big_scr) D.big[i].out_off += base;
    }
    U.stage(R.h);
    HIPCHK(ctx, hipMemcpyAsync(R.d, R.h, U.up_bytes, hipMemcpyHostToDevice, s));
    rc = launch_piece_decode(ctx, dp, d_body, R.d, D, pt, d_out, R.scratch, d_out, s, BY_WINDOW);
    if (rc) return rc;
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
    ATSC_API_END
}

// Host call: walks the headers up to the window's last record, plans the touched records only and uploads only their bytes.
extern "C" int atsc_decompress_window(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t begin,
                                      uint64_t count, double *out, uint64_t out_cap, uint64_t *out_n)
{
    ATSC_API_BEGIN
    if (!ctx || !body || !out_n || (count && !out)) return fail(ctx, ATSC_E_INVALID, "decompress_window: null argument");
    *out_n = 0;
    static const bool trace = getenv("ATSC_TRACE_HOST") != nullptr;
    const uint64_t zero = 0;
    const HostBody hb{body, body_len, has_count};
    const int rc = window_host_call(
        ctx, "decompress_window", &hb, 1, 1, &begin, &count, out, count * sizeof(double), count * sizeof(double), trace,
        [&](bool) { return out_cap < count ? fail(ctx, ATSC_E_CAPACITY, "decompress_window: out_cap") : ATSC_OK; },
        [&](const QueryInput *in, const uint64_t *begin2, void *d_res, hipStream_t ws) {
            return atsc_decompress_windows_dev(ctx, in[0].dp, in[0].d_body, 1, begin2, &count, &zero, (double *)d_res, ws);
        },
        [](const void *) { return (size_t)0; });
    if (!rc) *out_n = count;
    return rc;
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// decoded samples of window pieces in scratch (the aggregate, the moments, the delta, the quantile and the histogram calls)
// ------------------------------------------------------------------------------------------
// Decoded samples reach the reduce and selection kernels through one scratch region, piece after piece in stream order.
static const uint64_t AGG_MIN_PIECE = 32ull * AGG_TILE;  // the least a piece holds, whatever the budget
// default piece length (samples) by the tier of the touched frames.  The sweep of profiles/aggregate_probe.json found no
// gain from pieces that fit the Infinity Cache (2^21-2^22 samples): fewer pieces win in both framings, most where the
// large tier's launch sequence (~65 us whatever its frame count) runs once per piece.
static const uint64_t AGG_PIECE_SMALL = 1ull << 24;
static const uint64_t AGG_PIECE_LARGE = 1ull << 24;

extern "C" int atsc_ctx_set_aggregate_scratch(atsc_ctx *ctx, uint64_t bytes)
{
    if (!ctx) return ATSC_E_INVALID;
    ctx->agg_budget = bytes;
    return ATSC_OK;
}

// the decoded samples a call's scratch may hold: the context's budget, else the default piece and room for two large
// frames cut by its ends
static uint64_t scratch_budget_samples(const atsc_ctx *ctx, bool large)
{
    return ctx->agg_budget ? ctx->agg_budget / sizeof(double)
                           : (large ? AGG_PIECE_LARGE + 2ull * MAX_FRAME : AGG_PIECE_SMALL);
}

// whether the covering intervals (stream index; org: the plan's first sample) touch a large frame
static bool spans_touch_large(const atsc_dplan *dp, uint64_t org, const std::vector<Span> &cov)
{
    for (const Span &c : cov) {
        uint64_t fb, fe;
        (void)atsc_dplan_find_frames(dp, c.first - org, c.second - c.first, &fb, &fe);
        for (uint64_t f = fb; f < fe; ++f)
            if (dp->h_cls[f] == CLASS_LARGE) return true;
    }
    return false;
}

// Piece length in samples, a multiple of `unit`: the budget less the spills, spill[k] being the room for two large frames
// of input k that cross the piece's ends (none when the covering intervals touch no large frame of it), shared evenly
// by the n_in inputs' regions, and at least AGG_MIN_PIECE.  Without a budget every input has the default of its own, or
// (one_default, the across' rule: a query over a list of streams) the inputs share the default of one.
static uint64_t piece_samples(const atsc_ctx *ctx, const QueryInput *in, int n_in, const std::vector<Span> &cov,
                              uint64_t unit, uint64_t *spill, bool one_default = false)
{
    uint64_t want = 0, spills = 0;
    bool any_large = false;
    for (int k = 0; k < n_in; ++k) {
        const bool large = spans_touch_large(in[k].dp, in[k].org, cov);
        spills += spill[k] = large ? 2ull * MAX_FRAME : 0;
        want += scratch_budget_samples(ctx, large);
        any_large = any_large || large;
    }
    if (ctx->agg_budget) want = ctx->agg_budget / sizeof(double);
    else if (one_default) want = scratch_budget_samples(ctx, any_large);
    return std::max<uint64_t>(AGG_MIN_PIECE, want > spills ? (want - spills) / n_in / unit * unit : 0);
}

// (one input)
static uint64_t piece_samples(const atsc_ctx *ctx, const atsc_dplan *dp, uint64_t org, const std::vector<Span> &cov,
                              uint64_t unit, uint64_t *spill)
{
    const QueryInput in{dp, nullptr, org};
    return piece_samples(ctx, &in, 1, cov, unit, spill);
}

// The decode tasks of the piece [S0, S1) into scratch[0, S1 - S0): per touched frame, the hull of its covered samples
// inside the piece.  cov: ascending disjoint covering intervals, *ci the first that may still meet the piece (advanced
// past those that end before it).  A large frame is decoded whole: in place when it lies inside the piece, else into
// one of two spill slots behind the region (scratch[region + MAX_FRAME k]) and copied from there (k_window_gather).
// false: more than two spill slots (only the frames across S0 and S1 can stick out).
static bool emit_piece_decode(const atsc_dplan *dp, uint64_t org, const std::vector<Span> &cov, size_t &ci, uint64_t S0,
                              uint64_t S1, uint64_t region, DecodeTasks &D, PieceDecode &pt)
{
    const auto &F = dp->h_frames;
    for (int c = 0; c < CLASS_LARGE; ++c) pt.small_at[c] = D.small[c].size();
    pt.big_at = D.big.size();
    pt.gat_at = D.gat.size();
    pt.max_len = 0;
    uint32_t n_spill = 0;
    auto emit = [&](uint64_t f, uint64_t lo, uint64_t hi) {
        const uint64_t fo = org + F[f].out_off, fn = F[f].n;
        const int c = dp->h_cls[f];
        if (c != CLASS_LARGE) {
            D.small[c].push_back(DevWTask{fo + lo - S0, (uint32_t)f, (uint32_t)lo, (uint32_t)hi, 0});
            return;
        }
        DevDFrame d = F[f];
        if (fo >= S0 && fo + fn <= S1) {
            d.out_off = fo - S0;
        } else {
            const uint64_t sp = region + (uint64_t)MAX_FRAME * n_spill++;
            d.out_off = sp;
            D.gat.push_back(DevWGather{sp + lo, fo + lo - S0, (uint32_t)(hi - lo), 0});
            pt.max_len = std::max(pt.max_len, (uint32_t)(hi - lo));
        }
        D.big.push_back(d);
    };
    while (ci < cov.size() && cov[ci].second <= S0) ++ci;
    uint64_t hf = ~0ull, hlo = 0, hhi = 0;
    for (size_t c = ci; c < cov.size() && cov[c].first < S1; ++c) {
        const uint64_t a = std::max(cov[c].first, S0), z = std::min(cov[c].second, S1);
        uint64_t fb, fe;
        (void)atsc_dplan_find_frames(dp, a - org, z - a, &fb, &fe);
        for (uint64_t f = fb; f < fe; ++f) {
            const uint64_t fo = org + F[f].out_off, fn = F[f].n;
            const uint64_t lo = std::max(a, fo) - fo, hi = std::min(z, fo + fn) - fo;
            if (f == hf) { hhi = hi; continue; }
            if (hf != ~0ull) emit(hf, hlo, hhi);
            hf = f;
            hlo = lo;
            hhi = hi;
        }
    }
    if (hf != ~0ull) emit(hf, hlo, hhi);
    if (n_spill > 2) return false;
    D.spills_used = std::max(D.spills_used, n_spill);
    for (int c = 0; c < CLASS_LARGE; ++c) pt.small_n[c] = (uint32_t)(D.small[c].size() - pt.small_at[c]);
    pt.big_n = (uint32_t)(D.big.size() - pt.big_at);
    pt.gat_n = (uint32_t)(D.gat.size() - pt.gat_at);
    D.max_big = std::max(D.max_big, pt.big_n);
    return true;
}

// The decode tasks of every piece of one input, piece after piece (emit_piece_decode): piece p holds samples
// [pcs[p].first * unit, pcs[p].second * unit).  `call` names the caller in the message.
static int emit_pieces_decode(atsc_ctx *ctx, const char *call, const atsc_dplan *dp, uint64_t org, const std::vector<Span> &cov,
                              const std::vector<Span> &pcs, uint64_t unit, uint64_t region, DecodeTasks &D,
                              std::vector<PieceDecode> &pdec)
{
    pdec.resize(pcs.size());
    size_t ci = 0;
    for (size_t p = 0; p < pcs.size(); ++p)
        if (!emit_piece_decode(dp, org, cov, ci, pcs[p].first * unit, pcs[p].second * unit, region, D, pdec[p]))
            return fail_in(ctx, ATSC_E_INVALID, call, "internal error (spill slots)");
    return ATSC_OK;
}

// The scratch of a call over n_in inputs: every input's region and behind it the spill slots it uses.  at[k]: where
// input k's region begins; hands back the samples of them all.  region and MAX_FRAME are even numbers of doubles, so every
// region begins at a multiple of 16 bytes, as the kernels' 16-byte loads need.
static uint64_t place_regions(const DecodeTasks *D, int n_in, uint64_t region, uint64_t *at)
{
    static_assert(AGG_TILE % 2 == 0 && MAX_FRAME % 2 == 0, "16-byte aligned regions");
    uint64_t scr_n = 0;
    for (int k = 0; k < n_in; ++k) {
        at[k] = scr_n;
        scr_n += region + (uint64_t)MAX_FRAME * D[k].spills_used;
    }
    return scr_n;
}

// ------------------------------------------------------------------------------------------
// windowed aggregates: count / min / max / sum / first / last of sample windows (atsc_aggregate.hip)
// ------------------------------------------------------------------------------------------
// The scratch region holds whole tiles: the windows' union ("covering intervals") is cut into pieces at multiples of
// AGG_TILE.  Covered tile ranges closer than AGG_GAP_TILES share a span, so that scattered windows do not each cost a
// piece of launches.
static const uint64_t AGG_GAP_TILES = 64;

template <class Q>
static int reduce_dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                      void *d_out, void *stream, const Q &q);

// A query's descriptor: what query_host and query_stream (below) need of it, and for the four reductions over tiles
// what reduce_dev does.  The front end's part:
//   CALL                the call's name in the messages
//   INPUTS              the streams the query reads: 1, or 2 (PairQuery) -- that many bodies, streams or plans; 0 where
//                       the number is the call's own (AcrossQuery, PairMatrixQuery), which inputs() then gives (query_inputs)
//   out_bytes(n)        bytes of the result of n windows
//   check(ctx)          the check of the call's parameters (ctx may be null: then no message is kept)
//   fill_empty(out, n)  the result of n empty windows
//   dev(...)            the device call; org: the stream index of the plan's first sample (INPUTS == 2: the list of
//                       inputs in its place, see query_dev)
// What the reductions over tiles differ in: the aggregates (atsc_aggregate.hip), the moments (atsc_moments.hip), the
// deltas (atsc_delta.hip), the runs (atsc_runs.hip), the extremes (atsc_extremes.hip) and the value counts
// (atsc_values.hip).
//   Tile, tile(t, k)   the tile kernel's task, from the plan's DevAggTile of tile k of the stream
//   tiles(.., scr, ..) the tile kernel's launch; scr[k]: input k's scratch region (a query over a list, INPUTS == 0: the
//                      scratch, the table of the regions' places and the number of partials, see reduce_dev)
//   part()             bytes of a partial: a member call, so that a query may size its partials by a parameter of the
//                      call (ExtQuery and ValQuery, by k); the others hand back their static PART
//   SIDE               the table both kernels share beside the partials: the windows' first / last samples, which the
//                      tile kernel writes (device only), or the windows' begins in the stream's index (uploaded)
//   CARRY, carried(t)  the tile kernel looks at the sample in front of a tile: the side table is one carry slot (device
//                      only), which holds the previous piece's last sample for a piece's first tile where carried(t)
struct AggQuery {
    static constexpr int INPUTS = 1;
    using Tile = DevAggTile;
    static constexpr const char *CALL = "aggregate_windows", *RES_NAME = "d_stats", *NO_KERNELS = "no aggregate kernels",
                                *TILES = "launch k_agg_tiles", *COMBINE = "launch k_agg_combine";
    static constexpr size_t PART = sizeof(DevAggPart);
    static size_t part() { return PART; }
    static constexpr bool SIDE_BEGINS = false;
    static constexpr QueryKind KIND = Q_AGGREGATE;
    static const DecodeCaller &who() { return BY_AGGREGATE; }
    static bool have() { return launch_agg_tiles && launch_agg_combine; }
    static constexpr bool CARRY = false;
    static Tile tile(const DevAggTile &t, uint64_t) { return t; }
    static bool carried(const Tile &) { return false; }
    static hipError_t tiles(const Tile *t, uint32_t n, const double *const *scr, void *part, void *side, hipStream_t s)
    {
        return launch_agg_tiles(t, n, scr[0], (DevAggPart *)part, (double *)side, s);
    }
    static hipError_t combine(const DevAggComb *c, uint32_t n, void *part, const void *side, void *out, hipStream_t s)
    {
        return launch_agg_combine(c, n, (DevAggPart *)part, (const double *)side, out, s);
    }
    static size_t out_bytes(uint64_t n) { return n * sizeof(atsc_window_stats); }
    static int check(atsc_ctx *) { return ATSC_OK; }
    static void fill_empty(void *out, uint64_t n)
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (uint64_t i = 0; i < n; ++i) {
            atsc_window_stats &r = ((atsc_window_stats *)out)[i];
            r.count = 0;
            r.min = r.max = r.first = r.last = nan;
            r.sum = 0.0;
        }
    }
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        const QueryInput in{dp, d_body, org};
        return reduce_dev(ctx, &in, n_windows, begin, count, d_res, stream, *this);
    }
};
// the tile task of the moments, the runs and the extremes, whose kernels take the tile's place in the stream
static DevPosTile pos_tile(const DevAggTile &t, uint64_t k) { return DevPosTile{t.src, t.dst, k * AGG_TILE, t.lo, t.hi}; }

struct MomQuery {
    static constexpr int INPUTS = 1;
    using Tile = DevPosTile;
    static constexpr const char *CALL = "moments_windows", *RES_NAME = "d_out", *NO_KERNELS = "no moments kernels",
                                *TILES = "launch k_mom_tiles", *COMBINE = "launch k_mom_combine";
    static constexpr size_t PART = sizeof(DevMomPart);
    static size_t part() { return PART; }
    static constexpr bool SIDE_BEGINS = true;
    static constexpr QueryKind KIND = Q_MOMENTS;
    static const DecodeCaller &who() { return BY_MOMENTS; }
    static bool have() { return launch_mom_tiles && launch_mom_combine; }
    static constexpr bool CARRY = false;
    static Tile tile(const DevAggTile &t, uint64_t k) { return pos_tile(t, k); }
    static bool carried(const Tile &) { return false; }
    static hipError_t tiles(const Tile *t, uint32_t n, const double *const *scr, void *part, void *, hipStream_t s)
    {
        return launch_mom_tiles(t, n, scr[0], (DevMomPart *)part, s);
    }
    static hipError_t combine(const DevAggComb *c, uint32_t n, void *part, const void *side, void *out, hipStream_t s)
    {
        return launch_mom_combine(c, n, (DevMomPart *)part, (const uint64_t *)side, out, s);
    }
    static size_t out_bytes(uint64_t n) { return n * sizeof(atsc_window_moments); }
    static int check(atsc_ctx *) { return ATSC_OK; }
    static void fill_empty(void *out, uint64_t n)
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (uint64_t i = 0; i < n; ++i) {
            atsc_window_moments &r = ((atsc_window_moments *)out)[i];
            r.count = 0;
            r.mean = r.m2 = r.t_mean = r.t_m2 = r.c_tx = nan;
        }
    }
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        const QueryInput in{dp, d_body, org};
        return reduce_dev(ctx, &in, n_windows, begin, count, d_res, stream, *this);
    }
};

struct DltQuery {
    static constexpr int INPUTS = 1;
    using Tile = DevDltTile;
    static constexpr const char *CALL = "delta_windows", *RES_NAME = "d_out", *NO_KERNELS = "no delta kernels",
                                *TILES = "launch k_dlt_tiles", *COMBINE = "launch k_dlt_combine";
    static constexpr size_t PART = sizeof(DevDltPart);
    static size_t part() { return PART; }
    static constexpr bool SIDE_BEGINS = false;
    static constexpr bool CARRY = true;
    static constexpr QueryKind KIND = Q_DELTA;
    static const DecodeCaller &who() { return BY_DELTA; }
    static bool have() { return launch_dlt_tiles && launch_dlt_combine; }
    // every tile but a window's first continues from the slot in front of it (the window covers that slot, so it was
    // decoded): scratch[src - 1], or the carry slot where the tile is the first of its piece
    static Tile tile(const DevAggTile &t, uint64_t)
    {
        const uint32_t cont = (t.flags & AGG_FIRST) ? 0u : (uint32_t)DLT_CONT;
        return Tile{t.src, t.dst, t.lo, t.hi, cont | (cont && t.src == 0 ? (uint32_t)DLT_CARRY : 0u), 0};
    }
    static bool carried(const Tile &t) { return (t.flags & DLT_CARRY) != 0; }
    static hipError_t tiles(const Tile *t, uint32_t n, const double *const *scr, void *part, void *side, hipStream_t s)
    {
        return launch_dlt_tiles(t, n, scr[0], (const double *)side, (DevDltPart *)part, s);
    }
    static hipError_t combine(const DevAggComb *c, uint32_t n, void *part, const void *, void *out, hipStream_t s)
    {
        return launch_dlt_combine(c, n, (DevDltPart *)part, out, s);
    }
    static size_t out_bytes(uint64_t n) { return n * sizeof(atsc_window_delta); }
    static int check(atsc_ctx *) { return ATSC_OK; }
    static void fill_empty(void *out, uint64_t n)
    {
        for (uint64_t i = 0; i < n; ++i) {
            atsc_window_delta &r = ((atsc_window_delta *)out)[i];
            r.pairs = r.rises = r.falls = 0;
            r.up = r.down = r.after_falls = r.max_rise = r.max_fall = 0.0;
        }
    }
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        const QueryInput in{dp, d_body, org};
        return reduce_dev(ctx, &in, n_windows, begin, count, d_res, stream, *this);
    }
};

// the runs' check of a call's condition (the rolling runs' too); `call` names the caller in the message
static int runs_condition_check(atsc_ctx *ctx, const char *call, int op, double limit)
{
    if (op < ATSC_RUNS_GT || op > ATSC_RUNS_NE) return fail_in(ctx, ATSC_E_INVALID, call, "unknown op");
    if (std::isnan(limit)) return fail_in(ctx, ATSC_E_INVALID, call, "limit is NaN");
    return ATSC_OK;
}

static void run_empty_record(atsc_window_runs &r)
{
    r.samples = r.inside = r.runs = r.longest = r.head = r.tail = 0;
    r.longest_at = r.first_at = r.last_at = ATSC_RUNS_NONE;
    r.excess = 0.0;
}

// The runs (atsc_runs.hip).  The one reduction with parameters of a call, the condition: they are the query object's
// members, which reduce_dev hands to tiles() by calling it on that object.  No carry: the merge joins a run across two
// tiles, whichever pieces they lie in.
struct RunQuery {
    static constexpr int INPUTS = 1;
    using Tile = DevPosTile;
    static constexpr const char *CALL = "runs_windows", *RES_NAME = "d_out", *NO_KERNELS = "no runs kernels",
                                *TILES = "launch k_run_tiles", *COMBINE = "launch k_run_combine";
    static constexpr size_t PART = sizeof(DevRunPart);
    static size_t part() { return PART; }
    static constexpr bool SIDE_BEGINS = true;
    static constexpr bool CARRY = false;
    static constexpr QueryKind KIND = Q_RUNS;
    int op;
    double limit;
    static const DecodeCaller &who() { return BY_RUNS; }
    static bool have() { return launch_run_tiles && launch_run_combine; }
    static Tile tile(const DevAggTile &t, uint64_t k) { return pos_tile(t, k); }
    static bool carried(const Tile &) { return false; }
    hipError_t tiles(const Tile *t, uint32_t n, const double *const *scr, void *part, void *, hipStream_t s) const
    {
        return launch_run_tiles(t, n, scr[0], op, limit, (DevRunPart *)part, s);
    }
    static hipError_t combine(const DevAggComb *c, uint32_t n, void *part, const void *side, void *out, hipStream_t s)
    {
        return launch_run_combine(c, n, (DevRunPart *)part, (const uint64_t *)side, out, s);
    }
    static size_t out_bytes(uint64_t n) { return n * sizeof(atsc_window_runs); }
    int check(atsc_ctx *ctx) const { return runs_condition_check(ctx, CALL, op, limit); }
    static void fill_empty(void *out, uint64_t n)
    {
        for (uint64_t i = 0; i < n; ++i) run_empty_record(((atsc_window_runs *)out)[i]);
    }
    // (the condition is checked in front of the arguments)
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        const int rc = check(ctx);
        const QueryInput in{dp, d_body, org};
        return rc ? rc : reduce_dev(ctx, &in, n_windows, begin, count, d_res, stream, *this);
    }
};

static void ext_empty_record(void *rec, uint32_t k)
{
    atsc_window_extremes_head *h = (atsc_window_extremes_head *)rec;
    h->count = h->nans = 0;
    atsc_extreme *e = (atsc_extreme *)(h + 1);
    for (uint32_t j = 0; j < 2 * k; ++j) {
        e[j].value = std::numeric_limits<double>::quiet_NaN();
        e[j].at = ATSC_EXTREMES_NONE;
    }
}

// The extremes (atsc_extremes.hip).  k is the call's parameter and a member, as the runs' condition is; it also sizes the
// partials, which have the record's layout (2 + 4 k words) with positions as stream indices, so that a shared mid
// tile's partial serves every window that shares it; the final combine pass subtracts the window's begin.  No carry.
struct ExtQuery {
    static constexpr int INPUTS = 1;
    using Tile = DevPosTile;
    static constexpr const char *CALL = "extremes_windows", *RES_NAME = "d_out", *NO_KERNELS = "no extremes kernels",
                                *TILES = "launch k_ext_tiles", *COMBINE = "launch k_ext_combine";
    static constexpr bool SIDE_BEGINS = true;
    static constexpr bool CARRY = false;
    static constexpr QueryKind KIND = Q_EXTREMES;
    uint32_t k;
    size_t part() const { return ATSC_EXTREMES_BYTES(k); }
    static const DecodeCaller &who() { return BY_EXTREMES; }
    static bool have() { return launch_ext_tiles && launch_ext_combine; }
    static Tile tile(const DevAggTile &t, uint64_t kt) { return pos_tile(t, kt); }
    static bool carried(const Tile &) { return false; }
    hipError_t tiles(const Tile *t, uint32_t n, const double *const *scr, void *part, void *, hipStream_t s) const
    {
        return launch_ext_tiles(t, n, scr[0], k, part, s);
    }
    hipError_t combine(const DevAggComb *c, uint32_t n, void *part, const void *side, void *out, hipStream_t s) const
    {
        return launch_ext_combine(c, n, k, part, (const uint64_t *)side, out, s);
    }
    size_t out_bytes(uint64_t n) const { return n * ATSC_EXTREMES_BYTES(k); }
    int check(atsc_ctx *ctx) const
    {
        if (k == 0 || k > ATSC_EXTREMES_MAX_K) return fail(ctx, ATSC_E_INVALID, "extremes_windows: k outside [1, 16]");
        return ATSC_OK;
    }
    void fill_empty(void *out, uint64_t n) const
    {
        for (uint64_t i = 0; i < n; ++i) ext_empty_record((char *)out + i * ATSC_EXTREMES_BYTES(k), k);
    }
    // (k is checked in front of the arguments)
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        const int rc = check(ctx);
        const QueryInput in{dp, d_body, org};
        return rc ? rc : reduce_dev(ctx, &in, n_windows, begin, count, d_res, stream, *this);
    }
};

static void val_empty_record(void *rec, uint32_t k)
{
    atsc_window_values_head *h = (atsc_window_values_head *)rec;
    h->count = h->nans = h->below = 0;
    h->distinct = h->more = 0;
    atsc_value_count *e = (atsc_value_count *)(h + 1);
    for (uint32_t j = 0; j < k; ++j) {
        e[j].value = std::numeric_limits<double>::quiet_NaN();
        e[j].n = 0;
    }
}

// A value's key, as the kernels compute it (sample_key, atsc_tile_reduce.h): unsigned order is value order, both zeros
// on +0.0's key; 0 for NaN.
static uint64_t val_key(double v)
{
    if (v != v) return 0;
    uint64_t b;
    memcpy(&b, &v, 8);
    if (v == 0.0) b = 0;
    return b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
}

// The value counts (atsc_values.hip).  k and above are the call's parameters and members, as the extremes' k is; k
// sizes the partials, which have the record's layout (4 + 2 k words).  A partial holds no position, so a shared mid
// tile's partial serves every window as it is: no side table, and no carry.
// The call keeps its tables, partials and scratch in the plan's slot of the extremes (KIND): the two selections over
// tiles share one set of per-plan resources, so a call of either kind waits (host side) for the plan's previous call of
// either kind, and the plan's layout and the host code outside this file stay what they were.
struct ValQuery {
    static constexpr int INPUTS = 1;
    using Tile = DevAggTile;
    static constexpr const char *CALL = "values_windows", *RES_NAME = "d_out", *NO_KERNELS = "no values kernels",
                                *TILES = "launch k_val_tiles", *COMBINE = "launch k_val_combine";
    static constexpr bool SIDE_BEGINS = false, NO_SIDE = true;
    static constexpr bool CARRY = false;
    static constexpr QueryKind KIND = Q_EXTREMES;
    uint32_t k;
    double above;
    size_t part() const { return ATSC_VALUES_BYTES(k); }
    static const DecodeCaller &who() { return BY_VALUES; }
    static bool have() { return launch_val_tiles && launch_val_combine; }
    static Tile tile(const DevAggTile &t, uint64_t) { return t; }
    static bool carried(const Tile &) { return false; }
    hipError_t tiles(const Tile *t, uint32_t n, const double *const *scr, void *part, void *, hipStream_t s) const
    {
        return launch_val_tiles(t, n, scr[0], k, val_key(above), part, s);
    }
    hipError_t combine(const DevAggComb *c, uint32_t n, void *part, const void *, void *out, hipStream_t s) const
    {
        return launch_val_combine(c, n, k, part, out, s);
    }
    size_t out_bytes(uint64_t n) const { return n * ATSC_VALUES_BYTES(k); }
    int check(atsc_ctx *ctx) const
    {
        if (k == 0 || k > ATSC_VALUES_MAX_K) return fail(ctx, ATSC_E_INVALID, "values_windows: k outside [1, 32]");
        return ATSC_OK;
    }
    void fill_empty(void *out, uint64_t n) const
    {
        for (uint64_t i = 0; i < n; ++i) val_empty_record((char *)out + i * ATSC_VALUES_BYTES(k), k);
    }
    // (k is checked in front of the arguments)
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        const int rc = check(ctx);
        const QueryInput in{dp, d_body, org};
        return rc ? rc : reduce_dev(ctx, &in, n_windows, begin, count, d_res, stream, *this);
    }
};

// The pair moments (atsc_pair.hip): the one reduction over two inputs.  Its kernels read the same slots of the two
// inputs' regions; the partial is the moments' node with the second stream's value where that has the position.  No
// position is counted from a window's begin: no side table.  No carry.
struct PairQuery {
    static constexpr int INPUTS = 2;
    using Tile = DevPosTile;
    static constexpr const char *CALL = "pair_windows", *RES_NAME = "d_out", *NO_KERNELS = "no pair kernels",
                                *TILES = "launch k_pair_tiles", *COMBINE = "launch k_pair_combine";
    static constexpr size_t PART = sizeof(DevMomPart);
    static size_t part() { return PART; }
    static constexpr bool SIDE_BEGINS = false, NO_SIDE = true;
    static constexpr bool CARRY = false;
    static constexpr QueryKind KIND = Q_PAIR;
    static const DecodeCaller &who() { return BY_PAIR; }
    static bool have() { return launch_pair_tiles && launch_pair_combine; }
    static Tile tile(const DevAggTile &t, uint64_t k) { return pos_tile(t, k); }
    static bool carried(const Tile &) { return false; }
    static hipError_t tiles(const Tile *t, uint32_t n, const double *const *scr, void *part, void *, hipStream_t s)
    {
        return launch_pair_tiles(t, n, scr[0], scr[1], (DevMomPart *)part, s);
    }
    static hipError_t combine(const DevAggComb *c, uint32_t n, void *part, const void *, void *out, hipStream_t s)
    {
        return launch_pair_combine(c, n, (DevMomPart *)part, out, s);
    }
    static size_t out_bytes(uint64_t n) { return n * sizeof(atsc_window_pair); }
    static int check(atsc_ctx *) { return ATSC_OK; }
    static void fill_empty(void *out, uint64_t n)
    {
        const double nan = std::numeric_limits<double>::quiet_NaN();
        for (uint64_t i = 0; i < n; ++i) {
            atsc_window_pair &r = ((atsc_window_pair *)out)[i];
            r.count = 0;
            r.mean_x = r.m2_x = r.mean_y = r.m2_y = r.c_xy = nan;
        }
    }
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
            void *d_res, void *stream) const
    {
        return reduce_dev(ctx, in, n_windows, begin, count, d_res, stream, *this);
    }
};

extern "C" uint64_t atsc_pair_matrix_records(uint32_t n_streams) { return (uint64_t)n_streams * ((uint64_t)n_streams + 1) / 2; }

extern "C" uint64_t atsc_pair_matrix_index(uint32_t n_streams, uint32_t i, uint32_t j)
{
    if (i > j || j >= n_streams) return ~0ull;
    return (uint64_t)i * (2ull * n_streams - i + 1) / 2 + (j - i);
}

// The pair matrix (atsc_pair_matrix.hip): the pair moments of every pair (i, j), i <= j, of a list of n_streams inputs.
// The one reduction over a list (INPUTS == 0, see reduce_dev): its partial is a block of P = n_streams (n_streams + 1) / 2
// of the pair's nodes, which the kernels keep pair-major (pair p's node of partial d at part[p part_n + d]); its kernels
// make their grids from the tile tasks and the combine groups, so the host lists nothing per pair.  No side table, no
// carry.  n_windows is a member for the check of the result's size.
struct PairMatrixQuery {
    static constexpr int INPUTS = 0;
    using Tile = DevPosTile;
    static constexpr const char *CALL = "pair_matrix_windows", *RES_NAME = "d_out", *NO_KERNELS = "no pair matrix kernels",
                                *TILES = "launch k_pmx_tiles", *COMBINE = "launch k_pmx_combine";
    static constexpr bool SIDE_BEGINS = false, NO_SIDE = true;
    static constexpr bool CARRY = false;
    static constexpr QueryKind KIND = Q_PAIR_MATRIX;
    uint32_t n_streams;
    uint64_t n_windows;
    int inputs() const { return (int)n_streams; }
    uint64_t pairs() const { return atsc_pair_matrix_records(n_streams); }
    size_t part() const { return pairs() * sizeof(DevMomPart); }
    static const DecodeCaller &who() { return BY_PAIR_MATRIX; }
    static bool have() { return launch_pmx_tiles && launch_pmx_combine; }
    static Tile tile(const DevAggTile &t, uint64_t k) { return pos_tile(t, k); }
    static bool carried(const Tile &) { return false; }
    hipError_t tiles(const Tile *t, uint32_t n, const double *scratch, const uint64_t *reg, void *part, uint64_t part_n,
                     hipStream_t s) const
    {
        return launch_pmx_tiles(t, n, scratch, reg, n_streams, (DevMomPart *)part, part_n, s);
    }
    hipError_t combine(const DevAggComb *c, uint32_t n, void *part, uint64_t part_n, void *out, hipStream_t s) const
    {
        return launch_pmx_combine(c, n, (DevMomPart *)part, part_n, n_streams, out, s);
    }
    size_t out_bytes(uint64_t n) const { return n * pairs() * sizeof(atsc_window_pair); }
    int check(atsc_ctx *ctx) const
    {
        if (n_streams == 0 || n_streams > ATSC_ACROSS_MAX_STREAMS) return fail_in(ctx, ATSC_E_INVALID, CALL, "n_streams outside [1, 64]");
        if (n_windows > 0xfffffffeull / pairs()) return fail_in(ctx, ATSC_E_INVALID, CALL, "more than 2^32 - 2 records");
        return ATSC_OK;
    }
    void fill_empty(void *out, uint64_t n) const { PairQuery::fill_empty(out, n * pairs()); }
    // (the list's length and the result's size are checked in front of the arguments)
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n, const uint64_t *begin, const uint64_t *count, void *d_res,
            void *stream) const
    {
        const int rc = check(ctx);
        return rc ? rc : reduce_dev(ctx, in, n, begin, count, d_res, stream, *this);
    }
};

// The device call of a reduction over tiles (Q: AggQuery, MomQuery, DltQuery, RunQuery, ExtQuery, ValQuery, PairQuery or
// PairMatrixQuery;
// the kernels named below are the aggregates').  q: the query's parameters of this call, where it has any (RunQuery,
// ExtQuery, ValQuery).  in: the query_inputs(q) streams it reads, each a plan, its record bytes on the device and the stream index of
// the plan's first sample; begin[] counts from in[0].org.  Everything below is computed once, in the stream's index,
// which the inputs share; per piece every input is decoded into a scratch region of its own, with its own decode tasks
// and spill slots, and the tile kernel gets every region's pointer.  The call's tables, partials and regions are
// in[0].dp's (res[Q::KIND]).
// Host work: covering intervals, pieces, the decode tasks of every piece (one per touched frame: its
// covered samples' hull in the piece), the tile tasks (a full tile that windows cover past their first tile and before
// their last one is reduced once, into a shared partial; every window's first and last tile are reduced for it alone)
// and the combine passes (groups of 64 partials until one is left per window).  All of it goes up in one copy; then,
// per piece, the window decode's launchers into scratch and k_agg_tiles, and k_agg_combine once per pass.
// org (of an input): the stream index of the plan's first sample (a plan of the touched records only, in the host call):
// tiles lie at multiples of AGG_TILE in the stream's index, not the plan's.  Indices below are the stream's unless named otherwise.
// Q::CARRY: a piece's decode overwrites the scratch, and with it the sample in front of the next piece's first tile.
// Where a window runs on into the next piece, an 8-byte copy behind the piece's tile launch (stream-ordered: behind
// the launch that read the slot's previous value, in front of the next decode) takes the piece's last sample to the
// carry slot in the call's tables.  The tile kernel never writes that slot.
// A query whose kernels share no table beside the partials says so (PairQuery::NO_SIDE, ValQuery::NO_SIDE).
// A query over a list of streams (INPUTS == 0: PairMatrixQuery, whose partial is a block of nodes, one per pair) reads
// inputs() of them, at most MAX_INPUTS.  Its regions share one input's default budget, as the across' do (across_dev);
// the regions' places in the scratch go up as a table, which the tile kernel gets with the scratch in place of the
// list of pointers; and both kernels get the number of partials.  The geometry -- tiles, shared mid tiles, combine
// passes -- does not look inside a partial and is the same.
template <class Q, class = void>
struct NoSide : std::false_type {};
template <class Q>
struct NoSide<Q, std::void_t<decltype(Q::NO_SIDE)>> : std::true_type {};

// The streams a query reads: its INPUTS constant, or for a query over a runtime number of them (INPUTS == 0) the call's own.
template <class Q>
static int query_inputs(const Q &q)
{
    if constexpr (Q::INPUTS > 0) return Q::INPUTS;
    else return q.inputs();
}

template <class Q>
static int reduce_dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                      void *d_out, void *stream, const Q &q)
{
    constexpr bool LIST = Q::INPUTS == 0;
    static_assert(Q::INPUTS <= 2, "one or two inputs, or a list");
    if (!ctx) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "null argument");
    const int NI = query_inputs(q);
    if (NI < 1 || NI > MAX_INPUTS) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "n_streams outside [1, 64]");
    for (int k = 0; k < NI; ++k)
        if (!in[k].dp || (n_windows && !in[k].d_body)) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "null argument");
    if (n_windows && (!begin || !count || !d_out)) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "null argument");
    for (int k = 1; k < NI; ++k)
        if (in[k].dp->ctx != in[0].dp->ctx) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "plans of different contexts");
    const uint64_t org = in[0].org;  // begin[] counts from here
    int rc = ATSC_OK;
    for (int k = 0; k < NI && !rc; ++k)
        rc = check_windows(ctx, Q::CALL, in[k].dp, d_out, Q::RES_NAME, n_windows, begin, count, 0xfffffffeull, org, in[k].org);
    if (rc || n_windows == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !Q::have()) return fail_in(ctx, ATSC_E_UNSUPPORTED, Q::CALL, Q::NO_KERNELS);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t T = AGG_TILE, W = n_windows;
    // covering intervals: the union of the non-empty windows
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i)
        if (count[i]) cov.emplace_back(org + begin[i], org + begin[i] + count[i]);
    merge_spans(cov);
    uint64_t spill[MAX_INPUTS];
    const uint64_t piece_tiles = piece_samples(ctx, in, NI, cov, T, spill, LIST) / T;
    std::vector<Span> pcs;  // tiles [first, second): samples [first T, second T) at scratch[0, (second - first) T)
    const uint64_t region = cut_pieces(cov, T, piece_tiles, AGG_GAP_TILES, pcs) * T;
    // shared full tiles: the tiles past a window's first and before its last, merged over the windows
    std::vector<Span> mids;
    for (uint64_t i = 0; i < W; ++i) {
        if (!count[i]) continue;
        const uint64_t kb = (org + begin[i]) / T, ke = (org + begin[i] + count[i] - 1) / T;
        if (ke >= kb + 2) mids.emplace_back(kb + 1, ke);
    }
    merge_spans(mids);
    std::vector<uint64_t> mid_at(mids.size());
    uint64_t U = 0;
    for (size_t r = 0; r < mids.size(); ++r) { mid_at[r] = U; U += mids[r].second - mids[r].first; }
    auto shared_index = [&](uint64_t k) {  // index of full tile k among the shared partials
        const size_t r = (size_t)(std::upper_bound(mids.begin(), mids.end(), Span(k, ~0ull)) - mids.begin()) - 1;
        return mid_at[r] + (k - mids[r].first);
    };
    // tile tasks, by tile; part[] = [U shared | first, last tile of each window | combine levels]
    struct TT {
        uint64_t k;
        DevAggTile t;
    };
    std::vector<TT> tt;
    tt.reserve(U + 2 * W);
    for (size_t r = 0; r < mids.size(); ++r)
        for (uint64_t k = mids[r].first; k < mids[r].second; ++k)
            tt.push_back(TT{k, DevAggTile{0, mid_at[r] + (k - mids[r].first), 0, (uint32_t)T, 0, 0}});
    struct Lv {
        uint64_t head, tail, mid, n;
    };
    std::vector<Lv> lv(W);
    for (uint64_t i = 0; i < W; ++i) {
        if (!count[i]) { lv[i] = Lv{0, 0, 0, 0}; continue; }
        const uint64_t b = org + begin[i], e = b + count[i], kb = b / T, ke = (e - 1) / T;
        tt.push_back(TT{kb, DevAggTile{0, U + 2 * i, (uint32_t)(b - kb * T), (uint32_t)(std::min(e, (kb + 1) * T) - kb * T),
                                       (uint32_t)i, AGG_FIRST | (ke == kb ? AGG_LAST : 0u)}});
        if (ke > kb) tt.push_back(TT{ke, DevAggTile{0, U + 2 * i + 1, 0, (uint32_t)(e - ke * T), (uint32_t)i, AGG_LAST}});
        lv[i] = Lv{U + 2 * i, ke > kb ? U + 2 * i + 1 : U + 2 * i, ke >= kb + 2 ? shared_index(kb + 1) - 1 : 0, ke - kb + 1};
    }
    std::stable_sort(tt.begin(), tt.end(), [](const TT &x, const TT &y) { return x.k < y.k; });
    // combine passes: groups of 64 entries of each window's list until one is left
    uint64_t part_n = U + 2 * W;
    std::vector<DevAggComb> comb;
    std::vector<size_t> pass_at{0};
    {
        std::vector<uint32_t> live(W), next;
        for (uint64_t i = 0; i < W; ++i) live[i] = (uint32_t)i;
        while (!live.empty()) {
            next.clear();
            for (uint32_t i : live) {
                Lv &l = lv[i];
                const uint64_t G = std::max<uint64_t>(1, (l.n + 63) / 64);
                if (G == 1) {
                    comb.push_back(DevAggComb{l.head, l.tail, l.mid, i, (uint32_t)l.n, 0, i, 1});
                    continue;
                }
                const uint64_t base = part_n;
                part_n += G;
                for (uint64_t g = 0; g < G; ++g) comb.push_back(DevAggComb{l.head, l.tail, l.mid, base + g, (uint32_t)l.n, (uint32_t)g, i, 0});
                l = Lv{base, base + G - 1, base, G};
                next.push_back(i);
            }
            pass_at.push_back(comb.size());
            live.swap(next);
        }
    }
    // decode tasks of every piece, once per input, and every piece's tile tasks
    std::vector<std::vector<PieceDecode>> pdec(NI);
    std::vector<DecodeTasks> D(NI);
    for (int k = 0; k < NI && !rc; ++k) rc = emit_pieces_decode(ctx, Q::CALL, in[k].dp, in[k].org, cov, pcs, T, region, D[k], pdec[k]);
    if (rc) return rc;
    std::vector<size_t> tile_at(pcs.size());
    std::vector<uint32_t> tile_n(pcs.size());
    std::vector<char> carry_in(pcs.size(), 0);  // the piece's first tile reads the previous piece's last sample
    std::vector<typename Q::Tile> tiles;
    tiles.reserve(tt.size());
    size_t ti = 0;
    for (size_t p = 0; p < pcs.size(); ++p) {
        tile_at[p] = tiles.size();
        for (; ti < tt.size() && tt[ti].k < pcs[p].second; ++ti) {
            DevAggTile t = tt[ti].t;
            t.src = (tt[ti].k - pcs[p].first) * T;
            tiles.push_back(Q::tile(t, tt[ti].k));
            if (Q::carried(tiles.back())) carry_in[p] = 1;
        }
        // (a window that covers the slot in front of the piece covers the tile in front: the previous piece ends there)
        if (carry_in[p] && (p == 0 || pcs[p - 1].second != pcs[p].first))
            return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "internal error (carry without a previous piece)");
        tile_n[p] = (uint32_t)(tiles.size() - tile_at[p]);
    }
    if (ti != tt.size()) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "internal error (tile outside the pieces)");
    std::vector<uint64_t> wb;  // the windows' begins in the stream's index
    if (Q::SIDE_BEGINS) {
        wb.resize(W);
        for (uint64_t i = 0; i < W; ++i) wb[i] = org + begin[i];
    }
    QueryRes &R = in[0].dp->res[Q::KIND];
    HIPCHK(ctx, R.wait());
    // one upload: the decode tasks of every input, tile tasks, combine tasks (and the begins); behind them (device only)
    // the partials (and the windows' first / last samples, or the carry slot)
    Upload up;
    for (int k = 0; k < NI; ++k) D[k].place(up);
    const size_t off_tiles = up.add(tiles), off_comb = up.add(comb);
    const size_t off_begins = Q::SIDE_BEGINS ? up.add(wb) : 0;
    uint64_t scr_at[MAX_INPUTS];
    const uint64_t scr_n = place_regions(D.data(), NI, region, scr_at);
    const size_t off_reg = LIST ? up.add(scr_at, NI * sizeof(uint64_t)) : 0;
    const size_t off_part = up.device_only(part_n * q.part());
    const size_t off_side = Q::SIDE_BEGINS    ? off_begins
                            : NoSide<Q>::value ? off_part
                                               : up.device_only(Q::CARRY ? sizeof(double) : 2 * W * sizeof(double));
    rc = stage_upload(ctx, R, up, scr_n, s);
    if (rc) return rc;
    unsigned char *d = R.d;
    double *scr[MAX_INPUTS];
    for (int k = 0; k < NI; ++k) scr[k] = R.scratch + scr_at[k];
    void *part = d + off_part, *side = d + off_side;
    // a query over a list: the tile kernel takes the scratch and the table of the regions' places in it, and both
    // kernels the number of partials, which is how far one pair's nodes lie from the next pair's
    auto run_tiles = [&](size_t p) {
        const typename Q::Tile *t = (const typename Q::Tile *)(d + off_tiles) + tile_at[p];
        if constexpr (LIST) return q.tiles(t, tile_n[p], R.scratch, (const uint64_t *)(d + off_reg), part, part_n, s);
        else return q.tiles(t, tile_n[p], scr, part, side, s);
    };
    auto run_combine = [&](size_t a) {
        const DevAggComb *c = (const DevAggComb *)(d + off_comb) + pass_at[a];
        const uint32_t n = (uint32_t)(pass_at[a + 1] - pass_at[a]);
        if constexpr (LIST) return q.combine(c, n, part, part_n, d_out, s);
        else return q.combine(c, n, part, side, d_out, s);
    };
    for (size_t p = 0; p < pcs.size(); ++p) {
        for (int k = 0; k < NI; ++k) {
            rc = launch_piece_decode(ctx, in[k].dp, in[k].d_body, d, D[k], pdec[k][p], scr[k], scr[k], scr[k], s, Q::who());
            if (rc) return rc;
        }
        LAUNCHCHK(ctx, Q::TILES, run_tiles(p));
        if (Q::CARRY && p + 1 < pcs.size() && carry_in[p + 1])
            HIPCHK(ctx, hipMemcpyAsync(side, scr[0] + (pcs[p].second - pcs[p].first) * T - 1, sizeof(double), hipMemcpyDeviceToDevice, s));
    }
    for (size_t a = 0; a + 1 < pass_at.size(); ++a) LAUNCHCHK(ctx, Q::COMBINE, run_combine(a));
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// A query whose result's size depends on the data (SelQuery) has two members more: head_bytes(n), the part of the result
// that says how much of the rest is in use, and used_bytes(head, n), that amount.  The others' results come back whole.
template <class Q, class = void>
struct BlockResult : std::false_type {};
template <class Q>
struct BlockResult<Q, std::void_t<decltype(&Q::used_bytes)>> : std::true_type {};
template <class Q>
static size_t result_head_bytes(const Q &q, uint64_t n)
{
    if constexpr (BlockResult<Q>::value) return q.head_bytes(n);
    else return q.out_bytes(n);
}
template <class Q>
static size_t result_used_bytes(const Q &q, const void *head, uint64_t n)
{
    if constexpr (BlockResult<Q>::value) return q.used_bytes(head, n);
    else return q.out_bytes(n);
}

// The device call of a query on the plans in[0 .. query_inputs(q)): a query over one stream takes its plan, bytes and origin.
template <class Q>
static int query_dev(const Q &q, atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin,
                     const uint64_t *count, void *d_res, void *stream)
{
    if constexpr (Q::INPUTS == 1) return q.dev(ctx, in[0].dp, in[0].d_body, n_windows, begin, count, d_res, stream, in[0].org);
    else return q.dev(ctx, in, n_windows, begin, count, d_res, stream);
}

// The host call of a query over the bodies hb[0 .. query_inputs(q)), at most MAX_INPUTS of them: the argument check, the
// query's own, then window_host_call into its device call.
template <class Q>
static int query_host(atsc_ctx *ctx, const HostBody *hb, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                      void *out, const Q &q)
{
    const int n_in = query_inputs(q);
    bool bodies = true;
    for (int k = 0; k < n_in; ++k) bodies = bodies && hb[k].body;
    if (!ctx || !bodies || (n_windows && (!begin || !count || !out))) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "null argument");
    const int rc = q.check(ctx);
    if (rc) return rc;
    if (n_windows == 0) return ATSC_OK;
    return window_host_call(
        ctx, Q::CALL, hb, n_in, n_windows, begin, count, out, q.out_bytes(n_windows), result_head_bytes(q, n_windows),
        false,
        [&](bool any) {
            if (!any) q.fill_empty(out, n_windows);
            return ATSC_OK;
        },
        [&](const QueryInput *in, const uint64_t *begin2, void *d_res, hipStream_t ws) {
            return query_dev(q, ctx, in, n_windows, begin2, count, d_res, ws);
        },
        [&](const void *head) { return result_used_bytes(q, head, n_windows); });
}
// (one body)
template <class Q>
static int query_host(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                      const uint64_t *begin, const uint64_t *count, void *out, const Q &q)
{
    const HostBody hb{body, body_len, has_count};
    return query_host(ctx, &hb, n_windows, begin, count, out, q);
}

extern "C" int atsc_aggregate_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                          const uint64_t *begin, const uint64_t *count, atsc_window_stats *d_stats,
                                          void *stream)
{
    ATSC_API_BEGIN
    return AggQuery().dev(ctx, dp, d_body, n_windows, begin, count, d_stats, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_aggregate_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                      const uint64_t *begin, const uint64_t *count, atsc_window_stats *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, AggQuery());
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// windowed moments: centred moments of value and position of sample windows (atsc_moments.hip)
// ------------------------------------------------------------------------------------------
extern "C" int atsc_moments_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                        const uint64_t *begin, const uint64_t *count, atsc_window_moments *d_out,
                                        void *stream)
{
    ATSC_API_BEGIN
    return MomQuery().dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_moments_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                    const uint64_t *begin, const uint64_t *count, atsc_window_moments *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, MomQuery());
    ATSC_API_END
}

// Host only: what a caller reads off the moments.  Each line is one rounded operation, as include/atsc_hip.h states it.
extern "C" int atsc_moments_fit(const atsc_window_moments *m, uint64_t n, atsc_window_fit *out)
{
    if (n && (!m || !out)) return ATSC_E_INVALID;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint64_t i = 0; i < n; ++i) {
        const atsc_window_moments &a = m[i];
        atsc_window_fit &r = out[i];
        if (a.count == 0) {
            r.mean = r.variance = r.stddev = r.sample_variance = r.sample_stddev = r.slope = r.intercept = nan;
            continue;
        }
        r.mean = a.mean;
        r.variance = a.m2 / (double)a.count;
        r.stddev = std::sqrt(r.variance);
        r.sample_variance = a.count < 2 ? nan : a.m2 / (double)(a.count - 1);
        r.sample_stddev = std::sqrt(r.sample_variance);
        r.slope = a.t_m2 > 0.0 ? a.c_tx / a.t_m2 : nan;
        const double st = r.slope * a.t_mean;
        r.intercept = a.mean - st;
    }
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// windowed pair moments: centred moments and co-moment of the values of two streams over sample windows (atsc_pair.hip)
// ------------------------------------------------------------------------------------------
extern "C" int atsc_pair_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp_x, const uint8_t *d_body_x, const atsc_dplan *dp_y,
                                     const uint8_t *d_body_y, uint64_t n_windows, const uint64_t *begin,
                                     const uint64_t *count, atsc_window_pair *d_out, void *stream)
{
    ATSC_API_BEGIN
    const QueryInput in[2] = {{dp_x, d_body_x, 0}, {dp_y, d_body_y, 0}};
    return PairQuery().dev(ctx, in, n_windows, begin, count, d_out, stream);
    ATSC_API_END
}

extern "C" int atsc_pair_windows(atsc_ctx *ctx, const uint8_t *body_x, uint64_t len_x, int has_count_x, const uint8_t *body_y,
                                 uint64_t len_y, int has_count_y, uint64_t n_windows, const uint64_t *begin,
                                 const uint64_t *count, atsc_window_pair *out)
{
    ATSC_API_BEGIN
    const HostBody hb[2] = {{body_x, len_x, has_count_x}, {body_y, len_y, has_count_y}};
    return query_host(ctx, hb, n_windows, begin, count, out, PairQuery());
    ATSC_API_END
}

// Host only: what a caller reads off the pair moments.  Each line is one rounded operation, as include/atsc_hip.h states it.
extern "C" int atsc_pair_fit(const atsc_window_pair *p, uint64_t n, atsc_window_pair_fit *out)
{
    if (n && (!p || !out)) return ATSC_E_INVALID;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint64_t i = 0; i < n; ++i) {
        const atsc_window_pair &a = p[i];
        atsc_window_pair_fit &r = out[i];
        if (a.count == 0) {
            r.covariance = r.sample_covariance = r.correlation = r.slope = r.intercept = r.r2 = r.mean_diff = nan;
            continue;
        }
        r.covariance = a.c_xy / (double)a.count;
        r.sample_covariance = a.count < 2 ? nan : a.c_xy / (double)(a.count - 1);
        if (a.m2_x > 0.0 && a.m2_y > 0.0) {
            const double sx = std::sqrt(a.m2_x), sy = std::sqrt(a.m2_y);
            const double c = (a.c_xy / sx) / sy;
            r.correlation = c > 1.0 ? 1.0 : c < -1.0 ? -1.0 : c;  // (a NaN stays)
        } else {
            r.correlation = nan;
        }
        r.slope = a.m2_x > 0.0 ? a.c_xy / a.m2_x : nan;
        const double sm = r.slope * a.mean_x;
        r.intercept = a.mean_y - sm;
        r.r2 = r.correlation * r.correlation;
        r.mean_diff = a.mean_x - a.mean_y;
    }
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// windowed deltas: counted pairs, rises, falls, their sums and largest steps of sample windows (atsc_delta.hip)
// ------------------------------------------------------------------------------------------
extern "C" int atsc_delta_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                      const uint64_t *begin, const uint64_t *count, atsc_window_delta *d_out, void *stream)
{
    ATSC_API_BEGIN
    return DltQuery().dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_delta_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                  const uint64_t *begin, const uint64_t *count, atsc_window_delta *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, DltQuery());
    ATSC_API_END
}

// Host only: what a caller reads off the deltas.  Each line is one rounded operation, as include/atsc_hip.h states it.
extern "C" int atsc_delta_derive(const atsc_window_delta *d, uint64_t n, atsc_window_delta_fit *out)
{
    if (n && (!d || !out)) return ATSC_E_INVALID;
    for (uint64_t i = 0; i < n; ++i) {
        const atsc_window_delta &a = d[i];
        atsc_window_delta_fit &r = out[i];
        r.changes = a.rises + a.falls;
        r.variation = a.up + a.down;
        r.net = a.up - a.down;
        r.increase = a.up + a.after_falls;
        r.mean_step = a.pairs ? r.variation / (double)a.pairs : std::numeric_limits<double>::quiet_NaN();
    }
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// windowed runs: the samples that meet a condition and the runs of adjacent ones among them (atsc_runs.hip)
// ------------------------------------------------------------------------------------------
extern "C" int atsc_runs_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                     const uint64_t *begin, const uint64_t *count, int op, double limit,
                                     atsc_window_runs *d_out, void *stream)
{
    ATSC_API_BEGIN
    return RunQuery{op, limit}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_runs_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                 const uint64_t *begin, const uint64_t *count, int op, double limit, atsc_window_runs *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, RunQuery{op, limit});
    ATSC_API_END
}

// Host only: the records of adjacent windows, left to right, into the record of their union (include/atsc_hip.h's rule).
extern "C" int atsc_runs_merge(const atsc_window_runs *r, uint64_t n, atsc_window_runs *out)
{
    if (!out || (n && !r)) return ATSC_E_INVALID;
    atsc_window_runs a;
    run_empty_record(a);
    for (uint64_t i = 0; i < n; ++i) {
        const atsc_window_runs &b = r[i];
        if (b.samples == 0) continue;
        if (a.samples == 0) { a = b; continue; }
        const uint64_t o = a.samples;
        const bool join = a.tail && b.head;
        if (join && a.tail + b.head > a.longest) { a.longest = a.tail + b.head; a.longest_at = o - a.tail; }
        if (b.longest > a.longest) { a.longest = b.longest; a.longest_at = b.longest_at + o; }
        a.runs = a.runs + b.runs - (join ? 1 : 0);
        if (a.head == a.samples) a.head = a.samples + b.head;
        a.tail = b.tail == b.samples ? b.samples + a.tail : b.tail;
        if (!a.inside) a.first_at = b.inside ? b.first_at + o : ATSC_RUNS_NONE;
        if (b.inside) a.last_at = b.last_at + o;
        a.samples += b.samples;
        a.inside += b.inside;
        a.excess = a.excess + b.excess;
    }
    *out = a;
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// windowed extremes: the k largest and the k smallest samples of sample windows and where they are (atsc_extremes.hip)
// ------------------------------------------------------------------------------------------
extern "C" int atsc_extremes_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                         const uint64_t *begin, const uint64_t *count, uint32_t k, void *d_out,
                                         void *stream)
{
    ATSC_API_BEGIN
    return ExtQuery{k}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_extremes_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                     const uint64_t *begin, const uint64_t *count, uint32_t k, void *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, ExtQuery{k});
    ATSC_API_END
}

// Host only: the records of adjacent windows, left to right, into the record of their union (include/atsc_hip.h's rule).
// A list of the union is the first k of its parts' lists merged in the list's order; a part's entries are in that order
// already, and of equal values the earlier part's come first, so taking from the merged list so far unless the next
// part's head is strictly better keeps the earliest position in front.
extern "C" int atsc_extremes_merge(const void *records, uint64_t n, uint32_t k, void *out)
{
    if (!out || (n && !records) || k == 0 || k > ATSC_EXTREMES_MAX_K) return ATSC_E_INVALID;
    const size_t bytes = ATSC_EXTREMES_BYTES(k);
    alignas(8) unsigned char acc[ATSC_EXTREMES_BYTES(ATSC_EXTREMES_MAX_K)], next[ATSC_EXTREMES_BYTES(ATSC_EXTREMES_MAX_K)];
    ext_empty_record(acc, k);
    atsc_window_extremes_head *a = (atsc_window_extremes_head *)acc;
    for (uint64_t i = 0; i < n; ++i) {
        alignas(8) unsigned char part[ATSC_EXTREMES_BYTES(ATSC_EXTREMES_MAX_K)];
        memcpy(part, (const char *)records + i * bytes, bytes);
        const atsc_window_extremes_head *b = (const atsc_window_extremes_head *)part;
        if (b->count == 0) continue;
        ext_empty_record(next, k);
        for (int end = 0; end < 2; ++end) {
            const atsc_extreme *la = (const atsc_extreme *)(a + 1) + end * k, *lb = (const atsc_extreme *)(b + 1) + end * k;
            atsc_extreme *lo = (atsc_extreme *)((atsc_window_extremes_head *)next + 1) + end * k;
            uint32_t ia = 0, ib = 0;
            for (uint32_t j = 0; j < k; ++j) {
                const bool ha = ia < k && la[ia].at != ATSC_EXTREMES_NONE, hb = ib < k && lb[ib].at != ATSC_EXTREMES_NONE;
                if (!ha && !hb) break;
                const bool take_b = hb && (!ha || (end ? lb[ib].value < la[ia].value : lb[ib].value > la[ia].value));
                if (take_b) {
                    lo[j].value = lb[ib].value;
                    lo[j].at = lb[ib++].at + a->count;
                } else {
                    lo[j] = la[ia++];
                }
            }
        }
        atsc_window_extremes_head *nh = (atsc_window_extremes_head *)next;
        nh->count = a->count + b->count;
        nh->nans = a->nans + b->nans;
        memcpy(acc, next, bytes);
    }
    memcpy(out, acc, bytes);
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// windowed value counts: the k smallest distinct values of sample windows and how often each occurs (atsc_values.hip)
// ------------------------------------------------------------------------------------------
extern "C" int atsc_values_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                       const uint64_t *begin, const uint64_t *count, uint32_t k, double above, void *d_out,
                                       void *stream)
{
    ATSC_API_BEGIN
    return ValQuery{k, above}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_values_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                   const uint64_t *begin, const uint64_t *count, uint32_t k, double above, void *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, ValQuery{k, above});
    ATSC_API_END
}

// Host only: the records of pairwise disjoint windows into the record of their union (include/atsc_hip.h's rule and
// its argument).  The heads add; the lists merge by value, the n of equal values added, and the result is cut at k.
extern "C" int atsc_values_merge(const void *records, uint64_t n, uint32_t k, void *out)
{
    if (!out || (n && !records) || k == 0 || k > ATSC_VALUES_MAX_K) return ATSC_E_INVALID;
    const size_t bytes = ATSC_VALUES_BYTES(k);
    alignas(8) unsigned char acc[ATSC_VALUES_BYTES(ATSC_VALUES_MAX_K)], next[ATSC_VALUES_BYTES(ATSC_VALUES_MAX_K)];
    val_empty_record(acc, k);
    atsc_window_values_head *a = (atsc_window_values_head *)acc;
    for (uint64_t i = 0; i < n; ++i) {
        alignas(8) unsigned char part[ATSC_VALUES_BYTES(ATSC_VALUES_MAX_K)];
        memcpy(part, (const char *)records + i * bytes, bytes);
        const atsc_window_values_head *b = (const atsc_window_values_head *)part;
        if (b->count == 0) continue;
        val_empty_record(next, k);
        atsc_window_values_head *nh = (atsc_window_values_head *)next;
        const atsc_value_count *la = (const atsc_value_count *)(a + 1), *lb = (const atsc_value_count *)(b + 1);
        atsc_value_count *lo = (atsc_value_count *)(nh + 1);
        const uint32_t na = std::min(a->distinct, k), nb = std::min(b->distinct, k);
        uint32_t ia = 0, ib = 0, j = 0;
        for (; j < k && (ia < na || ib < nb); ++j) {
            const bool ta = ia < na && (ib == nb || la[ia].value <= lb[ib].value);
            const bool tb = ib < nb && (ia == na || lb[ib].value <= la[ia].value);
            lo[j].value = ta ? la[ia].value : lb[ib].value;  // (of the zeros only +0.0 is ever listed)
            lo[j].n = (ta ? la[ia].n : 0) + (tb ? lb[ib].n : 0);
            ia += ta;
            ib += tb;
        }
        nh->count = a->count + b->count;
        nh->nans = a->nans + b->nans;
        nh->below = a->below + b->below;
        nh->distinct = j;
        nh->more = (ia < na || ib < nb || a->more || b->more) ? 1 : 0;
        memcpy(acc, next, bytes);
    }
    memcpy(out, acc, bytes);
    return ATSC_OK;
}

// Host only: the listed entry with the largest n of every record, of equal n the smallest value.
extern "C" int atsc_values_mode(const void *records, uint64_t n, uint32_t k, atsc_value_mode *out)
{
    if ((n && (!records || !out)) || k == 0 || k > ATSC_VALUES_MAX_K) return ATSC_E_INVALID;
    for (uint64_t i = 0; i < n; ++i) {
        alignas(8) unsigned char rec[ATSC_VALUES_BYTES(ATSC_VALUES_MAX_K)];
        memcpy(rec, (const char *)records + i * ATSC_VALUES_BYTES(k), ATSC_VALUES_BYTES(k));
        const atsc_window_values_head *h = (const atsc_window_values_head *)rec;
        const atsc_value_count *e = (const atsc_value_count *)(h + 1);
        atsc_value_mode r;
        r.value = std::numeric_limits<double>::quiet_NaN();
        r.n = 0;
        r.exact = h->more == 0;
        r.pad = 0;
        for (uint32_t j = 0; j < std::min(h->distinct, k); ++j)
            if (e[j].n > r.n) { r.value = e[j].value; r.n = e[j].n; }
        out[i] = r;
    }
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// windowed quantiles: exact order statistics of sample windows (atsc_quantile.hip)
// ------------------------------------------------------------------------------------------
// ctx may be null: then no message is kept
// (the levels and the method of the windowed quantiles and of the across quantiles; `call` names the caller in the message)
static int quantile_check_levels(atsc_ctx *ctx, const char *call, uint32_t n_q, const double *q, int method)
{
    if (!q) return fail_in(ctx, ATSC_E_INVALID, call, "null argument");
    if (n_q == 0 || n_q > QNT_MAX_LEVELS) return fail_in(ctx, ATSC_E_INVALID, call, "n_q outside [1, 64]");
    for (uint32_t j = 0; j < n_q; ++j)
        if (!(q[j] >= 0.0 && q[j] <= 1.0)) return fail_in(ctx, ATSC_E_INVALID, call, "a level is NaN or outside [0, 1]");
    if (method < ATSC_QUANTILE_LINEAR || method > ATSC_QUANTILE_NEAREST) return fail_in(ctx, ATSC_E_INVALID, call, "unknown method");
    return ATSC_OK;
}

// The device call.  Every window is held whole in scratch: the windows, by begin, go into pieces of at most L samples
// (a piece starts at the first window not yet placed and takes every unplaced window that ends within L of that
// start; pieces overlap where windows do).  Per piece: the decode tasks of its windows' union (emit_piece_decode), then
// the tiers by window length: short and medium windows one launch each (medium: one per power-of-two key count), long
// windows QNT_PASSES histogram + pick launches whatever their number.  Everything goes up in one copy; nothing waits
// on the host between pieces.  org: the stream index of the plan's first sample (see reduce_dev).
static int quantile_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                        const uint64_t *begin, const uint64_t *count, uint32_t n_q, const double *q, int method,
                        double *d_out, void *stream, uint64_t org)
{
    if (!ctx || !dp || (n_windows && (!d_body || !begin || !count || !d_out)))
        return fail(ctx, ATSC_E_INVALID, "quantile_windows: null argument");
    int rc = quantile_check_levels(ctx, "quantile_windows", n_q, q, method);
    if (rc) return rc;
    rc = check_windows(ctx, "quantile_windows", dp, d_out, "d_out", n_windows, begin, count, 0xfffffffeull);
    if (rc || n_windows == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !launch_qnt_short || !launch_qnt_medium || !launch_qnt_hist ||
        !launch_qnt_pick)
        return fail(ctx, ATSC_E_UNSUPPORTED, "quantile_windows: no quantile kernels");
    const uint64_t W = n_windows;
    std::vector<uint32_t> ord;  // the non-empty windows by begin
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i)
        if (count[i]) { ord.push_back((uint32_t)i); cov.emplace_back(org + begin[i], org + begin[i] + count[i]); }
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return begin[a] < begin[b]; });
    merge_spans(cov);
    uint64_t spill;
    const uint64_t L = piece_samples(ctx, dp, org, cov, 1, &spill);
    for (uint32_t i : ord) {
        if (count[i] <= L && count[i] < (1ull << 32)) continue;
        char msg[192];
        if (count[i] >= (1ull << 32))
            snprintf(msg, sizeof msg, "quantile_windows: window %u holds %llu samples, more than 2^32 - 1", i,
                     (unsigned long long)count[i]);
        else
            snprintf(msg, sizeof msg,
                     "quantile_windows: window %u (%llu samples) does not fit one scratch piece; an aggregate scratch "
                     "budget of %llu bytes would hold it", i, (unsigned long long)count[i],
                     (unsigned long long)((count[i] + spill) * sizeof(double)));
        return fail(ctx, ATSC_E_CAPACITY, msg);
    }
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // pieces: windows ord[w_at, w_at + w_n) of pw, samples [S0, S1) of the stream at scratch[0, S1 - S0)
    struct Piece {
        uint64_t S0, S1;
        size_t w_at, w_n;
    };
    std::vector<Piece> pcs;
    std::vector<uint32_t> pw;
    pw.reserve(ord.size());
    {
        std::vector<char> placed(ord.size(), 0);
        size_t a = 0;
        while (a < ord.size()) {
            Piece pc{org + begin[ord[a]], 0, pw.size(), 0};
            pc.S1 = pc.S0;
            for (size_t k = a; k < ord.size() && org + begin[ord[k]] < pc.S0 + L; ++k) {
                const uint64_t e = org + begin[ord[k]] + count[ord[k]];
                if (placed[k] || e > pc.S0 + L) continue;
                placed[k] = 1;
                pw.push_back(ord[k]);
                pc.S1 = std::max(pc.S1, e);
            }
            pc.w_n = pw.size() - pc.w_at;
            pcs.push_back(pc);
            while (a < ord.size() && placed[a]) ++a;
        }
    }
    uint64_t region = 0;
    for (const Piece &pc : pcs) region = std::max(region, pc.S1 - pc.S0);
    // per piece: decode tasks, then the windows by tier
    const uint32_t n_med = 6;  // medium key counts 2^9 .. 2^14 (the ones up to QNT_MEDIUM_MAX are used)
    struct PieceQ {
        size_t short_at, med_at[n_med], long_at, chunk_at;
        uint32_t short_n, med_n[n_med], long_n, chunk_n;
    };
    std::vector<PieceDecode> pdec(pcs.size());
    std::vector<PieceQ> pq(pcs.size());
    DecodeTasks D;
    std::vector<DevQTask> shorts, meds, longs;
    std::vector<DevQTask> med_class[n_med];
    std::vector<DevQChunk> chunks;
    std::vector<Span> pcov;
    uint32_t max_long = 0;
    for (size_t p = 0; p < pcs.size(); ++p) {
        const Piece &pc = pcs[p];
        pcov.clear();  // the piece's windows come by begin: merged as they come
        for (size_t k = pc.w_at; k < pc.w_at + pc.w_n; ++k) {
            const Span x(org + begin[pw[k]], org + begin[pw[k]] + count[pw[k]]);
            if (pcov.empty() || !absorb_span(pcov.back(), x)) pcov.push_back(x);
        }
        size_t ci = 0;
        if (!emit_piece_decode(dp, org, pcov, ci, pc.S0, pc.S1, region, D, pdec[p]))
            return fail(ctx, ATSC_E_INVALID, "quantile_windows: internal error (spill slots)");
        PieceQ &t = pq[p];
        t.short_at = shorts.size();
        t.long_at = longs.size();
        t.chunk_at = chunks.size();
        for (uint32_t c = 0; c < n_med; ++c) med_class[c].clear();
        for (size_t k = pc.w_at; k < pc.w_at + pc.w_n; ++k) {
            const uint32_t i = pw[k];
            const uint64_t src = org + begin[i] - pc.S0, n = count[i];
            if (n <= QNT_SHORT_MAX) {
                shorts.push_back(DevQTask{src, n, i, 0});
            } else if (n <= QNT_MEDIUM_MAX) {
                uint32_t c = 0;
                while ((512ull << c) < n) ++c;
                med_class[c].push_back(DevQTask{src, n, i, 0});
            } else {
                const uint32_t slot = (uint32_t)(longs.size() - t.long_at);
                longs.push_back(DevQTask{src, n, i, slot});
                for (uint64_t o = 0; o < n; o += QNT_CHUNK)
                    chunks.push_back(DevQChunk{src + o, (uint32_t)std::min<uint64_t>(QNT_CHUNK, n - o), slot});
            }
        }
        for (uint32_t c = 0; c < n_med; ++c) {
            t.med_at[c] = meds.size();
            t.med_n[c] = (uint32_t)med_class[c].size();
            meds.insert(meds.end(), med_class[c].begin(), med_class[c].end());
        }
        t.short_n = (uint32_t)(shorts.size() - t.short_at);
        t.long_n = (uint32_t)(longs.size() - t.long_at);
        t.chunk_n = (uint32_t)(chunks.size() - t.chunk_at);
        max_long = std::max(max_long, t.long_n);
    }
    // empty windows: NaN from the short tier, once
    const size_t empty_at = shorts.size();
    for (uint64_t i = 0; i < W; ++i)
        if (!count[i]) shorts.push_back(DevQTask{0, 0, (uint32_t)i, 0});
    const uint32_t empty_n = (uint32_t)(shorts.size() - empty_at);
    QueryRes &R = dp->res[Q_QUANTILE];
    HIPCHK(ctx, R.wait());
    // one upload: the decode tasks, the levels, the tiers' task lists, the chunks; behind them (device only) the long
    // tier's state and counts
    const uint32_t rows = 2 * n_q;
    Upload up;
    D.place(up);
    const size_t off_q = up.add(q, n_q * sizeof(double)), off_short = up.add(shorts), off_med = up.add(meds),
                 off_long = up.add(longs), off_chunk = up.add(chunks);
    const size_t hist_bytes = (size_t)max_long * rows * 256 * sizeof(uint32_t);
    const size_t off_state = up.device_only((size_t)max_long * sizeof(DevQState)), off_hist = up.device_only(hist_bytes);
    rc = stage_upload(ctx, R, up, std::max<uint64_t>(1, region + (uint64_t)MAX_FRAME * D.spills_used), s);
    if (rc) return rc;
    unsigned char *d = R.d;
    if (hist_bytes) HIPCHK(ctx, hipMemsetAsync(d + off_hist, 0, hist_bytes, s));  // k_qnt_pick clears what it reads
    double *scr = R.scratch;
    const double *dq = (const double *)(d + off_q);
    const DevQTask *d_short = (const DevQTask *)(d + off_short), *d_med = (const DevQTask *)(d + off_med),
                   *d_long = (const DevQTask *)(d + off_long);
    const DevQChunk *d_chunk = (const DevQChunk *)(d + off_chunk);
    DevQState *st = (DevQState *)(d + off_state);
    uint32_t *hist = (uint32_t *)(d + off_hist);
    LAUNCHCHK(ctx, "launch k_qnt_short", launch_qnt_short(d_short + empty_at, empty_n, scr, dq, n_q, method, d_out, s));
    for (size_t p = 0; p < pcs.size(); ++p) {
        rc = launch_piece_decode(ctx, dp, d_body, d, D, pdec[p], scr, scr, scr, s, BY_QUANTILE);
        if (rc) return rc;
        const PieceQ &t = pq[p];
        LAUNCHCHK(ctx, "launch k_qnt_short", launch_qnt_short(d_short + t.short_at, t.short_n, scr, dq, n_q, method, d_out, s));
        for (uint32_t c = 0; c < n_med; ++c)
            LAUNCHCHK(ctx, "launch k_qnt_medium",
                      launch_qnt_medium(d_med + t.med_at[c], t.med_n[c], 512u << c, scr, dq, n_q, method, d_out, s));
        if (!t.long_n) continue;
        for (uint32_t pass = 0; pass < QNT_PASSES; ++pass) {
            LAUNCHCHK(ctx, "launch k_qnt_hist", launch_qnt_hist(d_chunk + t.chunk_at, t.chunk_n, scr, st, hist, rows, pass, s));
            LAUNCHCHK(ctx, "launch k_qnt_pick",
                      launch_qnt_pick(d_long + t.long_at, t.long_n, st, hist, rows, pass, dq, n_q, method, d_out, s));
        }
    }
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// the quantiles' descriptor (see AggQuery): the levels and the method are the call's parameters
struct QntQuery {
    static constexpr int INPUTS = 1;
    static constexpr const char *CALL = "quantile_windows";
    uint32_t n_q;
    const double *q;
    int method;
    size_t out_bytes(uint64_t n) const { return n * n_q * sizeof(double); }
    int check(atsc_ctx *ctx) const { return quantile_check_levels(ctx, CALL, n_q, q, method); }
    void fill_empty(void *out, uint64_t n) const
    {
        for (uint64_t i = 0; i < n * n_q; ++i) ((double *)out)[i] = std::numeric_limits<double>::quiet_NaN();
    }
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        return quantile_dev(ctx, dp, d_body, n_windows, begin, count, n_q, q, method, (double *)d_res, stream, org);
    }
};

extern "C" int atsc_quantile_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                         const uint64_t *begin, const uint64_t *count, uint32_t n_q, const double *q,
                                         int method, double *d_out, void *stream)
{
    ATSC_API_BEGIN
    return QntQuery{n_q, q, method}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_quantile_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                     const uint64_t *begin, const uint64_t *count, uint32_t n_q, const double *q, int method,
                                     double *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, QntQuery{n_q, q, method});
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// windowed histograms: per-window counts of the samples over value bins (atsc_histogram.hip)
// ------------------------------------------------------------------------------------------
// Covering intervals closer than this share a span of pieces, as the aggregates' AGG_GAP_TILES tiles
static const uint64_t HST_GAP = 64ull * AGG_TILE;

// ctx may be null: then no message is kept; `call` names the caller in the message
static int histogram_check_edges(atsc_ctx *ctx, uint32_t n_edges, const double *edges, int closed,
                                 const char *call = "histogram_windows")
{
    if (!edges) return fail_in(ctx, ATSC_E_INVALID, call, "null argument");
    if (n_edges == 0 || n_edges > HST_MAX_EDGES) return fail_in(ctx, ATSC_E_INVALID, call, "n_edges outside [1, 1024]");
    for (uint32_t j = 0; j < n_edges; ++j)
        if (edges[j] != edges[j]) return fail_in(ctx, ATSC_E_INVALID, call, "an edge is NaN");
    for (uint32_t j = 1; j < n_edges; ++j)
        if (!(edges[j - 1] < edges[j])) return fail_in(ctx, ATSC_E_INVALID, call, "edges are not strictly ascending");
    if (closed != ATSC_HIST_LEFT_CLOSED && closed != ATSC_HIST_RIGHT_CLOSED)
        return fail_in(ctx, ATSC_E_INVALID, call, "unknown closed");
    return ATSC_OK;
}

extern "C" int atsc_histogram_edges_uniform(double lo, double hi, uint32_t n_bins, double *edges)
{
    if (!edges || !(lo - lo == 0.0) || !(hi - hi == 0.0) || !(hi > lo)) return ATSC_E_INVALID;
    if (n_bins == 0 || n_bins >= HST_MAX_EDGES) return ATSC_E_INVALID;
    const double step = (hi - lo) / (double)n_bins;
    if (!(step > 0.0)) return ATSC_E_INVALID;
    double e[HST_MAX_EDGES];
    for (uint32_t k = 0; k < n_bins; ++k) e[k] = (double)k * step + lo;
    e[n_bins] = hi;
    for (uint32_t k = 0; k < n_bins; ++k)
        if (!(e[k] < e[k + 1])) return ATSC_E_INVALID;  // a width of a few ulps of lo, or a step that overflowed
    memcpy(edges, e, ((size_t)n_bins + 1) * sizeof(double));
    return ATSC_OK;
}

// The device call.  Host work: covering intervals; spans of them cut into pieces of at most one scratch piece, at any
// sample; the decode tasks of every piece (emit_piece_decode); per window and touched piece, the window's stretch
// inside the piece cut into tasks of at most HST_CHUNK samples (a task of at most HST_SHORT_MAX samples goes to the
// one-wavefront tier, so a call of many short windows is one launch of few workgroups).  A window with a single task
// owns its row (HST_OWN: stored whole); when any window has none or several, the result is cleared first and the
// tasks add.  Everything, the edges included, goes up in one copy; nothing waits on the host between pieces.
// org: the stream index of the plan's first sample (see reduce_dev).
static int histogram_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                         const uint64_t *begin, const uint64_t *count, uint32_t n_edges, const double *edges, int closed,
                         uint64_t *d_out, void *stream, uint64_t org)
{
    if (!ctx || !dp || (n_windows && (!d_body || !begin || !count || !d_out)))
        return fail(ctx, ATSC_E_INVALID, "histogram_windows: null argument");
    int rc = histogram_check_edges(ctx, n_edges, edges, closed);
    if (rc) return rc;
    rc = check_windows(ctx, "histogram_windows", dp, d_out, "d_out", n_windows, begin, count, 0xfffffffeull);
    if (rc || n_windows == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !launch_hst_short || !launch_hst_chunk)
        return fail(ctx, ATSC_E_UNSUPPORTED, "histogram_windows: no histogram kernels");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t W = n_windows, rows = (uint64_t)n_edges + 2;
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i)
        if (count[i]) cov.emplace_back(org + begin[i], org + begin[i] + count[i]);
    if (cov.empty()) {  // only empty windows
        HIPCHK(ctx, hipMemsetAsync(d_out, 0, W * rows * sizeof(uint64_t), s));
        return ATSC_OK;
    }
    bool all_own = cov.size() == W;
    merge_spans(cov);
    uint64_t spill;
    const uint64_t L = piece_samples(ctx, dp, org, cov, 1, &spill);
    // pieces: samples [S0, S1) of the stream at scratch[0, S1 - S0), ascending and disjoint
    std::vector<Span> pcs;
    const uint64_t region = cut_pieces(cov, 1, L, HST_GAP, pcs);
    // tasks, by tier: a window cut by a piece boundary gets tasks on each side
    using PT = Placed<DevHistTask>;
    std::vector<PT> tk[2];  // 0: short, 1: chunk
    tk[0].reserve(W);
    for (uint64_t i = 0; i < W; ++i) {
        if (!count[i]) continue;
        const uint64_t b = org + begin[i], e = b + count[i];
        size_t p = (size_t)(std::upper_bound(pcs.begin(), pcs.end(), b, [](uint64_t v, const Span &x) { return v < x.second; }) -
                            pcs.begin());
        uint32_t n_tasks = 0;
        PT *last = nullptr;
        for (; p < pcs.size() && pcs[p].first < e; ++p) {
            const uint64_t lo = std::max(b, pcs[p].first), hi = std::min(e, pcs[p].second);
            for (uint64_t o = lo; o < hi; o += HST_CHUNK) {
                const uint32_t len = (uint32_t)std::min<uint64_t>(HST_CHUNK, hi - o);
                std::vector<PT> &v = tk[len <= HST_SHORT_MAX ? 0 : 1];
                v.push_back(PT{(uint32_t)p, DevHistTask{o - pcs[p].first, len, (uint32_t)i}});
                last = &v.back();
                ++n_tasks;
            }
        }
        if (n_tasks == 1) last->t.len |= HST_OWN;
        else all_own = false;
    }
    const size_t P = pcs.size();
    std::vector<DevHistTask> tasks[2];
    std::vector<size_t> at[2];
    for (int k = 0; k < 2; ++k) {
        group_tasks(tk[k], P, tasks[k], at[k]);
        for (size_t p = 0; p < P; ++p)
            if (at[k][p + 1] - at[k][p] > 0x7fffffffull)
                return fail(ctx, ATSC_E_INVALID, "histogram_windows: more than 2^31 - 1 tasks in a piece");
    }
    // decode tasks of every piece
    std::vector<PieceDecode> pdec;
    DecodeTasks D;
    rc = emit_pieces_decode(ctx, "histogram_windows", dp, org, cov, pcs, 1, region, D, pdec);
    if (rc) return rc;
    QueryRes &R = dp->res[Q_HISTOGRAM];
    HIPCHK(ctx, R.wait());
    // one upload: the decode tasks, the edges, the two tiers' task lists
    Upload up;
    D.place(up);
    const size_t off_edges = up.add(edges, n_edges * sizeof(double)), off_short = up.add(tasks[0]), off_chunk = up.add(tasks[1]);
    rc = stage_upload(ctx, R, up, std::max<uint64_t>(1, region + (uint64_t)MAX_FRAME * D.spills_used), s);
    if (rc) return rc;
    unsigned char *d = R.d;
    if (!all_own) HIPCHK(ctx, hipMemsetAsync(d_out, 0, W * rows * sizeof(uint64_t), s));
    double *scr = R.scratch;
    const double *d_edges = (const double *)(d + off_edges);
    const DevHistTask *d_short = (const DevHistTask *)(d + off_short), *d_chunk = (const DevHistTask *)(d + off_chunk);
    for (size_t p = 0; p < P; ++p) {
        rc = launch_piece_decode(ctx, dp, d_body, d, D, pdec[p], scr, scr, scr, s, BY_HISTOGRAM);
        if (rc) return rc;
        LAUNCHCHK(ctx, "launch k_hst_short",
                  launch_hst_short(d_short + at[0][p], (uint32_t)(at[0][p + 1] - at[0][p]), scr, d_edges, n_edges, closed, d_out, s));
        LAUNCHCHK(ctx, "launch k_hst_chunk",
                  launch_hst_chunk(d_chunk + at[1][p], (uint32_t)(at[1][p + 1] - at[1][p]), scr, d_edges, n_edges, closed, d_out, s));
    }
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// the histograms' descriptor (see AggQuery): the edges and the closed side are the call's parameters
struct HstQuery {
    static constexpr int INPUTS = 1;
    static constexpr const char *CALL = "histogram_windows";
    uint32_t n_edges;
    const double *edges;
    int closed;
    size_t out_bytes(uint64_t n) const { return n * ((size_t)n_edges + 2) * sizeof(uint64_t); }
    int check(atsc_ctx *ctx) const { return histogram_check_edges(ctx, n_edges, edges, closed); }
    void fill_empty(void *out, uint64_t n) const
    {
        if (n) memset(out, 0, out_bytes(n));
    }
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        return histogram_dev(ctx, dp, d_body, n_windows, begin, count, n_edges, edges, closed, (uint64_t *)d_res, stream, org);
    }
};

extern "C" int atsc_histogram_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                          const uint64_t *begin, const uint64_t *count, uint32_t n_edges,
                                          const double *edges, int closed, uint64_t *d_out, void *stream)
{
    ATSC_API_BEGIN
    return HstQuery{n_edges, edges, closed}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_histogram_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                      const uint64_t *begin, const uint64_t *count, uint32_t n_edges, const double *edges,
                                      int closed, uint64_t *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, HstQuery{n_edges, edges, closed});
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// windowed select: the samples of sample windows that meet a condition, and where they are (atsc_select.hip)
// ------------------------------------------------------------------------------------------
// ctx may be null: then no message is kept
static int select_check(atsc_ctx *ctx, int op, double limit)
{
    if (op < ATSC_RUNS_GT || op > ATSC_RUNS_NE) return fail(ctx, ATSC_E_INVALID, "select_windows: unknown op");
    if (std::isnan(limit)) return fail(ctx, ATSC_E_INVALID, "select_windows: limit is NaN");
    return ATSC_OK;
}

// The device call.  Host work: covering intervals and pieces as histogram_dev's; per window, in the order given, and per
// touched piece, the window's stretch inside the piece cut into tasks of at most SEL_TASK samples, numbered as they come:
// a task's slot is its place in (window, position) order, and first[i] the slot of window i's first task (an empty
// window's: the next window's; first[n_windows]: the number of tasks).  The tasks go up sorted by piece, so that every
// piece's are one launch.  Then count per piece into cnt[slot], one scan over cnt[] in slot order, the windows' offsets
// off it, and the write step per piece.  A call whose windows fit one piece writes from the samples the count step left
// in the scratch; a call of several pieces decodes each piece a second time for the write step.  cap == 0 has no write
// step.  Everything goes up in one copy; nothing waits on the host between the steps.
// The scratch is one slot longer than its longest piece: the task kernels load pairs of slots from an even slot on.
// org: the stream index of the plan's first sample (see reduce_dev).
static int select_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
                      const uint64_t *count, int op, double limit, uint64_t cap, void *d_out, void *stream, uint64_t org)
{
    if (!ctx || !dp || (n_windows && (!d_body || !begin || !count || !d_out)))
        return fail(ctx, ATSC_E_INVALID, "select_windows: null argument");
    int rc = select_check(ctx, op, limit);
    if (rc) return rc;
    rc = check_windows(ctx, "select_windows", dp, d_out, "d_out", n_windows, begin, count, 0xfffffffeull);
    if (rc || n_windows == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !launch_sel_count || !launch_sel_scan || !launch_sel_offsets ||
        !launch_sel_write)
        return fail(ctx, ATSC_E_UNSUPPORTED, "select_windows: no select kernels");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t W = n_windows;
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i)
        if (count[i]) cov.emplace_back(org + begin[i], org + begin[i] + count[i]);
    if (cov.empty()) {  // only empty windows
        HIPCHK(ctx, hipMemsetAsync(d_out, 0, (W + 1) * sizeof(uint64_t), s));
        return ATSC_OK;
    }
    merge_spans(cov);
    uint64_t spill;
    const uint64_t L = piece_samples(ctx, dp, org, cov, 1, &spill);
    // pieces: samples [S0, S1) of the stream at scratch[0, S1 - S0), ascending and disjoint
    std::vector<Span> pcs;
    uint64_t region = cut_pieces(cov, 1, L, HST_GAP, pcs);
    region += 1;  // the pair load's slot behind a piece's last sample
    const size_t P = pcs.size();
    // tasks in (window, position) order
    std::vector<Placed<DevSelTask>> tk;
    tk.reserve(W);
    std::vector<uint32_t> first(W + 1);
    uint64_t n_tasks = 0;
    for (uint64_t i = 0; i < W; ++i) {
        first[i] = (uint32_t)n_tasks;
        if (!count[i]) continue;
        const uint64_t b = org + begin[i], e = b + count[i];
        size_t p = (size_t)(std::upper_bound(pcs.begin(), pcs.end(), b, [](uint64_t v, const Span &x) { return v < x.second; }) -
                            pcs.begin());
        for (; p < P && pcs[p].first < e; ++p) {
            const uint64_t lo = std::max(b, pcs[p].first), hi = std::min(e, pcs[p].second);
            for (uint64_t o = lo; o < hi; o += SEL_TASK) {
                if (n_tasks >= 0x7fffffffull) return fail(ctx, ATSC_E_INVALID, "select_windows: more than 2^31 - 1 tasks");
                tk.push_back({(uint32_t)p, DevSelTask{o - pcs[p].first, o - b, (uint32_t)std::min<uint64_t>(SEL_TASK, hi - o),
                                                      (uint32_t)n_tasks++}});
            }
        }
    }
    first[W] = (uint32_t)n_tasks;
    std::vector<DevSelTask> tasks;
    std::vector<size_t> at;
    group_tasks(tk, P, tasks, at);
    // decode tasks of every piece
    std::vector<PieceDecode> pdec;
    DecodeTasks D;
    rc = emit_pieces_decode(ctx, "select_windows", dp, org, cov, pcs, 1, region, D, pdec);
    if (rc) return rc;
    QueryRes &R = dp->res[Q_SELECT];
    HIPCHK(ctx, R.wait());
    // one upload: the decode tasks, the select tasks, the windows' first slots; behind them (device only) the counts,
    // one more than the tasks for the total, and the scan's block sums
    Upload up;
    D.place(up);
    const size_t off_tasks = up.add(tasks), off_first = up.add(first);
    const size_t off_cnt = up.device_only((n_tasks + 1) * sizeof(uint64_t));
    const size_t off_sums = up.device_only(sel_scan_sums(n_tasks + 1) * sizeof(uint64_t));
    rc = stage_upload(ctx, R, up, region + (uint64_t)MAX_FRAME * D.spills_used, s);
    if (rc) return rc;
    unsigned char *d = R.d;
    double *scr = R.scratch;
    const DevSelTask *d_tasks = (const DevSelTask *)(d + off_tasks);
    uint64_t *cnt = (uint64_t *)(d + off_cnt);
    for (size_t p = 0; p < P; ++p) {
        rc = launch_piece_decode(ctx, dp, d_body, d, D, pdec[p], scr, scr, scr, s, BY_SELECT);
        if (rc) return rc;
        LAUNCHCHK(ctx, "launch k_sel_count", launch_sel_count(d_tasks + at[p], (uint32_t)(at[p + 1] - at[p]), scr, op, limit, cnt, s));
    }
    LAUNCHCHK(ctx, "launch k_sel_scan", launch_sel_scan(cnt, n_tasks, (uint64_t *)(d + off_sums), s));
    LAUNCHCHK(ctx, "launch k_sel_offsets", launch_sel_offsets(cnt, (const uint32_t *)(d + off_first), W + 1, (uint64_t *)d_out, s));
    for (size_t p = 0; cap && p < P; ++p) {
        if (P > 1) {  // the scratch holds the last piece: this one's samples again
            rc = launch_piece_decode(ctx, dp, d_body, d, D, pdec[p], scr, scr, scr, s, BY_SELECT);
            if (rc) return rc;
        }
        LAUNCHCHK(ctx, "launch k_sel_write",
                  launch_sel_write(d_tasks + at[p], (uint32_t)(at[p + 1] - at[p]), scr, op, limit, cnt, cap,
                                   (char *)d_out + (W + 1) * sizeof(uint64_t), s));
    }
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// the select's descriptor (see AggQuery): the condition and the entries' capacity are the call's parameters.  Its result
// is a block whose use depends on the data (BlockResult): the offsets say how many entries there are.
struct SelQuery {
    static constexpr int INPUTS = 1;
    static constexpr const char *CALL = "select_windows";
    int op;
    double limit;
    uint64_t cap;
    size_t out_bytes(uint64_t n) const { return ATSC_SELECT_BYTES(n, cap); }
    static size_t head_bytes(uint64_t n) { return ATSC_SELECT_BYTES(n, 0); }
    size_t used_bytes(const void *head, uint64_t n) const
    {
        return ATSC_SELECT_BYTES(n, std::min(((const uint64_t *)head)[n], cap));
    }
    int check(atsc_ctx *ctx) const { return select_check(ctx, op, limit); }
    static void fill_empty(void *out, uint64_t n)
    {
        if (n) memset(out, 0, head_bytes(n));
    }
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *count, void *d_res, void *stream, uint64_t org) const
    {
        return select_dev(ctx, dp, d_body, n_windows, begin, count, op, limit, cap, d_res, stream, org);
    }
};

extern "C" int atsc_select_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                       const uint64_t *begin, const uint64_t *count, int op, double limit, uint64_t cap,
                                       void *d_out, void *stream)
{
    ATSC_API_BEGIN
    return SelQuery{op, limit, cap}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_select_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                   const uint64_t *begin, const uint64_t *count, int op, double limit, uint64_t cap,
                                   void *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, SelQuery{op, limit, cap});
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// windowed rolling: count / min / max / sum of the window at every position of sample ranges (atsc_rolling.hip)
// ------------------------------------------------------------------------------------------
extern "C" uint64_t atsc_rolling_outputs(uint64_t count, uint64_t width, uint64_t stride)
{
    return width && stride && count >= width ? (count - width) / stride + 1 : 0;
}

// The check of the call's parameters and the records of its ranges (ctx may be null: then no message is kept); `call`
// names the caller in the message.
static int rolling_check(atsc_ctx *ctx, const char *call, uint64_t n, const uint64_t *count, uint64_t width, uint64_t stride,
                         uint64_t *total)
{
    if (width == 0 || width > ATSC_ROLLING_MAX_WIDTH) return fail_in(ctx, ATSC_E_INVALID, call, "width outside [1, 2^20]");
    if (stride == 0) return fail_in(ctx, ATSC_E_INVALID, call, "stride is 0");
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; ++i) {
        sum += atsc_rolling_outputs(count[i], width, stride);
        if (sum > 0xfffffffeull) return fail_in(ctx, ATSC_E_INVALID, call, "more than 2^32 - 2 records");
    }
    if (total) *total = sum;
    return ATSC_OK;
}

// What differs between the device calls that read every position's window off a pyramid of chunk partials
// (rolling_dev): the rolling, the rolling deltas, the rolling moments, the rolling pair moments and the rolling runs.  The
// launchers take the list of the inputs' regions and the call's condition (RollCond: the rolling runs' op and limit, the
// one parameter of a call that a pyramid depends on): the adapters below forward scr[0], or scr[0] and scr[1], and where
// the kernels take it the condition, to the kernels' own.
struct RollCond {
    int op;
    double limit;
};
using RollPyramidFn = hipError_t (*)(const double *const *scr, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax,
                                     const RollCond &cond, hipStream_t s);
using RollPositionsFn = hipError_t (*)(const DevRollTask *tasks, uint32_t n, const double *const *scr, const void *pyr,
                                       const DevRollPiece *pc, uint64_t w, uint64_t stride, const RollCond &cond, void *out,
                                       hipStream_t s);
template <decltype(&launch_roll_pyramid) F>
static hipError_t roll_pyramid_one(const double *const *scr, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax,
                                   const RollCond &, hipStream_t s)
{
    return F(scr[0], n_tiles, pyr, pc, lmax, s);
}
template <decltype(&launch_roll_positions) F>
static hipError_t roll_positions_one(const DevRollTask *tasks, uint32_t n, const double *const *scr, const void *pyr,
                                     const DevRollPiece *pc, uint64_t w, uint64_t stride, const RollCond &, void *out,
                                     hipStream_t s)
{
    return F(tasks, n, scr[0], pyr, pc, w, stride, out, s);
}
static hipError_t roll_pyramid_pair(const double *const *scr, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax,
                                    const RollCond &, hipStream_t s)
{
    return launch_rpa_pyramid(scr[0], scr[1], n_tiles, pyr, pc, lmax, s);
}
static hipError_t roll_positions_pair(const DevRollTask *tasks, uint32_t n, const double *const *scr, const void *pyr,
                                      const DevRollPiece *pc, uint64_t w, uint64_t stride, const RollCond &, void *out,
                                      hipStream_t s)
{
    return launch_rpa_positions(tasks, n, scr[0], scr[1], pyr, pc, w, stride, out, s);
}
static hipError_t roll_pyramid_runs(const double *const *scr, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax,
                                    const RollCond &cond, hipStream_t s)
{
    return launch_rru_pyramid(scr[0], n_tiles, pyr, pc, lmax, cond.op, cond.limit, s);
}
static hipError_t roll_positions_runs(const DevRollTask *tasks, uint32_t n, const double *const *scr, const void *pyr,
                                      const DevRollPiece *pc, uint64_t w, uint64_t stride, const RollCond &cond, void *out,
                                      hipStream_t s)
{
    return launch_rru_positions(tasks, n, scr[0], pyr, pc, w, stride, cond.op, cond.limit, out, s);
}

struct RollKernel {
    const char *call;            // names the call in the messages
    const char *no_kernels;      // ATSC_E_UNSUPPORTED's message
    const char *launch_name[3];  // ATSC_E_HIP's messages: pyramid, upper, positions
    const DecodeCaller &who;
    uint32_t part_bytes;         // a partial of the pyramid: a multiple of 16
    uint32_t low;                // the lowest stored level
    uint32_t first;              // a window's chunks are those of [lo + first, lo + w): 0, or 1 where the leaf is a pair
    uint32_t rec_bytes;          // a position's record
    int inputs;                  // the streams the kernels read: 1, or 2 (the pair)
    bool have;                   // the kernels' launchers are linked in (they are weak)
    RollPyramidFn pyramid;
    decltype(&launch_roll_upper) upper;
    RollPositionsFn positions;
    RollCond cond = {0, 0.0};    // the call's condition (the rolling runs'); the other calls' kernels take none
    // the pyramid's bytes per sample of the region: the levels low, low + 1, .. hold less than 2 / 2^low partials a sample
    uint64_t pyramid_bytes() const { return (2ull * part_bytes) >> low; }
};

// The device call.  Host work, all of it in the stream's index (org: the stream index of the plan's first sample, see
// reduce_dev): the covering intervals of the ranges' windows (a range's samples behind its last position's window are
// not decoded), merged where they lie closer than HST_GAP, and cut into pieces of at most Lp samples that overlap by
// width - 1, so that every position's window lies whole in a piece: the first one that holds it computes it.  A piece
// lies in the scratch from the multiple of ROLL_TILE at or in front of its first sample on, so that a slot's place in
// the region and its stream index agree modulo ROLL_TILE; the pyramid of the piece's chunk partials (levels K.low ..
// floor(log2(width - K.first)); the rolling's and the rolling runs' 32 bytes each: at most 8 bytes a sample, the rolling
// deltas' and the rolling moments' 48: at most 12)
// follows the region and the spill slots in the same scratch.  Region and pyramid share the budget in the proportion of
// their bytes per sample, 8 to K.pyramid_bytes(): a region holds at most that share of piece_samples' length, Lr (the
// rolling's half, the rolling deltas' two fifths), and a piece Lp = Lr - 3 ROLL_TILE samples.  A width above Lp is
// ATSC_E_CAPACITY.  Per range and per piece, the run of positions the piece computes is cut into tasks of ROLL_TASK
// positions.  One upload (decode tasks, tasks, the pieces' level tables); then per piece the decode, the pyramid (with
// the levels above 11 and above 17 a small launch each) and the positions.
// in: the K.inputs streams the kernels read (1, or the pair's 2), as reduce_dev takes them; begin[] counts from
// in[0].org.  All of the above is computed once, in the stream's index, which the inputs share; per piece every input is
// decoded with its own decode tasks into a region of its own, its spill slots behind it (place_regions), and the one
// pyramid follows all regions.  A slot then costs 8 K.inputs + K.pyramid_bytes() bytes: Lr is that share of all the
// inputs' piece_samples together.  Every input's windows are checked against its own plan; the call's tables and scratch
// are in[0].dp's (res[Q_ROLLING]).
static int rolling_dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                       uint64_t width, uint64_t stride, void *d_out, void *stream, const RollKernel &K)
{
    const char *const CALL = K.call;
    const int NI = K.inputs;
    if (!ctx || NI < 1 || NI > 2 || (n_windows && (!begin || !count))) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    for (int k = 0; k < NI; ++k)
        if (!in[k].dp || (n_windows && !in[k].d_body)) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    for (int k = 1; k < NI; ++k)
        if (in[k].dp->ctx != in[0].dp->ctx) return fail_in(ctx, ATSC_E_INVALID, CALL, "plans of different contexts");
    const atsc_dplan *const dp = in[0].dp;
    const uint64_t org = in[0].org;  // begin[] counts from here
    uint64_t total = 0;
    int rc = rolling_check(ctx, CALL, n_windows, count, width, stride, &total);
    if (rc) return rc;
    if (total && !d_out) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    for (int k = 0; k < NI && !rc; ++k)
        rc = check_windows(ctx, CALL, in[k].dp, d_out, "d_out", n_windows, begin, count, ~0ull, org, in[k].org);
    if (rc || total == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !K.have) return fail_in(ctx, ATSC_E_UNSUPPORTED, CALL, K.no_kernels);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t W = n_windows, T = ROLL_TILE, w = width;
    std::vector<uint64_t> m(W);
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i) {
        m[i] = atsc_rolling_outputs(count[i], w, stride);
        if (m[i]) cov.emplace_back(org + begin[i], org + begin[i] + (m[i] - 1) * stride + w);
    }
    merge_spans(cov);
    uint64_t spill[2] = {0, 0};
    const uint64_t slot_bytes = sizeof(double) * NI + K.pyramid_bytes();  // of one slot: its sample in every region, its share of the pyramid
    const uint64_t L = piece_samples(ctx, in, NI, cov, 1, spill);
    const uint64_t Lr = std::max<uint64_t>(AGG_MIN_PIECE, L * NI * sizeof(double) / slot_bytes / T * T);
    const uint64_t Lp = Lr - 3 * T;
    if (w > Lp) {
        char msg[192];
        snprintf(msg, sizeof msg,
                 "%s: a window of %llu samples does not fit one scratch piece; an aggregate scratch budget of "
                 "%llu bytes would hold it", CALL, (unsigned long long)w,
                 (unsigned long long)((w + 4 * T) * slot_bytes + (spill[0] + spill[1]) * sizeof(double)));
        return fail(ctx, ATSC_E_CAPACITY, msg);
    }
    // pieces: samples [first, second) of the stream, ascending; scratch[0] is sample first / T * T
    std::vector<Span> pcs;
    uint64_t region = 0;
    for (size_t a = 0; a < cov.size();) {
        const uint64_t s0 = cov[a].first;
        uint64_t s1 = cov[a].second;
        size_t z = a + 1;
        while (z < cov.size() && cov[z].first < s1 + HST_GAP) s1 = cov[z++].second;
        for (uint64_t p = s0;;) {
            const uint64_t e = std::min(s1, p + Lp);
            pcs.emplace_back(p, e);
            region = std::max(region, (e + T - 1) / T * T - p / T * T);
            if (e == s1) break;
            p = e - (w - 1);
        }
        a = z;
    }
    const size_t P = pcs.size();
    // tasks, by piece: per range the runs of positions whose windows end inside the piece and not inside an earlier one
    std::vector<Placed<DevRollTask>> tk;
    uint64_t rec = 0;
    for (uint64_t i = 0; i < W; ++i) {
        if (!m[i]) continue;
        const uint64_t b = org + begin[i];
        size_t p = (size_t)(std::lower_bound(pcs.begin(), pcs.end(), b + w, [](const Span &x, uint64_t v) { return x.second < v; }) -
                            pcs.begin());
        for (uint64_t j = 0; j < m[i];) {
            const uint64_t lo = b + j * stride;
            while (p < P && pcs[p].second < lo + w) ++p;  // (a stride longer than a piece skips pieces)
            if (p >= P || pcs[p].first > lo)
                return fail_in(ctx, ATSC_E_INVALID, CALL, "internal error (position outside the pieces)");
            const uint64_t je = std::min(m[i], (pcs[p].second - w - b) / stride + 1);  // positions whose windows end in the piece
            for (; j < je; j += ROLL_TASK)
                tk.push_back({(uint32_t)p, DevRollTask{b + j * stride, rec + j, (uint32_t)std::min<uint64_t>(ROLL_TASK, je - j), 0}});
            j = je;
        }
        rec += m[i];
    }
    std::vector<DevRollTask> tasks;
    std::vector<size_t> at;
    group_tasks(tk, P, tasks, at);
    // the levels' places in the pyramid, the same in every piece: level l has room for (region >> l) + 2 chunks
    uint32_t lmax = 0;
    while (lmax < ROLL_MAX_LEVEL && (2ull << lmax) <= w - K.first) ++lmax;
    std::vector<DevRollPiece> pieces(P);
    std::vector<Span> dec(P);  // what a piece decodes: its samples and, in front of them, what the ranges cover of its first tile
    uint64_t pyr_n = 0;
    {
        DevRollPiece lv{};
        for (uint32_t l = K.low; l <= lmax; ++l) { lv.off[l] = pyr_n; pyr_n += (region >> l) + 2; }
        for (size_t p = 0; p < P; ++p) {
            pieces[p] = lv;
            pieces[p].a0 = pcs[p].first / T * T;
            pieces[p].a1 = (pcs[p].second + T - 1) / T * T;
            dec[p] = Span(pieces[p].a0, pcs[p].second);
        }
    }
    std::vector<PieceDecode> pdec[2];
    DecodeTasks D[2];
    for (int k = 0; k < NI && !rc; ++k) rc = emit_pieces_decode(ctx, CALL, in[k].dp, in[k].org, cov, dec, 1, region, D[k], pdec[k]);
    if (rc) return rc;
    QueryRes &R = dp->res[Q_ROLLING];
    HIPCHK(ctx, R.wait());
    Upload up;
    for (int k = 0; k < NI; ++k) D[k].place(up);
    const size_t off_tasks = up.add(tasks), off_pieces = up.add(pieces);
    // the scratch: every input's region and spill slots, then the pyramid (four or six doubles a partial; region and
    // MAX_FRAME are even numbers of doubles, so the pyramid begins at a multiple of 16 bytes, as its 16-byte loads and
    // stores need)
    uint64_t scr_at[2] = {0, 0};
    const uint64_t pyr_at = place_regions(D, NI, region, scr_at);
    rc = stage_upload(ctx, R, up, pyr_at + K.part_bytes / sizeof(double) * pyr_n, s);
    if (rc) return rc;
    unsigned char *d = R.d;
    double *scr[2] = {R.scratch + scr_at[0], R.scratch + scr_at[1]};
    void *pyr = R.scratch + pyr_at;
    const DevRollTask *d_tasks = (const DevRollTask *)(d + off_tasks);
    const DevRollPiece *d_pieces = (const DevRollPiece *)(d + off_pieces);
    for (size_t p = 0; p < P; ++p) {
        for (int k = 0; k < NI; ++k) {
            rc = launch_piece_decode(ctx, in[k].dp, in[k].d_body, d, D[k], pdec[k][p], scr[k], scr[k], scr[k], s, K.who);
            if (rc) return rc;
        }
        const uint64_t a0 = pieces[p].a0, last = pieces[p].a1 - 1;
        LAUNCHCHK(ctx, K.launch_name[0], K.pyramid(scr, (uint32_t)((pieces[p].a1 - a0) / T), pyr, d_pieces + p, lmax, K.cond, s));
        for (uint32_t src = ROLL_TILE_LOG; src < lmax; src += 6)
            LAUNCHCHK(ctx, K.launch_name[1],
                      K.upper(pyr, d_pieces + p, (uint32_t)(((last >> src) >> 6) - ((a0 >> src) >> 6) + 1), src, lmax, s));
        LAUNCHCHK(ctx, K.launch_name[2],
                  K.positions(d_tasks + at[p], (uint32_t)(at[p + 1] - at[p]), scr, pyr, d_pieces + p, w, stride, K.cond, d_out, s));
    }
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// The rolling's descriptor (see AggQuery): the width and the stride are the call's parameters, and the size of its result
// follows from the ranges' lengths, not from their number and not from the data.  KERNEL: whose pyramid and records
// (RollKernel): the rolling's, the rolling deltas' or the rolling moments'.
struct RollKernelPlain {
    static constexpr const char *CALL = "rolling_windows";
    static RollKernel kernel()
    {
        return RollKernel{CALL, "no rolling kernels", {"launch k_roll_pyramid", "launch k_roll_upper", "launch k_roll_positions"},
                          BY_ROLLING, sizeof(DevAggPart), ROLL_LOW, 0, sizeof(atsc_window_rolling), 1,
                          launch_roll_pyramid && launch_roll_upper && launch_roll_positions,
                          &roll_pyramid_one<&launch_roll_pyramid>, &launch_roll_upper, &roll_positions_one<&launch_roll_positions>};
    }
};
struct RollKernelDelta {
    static constexpr const char *CALL = "rolling_delta_windows";
    static RollKernel kernel()
    {
        return RollKernel{CALL, "no rolling delta kernels", {"launch k_rdl_pyramid", "launch k_rdl_upper", "launch k_rdl_positions"},
                          BY_ROLLING_DELTA, ROLL_DELTA_PART, ROLL_DELTA_LOW, 1, sizeof(atsc_window_delta), 1,
                          launch_rdl_pyramid && launch_rdl_upper && launch_rdl_positions,
                          &roll_pyramid_one<&launch_rdl_pyramid>, &launch_rdl_upper, &roll_positions_one<&launch_rdl_positions>};
    }
};
struct RollKernelMoments {
    static constexpr const char *CALL = "rolling_moments_windows";
    static RollKernel kernel()
    {
        return RollKernel{CALL, "no rolling moments kernels", {"launch k_rmo_pyramid", "launch k_rmo_upper", "launch k_rmo_positions"},
                          BY_ROLLING_MOMENTS, ROLL_MOMENTS_PART, ROLL_MOMENTS_LOW, 0, sizeof(atsc_window_moments), 1,
                          launch_rmo_pyramid && launch_rmo_upper && launch_rmo_positions,
                          &roll_pyramid_one<&launch_rmo_pyramid>, &launch_rmo_upper, &roll_positions_one<&launch_rmo_positions>};
    }
};
// the rolling pair moments: two inputs, the rolling moments' partial and its upper levels (they merge partials only)
struct RollKernelPair {
    static constexpr const char *CALL = "rolling_pair_windows";
    static RollKernel kernel()
    {
        return RollKernel{CALL, "no rolling pair kernels", {"launch k_rpa_pyramid", "launch k_rmo_upper", "launch k_rpa_positions"},
                          BY_ROLLING_PAIR, ROLL_MOMENTS_PART, ROLL_MOMENTS_LOW, 0, sizeof(atsc_window_pair), 2,
                          launch_rpa_pyramid && launch_rmo_upper && launch_rpa_positions,
                          &roll_pyramid_pair, &launch_rmo_upper, &roll_positions_pair};
    }
};
template <class KERNEL>
struct RollQueryOf {
    static constexpr int INPUTS = 1;
    static constexpr const char *CALL = KERNEL::CALL;
    uint64_t width, stride;
    const uint64_t *count;  // the call's ranges' lengths
    uint64_t n_ranges;
    size_t out_bytes(uint64_t n) const
    {
        uint64_t total = 0;
        for (uint64_t i = 0; count && i < n; ++i) total += atsc_rolling_outputs(count[i], width, stride);
        return total * KERNEL::kernel().rec_bytes;
    }
    int check(atsc_ctx *ctx) const { return rolling_check(ctx, CALL, count ? n_ranges : 0, count, width, stride, nullptr); }
    static void fill_empty(void *, uint64_t) {}  // ranges without a sample have no record
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *cnt, void *d_res, void *stream, uint64_t org) const
    {
        const QueryInput in{dp, d_body, org};
        return rolling_dev(ctx, &in, n_windows, begin, cnt, width, stride, d_res, stream, KERNEL::kernel());
    }
};
// The rolling pair moments' descriptor (see PairQuery): the one rolling call over two inputs.
struct RollPairQuery {
    static constexpr int INPUTS = 2;
    static constexpr const char *CALL = RollKernelPair::CALL;
    uint64_t width, stride;
    const uint64_t *count;  // the call's ranges' lengths
    uint64_t n_ranges;
    size_t out_bytes(uint64_t n) const
    {
        uint64_t total = 0;
        for (uint64_t i = 0; count && i < n; ++i) total += atsc_rolling_outputs(count[i], width, stride);
        return total * sizeof(atsc_window_pair);
    }
    int check(atsc_ctx *ctx) const { return rolling_check(ctx, CALL, count ? n_ranges : 0, count, width, stride, nullptr); }
    static void fill_empty(void *, uint64_t) {}  // ranges without a sample have no record
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream) const
    {
        return rolling_dev(ctx, in, n_windows, begin, cnt, width, stride, d_res, stream, RollKernelPair::kernel());
    }
};
// The rolling runs' descriptor: the rolling's, with the runs' condition, which is checked in front of the rolling's own
// parameters and handed to the kernels through the RollKernel (the runs' rule: RunQuery::check).
struct RollKernelRuns {
    static constexpr const char *CALL = "rolling_runs_windows";
    static RollKernel kernel(int op, double limit)
    {
        return RollKernel{CALL, "no rolling runs kernels", {"launch k_rru_pyramid", "launch k_rru_upper", "launch k_rru_positions"},
                          BY_ROLLING_RUNS, ROLL_RUNS_PART, ROLL_RUNS_LOW, 0, sizeof(atsc_window_runs), 1,
                          launch_rru_pyramid && launch_rru_upper && launch_rru_positions,
                          &roll_pyramid_runs, &launch_rru_upper, &roll_positions_runs, RollCond{op, limit}};
    }
};
struct RollRunsQuery {
    static constexpr int INPUTS = 1;
    static constexpr const char *CALL = RollKernelRuns::CALL;
    uint64_t width, stride;
    int op;
    double limit;
    const uint64_t *count;  // the call's ranges' lengths
    uint64_t n_ranges;
    size_t out_bytes(uint64_t n) const
    {
        uint64_t total = 0;
        for (uint64_t i = 0; count && i < n; ++i) total += atsc_rolling_outputs(count[i], width, stride);
        return total * sizeof(atsc_window_runs);
    }
    int check(atsc_ctx *ctx) const
    {
        const int rc = runs_condition_check(ctx, CALL, op, limit);
        return rc ? rc : rolling_check(ctx, CALL, count ? n_ranges : 0, count, width, stride, nullptr);
    }
    static void fill_empty(void *, uint64_t) {}  // ranges without a sample have no record
    // (the condition is checked in front of the arguments, as RunQuery's is)
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *cnt, void *d_res, void *stream, uint64_t org) const
    {
        const int rc = runs_condition_check(ctx, CALL, op, limit);
        if (rc) return rc;
        const QueryInput in{dp, d_body, org};
        return rolling_dev(ctx, &in, n_windows, begin, cnt, width, stride, d_res, stream, RollKernelRuns::kernel(op, limit));
    }
};
using RollQuery = RollQueryOf<RollKernelPlain>;
using RollDeltaQuery = RollQueryOf<RollKernelDelta>;
using RollMomentsQuery = RollQueryOf<RollKernelMoments>;

extern "C" int atsc_rolling_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                        const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                        atsc_window_rolling *d_out, void *stream)
{
    ATSC_API_BEGIN
    return RollQuery{width, stride, count, n_windows}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_rolling_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                    const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                    atsc_window_rolling *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, RollQuery{width, stride, count, n_windows});
    ATSC_API_END
}

// windowed rolling deltas: the deltas' record of the window at every position of sample ranges (atsc_rolling_delta.hip),
// through the rolling's device call: its tables and scratch are the rolling's, dp->res[Q_ROLLING]
extern "C" int atsc_rolling_delta_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                              const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                              atsc_window_delta *d_out, void *stream)
{
    ATSC_API_BEGIN
    return RollDeltaQuery{width, stride, count, n_windows}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_rolling_delta_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                          const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                          atsc_window_delta *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, RollDeltaQuery{width, stride, count, n_windows});
    ATSC_API_END
}

// windowed rolling runs: the runs' record of the window at every position of sample ranges under the condition x OP limit
// (atsc_rolling_runs.hip), through the rolling's device call: its tables and scratch are the rolling's, dp->res[Q_ROLLING]
extern "C" int atsc_rolling_runs_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                             const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                             int op, double limit, atsc_window_runs *d_out, void *stream)
{
    ATSC_API_BEGIN
    return RollRunsQuery{width, stride, op, limit, count, n_windows}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_rolling_runs_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                         const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride, int op,
                                         double limit, atsc_window_runs *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out,
                      RollRunsQuery{width, stride, op, limit, count, n_windows});
    ATSC_API_END
}

// windowed rolling moments: the moments' record of the window at every position of sample ranges
// (atsc_rolling_moments.hip), through the rolling's device call: its tables and scratch are the rolling's,
// dp->res[Q_ROLLING]
extern "C" int atsc_rolling_moments_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                                const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                                atsc_window_moments *d_out, void *stream)
{
    ATSC_API_BEGIN
    return RollMomentsQuery{width, stride, count, n_windows}.dev(ctx, dp, d_body, n_windows, begin, count, d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_rolling_moments_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count, uint64_t n_windows,
                                            const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                            atsc_window_moments *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out, RollMomentsQuery{width, stride, count, n_windows});
    ATSC_API_END
}

// windowed rolling pair moments: the pair moments' record of the window at every position of sample ranges of two
// streams (atsc_rolling_pair.hip), through the rolling's device call with two inputs: its tables and scratch are the
// rolling's of dp_x, dp_x->res[Q_ROLLING]
extern "C" int atsc_rolling_pair_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp_x, const uint8_t *d_body_x, const atsc_dplan *dp_y,
                                             const uint8_t *d_body_y, uint64_t n_windows, const uint64_t *begin,
                                             const uint64_t *count, uint64_t width, uint64_t stride, atsc_window_pair *d_out,
                                             void *stream)
{
    ATSC_API_BEGIN
    const QueryInput in[2] = {{dp_x, d_body_x, 0}, {dp_y, d_body_y, 0}};
    return RollPairQuery{width, stride, count, n_windows}.dev(ctx, in, n_windows, begin, count, d_out, stream);
    ATSC_API_END
}

extern "C" int atsc_rolling_pair_windows(atsc_ctx *ctx, const uint8_t *body_x, uint64_t len_x, int has_count_x,
                                         const uint8_t *body_y, uint64_t len_y, int has_count_y, uint64_t n_windows,
                                         const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                         atsc_window_pair *out)
{
    ATSC_API_BEGIN
    const HostBody hb[2] = {{body_x, len_x, has_count_x}, {body_y, len_y, has_count_y}};
    return query_host(ctx, hb, n_windows, begin, count, out, RollPairQuery{width, stride, count, n_windows});
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// windowed rolling quantiles: the levels of the window at every position of sample ranges (atsc_rolling_quantile.hip)
// ------------------------------------------------------------------------------------------
// rolling_check with the rolling quantiles' width limit, then the quantiles' levels and method
static int rolling_quantile_check(atsc_ctx *ctx, const char *call, uint64_t n, const uint64_t *count, uint64_t width,
                                  uint64_t stride, uint32_t n_q, const double *q, int method, uint64_t *total)
{
    if (width > ATSC_ROLLING_QUANTILE_MAX_WIDTH)
        return fail_in(ctx, ATSC_E_INVALID, call,
                       "width above 8192 (ATSC_ROLLING_QUANTILE_MAX_WIDTH); wider windows: atsc_quantile_windows with listed windows");
    const int rc = rolling_check(ctx, call, n, count, width, stride, total);
    return rc ? rc : quantile_check_levels(ctx, call, n_q, q, method);
}

// The device call.  Covering intervals, pieces that overlap by width - 1 and the rule "the first piece that holds a
// position's window computes it" are rolling_dev's; there is no pyramid, so a piece takes the whole of piece_samples'
// length and lies in the scratch from its first sample on.  width <= 8192 is far below the least piece, so every window
// fits one.  Per range and per piece, the run of positions the piece computes is cut into tasks of B = (P - width) /
// stride + 1 positions, P = rq_span_keys(width): a task's windows cover at most P samples.  One upload (decode tasks,
// levels, tasks); then per piece the decode and the one launch, which is told B: where no task holds more than one
// position the kernel sorts the keys without their places in the span.
static int rolling_quantile_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride, uint32_t n_q,
                                const double *q, int method, double *d_out, void *stream, uint64_t org)
{
    static const char *const CALL = "rolling_quantile_windows";
    if (!ctx || !dp || (n_windows && (!d_body || !begin || !count))) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    uint64_t total = 0;
    int rc = rolling_quantile_check(ctx, CALL, n_windows, count, width, stride, n_q, q, method, &total);
    if (rc) return rc;
    if (total && !d_out) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    rc = check_windows(ctx, CALL, dp, d_out, "d_out", n_windows, begin, count, ~0ull);
    if (rc || total == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !launch_rq_span)
        return fail_in(ctx, ATSC_E_UNSUPPORTED, CALL, "no rolling quantile kernels");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t W = n_windows, w = width;
    std::vector<uint64_t> m(W);
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i) {
        m[i] = atsc_rolling_outputs(count[i], w, stride);
        if (m[i]) cov.emplace_back(org + begin[i], org + begin[i] + (m[i] - 1) * stride + w);
    }
    merge_spans(cov);
    uint64_t spill;
    const uint64_t Lp = piece_samples(ctx, dp, org, cov, 1, &spill);
    static_assert(ATSC_ROLLING_QUANTILE_MAX_WIDTH < AGG_MIN_PIECE, "a window fits the least piece");
    // pieces: samples [first, second) of the stream, ascending; scratch[0] is sample first
    std::vector<Span> pcs;
    uint64_t region = 0;
    for (size_t a = 0; a < cov.size();) {
        const uint64_t s0 = cov[a].first;
        uint64_t s1 = cov[a].second;
        size_t z = a + 1;
        while (z < cov.size() && cov[z].first < s1 + HST_GAP) s1 = cov[z++].second;
        for (uint64_t p = s0;;) {
            const uint64_t e = std::min(s1, p + Lp);
            pcs.emplace_back(p, e);
            region = std::max(region, e - p);
            if (e == s1) break;
            p = e - (w - 1);
        }
        a = z;
    }
    region += region & 1;  // an even number of doubles, as the spill slots behind it expect
    const size_t P = pcs.size();
    // tasks, by piece: per range the runs of positions whose windows end inside the piece and not inside an earlier one
    const uint32_t keys = rq_span_keys(w);
    const uint64_t B = (keys - w) / stride + 1;
    std::vector<Placed<DevRollTask>> tk;
    uint64_t rec = 0;
    for (uint64_t i = 0; i < W; ++i) {
        if (!m[i]) continue;
        const uint64_t b = org + begin[i];
        size_t p = (size_t)(std::lower_bound(pcs.begin(), pcs.end(), b + w, [](const Span &x, uint64_t v) { return x.second < v; }) -
                            pcs.begin());
        for (uint64_t j = 0; j < m[i];) {
            const uint64_t lo = b + j * stride;
            while (p < P && pcs[p].second < lo + w) ++p;  // (a stride longer than a piece skips pieces)
            if (p >= P || pcs[p].first > lo)
                return fail_in(ctx, ATSC_E_INVALID, CALL, "internal error (position outside the pieces)");
            const uint64_t je = std::min(m[i], (pcs[p].second - w - b) / stride + 1);  // positions whose windows end in the piece
            for (; j < je; j += B)
                tk.push_back({(uint32_t)p, DevRollTask{b + j * stride, rec + j, (uint32_t)std::min<uint64_t>(B, je - j), 0}});
            j = je;
        }
        rec += m[i];
    }
    std::vector<DevRollTask> tasks;
    std::vector<size_t> at;
    group_tasks(tk, P, tasks, at);
    std::vector<PieceDecode> pdec;
    DecodeTasks D;
    rc = emit_pieces_decode(ctx, CALL, dp, org, cov, pcs, 1, region, D, pdec);
    if (rc) return rc;
    QueryRes &R = dp->res[Q_ROLLING];
    HIPCHK(ctx, R.wait());
    Upload up;
    D.place(up);
    const size_t off_q = up.add(q, n_q * sizeof(double)), off_tasks = up.add(tasks);
    rc = stage_upload(ctx, R, up, region + (uint64_t)MAX_FRAME * D.spills_used, s);
    if (rc) return rc;
    unsigned char *d = R.d;
    double *scr = R.scratch;
    const double *dq = (const double *)(d + off_q);
    const DevRollTask *d_tasks = (const DevRollTask *)(d + off_tasks);
    for (size_t p = 0; p < P; ++p) {
        rc = launch_piece_decode(ctx, dp, d_body, d, D, pdec[p], scr, scr, scr, s, BY_ROLLING_QUANTILE);
        if (rc) return rc;
        LAUNCHCHK(ctx, "launch k_rq_span",
                  launch_rq_span(d_tasks + at[p], (uint32_t)(at[p + 1] - at[p]), keys, B, scr, pcs[p].first, (uint32_t)w, stride,
                                 dq, n_q, method, d_out, s));
    }
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// The rolling quantiles' descriptor (see AggQuery): RollQueryOf's shape with the levels and the method; a position's row
// is n_q doubles.
struct RollQuantileQuery {
    static constexpr int INPUTS = 1;
    static constexpr const char *CALL = "rolling_quantile_windows";
    uint64_t width, stride;
    const uint64_t *count;  // the call's ranges' lengths
    uint64_t n_ranges;
    uint32_t n_q;
    const double *q;
    int method;
    size_t out_bytes(uint64_t n) const
    {
        uint64_t total = 0;
        for (uint64_t i = 0; count && i < n; ++i) total += atsc_rolling_outputs(count[i], width, stride);
        return total * n_q * sizeof(double);
    }
    int check(atsc_ctx *ctx) const
    {
        return rolling_quantile_check(ctx, CALL, count ? n_ranges : 0, count, width, stride, n_q, q, method, nullptr);
    }
    static void fill_empty(void *, uint64_t) {}  // ranges without a sample have no row
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *cnt, void *d_res, void *stream, uint64_t org) const
    {
        return rolling_quantile_dev(ctx, dp, d_body, n_windows, begin, cnt, width, stride, n_q, q, method, (double *)d_res,
                                    stream, org);
    }
};

extern "C" int atsc_rolling_quantile_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                                 const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                                 uint32_t n_q, const double *q, int method, double *d_out, void *stream)
{
    ATSC_API_BEGIN
    return RollQuantileQuery{width, stride, count, n_windows, n_q, q, method}.dev(ctx, dp, d_body, n_windows, begin, count, d_out,
                                                                                  stream, 0);
    ATSC_API_END
}

extern "C" int atsc_rolling_quantile_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count,
                                             uint64_t n_windows, const uint64_t *begin, const uint64_t *count, uint64_t width,
                                             uint64_t stride, uint32_t n_q, const double *q, int method, double *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out,
                      RollQuantileQuery{width, stride, count, n_windows, n_q, q, method});
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// windowed rolling histograms: the value-bin counts of the window at every position of sample ranges
// (atsc_rolling_histogram.hip)
// ------------------------------------------------------------------------------------------
// rolling_check, then the histograms' edges, then the limit that keeps a counter's index in 32 bits
static int rolling_histogram_check(atsc_ctx *ctx, const char *call, uint64_t n, const uint64_t *count, uint64_t width,
                                   uint64_t stride, uint32_t n_edges, const double *edges, int closed, uint64_t *total)
{
    uint64_t sum = 0;
    int rc = rolling_check(ctx, call, n, count, width, stride, &sum);
    if (!rc) rc = histogram_check_edges(ctx, n_edges, edges, closed, call);
    if (rc) return rc;
    if (sum * ((uint64_t)n_edges + 2) > 0xfffffffeull)  // (sum < 2^32 and n_edges + 2 <= 1026: no overflow)
        return fail_in(ctx, ATSC_E_INVALID, call, "positions x (n_edges + 2) is not below 2^32 - 1 counters");
    if (total) *total = sum;
    return ATSC_OK;
}

// The device call.  Covering intervals, pieces that overlap by width - 1 and the rule "the first piece that holds a
// position's window computes it" are rolling_quantile_dev's: there is no pyramid, so a piece takes the whole of
// piece_samples' length and lies in the scratch from its first sample on, and the scratch holds decoded samples only.  A
// width above a piece is ATSC_E_CAPACITY, as in rolling_dev.  Per range and per piece, the run of positions the piece
// computes is cut into tasks of B = rh_task_positions(width, stride) positions.  One upload (decode tasks, edges,
// tasks); then per piece the decode and the one launch.
static int rolling_histogram_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                 const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                 uint32_t n_edges, const double *edges, int closed, uint64_t *d_out, void *stream, uint64_t org)
{
    static const char *const CALL = "rolling_histogram_windows";
    if (!ctx || !dp || (n_windows && (!d_body || !begin || !count))) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    uint64_t total = 0;
    int rc = rolling_histogram_check(ctx, CALL, n_windows, count, width, stride, n_edges, edges, closed, &total);
    if (rc) return rc;
    if (total && !d_out) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    rc = check_windows(ctx, CALL, dp, d_out, "d_out", n_windows, begin, count, ~0ull);
    if (rc || total == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !launch_rh_slide)
        return fail_in(ctx, ATSC_E_UNSUPPORTED, CALL, "no rolling histogram kernels");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t W = n_windows, w = width;
    std::vector<uint64_t> m(W);
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i) {
        m[i] = atsc_rolling_outputs(count[i], w, stride);
        if (m[i]) cov.emplace_back(org + begin[i], org + begin[i] + (m[i] - 1) * stride + w);
    }
    merge_spans(cov);
    uint64_t spill;
    const uint64_t Lp = piece_samples(ctx, dp, org, cov, 1, &spill);
    if (w > Lp) {
        char msg[192];
        snprintf(msg, sizeof msg,
                 "%s: a window of %llu samples does not fit one scratch piece; an aggregate scratch budget of "
                 "%llu bytes would hold it", CALL, (unsigned long long)w, (unsigned long long)((w + spill) * sizeof(double)));
        return fail(ctx, ATSC_E_CAPACITY, msg);
    }
    // pieces: samples [first, second) of the stream, ascending; scratch[0] is sample first
    std::vector<Span> pcs;
    uint64_t region = 0;
    for (size_t a = 0; a < cov.size();) {
        const uint64_t s0 = cov[a].first;
        uint64_t s1 = cov[a].second;
        size_t z = a + 1;
        while (z < cov.size() && cov[z].first < s1 + HST_GAP) s1 = cov[z++].second;
        for (uint64_t p = s0;;) {
            const uint64_t e = std::min(s1, p + Lp);
            pcs.emplace_back(p, e);
            region = std::max(region, e - p);
            if (e == s1) break;
            p = e - (w - 1);
        }
        a = z;
    }
    region += region & 1;  // an even number of doubles, as the spill slots behind it expect
    const size_t P = pcs.size();
    // tasks, by piece: per range the runs of positions whose windows end inside the piece and not inside an earlier one
    const uint64_t B = rh_task_positions(w, stride);
    std::vector<Placed<DevRollTask>> tk;
    uint64_t rec = 0;
    for (uint64_t i = 0; i < W; ++i) {
        if (!m[i]) continue;
        const uint64_t b = org + begin[i];
        size_t p = (size_t)(std::lower_bound(pcs.begin(), pcs.end(), b + w, [](const Span &x, uint64_t v) { return x.second < v; }) -
                            pcs.begin());
        for (uint64_t j = 0; j < m[i];) {
            const uint64_t lo = b + j * stride;
            while (p < P && pcs[p].second < lo + w) ++p;  // (a stride longer than a piece skips pieces)
            if (p >= P || pcs[p].first > lo)
                return fail_in(ctx, ATSC_E_INVALID, CALL, "internal error (position outside the pieces)");
            const uint64_t je = std::min(m[i], (pcs[p].second - w - b) / stride + 1);  // positions whose windows end in the piece
            for (; j < je; j += B)
                tk.push_back({(uint32_t)p, DevRollTask{b + j * stride, rec + j, (uint32_t)std::min<uint64_t>(B, je - j), 0}});
            j = je;
        }
        rec += m[i];
    }
    std::vector<DevRollTask> tasks;
    std::vector<size_t> at;
    group_tasks(tk, P, tasks, at);
    std::vector<PieceDecode> pdec;
    DecodeTasks D;
    rc = emit_pieces_decode(ctx, CALL, dp, org, cov, pcs, 1, region, D, pdec);
    if (rc) return rc;
    QueryRes &R = dp->res[Q_ROLLING];
    HIPCHK(ctx, R.wait());
    Upload up;
    D.place(up);
    const size_t off_edges = up.add(edges, n_edges * sizeof(double)), off_tasks = up.add(tasks);
    rc = stage_upload(ctx, R, up, region + (uint64_t)MAX_FRAME * D.spills_used, s);
    if (rc) return rc;
    unsigned char *d = R.d;
    double *scr = R.scratch;
    const double *d_edges = (const double *)(d + off_edges);
    const DevRollTask *d_tasks = (const DevRollTask *)(d + off_tasks);
    for (size_t p = 0; p < P; ++p) {
        rc = launch_piece_decode(ctx, dp, d_body, d, D, pdec[p], scr, scr, scr, s, BY_ROLLING_HISTOGRAM);
        if (rc) return rc;
        LAUNCHCHK(ctx, "launch k_rh_slide",
                  launch_rh_slide(d_tasks + at[p], (uint32_t)(at[p + 1] - at[p]), scr, pcs[p].first, (uint32_t)w, stride, d_edges,
                                  n_edges, closed, d_out, s));
    }
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// The rolling histograms' descriptor (see AggQuery): RollQuantileQuery's shape with the edges and the closed side; a
// position's row is n_edges + 2 counters.
struct RollHistogramQuery {
    static constexpr int INPUTS = 1;
    static constexpr const char *CALL = "rolling_histogram_windows";
    uint64_t width, stride;
    const uint64_t *count;  // the call's ranges' lengths
    uint64_t n_ranges;
    uint32_t n_edges;
    const double *edges;
    int closed;
    size_t out_bytes(uint64_t n) const
    {
        uint64_t total = 0;
        for (uint64_t i = 0; count && i < n; ++i) total += atsc_rolling_outputs(count[i], width, stride);
        return total * ((size_t)n_edges + 2) * sizeof(uint64_t);
    }
    int check(atsc_ctx *ctx) const
    {
        return rolling_histogram_check(ctx, CALL, count ? n_ranges : 0, count, width, stride, n_edges, edges, closed, nullptr);
    }
    static void fill_empty(void *, uint64_t) {}  // ranges without a sample have no row
    int dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows, const uint64_t *begin,
            const uint64_t *cnt, void *d_res, void *stream, uint64_t org) const
    {
        return rolling_histogram_dev(ctx, dp, d_body, n_windows, begin, cnt, width, stride, n_edges, edges, closed,
                                     (uint64_t *)d_res, stream, org);
    }
};

extern "C" int atsc_rolling_histogram_windows_dev(atsc_ctx *ctx, const atsc_dplan *dp, const uint8_t *d_body, uint64_t n_windows,
                                                  const uint64_t *begin, const uint64_t *count, uint64_t width, uint64_t stride,
                                                  uint32_t n_edges, const double *edges, int closed, uint64_t *d_out,
                                                  void *stream)
{
    ATSC_API_BEGIN
    return RollHistogramQuery{width, stride, count, n_windows, n_edges, edges, closed}.dev(ctx, dp, d_body, n_windows, begin, count,
                                                                                          d_out, stream, 0);
    ATSC_API_END
}

extern "C" int atsc_rolling_histogram_windows(atsc_ctx *ctx, const uint8_t *body, uint64_t body_len, int has_count,
                                              uint64_t n_windows, const uint64_t *begin, const uint64_t *count, uint64_t width,
                                              uint64_t stride, uint32_t n_edges, const double *edges, int closed, uint64_t *out)
{
    ATSC_API_BEGIN
    return query_host(ctx, body, body_len, has_count, n_windows, begin, count, out,
                      RollHistogramQuery{width, stride, count, n_windows, n_edges, edges, closed});
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// windowed across: count / min / max / sum over N streams at every position of sample ranges (atsc_across.hip)
// ------------------------------------------------------------------------------------------
extern "C" uint64_t atsc_across_outputs(uint64_t count, uint64_t stride)
{
    return count && stride ? (count - 1) / stride + 1 : 0;
}

// The check of the call's parameters and the records of its ranges (ctx may be null: then no message is kept); `call`
// names the caller in the message.
static int across_check(atsc_ctx *ctx, const char *call, uint32_t n_streams, uint64_t n, const uint64_t *count, uint64_t stride,
                        uint64_t *total)
{
    if (n_streams == 0 || n_streams > ATSC_ACROSS_MAX_STREAMS) return fail_in(ctx, ATSC_E_INVALID, call, "n_streams outside [1, 64]");
    if (stride == 0) return fail_in(ctx, ATSC_E_INVALID, call, "stride is 0");
    uint64_t sum = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t m = atsc_across_outputs(count[i], stride);
        if (m > 0xfffffffeull || (sum += m) > 0xfffffffeull)
            return fail_in(ctx, ATSC_E_INVALID, call, "more than 2^32 - 2 records");
    }
    if (total) *total = sum;
    return ATSC_OK;
}

// What differs between the device calls that work on the N samples of a position (across_dev): the across and the
// across quantiles, the across extremes, the across moments, the across histograms and the across value counts.
struct AcrossKernel {
    const char *call;          // names the call in the messages
    const char *no_kernels;    // ATSC_E_UNSUPPORTED's message
    const char *launch_name;   // ATSC_E_HIP's message
    QueryKind kind;            // whose tables and scratch of in[0].dp
    const DecodeCaller &who;
    bool present;              // the position kernel is linked in
    const void *table;         // table_bytes more bytes of the upload (8-byte aligned), handed to launch() on the device
    size_t table_bytes;
    // the position kernel over one piece's tasks: slot 0 of every region is sample a0; records from d_out on, whose size
    // is the kernel's own business (the tasks number records, not bytes)
    std::function<hipError_t(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint64_t a0,
                             const void *d_table, void *d_out, hipStream_t s)>
        launch;
};

// The device call over the plans in[0 .. n_in).  Host work, all of it in the stream's index, which the inputs share
// (in[k].org: the stream index of plan k's first sample, see reduce_dev; begin[] counts from in[0].org): the covering
// intervals of the ranges -- a range is decoded whole whatever the stride -- cut into pieces at multiples of AGG_TILE
// as reduce_dev cuts them; per piece and per input the decode tasks into the input's own region (its spill slots behind
// it); per range and per piece the run of positions that lie in the piece, cut into tasks of ACR_TASK positions.  A
// position needs one slot of every region and nothing else, so pieces do not overlap and a position is computed by the
// piece that holds it.
// Piece length: the budget (without one, the default of ONE input, whatever n_in is) less the inputs' spills, shared
// evenly by the n_in regions, a multiple of AGG_TILE and at least AGG_MIN_PIECE.
// One upload (every input's decode tasks, the tasks, the regions' places in the scratch: they differ in spill slots,
// so they are a table and not base + k x length); then per piece n_in decodes and one launch of the position kernel.
// The call's tables and scratch are in[0].dp's (res[K.kind]); K's table goes up with the others.
static int across_dev(atsc_ctx *ctx, const QueryInput *in, int n_in, uint64_t n_windows, const uint64_t *begin,
                      const uint64_t *count, uint64_t stride, void *d_out, void *stream, const AcrossKernel &K)
{
    const char *const CALL = K.call;
    if (!ctx || !in || (n_windows && (!begin || !count))) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    uint64_t total = 0;
    int rc = across_check(ctx, CALL, (uint32_t)n_in, n_windows, count, stride, &total);
    if (rc) return rc;
    for (int k = 0; k < n_in; ++k)
        if (!in[k].dp || !in[k].d_body) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    if (total && !d_out) return fail_in(ctx, ATSC_E_INVALID, CALL, "null argument");
    for (int k = 1; k < n_in; ++k)
        if (in[k].dp->ctx != in[0].dp->ctx) return fail_in(ctx, ATSC_E_INVALID, CALL, "plans of different contexts");
    const uint64_t org = in[0].org;  // begin[] counts from here
    for (int k = 0; k < n_in && !rc; ++k)
        rc = check_windows(ctx, CALL, in[k].dp, d_out, "d_out", n_windows, begin, count, ~0ull, org, in[k].org);
    if (rc || total == 0) return rc;
    if (!launch_decompress_window || !launch_window_gather || !K.present)
        return fail_in(ctx, ATSC_E_UNSUPPORTED, CALL, K.no_kernels);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t T = AGG_TILE, W = n_windows;
    std::vector<uint64_t> m(W);
    std::vector<Span> cov;
    for (uint64_t i = 0; i < W; ++i) {
        m[i] = atsc_across_outputs(count[i], stride);
        if (m[i]) cov.emplace_back(org + begin[i], org + begin[i] + count[i]);
    }
    merge_spans(cov);
    // piece length
    uint64_t spills = 0;
    bool large = false;
    for (int k = 0; k < n_in; ++k)
        if (spans_touch_large(in[k].dp, in[k].org, cov)) {
            large = true;
            spills += 2ull * MAX_FRAME;
        }
    const uint64_t want = scratch_budget_samples(ctx, large);
    const uint64_t piece_tiles =
        std::max<uint64_t>(AGG_MIN_PIECE, want > spills ? (want - spills) / (uint64_t)n_in / T * T : 0) / T;
    std::vector<Span> pcs;  // tiles [first, second)
    const uint64_t region = cut_pieces(cov, T, piece_tiles, AGG_GAP_TILES, pcs) * T;
    const size_t P = pcs.size();
    // tasks, by piece: per range the runs of positions inside each piece
    std::vector<Placed<DevRollTask>> tk;
    uint64_t rec = 0;
    for (uint64_t i = 0; i < W; ++i) {
        if (!m[i]) continue;
        const uint64_t b = org + begin[i];
        size_t p = (size_t)(std::upper_bound(pcs.begin(), pcs.end(), b / T, [](uint64_t v, const Span &x) { return v < x.second; }) -
                            pcs.begin());
        for (uint64_t j = 0; j < m[i];) {
            const uint64_t lo = b + j * stride;
            while (p < P && pcs[p].second * T <= lo) ++p;  // (a stride longer than a piece skips pieces)
            if (p >= P || pcs[p].first * T > lo)
                return fail_in(ctx, ATSC_E_INVALID, CALL, "internal error (position outside the pieces)");
            const uint64_t je = std::min(m[i], (pcs[p].second * T - 1 - b) / stride + 1);  // positions in front of the piece's end
            for (; j < je; j += ACR_TASK)
                tk.push_back({(uint32_t)p, DevRollTask{b + j * stride, rec + j, (uint32_t)std::min<uint64_t>(ACR_TASK, je - j), 0}});
            j = je;
        }
        rec += m[i];
    }
    std::vector<DevRollTask> tasks;
    std::vector<size_t> at;
    group_tasks(tk, P, tasks, at);
    // decode tasks of every piece, once per input
    std::vector<DecodeTasks> D(n_in);
    std::vector<std::vector<PieceDecode>> pdec(n_in);
    for (int k = 0; k < n_in && !rc; ++k) rc = emit_pieces_decode(ctx, CALL, in[k].dp, in[k].org, cov, pcs, T, region, D[k], pdec[k]);
    if (rc) return rc;
    std::vector<uint64_t> reg(n_in);  // the regions' places in the scratch: a table of the upload
    const uint64_t scr_n = place_regions(D.data(), n_in, region, reg.data());
    QueryRes &R = in[0].dp->res[K.kind];
    HIPCHK(ctx, R.wait());
    Upload up;
    for (int k = 0; k < n_in; ++k) D[k].place(up);
    const size_t off_tasks = up.add(tasks), off_reg = up.add(reg);
    const size_t off_table = K.table_bytes ? up.add(K.table, K.table_bytes) : 0;
    rc = stage_upload(ctx, R, up, scr_n, s);
    if (rc) return rc;
    unsigned char *d = R.d;
    const DevRollTask *d_tasks = (const DevRollTask *)(d + off_tasks);
    for (size_t p = 0; p < P; ++p) {
        for (int k = 0; k < n_in; ++k) {
            double *scr = R.scratch + reg[k];
            rc = launch_piece_decode(ctx, in[k].dp, in[k].d_body, d, D[k], pdec[k][p], scr, scr, scr, s, K.who);
            if (rc) return rc;
        }
        LAUNCHCHK(ctx, K.launch_name, K.launch(d_tasks + at[p], (uint32_t)(at[p + 1] - at[p]), R.scratch,
                                               (const uint64_t *)(d + off_reg), pcs[p].first * T, d + off_table, d_out, s));
    }
    HIPCHK(ctx, R.record(s));
    return ATSC_OK;
}

// What the six across descriptors share (see AggQuery): the number of streams is the call's own (INPUTS == 0, inputs());
// it and the stride are the call's parameters, and the size of a result follows from the ranges' lengths, as the
// rolling's does.  A query adds CALL, its own parameters, out_bytes (positions(n) records of its size), check (the
// ranges, then its parameters: the first check that fails decides the code and the message) and dev, which describes
// its position kernel to across_dev (run).  Every query but the across keeps its tables and scratch in the across
// quantiles' place on in[0].dp (Q_ACROSS_QUANTILE): those kinds of call on one first plan wait for each other, and
// atsc_dplan stays as it is (DESIGN.md "Windowed across extremes").
struct AcrossBase {
    static constexpr int INPUTS = 0;
    uint32_t n_streams;
    uint64_t stride;
    const uint64_t *count;  // the call's ranges' lengths
    uint64_t n_ranges;
    int inputs() const { return (int)n_streams; }
    uint64_t positions(uint64_t n) const
    {
        uint64_t total = 0;
        for (uint64_t i = 0; count && i < n; ++i) total += atsc_across_outputs(count[i], stride);
        return total;
    }
    int check_ranges(atsc_ctx *ctx, const char *call, uint64_t *total = nullptr) const
    {
        return across_check(ctx, call, n_streams, count ? n_ranges : 0, count, stride, total);
    }
    static void fill_empty(void *, uint64_t) {}  // ranges without a sample have no record
    int run(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream, const AcrossKernel &K) const
    {
        return across_dev(ctx, in, (int)n_streams, n_windows, begin, cnt, stride, d_res, stream, K);
    }
};

// the across' descriptor: no parameter of its own, and no check in front of across_dev's
struct AcrossQuery : AcrossBase {
    static constexpr const char *CALL = "across_windows";
    size_t out_bytes(uint64_t n) const { return positions(n) * sizeof(atsc_across_record); }
    int check(atsc_ctx *ctx) const { return check_ranges(ctx, CALL); }
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream) const
    {
        return run(ctx, in, n_windows, begin, cnt, d_res, stream,
                   {CALL, "no across kernels", "launch k_across_positions", Q_ACROSS, BY_ACROSS, launch_across_positions != nullptr,
                    nullptr, 0,
                    [this](const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint64_t a0,
                           const void *, void *d_out, hipStream_t s) {
                        return launch_across_positions(tasks, n, scratch, reg, n_streams, a0, stride, d_out, s);
                    }});
    }
};

// the across quantiles' descriptor: a row of n_q levels per record; the levels and the method are checked as the
// windowed quantiles check theirs (quantile_check_levels) and go up with the call's tables
struct AcrossQntQuery : AcrossBase {
    static constexpr const char *CALL = "across_quantile_windows";
    uint32_t n_q;
    const double *q;
    int method;
    size_t out_bytes(uint64_t n) const { return positions(n) * n_q * sizeof(double); }
    int check(atsc_ctx *ctx) const
    {
        const int rc = check_ranges(ctx, CALL);
        return rc ? rc : quantile_check_levels(ctx, CALL, n_q, q, method);
    }
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream) const
    {
        const int rc = check(ctx);
        if (rc) return rc;
        return run(ctx, in, n_windows, begin, cnt, d_res, stream,
                   {CALL, "no across quantile kernels", "launch k_across_quantile_positions", Q_ACROSS_QUANTILE, BY_ACROSS_QUANTILE,
                    launch_across_quantile_positions != nullptr, q, n_q * sizeof(double),
                    [this](const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint64_t a0,
                           const void *d_q, void *d_out, hipStream_t s) {
                        return launch_across_quantile_positions(tasks, n, scratch, reg, n_streams, a0, stride, (const double *)d_q,
                                                                n_q, method, (double *)d_out, s);
                    }});
    }
};

// the across extremes' descriptor: the windowed extremes' record (of k entries per list) per position; k is checked as
// the windowed extremes check theirs and goes to the kernel by value
struct AcrossExtQuery : AcrossBase {
    static constexpr const char *CALL = "across_extremes_windows";
    uint32_t k;
    size_t out_bytes(uint64_t n) const { return positions(n) * ATSC_EXTREMES_BYTES(std::min<uint32_t>(k, ATSC_EXTREMES_MAX_K)); }
    int check(atsc_ctx *ctx) const
    {
        const int rc = check_ranges(ctx, CALL);
        if (rc) return rc;
        if (k == 0 || k > ATSC_EXTREMES_MAX_K) return fail_in(ctx, ATSC_E_INVALID, CALL, "k outside [1, 16]");
        return ATSC_OK;
    }
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream) const
    {
        const int rc = check(ctx);
        if (rc) return rc;
        return run(ctx, in, n_windows, begin, cnt, d_res, stream,
                   {CALL, "no across extremes kernels", "launch k_across_extremes_positions", Q_ACROSS_QUANTILE, BY_ACROSS_EXTREMES,
                    launch_across_extremes_positions != nullptr, nullptr, 0,
                    [this](const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint64_t a0,
                           const void *, void *d_out, hipStream_t s) {
                        return launch_across_extremes_positions(tasks, n, scratch, reg, n_streams, a0, stride, k, d_out, s);
                    }});
    }
};

// the across moments' descriptor: an atsc_across_moments per position; no parameter of its own, and no check in front of
// across_dev's
struct AcrossMomQuery : AcrossBase {
    static constexpr const char *CALL = "across_moments_windows";
    size_t out_bytes(uint64_t n) const { return positions(n) * sizeof(atsc_across_moments); }
    int check(atsc_ctx *ctx) const { return check_ranges(ctx, CALL); }
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream) const
    {
        return run(ctx, in, n_windows, begin, cnt, d_res, stream,
                   {CALL, "no across moments kernels", "launch k_across_moments_positions", Q_ACROSS_QUANTILE, BY_ACROSS_MOMENTS,
                    launch_across_moments_positions != nullptr, nullptr, 0,
                    [this](const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint64_t a0,
                           const void *, void *d_out, hipStream_t s) {
                        return launch_across_moments_positions(tasks, n, scratch, reg, n_streams, a0, stride, d_out, s);
                    }});
    }
};

// the across histograms' descriptor: the histograms' row of n_edges + 2 counters per position; the edges and `closed` are
// checked as the windowed histograms check theirs (histogram_check_edges), the edges go up with the call's tables, and
// the rolling histograms' limit keeps a counter's index in 32 bits
struct AcrossHistQuery : AcrossBase {
    static constexpr const char *CALL = "across_histogram_windows";
    uint32_t n_edges;
    const double *edges;
    int closed;
    size_t out_bytes(uint64_t n) const { return positions(n) * ((size_t)n_edges + 2) * sizeof(uint64_t); }
    int check(atsc_ctx *ctx) const
    {
        uint64_t total = 0;
        int rc = check_ranges(ctx, CALL, &total);
        if (!rc) rc = histogram_check_edges(ctx, n_edges, edges, closed, CALL);
        if (rc) return rc;
        if (total * ((uint64_t)n_edges + 2) > 0xfffffffeull)  // (total < 2^32 and n_edges + 2 <= 1026: no overflow)
            return fail_in(ctx, ATSC_E_INVALID, CALL, "positions x (n_edges + 2) is not below 2^32 - 1 counters");
        return ATSC_OK;
    }
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream) const
    {
        const int rc = check(ctx);
        if (rc) return rc;
        return run(ctx, in, n_windows, begin, cnt, d_res, stream,
                   {CALL, "no across histogram kernels", "launch k_across_histogram_positions", Q_ACROSS_QUANTILE,
                    BY_ACROSS_HISTOGRAM, launch_across_histogram_positions != nullptr, edges, n_edges * sizeof(double),
                    [this](const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint64_t a0,
                           const void *d_edges, void *d_out, hipStream_t s) {
                        return launch_across_histogram_positions(tasks, n, scratch, reg, n_streams, a0, stride,
                                                                 (const double *)d_edges, n_edges, closed, (uint64_t *)d_out, s);
                    }});
    }
};

// the across value counts' descriptor: the windowed value counts' record (of k entries) per position; k is checked as the
// windowed value counts check theirs, and k and `above` (as its key, val_key) go to the kernel by value
struct AcrossValQuery : AcrossBase {
    static constexpr const char *CALL = "across_values_windows";
    uint32_t k;
    double above;
    size_t out_bytes(uint64_t n) const { return positions(n) * ATSC_VALUES_BYTES(std::min<uint32_t>(k, ATSC_VALUES_MAX_K)); }
    int check(atsc_ctx *ctx) const
    {
        const int rc = check_ranges(ctx, CALL);
        if (rc) return rc;
        if (k == 0 || k > ATSC_VALUES_MAX_K) return fail_in(ctx, ATSC_E_INVALID, CALL, "k outside [1, 32]");
        return ATSC_OK;
    }
    int dev(atsc_ctx *ctx, const QueryInput *in, uint64_t n_windows, const uint64_t *begin, const uint64_t *cnt, void *d_res,
            void *stream) const
    {
        const int rc = check(ctx);
        if (rc) return rc;
        const uint64_t ak = val_key(above);
        return run(ctx, in, n_windows, begin, cnt, d_res, stream,
                   {CALL, "no across values kernels", "launch k_across_values_positions", Q_ACROSS_QUANTILE, BY_ACROSS_VALUES,
                    launch_across_values_positions != nullptr, nullptr, 0,
                    [this, ak](const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg, uint64_t a0,
                               const void *, void *d_out, hipStream_t s) {
                        return launch_across_values_positions(tasks, n, scratch, reg, n_streams, a0, stride, k, ak, d_out, s);
                    }});
    }
};

// The entry points of a call over a list of streams (the six across calls and the pair matrix) are one statement each,
// as the single-stream queries' are.  What every such call checks of its lists before it reads them:
static bool across_lists(uint32_t n_streams, const void *const *a, const void *const *b)
{
    if (n_streams == 0 || n_streams > ATSC_ACROSS_MAX_STREAMS || !a) return false;
    for (uint32_t k = 0; k < n_streams; ++k)
        if (!a[k] || (b && !b[k])) return false;
    return true;
}
static constexpr const char *ACROSS_LISTS = "n_streams outside [1, 64], a null list or a null entry";
// whether a host or stream call tests that `out` lies at a multiple of 8 bytes: every call but the across' own and the
// pair matrix's host call
enum OutAlign { OUT_ANY, OUT_ALIGN8 };

// the device call: the lists, then the inputs, then the query's own dev
template <class Q>
static int across_call_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp, const uint8_t *const *d_body,
                           uint64_t n_windows, const uint64_t *begin, const uint64_t *count, void *d_out, void *stream, const Q &q)
{
    if (!ctx || !d_body || !across_lists(n_streams, (const void *const *)dp, (const void *const *)d_body))
        return fail_in(ctx, ATSC_E_INVALID, Q::CALL, ACROSS_LISTS);
    QueryInput in[MAX_INPUTS];
    for (uint32_t k = 0; k < n_streams; ++k) in[k] = QueryInput{dp[k], d_body[k], 0};
    return q.dev(ctx, in, n_windows, begin, count, d_out, stream);
}

// the host call: the lists, then out's alignment where the call tests it, then query_host
template <class Q>
static int across_call_host(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                            const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count, void *out,
                            OutAlign align, const Q &q)
{
    if (!ctx || !body_len || !has_count || !across_lists(n_streams, (const void *const *)body, nullptr))
        return fail_in(ctx, ATSC_E_INVALID, Q::CALL, ACROSS_LISTS);
    if (align == OUT_ALIGN8 && ((uintptr_t)out & 7u)) return fail_in(ctx, ATSC_E_INVALID, Q::CALL, "out is not 8-byte aligned");
    HostBody hb[MAX_INPUTS];
    for (uint32_t k = 0; k < n_streams; ++k) hb[k] = HostBody{body[k], body_len[k], has_count[k]};
    return query_host(ctx, hb, n_windows, begin, count, out, q);
}

extern "C" int atsc_across_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp, const uint8_t *const *d_body,
                                       uint64_t n_windows, const uint64_t *begin, const uint64_t *count, uint64_t stride,
                                       atsc_across_record *d_out, void *stream)
{
    ATSC_API_BEGIN
    return across_call_dev(ctx, n_streams, dp, d_body, n_windows, begin, count, d_out, stream,
                           AcrossQuery{{n_streams, stride, count, n_windows}});
    ATSC_API_END
}

extern "C" int atsc_across_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                   const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                   uint64_t stride, atsc_across_record *out)
{
    ATSC_API_BEGIN
    return across_call_host(ctx, n_streams, body, body_len, has_count, n_windows, begin, count, out, OUT_ANY,
                            AcrossQuery{{n_streams, stride, count, n_windows}});
    ATSC_API_END
}

extern "C" int atsc_across_quantile_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                                const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                                const uint64_t *count, uint64_t stride, uint32_t n_q, const double *q, int method,
                                                double *d_out, void *stream)
{
    ATSC_API_BEGIN
    return across_call_dev(ctx, n_streams, dp, d_body, n_windows, begin, count, d_out, stream,
                           AcrossQntQuery{{n_streams, stride, count, n_windows}, n_q, q, method});
    ATSC_API_END
}

extern "C" int atsc_across_quantile_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                            const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                            uint64_t stride, uint32_t n_q, const double *q, int method, double *out)
{
    ATSC_API_BEGIN
    return across_call_host(ctx, n_streams, body, body_len, has_count, n_windows, begin, count, out, OUT_ALIGN8,
                            AcrossQntQuery{{n_streams, stride, count, n_windows}, n_q, q, method});
    ATSC_API_END
}

extern "C" int atsc_across_extremes_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                                const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                                const uint64_t *count, uint64_t stride, uint32_t k, void *d_out, void *stream)
{
    ATSC_API_BEGIN
    return across_call_dev(ctx, n_streams, dp, d_body, n_windows, begin, count, d_out, stream,
                           AcrossExtQuery{{n_streams, stride, count, n_windows}, k});
    ATSC_API_END
}

extern "C" int atsc_across_extremes_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                            const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                            uint64_t stride, uint32_t k, void *out)
{
    ATSC_API_BEGIN
    return across_call_host(ctx, n_streams, body, body_len, has_count, n_windows, begin, count, out, OUT_ALIGN8,
                            AcrossExtQuery{{n_streams, stride, count, n_windows}, k});
    ATSC_API_END
}

extern "C" int atsc_across_values_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                              const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                              const uint64_t *count, uint64_t stride, uint32_t k, double above, void *d_out,
                                              void *stream)
{
    ATSC_API_BEGIN
    return across_call_dev(ctx, n_streams, dp, d_body, n_windows, begin, count, d_out, stream,
                           AcrossValQuery{{n_streams, stride, count, n_windows}, k, above});
    ATSC_API_END
}

extern "C" int atsc_across_values_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                          const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                          uint64_t stride, uint32_t k, double above, void *out)
{
    ATSC_API_BEGIN
    return across_call_host(ctx, n_streams, body, body_len, has_count, n_windows, begin, count, out, OUT_ALIGN8,
                            AcrossValQuery{{n_streams, stride, count, n_windows}, k, above});
    ATSC_API_END
}

extern "C" int atsc_across_moments_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                               const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                               const uint64_t *count, uint64_t stride, atsc_across_moments *d_out, void *stream)
{
    ATSC_API_BEGIN
    return across_call_dev(ctx, n_streams, dp, d_body, n_windows, begin, count, d_out, stream,
                           AcrossMomQuery{{n_streams, stride, count, n_windows}});
    ATSC_API_END
}

extern "C" int atsc_across_moments_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                           const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                           uint64_t stride, atsc_across_moments *out)
{
    ATSC_API_BEGIN
    return across_call_host(ctx, n_streams, body, body_len, has_count, n_windows, begin, count, out, OUT_ALIGN8,
                            AcrossMomQuery{{n_streams, stride, count, n_windows}});
    ATSC_API_END
}

extern "C" int atsc_across_histogram_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                                 const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                                 const uint64_t *count, uint64_t stride, uint32_t n_edges, const double *edges,
                                                 int closed, uint64_t *d_out, void *stream)
{
    ATSC_API_BEGIN
    return across_call_dev(ctx, n_streams, dp, d_body, n_windows, begin, count, d_out, stream,
                           AcrossHistQuery{{n_streams, stride, count, n_windows}, n_edges, edges, closed});
    ATSC_API_END
}

extern "C" int atsc_across_histogram_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body,
                                             const uint64_t *body_len, const int *has_count, uint64_t n_windows,
                                             const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t n_edges,
                                             const double *edges, int closed, uint64_t *out)
{
    ATSC_API_BEGIN
    return across_call_host(ctx, n_streams, body, body_len, has_count, n_windows, begin, count, out, OUT_ALIGN8,
                            AcrossHistQuery{{n_streams, stride, count, n_windows}, n_edges, edges, closed});
    ATSC_API_END
}

// Host only: the records of one position from consecutive sub-lists, folded from the left by the moments' Merge
// (node_merge, atsc_moment_rule.h: the kernels' own copy; this file is compiled with -ffp-contract=off as they are).
// The position half of a node stays zero.
extern "C" int atsc_across_moments_merge(const atsc_across_moments *records, uint64_t n, atsc_across_moments *out)
{
    struct HostNode {
        double mx, m2x, mt, m2t, c;
        uint64_t n;
    };
    if (!out || (n && !records)) return ATSC_E_INVALID;
    HostNode a{0.0, 0.0, 0.0, 0.0, 0.0, 0};
    uint64_t nans = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const atsc_across_moments &r = records[i];
        nans += r.nans;
        if (a.n + r.count > 0xFFFFFFFFull || nans > 0xFFFFFFFFull) return ATSC_E_INVALID;
        a = node_merge<false>(a, HostNode{r.mean, r.m2, 0.0, 0.0, 0.0, r.count});
    }
    const double nan = std::numeric_limits<double>::quiet_NaN();
    *out = atsc_across_moments{(uint32_t)a.n, (uint32_t)nans, a.n ? a.mx : nan, a.n ? a.m2x : nan};
    return ATSC_OK;
}

// Host only: what a caller reads off the across moments, by atsc_moments_fit's definitions.
extern "C" int atsc_across_moments_fit(const atsc_across_moments *m, uint64_t n, atsc_across_fit *out)
{
    if (n && (!m || !out)) return ATSC_E_INVALID;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint64_t i = 0; i < n; ++i) {
        const atsc_across_moments &a = m[i];
        atsc_across_fit &r = out[i];
        if (a.count == 0) {
            r.mean = r.variance = r.stddev = r.sample_variance = r.sample_stddev = nan;
            continue;
        }
        r.mean = a.mean;
        r.variance = a.m2 / (double)a.count;
        r.stddev = std::sqrt(r.variance);
        r.sample_variance = a.count < 2 ? nan : a.m2 / (double)(a.count - 1);
        r.sample_stddev = std::sqrt(r.sample_variance);
    }
    return ATSC_OK;
}

// ------------------------------------------------------------------------------------------
// windowed pair matrix: the pair moments of every pair of up to 64 streams over sample windows (atsc_pair_matrix.hip)
// ------------------------------------------------------------------------------------------
extern "C" int atsc_pair_matrix_windows_dev(atsc_ctx *ctx, uint32_t n_streams, const atsc_dplan *const *dp,
                                            const uint8_t *const *d_body, uint64_t n_windows, const uint64_t *begin,
                                            const uint64_t *count, atsc_window_pair *d_out, void *stream)
{
    ATSC_API_BEGIN
    return across_call_dev(ctx, n_streams, dp, d_body, n_windows, begin, count, d_out, stream,
                           PairMatrixQuery{n_streams, n_windows});
    ATSC_API_END
}

extern "C" int atsc_pair_matrix_windows(atsc_ctx *ctx, uint32_t n_streams, const uint8_t *const *body, const uint64_t *body_len,
                                        const int *has_count, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                        atsc_window_pair *out)
{
    ATSC_API_BEGIN
    return across_call_host(ctx, n_streams, body, body_len, has_count, n_windows, begin, count, out, OUT_ANY,
                            PairMatrixQuery{n_streams, n_windows});
    ATSC_API_END
}

// ------------------------------------------------------------------------------------------
// the same queries on a stream under construction (atsc_stream.cpp): its records, then the host call
// ------------------------------------------------------------------------------------------
// a stream without a frame holds only empty windows at 0
static bool only_empty_at_zero(uint64_t n_windows, const uint64_t *begin, const uint64_t *count)
{
    for (uint64_t i = 0; i < n_windows; ++i)
        if (begin[i] != 0 || count[i] != 0) return false;
    return true;
}

extern "C" int atsc_stream_decompress_window(atsc_stream *s, uint64_t begin, uint64_t count, double **out, uint64_t *n)
{
    ATSC_API_BEGIN
    if (!s || !out || !n) return ATSC_E_INVALID;
    *out = nullptr;
    *n = 0;
    std::vector<uint8_t> body;
    atsc_ctx *ctx = nullptr;
    int rc = stream_body(s, body, &ctx);
    if (rc) return rc;
    if (body.empty()) {
        if (!only_empty_at_zero(1, &begin, &count)) return ATSC_E_INVALID;
        *out = (double *)malloc(8);
        return *out ? ATSC_OK : ATSC_E_NOMEM;
    }
    double *buf = (double *)big_alloc((count ? count : 1) * sizeof(double));
    if (!buf) return ATSC_E_NOMEM;
    uint64_t got = 0;
    rc = atsc_decompress_window(ctx, body.data(), body.size(), 0, begin, count, buf, count, &got);
    if (rc) {
        atsc_free(buf);
        return rc;
    }
    *out = buf;
    *n = got;
    return ATSC_OK;
    ATSC_API_END
}

// The stream call of a query over the streams st[0 .. query_inputs(q)), which must share a context.  The query's own check
// comes without a context (it has never left a message on the stream's) and before the pending chunks are compressed; a
// stream without a frame admits only empty windows at 0, and where every stream is one they get the query's empty result.
template <class Q>
static int query_stream(atsc_stream *const *st, uint64_t n_windows, const uint64_t *begin, const uint64_t *count, void *out,
                        const Q &q)
{
    const int n_in = query_inputs(q);
    for (int k = 0; k < n_in; ++k)
        if (!st[k]) return ATSC_E_INVALID;
    if (n_windows && (!begin || !count || !out)) return ATSC_E_INVALID;
    int rc = q.check(nullptr);
    if (rc) return rc;
    std::vector<std::vector<uint8_t>> body(n_in);
    atsc_ctx *ctx[MAX_INPUTS] = {};
    HostBody hb[MAX_INPUTS];
    bool none = false;
    for (int k = 0; k < n_in; ++k) {
        rc = stream_body(st[k], body[k], &ctx[k]);
        if (rc) return rc;
        if (ctx[k] != ctx[0]) return fail_in(ctx[0], ATSC_E_INVALID, Q::CALL, "streams of different contexts");
        none = none || body[k].empty();
        hb[k] = HostBody{body[k].data(), body[k].size(), 0};
    }
    if (none) {
        if (!only_empty_at_zero(n_windows, begin, count)) return ATSC_E_INVALID;
        q.fill_empty(out, n_windows);
        return ATSC_OK;
    }
    return query_host(ctx[0], hb, n_windows, begin, count, out, q);
}
// (one stream)
template <class Q>
static int query_stream(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count, void *out, const Q &q)
{
    return query_stream(&s, n_windows, begin, count, out, q);
}
// (a list of streams: the across calls and the pair matrix; a bare code, as above, where the list or out's alignment fails)
template <class Q>
static int across_call_stream(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows, const uint64_t *begin,
                              const uint64_t *count, void *out, OutAlign align, const Q &q)
{
    if (!across_lists(n_streams, (const void *const *)streams, nullptr) || (align == OUT_ALIGN8 && ((uintptr_t)out & 7u)))
        return ATSC_E_INVALID;
    return query_stream(streams, n_windows, begin, count, out, q);
}

extern "C" int atsc_stream_aggregate_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                             atsc_window_stats *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, AggQuery());
    ATSC_API_END
}

extern "C" int atsc_stream_moments_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                           atsc_window_moments *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, MomQuery());
    ATSC_API_END
}

extern "C" int atsc_stream_delta_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                         atsc_window_delta *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, DltQuery());
    ATSC_API_END
}

extern "C" int atsc_stream_runs_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                        int op, double limit, atsc_window_runs *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, RunQuery{op, limit});
    ATSC_API_END
}

extern "C" int atsc_stream_extremes_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                            uint32_t k, void *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, ExtQuery{k});
    ATSC_API_END
}

extern "C" int atsc_stream_values_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                          uint32_t k, double above, void *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, ValQuery{k, above});
    ATSC_API_END
}

extern "C" int atsc_stream_quantile_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                            uint32_t n_q, const double *q, int method, double *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, QntQuery{n_q, q, method});
    ATSC_API_END
}

extern "C" int atsc_stream_histogram_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                             uint32_t n_edges, const double *edges, int closed, uint64_t *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, HstQuery{n_edges, edges, closed});
    ATSC_API_END
}

extern "C" int atsc_stream_select_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                          int op, double limit, uint64_t cap, void *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, SelQuery{op, limit, cap});
    ATSC_API_END
}

extern "C" int atsc_stream_rolling_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                           uint64_t width, uint64_t stride, atsc_window_rolling *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, RollQuery{width, stride, count, n_windows});
    ATSC_API_END
}

extern "C" int atsc_stream_rolling_delta_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                                 uint64_t width, uint64_t stride, atsc_window_delta *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, RollDeltaQuery{width, stride, count, n_windows});
    ATSC_API_END
}

extern "C" int atsc_stream_rolling_runs_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                                uint64_t width, uint64_t stride, int op, double limit, atsc_window_runs *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, RollRunsQuery{width, stride, op, limit, count, n_windows});
    ATSC_API_END
}

extern "C" int atsc_stream_rolling_moments_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin, const uint64_t *count,
                                                   uint64_t width, uint64_t stride, atsc_window_moments *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, RollMomentsQuery{width, stride, count, n_windows});
    ATSC_API_END
}

extern "C" int atsc_stream_rolling_quantile_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin,
                                                    const uint64_t *count, uint64_t width, uint64_t stride, uint32_t n_q,
                                                    const double *q, int method, double *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out, RollQuantileQuery{width, stride, count, n_windows, n_q, q, method});
    ATSC_API_END
}

extern "C" int atsc_stream_rolling_histogram_windows(atsc_stream *s, uint64_t n_windows, const uint64_t *begin,
                                                     const uint64_t *count, uint64_t width, uint64_t stride, uint32_t n_edges,
                                                     const double *edges, int closed, uint64_t *out)
{
    ATSC_API_BEGIN
    return query_stream(s, n_windows, begin, count, out,
                        RollHistogramQuery{width, stride, count, n_windows, n_edges, edges, closed});
    ATSC_API_END
}

extern "C" int atsc_stream_pair_windows(atsc_stream *x, atsc_stream *y, uint64_t n_windows, const uint64_t *begin,
                                        const uint64_t *count, atsc_window_pair *out)
{
    ATSC_API_BEGIN
    atsc_stream *const st[2] = {x, y};
    return query_stream(st, n_windows, begin, count, out, PairQuery());
    ATSC_API_END
}

extern "C" int atsc_stream_rolling_pair_windows(atsc_stream *x, atsc_stream *y, uint64_t n_windows, const uint64_t *begin,
                                                const uint64_t *count, uint64_t width, uint64_t stride, atsc_window_pair *out)
{
    ATSC_API_BEGIN
    atsc_stream *const st[2] = {x, y};
    return query_stream(st, n_windows, begin, count, out, RollPairQuery{width, stride, count, n_windows});
    ATSC_API_END
}

extern "C" int atsc_stream_across_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                          const uint64_t *begin, const uint64_t *count, uint64_t stride, atsc_across_record *out)
{
    ATSC_API_BEGIN
    return across_call_stream(streams, n_streams, n_windows, begin, count, out, OUT_ANY,
                              AcrossQuery{{n_streams, stride, count, n_windows}});
    ATSC_API_END
}

extern "C" int atsc_stream_across_quantile_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                                   const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t n_q,
                                                   const double *q, int method, double *out)
{
    ATSC_API_BEGIN
    return across_call_stream(streams, n_streams, n_windows, begin, count, out, OUT_ALIGN8,
                              AcrossQntQuery{{n_streams, stride, count, n_windows}, n_q, q, method});
    ATSC_API_END
}

extern "C" int atsc_stream_across_extremes_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                                   const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t k,
                                                   void *out)
{
    ATSC_API_BEGIN
    return across_call_stream(streams, n_streams, n_windows, begin, count, out, OUT_ALIGN8,
                              AcrossExtQuery{{n_streams, stride, count, n_windows}, k});
    ATSC_API_END
}

extern "C" int atsc_stream_across_values_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                                 const uint64_t *begin, const uint64_t *count, uint64_t stride, uint32_t k,
                                                 double above, void *out)
{
    ATSC_API_BEGIN
    return across_call_stream(streams, n_streams, n_windows, begin, count, out, OUT_ALIGN8,
                              AcrossValQuery{{n_streams, stride, count, n_windows}, k, above});
    ATSC_API_END
}

extern "C" int atsc_stream_across_moments_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                                  const uint64_t *begin, const uint64_t *count, uint64_t stride,
                                                  atsc_across_moments *out)
{
    ATSC_API_BEGIN
    return across_call_stream(streams, n_streams, n_windows, begin, count, out, OUT_ALIGN8,
                              AcrossMomQuery{{n_streams, stride, count, n_windows}});
    ATSC_API_END
}

extern "C" int atsc_stream_across_histogram_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                                    const uint64_t *begin, const uint64_t *count, uint64_t stride,
                                                    uint32_t n_edges, const double *edges, int closed, uint64_t *out)
{
    ATSC_API_BEGIN
    return across_call_stream(streams, n_streams, n_windows, begin, count, out, OUT_ALIGN8,
                              AcrossHistQuery{{n_streams, stride, count, n_windows}, n_edges, edges, closed});
    ATSC_API_END
}

extern "C" int atsc_stream_pair_matrix_windows(atsc_stream *const *streams, uint32_t n_streams, uint64_t n_windows,
                                               const uint64_t *begin, const uint64_t *count, atsc_window_pair *out)
{
    ATSC_API_BEGIN
    return across_call_stream(streams, n_streams, n_windows, begin, count, out, OUT_ALIGN8,
                              PairMatrixQuery{n_streams, n_windows});
    ATSC_API_END
}
