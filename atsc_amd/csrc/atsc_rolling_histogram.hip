// atsc_rolling_histogram.hip -- gfx950 kernel of the windowed rolling histograms (atsc_rolling_histogram_windows_dev):
// the value-bin counts of the window [lo, lo + w) at every position of a range, from decoded samples in the call's
// scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed rolling histograms"): a position's row is the row
// atsc_histogram_windows gives for the listed window (lo, w) -- n_edges + 2 u64 counters, bins 0 .. n_edges by bin_of
// (atsc_hist_bins.h, the text atsc_histogram.hip bins with), then the NaN samples.  Counts are integers, so the row at
// position p + 1 is the row at p less the `stride` samples that leave plus the `stride` that enter, bit for bit.
//
// A task (DevRollTask) is a run of B consecutive positions of one range inside one piece (rh_task_positions, the
// host's rule); its samples are (B - 1) stride + w consecutive slots of the scratch.  One wavefront runs one task, a
// workgroup of 256 threads four of them.  LDS: the edges once, then one row of u32 counters per wavefront (a count
// cannot pass w <= 2^20).
//   first   clear the row, bin the first window 64 samples a trip (count_bins), store the row;
//   slide   (stride < w) per trip the wavefront loads up to 64 leaving samples and the up to 64 entering ones w slots
//           behind them, both coalesced, and bins them all at once: floor(64 / stride) positions a trip for a stride of
//           at most 64, ceil(stride / 64) trips a position above.  Then position after position, in order, the lanes
//           that hold that position's samples add -1 at the leaving bin and +1 at the entering one (nothing where the
//           two are one bin), and the wavefront stores the row, 64 counters a trip, widened to u64;
//   recount (stride >= w) the windows are disjoint: every position is a first row.
// Visibility of the counters across lanes: the row a wavefront stores was written by other lanes' LDS atomics, and the
// next position's atomics follow other lanes' reads of the row.  Both are ordered in the source by rh_row_sync
// (atsc_hist_bins.h): a
// wavefront-scope release fence, __builtin_amdgcn_wave_barrier() and a wavefront-scope acquire fence (rds_fill's pair in
// atsc_device.h, with the acquire side spelled out), so wavefronts run their tasks with trip counts of their own and the
// workgroup synchronises once, behind the edges' load.
// No global atomics; nothing here clears the result: every counter of every row has one writer, which stores it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_device.h"
#include "atsc_hist_bins.h"

namespace atsc {

namespace {

// the wavefront's counters as one row of the result, then the barrier in front of the next change of the counters
__device__ __forceinline__ void rh_store_row(const uint32_t *cnt, uint32_t rows, uint64_t *__restrict__ row, uint32_t lane)
{
    rh_row_sync();
    for (uint32_t i = lane; i < rows; i += 64u) row[i] = cnt[i];
    rh_row_sync();
}

// clears the counters, counts the w samples from x on and stores the row
template <int CLOSED>
__device__ __forceinline__ void rh_recount(uint32_t *cnt, uint32_t rows, const double *__restrict__ x, uint32_t w,
                                           const double *s_edge, uint32_t n_edges, uint32_t steps,
                                           uint64_t *__restrict__ row, uint32_t lane)
{
    for (uint32_t i = lane; i < rows; i += 64u) cnt[i] = 0;
    rh_row_sync();
    for (uint32_t o = 0; o < w; o += 64u) {
        const uint32_t e = o + lane;
        const uint32_t bin = e < w ? bin_of<CLOSED>(x[e], s_edge, n_edges, steps) : HST_NONE;
        count_bins(cnt, bin, lane);
    }
    rh_store_row(cnt, rows, row, lane);
}

}  // namespace

// One wavefront per task: workgroup b runs tasks 4 b .. 4 b + 3.  a0: the stream index of scratch[0].  Dynamic LDS: the
// edges, then four counter rows.
template <int CLOSED>
__global__ __launch_bounds__(256) void k_rh_slide(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                  const double *__restrict__ scratch, uint64_t a0, uint32_t w,
                                                  uint64_t stride, const double *__restrict__ edges, uint32_t n_edges,
                                                  uint32_t steps, uint64_t *__restrict__ out)
{
    extern __shared__ double s_mem[];
    double *s_edge = s_mem;
    const uint32_t rows = n_edges + 2u, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t *cnt = (uint32_t *)(s_mem + n_edges) + wv * rows;
    load_edges(s_edge, edges, n_edges);
    __syncthreads();
    const uint32_t ti = blockIdx.x * 4u + wv;
    if (ti >= n) return;
    const DevRollTask t = tasks[ti];
    const double *x = scratch + (t.lo - a0);
    uint64_t *row = out + t.rec * (uint64_t)rows;
    rh_recount<CLOSED>(cnt, rows, x, w, s_edge, n_edges, steps, row, lane);
    if (stride >= w) {  // disjoint windows
        for (uint32_t p = 1; p < t.n; ++p)
            rh_recount<CLOSED>(cnt, rows, x + (uint64_t)p * stride, w, s_edge, n_edges, steps, row + (uint64_t)p * rows, lane);
        return;
    }
    const uint32_t s = (uint32_t)stride;  // below w <= 2^20; (t.n - 1) s + w stays far below 2^32 (rh_task_positions)
    if (s <= 64u) {
        const uint32_t k = 64u / s, grp = lane / s;  // positions a trip; the one this lane's samples belong to
        for (uint32_t p0 = 1; p0 < t.n; p0 += k) {
            const uint32_t kk = min(k, t.n - p0);
            const uint32_t j = (p0 - 1u) * s + lane;  // leaves at position p0 + grp; x[j + w] enters there
            uint32_t bl = HST_NONE, be = HST_NONE;
            if (grp < kk) {
                const double dl = x[j], de = x[j + w];
                bl = bin_of<CLOSED>(dl, s_edge, n_edges, steps);
                be = bin_of<CLOSED>(de, s_edge, n_edges, steps);
            }
            for (uint32_t q = 0; q < kk; ++q) {
                if (grp == q && bl != be) {
                    atomicSub(&cnt[bl], 1u);
                    atomicAdd(&cnt[be], 1u);
                }
                rh_store_row(cnt, rows, row + (uint64_t)(p0 + q) * rows, lane);
            }
        }
        return;
    }
    for (uint32_t p = 1; p < t.n; ++p) {
        const uint32_t base = (p - 1u) * s;
        for (uint32_t o = 0; o < s; o += 64u) {
            const uint32_t e = o + lane;
            if (e < s) {
                const double dl = x[base + e], de = x[base + e + w];
                const uint32_t bl = bin_of<CLOSED>(dl, s_edge, n_edges, steps);
                const uint32_t be = bin_of<CLOSED>(de, s_edge, n_edges, steps);
                if (bl != be) {
                    atomicSub(&cnt[bl], 1u);
                    atomicAdd(&cnt[be], 1u);
                }
            }
        }
        rh_store_row(cnt, rows, row + (uint64_t)p * rows, lane);
    }
}

hipError_t launch_rh_slide(const DevRollTask *tasks, uint32_t n, const double *scratch, uint64_t a0, uint32_t w,
                           uint64_t stride, const double *edges, uint32_t n_edges, int closed, uint64_t *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t grid = (n + 3u) / 4u;
    const size_t lds = (size_t)n_edges * sizeof(double) + 4u * (size_t)(n_edges + 2u) * sizeof(uint32_t);
    if (closed == ATSC_HIST_RIGHT_CLOSED)
        hipLaunchKernelGGL(k_rh_slide<ATSC_HIST_RIGHT_CLOSED>, dim3(grid), dim3(256), lds, s, tasks, n, scratch, a0, w, stride,
                           edges, n_edges, search_steps(n_edges), out);
    else
        hipLaunchKernelGGL(k_rh_slide<ATSC_HIST_LEFT_CLOSED>, dim3(grid), dim3(256), lds, s, tasks, n, scratch, a0, w, stride,
                           edges, n_edges, search_steps(n_edges), out);
    return hipGetLastError();
}

}  // namespace atsc
