// atsc_across_histogram.hip -- gfx950 kernel of the windowed across histograms (atsc_across_histogram_windows_dev): at
// every position of a range, how many of the call's N streams hold a sample in each value bin -- a fleet heat map,
// `count by (job)(x > 0.9)`, one `le` bucket of an SLO over hosts.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across histograms"): a position's row is n_edges + 2 u64
// counters, bins 0 .. n_edges by bin_of (atsc_hist_bins.h, the text atsc_histogram.hip bins with), then the NaN
// samples; it is the sum over the streams of atsc_histogram_windows' rows of the window (position, 1).  The regions, the
// tasks and the wavefront's 64 positions of a task are atsc_across_positions.h's (slab_wave); a workgroup of 256 threads
// runs four wavefronts.  Dynamic LDS: the edges once, then per wavefront G rows of byte counters (a count cannot pass
// 64 streams) at a pitch of an odd number of 4-byte words:
//   words = ceil((n_edges + 2) / 4) | 1,  pitch = 4 words,  G = min(64, floor(14336 / pitch))   (ah_rows_a_pass)
// -- 64 rows up to n_edges = 218, 62 at 219, 13 at 1024; 8 n_edges + 4 G pitch <= 65536 bytes a workgroup, and 3.2 KB
// at 10 edges, so that the wavefront slots and not the LDS bound the occupancy there.  The odd pitch sends the lanes of
// a half wavefront that land in one bin to 32 different banks.
// A wavefront works through its 64 positions in passes of G:
//   clear   the G rows, a word a lane;
//   count   lane g < G walks the streams, eight at a time: loads scratch[reg[k] + slot] of the eight (at stride 1, 8 G
//           consecutive bytes a stream), then bins each and adds one to its own row -- a plain read-modify-write in the
//           lane's program order: a row has one owner, so there are no LDS atomics and no question of visibility
//           between lanes while counting;
//   store   the G rows are G (n_edges + 2) consecutive u64 of the result: the wavefront stores them 64 counters a trip,
//           widened from the bytes.
// Between the steps one rh_row_sync (atsc_hist_bins.h) orders the LDS accesses of the wavefront's lanes; wavefronts run
// their passes on their own and the workgroup synchronises once, behind the edges' load.
// No global atomics; nothing here clears the result: every counter of every row has one writer, which stores it.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_across_positions.h"
#include "atsc_hist_bins.h"

namespace atsc {

constexpr uint32_t AH_BATCH = 8;  // streams whose samples a lane loads together

// Position p's row is the n_edges + 2 counters at out[(t.rec + p) (n_edges + 2) ..].  G rows of `pitch` bytes a wavefront
// (ah_rows_a_pass, ah_row_pitch).
template <int CLOSED>
__global__ __launch_bounds__(256) void k_across_histogram_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                                    const double *__restrict__ scratch,
                                                                    const uint64_t *__restrict__ reg, uint32_t ns, uint64_t a0,
                                                                    uint64_t stride, const double *__restrict__ edges,
                                                                    uint32_t n_edges, uint32_t steps, uint32_t G, uint32_t pitch,
                                                                    uint64_t *__restrict__ out)
{
    extern __shared__ double s_mem[];
    double *s_edge = s_mem;
    const uint32_t rows = n_edges + 2u, lane = wave_lane();
    uint32_t i, p0;  // the wavefront's task and its first position of it: the lanes change roles between the steps
    const bool listed = slab_wave(n, i, p0);
    uint8_t *cnt = (uint8_t *)(s_mem + n_edges) + (threadIdx.x >> 6) * G * pitch;
    load_edges(s_edge, edges, n_edges);
    __syncthreads();  // (in front of every return)
    if (!listed) return;
    const DevRollTask t = tasks[i];
    if (p0 >= t.n) return;
    const uint32_t m = min(64u, t.n - p0);
    const uint64_t s0 = t.lo - a0 + (uint64_t)p0 * stride;
    uint64_t *o = out + (t.rec + p0) * (uint64_t)rows;
    const uint32_t dr = 64u / rows, dc = 64u % rows;  // a lane's step from one trip of the store to the next
    for (uint32_t g0 = 0; g0 < m; g0 += G) {
        const uint32_t g = min(G, m - g0);
        for (uint32_t j = lane; j < g * (pitch / 4u); j += 64u) ((uint32_t *)cnt)[j] = 0;
        rh_row_sync();
        if (lane < g) {
            const uint64_t slot = s0 + (uint64_t)(g0 + lane) * stride;
            uint8_t *row = cnt + lane * pitch;
            // AH_BATCH streams' samples are loaded before the first of them is binned: a search waits for LDS only, and
            // the loads' latency is paid once a batch, not once a stream (the last batch reads stream ns - 1 again)
            for (uint32_t k0 = 0; k0 < ns; k0 += AH_BATCH) {
                double v[AH_BATCH];
#pragma unroll
                for (uint32_t u = 0; u < AH_BATCH; ++u) v[u] = scratch[reg[min(k0 + u, ns - 1u)] + slot];
#pragma unroll
                for (uint32_t u = 0; u < AH_BATCH; ++u) {
                    if (k0 + u < ns) {
                        const uint32_t b = bin_of<CLOSED>(v[u], s_edge, n_edges, steps);
                        row[b] = (uint8_t)(row[b] + 1u);
                    }
                }
            }
        }
        rh_row_sync();
        uint64_t *og = o + (uint64_t)g0 * rows;
        uint32_t r = lane / rows, c = lane % rows;
        for (uint32_t j = lane; j < g * rows; j += 64u) {
            og[j] = cnt[r * pitch + c];
            r += dr;
            c += dc;
            if (c >= rows) {
                c -= rows;
                ++r;
            }
        }
        rh_row_sync();
    }
}

hipError_t launch_across_histogram_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                             uint32_t n_streams, uint64_t a0, uint64_t stride, const double *edges,
                                             uint32_t n_edges, int closed, uint64_t *out, hipStream_t s)
{
    static_assert(8u * HST_MAX_EDGES + 4u * AH_WAVE_LDS <= 65536u, "a workgroup's LDS");
    if (n == 0) return hipSuccess;
    if (!slab_grid_fits(n)) return hipErrorInvalidValue;
    if (n_streams == 0 || n_streams > 255u || n_edges == 0 || n_edges > HST_MAX_EDGES || ((uintptr_t)out & 7u))
        return hipErrorInvalidValue;
    const uint32_t G = ah_rows_a_pass(n_edges), pitch = ah_row_pitch(n_edges), grid = (n * ACR_SLABS + 3u) / 4u;
    const size_t lds = (size_t)n_edges * sizeof(double) + 4u * (size_t)G * pitch;
    if (closed == ATSC_HIST_RIGHT_CLOSED)
        hipLaunchKernelGGL(k_across_histogram_positions<ATSC_HIST_RIGHT_CLOSED>, dim3(grid), dim3(256), lds, s, tasks, n, scratch,
                           reg, n_streams, a0, stride, edges, n_edges, search_steps(n_edges), G, pitch, out);
    else
        hipLaunchKernelGGL(k_across_histogram_positions<ATSC_HIST_LEFT_CLOSED>, dim3(grid), dim3(256), lds, s, tasks, n, scratch,
                           reg, n_streams, a0, stride, edges, n_edges, search_steps(n_edges), G, pitch, out);
    return hipGetLastError();
}

}  // namespace atsc
