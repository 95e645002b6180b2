// atsc_pair.hip -- gfx950 kernels of the windowed pair moments (atsc_pair_windows_dev): the centred moments and the
// co-moment of the values x and y of two streams over the same sample windows, reduced from the decoded samples of both
// in the call's two scratch regions.
//
// The node, its merge and the tree are atsc_moment_node.h's, which the windowed moments share, with the second stream's
// value where they have the position (the contract: include/atsc_hip.h, DESIGN.md "Windowed pair moments").  The leaf of
// stream index i is (1, x[i], 0, y[i], 0, 0); a slot outside the window, or one where x[i] or y[i] is NaN, the empty node.
// One wavefront reduces one tile (lane l holds the virtual lanes l, l + 64, l + 128, l + 192) or one group of 64 tile
// partials of a window.  No atomics: every partial has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_moment_node.h"

namespace atsc {

// One wavefront per DevPosTile: the slots [lo, hi) of the tile at sx[src] and sy[src] (the same slots of the two
// regions; t0 is not read) into part[dst].  A virtual lane's eight leaves are reduced as they are loaded, eight masked
// 16-byte loads.  Where every one of the wavefront's merges joins two nodes of the same non-zero count (a stretch
// without NaN in either stream that the window covers), the merges skip the divide behind a wave-uniform test: the
// same bits, see node_merge.
__global__ __launch_bounds__(256) void k_pair_tiles(const DevPosTile *__restrict__ tasks, uint32_t n,
                                                    const double *__restrict__ sx, const double *__restrict__ sy,
                                                    DevMomPart *__restrict__ part)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevPosTile t = tasks[i];
    const double *x = sx + t.src, *y = sy + t.src;
    bool full = true;
    Node s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = lane + 64u * k;
        double2 dx[4], dy[4];
        bool ok[8];
        bool all = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t j = tile_slot(v, q);
            dx[q] = tile_load(x, j, t.lo, t.hi, 0.0);
            dy[q] = tile_load(y, j, t.lo, t.hi, 0.0);
            ok[2 * q] = tile_in(j, t.lo, t.hi) && !__builtin_isnan(dx[q].x) && !__builtin_isnan(dy[q].x);
            ok[2 * q + 1] = tile_in(j + 1u, t.lo, t.hi) && !__builtin_isnan(dx[q].y) && !__builtin_isnan(dy[q].y);
            all = all && ok[2 * q] && ok[2 * q + 1];
        }
        auto leaf = [&](int q, int e) {
            return e ? node_leaf(dx[q].y, dy[q].y, ok[2 * q + 1]) : node_leaf(dx[q].x, dy[q].x, ok[2 * q]);
        };
        if (__all(all)) s[k] = lane_node<true>(leaf);
        else s[k] = lane_node<false>(leaf);
        full = full && all;
    }
    Node a;
    if (__all(full)) a = tile_node<true>(s);
    else a = tile_node<false>(s);
    if (lane == 0) part[t.dst] = DevMomPart{a.mx, a.m2x, a.mt, a.m2t, a.c, a.n};
}

// One wavefront per DevAggComb: the group's partials through comb_reduce (a missing right operand is the empty node),
// then, in the final pass, into the window's atsc_window_pair (six 8-byte fields, one per lane): NaN in the five doubles
// of a window without a sample.  No position is counted from a window's begin, so the kernel has no side table.
__global__ __launch_bounds__(256) void k_pair_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                      DevMomPart *__restrict__ part, uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const DevMomPart a =
        comb_reduce(c, lane, part, DevMomPart{0.0, 0.0, 0.0, 0.0, 0.0, 0}, node_merge<false, DevMomPart>);
    if (!c.final_) return;
    const uint64_t cnt = __shfl(a.n, 0, 64);
    const double mx = __shfl(a.mx, 0, 64), m2x = __shfl(a.m2x, 0, 64), my = __shfl(a.mt, 0, 64),
                 m2y = __shfl(a.m2t, 0, 64), cv = __shfl(a.c, 0, 64);
    if (lane < 6) {
        double v;
        switch (lane) {
        case 1: v = mx; break;
        case 2: v = m2x; break;
        case 3: v = my; break;
        case 4: v = m2y; break;
        default: v = cv; break;
        }
        out[6ull * c.dst + lane] = lane == 0 ? cnt : (uint64_t)__double_as_longlong(cnt ? v : __builtin_nan(""));
    }
}

hipError_t launch_pair_tiles(const DevPosTile *tasks, uint32_t n, const double *sx, const double *sy, DevMomPart *part,
                             hipStream_t s)
{
    return launch_wave_tasks(k_pair_tiles, n, s, tasks, n, sx, sy, part);
}

hipError_t launch_pair_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_pair_combine, n, s, tasks, n, part, (uint64_t *)out);
}

}  // namespace atsc
