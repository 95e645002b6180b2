// atsc_moments.hip -- gfx950 kernels of the windowed moments (atsc_moments_windows_dev): the centred moments of value x
// and sample position t of sample windows, reduced from decoded samples in the call's scratch.
//
// The node, its merge and the tree are atsc_moment_node.h's, which the windowed pair moments share (the contract:
// include/atsc_hip.h, DESIGN.md "Windowed moments").  The leaf of stream index i is (1, x[i], 0, (double)i, 0, 0), a slot
// outside the window or holding NaN the empty node.
// One wavefront reduces one tile (lane l holds the virtual lanes l, l + 64, l + 128, l + 192) or one group of 64 tile
// partials of a window.  No atomics: every partial has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_moment_node.h"

namespace atsc {

namespace {

// a virtual lane's eight leaves (four 16-byte loads d[q] at slots tile_slot(v, q), positions from t0) into its node
template <bool EQ>
__device__ __forceinline__ Node mom_lane_node(const double2 (&d)[4], const bool (&ok)[8], double t0)
{
    return lane_node<EQ>([&](int q, int e) {
        const double t = t0 + 512.0 * q;
        return e ? node_leaf(d[q].y, t + 1.0, ok[2 * q + 1]) : node_leaf(d[q].x, t, ok[2 * q]);
    });
}

}  // namespace

// One wavefront per DevPosTile: the slots [lo, hi) of the tile at scratch[src], whose slot 0 is sample t0 of the
// stream, into part[dst].  A virtual lane's eight leaves are reduced as they are loaded.  Where every one of the
// wavefront's merges joins two nodes of the same non-zero count (a NaN-free stretch that the window covers), the
// merges skip the divide behind a wave-uniform test: the same bits, see node_merge.
__global__ __launch_bounds__(256) void k_mom_tiles(const DevPosTile *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, DevMomPart *__restrict__ part)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevPosTile t = tasks[i];
    const double *x = scratch + t.src;
    // positions are exact in f64: a stream index is below 2^53, so (double)t0 + (double)j == (double)(t0 + j)
    const double tb = (double)t.t0;
    bool full = true;
    Node s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = lane + 64u * k;
        double2 d[4];
        bool ok[8];
        bool all = true;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t j = tile_slot(v, q);
            d[q] = tile_load(x, j, t.lo, t.hi, 0.0);
            ok[2 * q] = tile_in(j, t.lo, t.hi) && !__builtin_isnan(d[q].x);
            ok[2 * q + 1] = tile_in(j + 1u, t.lo, t.hi) && !__builtin_isnan(d[q].y);
            all = all && ok[2 * q] && ok[2 * q + 1];
        }
        const double t0 = tb + (double)(2u * v);
        if (__all(all)) s[k] = mom_lane_node<true>(d, ok, t0);
        else s[k] = mom_lane_node<false>(d, ok, t0);
        full = full && all;
    }
    Node a;
    if (__all(full)) a = tile_node<true>(s);
    else a = tile_node<false>(s);
    if (lane == 0) part[t.dst] = DevMomPart{a.mx, a.m2x, a.mt, a.m2t, a.c, a.n};
}

// One wavefront per DevAggComb: the group's partials through comb_reduce (a missing right operand is the empty node),
// then, in the final pass, into the window's atsc_window_moments (six 8-byte fields, one per lane): t_mean counted from
// the window's begin[win], and NaN in the five doubles of a window without a sample.
__global__ __launch_bounds__(256) void k_mom_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                     DevMomPart *__restrict__ part, const uint64_t *__restrict__ begin,
                                                     uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const DevMomPart a =
        comb_reduce(c, lane, part, DevMomPart{0.0, 0.0, 0.0, 0.0, 0.0, 0}, node_merge<false, DevMomPart>);
    if (!c.final_) return;
    const uint64_t cnt = __shfl(a.n, 0, 64);
    const double mx = __shfl(a.mx, 0, 64), m2x = __shfl(a.m2x, 0, 64), mt = __shfl(a.mt, 0, 64),
                 m2t = __shfl(a.m2t, 0, 64), cv = __shfl(a.c, 0, 64);
    if (lane < 6) {
        double v;
        switch (lane) {
        case 1: v = mx; break;
        case 2: v = m2x; break;
        case 3: v = mt - (double)begin[c.win]; break;
        case 4: v = m2t; break;
        default: v = cv; break;
        }
        out[6ull * c.dst + lane] = lane == 0 ? cnt : (uint64_t)__double_as_longlong(cnt ? v : __builtin_nan(""));
    }
}

hipError_t launch_mom_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, DevMomPart *part, hipStream_t s)
{
    return launch_wave_tasks(k_mom_tiles, n, s, tasks, n, scratch, part);
}

hipError_t launch_mom_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part, const uint64_t *begin, void *out,
                              hipStream_t s)
{
    return launch_wave_tasks(k_mom_combine, n, s, tasks, n, part, begin, (uint64_t *)out);
}

}  // namespace atsc
