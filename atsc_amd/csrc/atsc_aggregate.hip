// atsc_aggregate.hip -- gfx950 kernels of the windowed aggregates (atsc_aggregate_windows_dev): count, min, max, sum,
// first and last of sample windows, reduced from decoded samples in the call's scratch.
//
// The sum's order is part of the contract (include/atsc_hip.h, DESIGN.md "Windowed aggregates"):
//   * tiles of AGG_TILE = 2048 samples at multiples of 2048 in the stream index; a slot outside the window or holding
//     NaN contributes -0.0 (IEEE's exact additive identity);
//   * in a tile, virtual lane v (0..255) sums the pairs (x[512 t + 2 v] + x[512 t + 2 v + 1]) for t = 0..3 as
//     (p0 + p1) + (p2 + p3); the 256 lane sums then go through a halving tree, s[v] += s[v + h] for h = 128, 64, .., 1;
//   * a window's tile partials, in tile order, go through a pairwise tree: q[i] = q[2 i] + q[2 i + 1] level by level,
//     a missing right operand being -0.0.
// One wavefront reduces one tile (lane l holds the virtual lanes l, l + 64, l + 128, l + 192) or one group of 64 tile
// partials of a window.  No atomics: every partial has one writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// the term of one slot into s; min, max and count as they go
__device__ __forceinline__ void acc_take(double v, bool in, double &s, double &mn, double &mx, uint32_t &cnt)
{
    const bool ok = in && !__builtin_isnan(v);
    s = ok ? v : -0.0;
    mn = ok ? (v < mn ? v : mn) : mn;
    mx = ok ? (v > mx ? v : mx) : mx;
    cnt += ok ? 1u : 0u;
}

__device__ __forceinline__ DevAggPart acc_add(DevAggPart a, const DevAggPart &b)
{
    a.sum = a.sum + b.sum;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.count += b.count;
    return a;
}

}  // namespace

// One wavefront per DevAggTile: the slots [lo, hi) of the tile at scratch[src] into part[dst]; FIRST / LAST also copy
// the window's first (slot lo) / last (slot hi - 1) sample as it is, NaN included.
__global__ __launch_bounds__(256) void k_agg_tiles(const DevAggTile *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, DevAggPart *__restrict__ part,
                                                   double *__restrict__ fl)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevAggTile t = tasks[i];
    const double *x = scratch + t.src;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    uint32_t cnt = 0;
    double s[1];
    tile_lane_sums<1>(s, [&mn, &mx, &cnt, lane, x, t](uint32_t k, uint32_t q, double (&p)[1]) {
        const uint32_t j = tile_slot(lane + 64u * k, q);
        const double2 d = tile_load(x, j, t.lo, t.hi, -0.0);
        double a, b;
        acc_take(d.x, tile_in(j, t.lo, t.hi), a, mn, mx, cnt);
        acc_take(d.y, tile_in(j + 1u, t.lo, t.hi), b, mn, mx, cnt);
        p[0] = a + b;
    });
    const DevAggPart a = wave_halve(DevAggPart{s[0], mn, mx, cnt}, acc_add);
    if (lane == 0) {
        part[t.dst] = a;
        if (t.flags & AGG_FIRST) fl[2ull * t.win] = x[t.lo];
        if (t.flags & AGG_LAST) fl[2ull * t.win + 1] = x[t.hi - 1];
    }
}

// One wavefront per DevAggComb: the group's partials through comb_reduce, then, in the final pass, into the window's
// atsc_window_stats (six 8-byte fields, one per lane).
__global__ __launch_bounds__(256) void k_agg_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                     DevAggPart *__restrict__ part, const double *__restrict__ fl,
                                                     uint64_t *__restrict__ stats)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const DevAggPart a = comb_reduce(c, lane, part, DevAggPart{-0.0, __builtin_inf(), -__builtin_inf(), 0}, acc_add);
    if (!c.final_) return;
    const uint64_t cnt = __shfl(a.count, 0, 64);
    const double sum = __shfl(a.sum, 0, 64), mn = __shfl(a.mn, 0, 64), mx = __shfl(a.mx, 0, 64);
    const double nan = __builtin_nan("");
    if (lane < 6) {
        uint64_t w;
        switch (lane) {
        case 0: w = cnt; break;
        case 1: w = __double_as_longlong(cnt ? mn : nan); break;
        case 2: w = __double_as_longlong(cnt ? mx : nan); break;
        case 3: w = __double_as_longlong(cnt ? sum : 0.0); break;
        case 4: w = __double_as_longlong(c.n ? fl[2ull * c.win] : nan); break;
        default: w = __double_as_longlong(c.n ? fl[2ull * c.win + 1] : nan); break;
        }
        stats[6ull * c.dst + lane] = w;
    }
}

hipError_t launch_agg_tiles(const DevAggTile *tasks, uint32_t n, const double *scratch, DevAggPart *part, double *fl,
                            hipStream_t s)
{
    return launch_wave_tasks(k_agg_tiles, n, s, tasks, n, scratch, part, fl);
}

hipError_t launch_agg_combine(const DevAggComb *tasks, uint32_t n, DevAggPart *part, const double *fl, void *stats,
                              hipStream_t s)
{
    return launch_wave_tasks(k_agg_combine, n, s, tasks, n, part, fl, (uint64_t *)stats);
}

}  // namespace atsc
