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

#include "atsc_device.h"

namespace atsc {

namespace {

struct Acc {
    double sum, mn, mx;
    uint64_t count;
};

__device__ __forceinline__ Acc acc_identity() { return Acc{-0.0, __builtin_inf(), -__builtin_inf(), 0}; }

__device__ __forceinline__ void acc_take(double v, bool in, double &s, double &mn, double &mx, uint32_t &cnt)
{
    const bool ok = in && !__builtin_isnan(v);
    s = ok ? v : -0.0;
    mn = ok ? (v < mn ? v : mn) : mn;
    mx = ok ? (v > mx ? v : mx) : mx;
    cnt += ok ? 1u : 0u;
}

__device__ __forceinline__ Acc acc_shfl_down(const Acc &a, unsigned off)
{
    Acc o;
    o.sum = __shfl_down(a.sum, off, 64);
    o.mn = __shfl_down(a.mn, off, 64);
    o.mx = __shfl_down(a.mx, off, 64);
    o.count = __shfl_down(a.count, off, 64);
    return o;
}

__device__ __forceinline__ void acc_add(Acc &a, const Acc &b)
{
    a.sum = a.sum + b.sum;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.count += b.count;
}

}  // namespace

// One wavefront per DevAggTile: the slots [lo, hi) of the tile at scratch[src] into part[dst]; FIRST / LAST also copy
// the window's first (slot lo) / last (slot hi - 1) sample as it is, NaN included.
__global__ __launch_bounds__(256) void k_agg_tiles(const DevAggTile *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, DevAggPart *__restrict__ part,
                                                   double *__restrict__ fl)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n) return;
    const DevAggTile t = tasks[i];
    const double *x = scratch + t.src;
    double mn = __builtin_inf(), mx = -__builtin_inf();
    uint32_t cnt = 0;
    double s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t v = lane + 64u * k;
        double p[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t j = 512u * q + 2u * v;
            double2 d = make_double2(-0.0, -0.0);
            if (j < t.hi && j + 2u > t.lo) d = *(const double2 *)(x + j);  // 16-byte load; scratch tiles are 16-byte aligned
            double a, b;
            acc_take(d.x, j >= t.lo && j < t.hi, a, mn, mx, cnt);
            acc_take(d.y, j + 1u >= t.lo && j + 1u < t.hi, b, mn, mx, cnt);
            p[q] = a + b;
        }
        s[k] = (p[0] + p[1]) + (p[2] + p[3]);
    }
    // halving tree over the 256 virtual lanes: h = 128 and 64 inside the lane, then 32 .. 1 across the wavefront
    Acc a{(s[0] + s[2]) + (s[1] + s[3]), mn, mx, cnt};
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) acc_add(a, acc_shfl_down(a, off));
    if (lane == 0) {
        part[t.dst] = DevAggPart{a.sum, a.mn, a.mx, a.count};
        if (t.flags & AGG_FIRST) fl[2ull * t.win] = x[t.lo];
        if (t.flags & AGG_LAST) fl[2ull * t.win + 1] = x[t.hi - 1];
    }
}

// One wavefront per DevAggComb: partials j = 64 g .. 64 g + 63 of a window's list (j < n; j == 0 at head, j == n - 1 at
// tail, else at mid + j) through the pairwise tree (lane l + 2^k into lane l), then into part[dst] or, in the final pass,
// the window's atsc_window_stats (six 8-byte fields, one per lane).
__global__ __launch_bounds__(256) void k_agg_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                     DevAggPart *__restrict__ part, const double *__restrict__ fl,
                                                     uint64_t *__restrict__ stats)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const uint64_t j = 64ull * c.g + lane;
    Acc a = acc_identity();
    if (j < c.n) {
        const DevAggPart p = part[j == 0 ? c.head : j == c.n - 1 ? c.tail : c.mid + j];
        a = Acc{p.sum, p.mn, p.mx, p.count};
    }
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) acc_add(a, acc_shfl_down(a, off));
    if (!c.final_) {
        if (lane == 0) part[c.dst] = DevAggPart{a.sum, a.mn, a.mx, a.count};
        return;
    }
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
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_agg_tiles, dim3((n + 3) / 4), dim3(256), 0, s, tasks, n, scratch, part, fl);
    return hipGetLastError();
}

hipError_t launch_agg_combine(const DevAggComb *tasks, uint32_t n, DevAggPart *part, const double *fl, void *stats,
                              hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_agg_combine, dim3((n + 3) / 4), dim3(256), 0, s, tasks, n, part, fl, (uint64_t *)stats);
    return hipGetLastError();
}

}  // namespace atsc
