// atsc_rolling.hip -- gfx950 kernels of the windowed rolling (atsc_rolling_windows_dev): count, min, max and sum of the
// window [lo, lo + w) at every position of a range, from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed rolling").  term(j) is x[j], or -0.0 where x[j] is NaN;
// T(a, 0) = term(a) and T(a, l) = T(a, l - 1) + T(a + 2^(l-1), l - 1) for a a multiple of 2^l in the stream index; a
// window's sum is the left-to-right fold of T over its canonical chunks (from pos = lo: the largest l with pos a multiple
// of 2^l and pos + 2^l <= lo + w).  T does not depend on any window, so one pyramid of chunk partials per piece of the
// scratch serves every position in it:
//   pyramid    one workgroup per ROLL_TILE = 2048 aligned samples, eight consecutive ones a thread: the levels 1 .. 3 in
//              registers, 4 .. 9 across the wavefront by shuffles, 10 and 11 through LDS; the levels from ROLL_LOW = 3 up to
//              floor(log2 w) are stored;
//   upper      one wavefront per 64 aligned chunks of level 11 (and of level 17): the six levels above by shuffles;
//   positions  one wavefront per task, a lane per position: the lane walks its window's chunks left to right, a chunk
//              below ROLL_LOW formed from the samples by the same tree, the others read from the pyramid.
// A partial is (sum, min, max, count) and the signs of the zeros it holds.  No atomics: every partial and every record
// has one writer, and a chunk's value is the same bits wherever it is formed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// zeros: bit 0, a -0.0 sample; bit 1, a +0.0 sample
struct alignas(16) RollPart {
    double sum, mn, mx;
    uint32_t count, zeros;
};
static_assert(sizeof(RollPart) == 32 && sizeof(RollPart) == sizeof(DevAggPart), "a partial is 32 bytes");

// the record as the position kernel stores it: 32 bytes at once, at the 8-byte alignment the result has
struct alignas(8) RollRec {
    uint64_t count;
    double mn, mx, sum;
};
static_assert(sizeof(RollRec) == sizeof(atsc_window_rolling), "the record's layout");

DEVI RollPart roll_none() { return RollPart{-0.0, __builtin_inf(), -__builtin_inf(), 0u, 0u}; }

DEVI RollPart roll_leaf(double v)
{
    const bool ok = !__builtin_isnan(v);
    const uint32_t z = v == 0.0 ? ((uint64_t)__double_as_longlong(v) >> 63 ? 1u : 2u) : 0u;
    return RollPart{ok ? v : -0.0, ok ? v : __builtin_inf(), ok ? v : -__builtin_inf(), ok ? 1u : 0u, z};
}

// (the comparisons are the aggregates': atsc_aggregate.hip, acc_add)
DEVI RollPart roll_merge(RollPart a, const RollPart &b)
{
    a.sum = a.sum + b.sum;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    a.count += b.count;
    a.zeros |= b.zeros;
    return a;
}

DEVI RollPart roll_load(const RollPart *p)
{
    const double2 a = ((const double2 *)p)[0], b = ((const double2 *)p)[1];  // two 16-byte loads
    RollPart r;
    r.sum = a.x;
    r.mn = a.y;
    r.mx = b.x;
    const uint64_t w = (uint64_t)__double_as_longlong(b.y);
    r.count = (uint32_t)w;
    r.zeros = (uint32_t)(w >> 32);
    return r;
}

DEVI void roll_store(RollPart *p, const RollPart &r)
{
    ((double2 *)p)[0] = make_double2(r.sum, r.mn);
    ((double2 *)p)[1] = make_double2(r.mx, __longlong_as_double((long long)(((uint64_t)r.zeros << 32) | r.count)));
}

// The sign of a zero extreme of the window x[0, w) whose first sample is sample `lo` of the stream, where the window
// holds zeros of both signs: the aggregates' (atsc_aggregate.hip), whose comparisons keep the first of equal values in
// the order they visit the samples.  That is the window's first tile of 2048 with a zero in it, and of its zeros the
// first by real lane (the wave's halving tree prefers the lanes in bit-reversed order), virtual lane (0, 2, 1, 3),
// quarter and slot of the pair (tile_lane_sums, tile_slot).  true: -0.0.
DEVI bool roll_zero_sign(const double *x, uint64_t lo, uint64_t w)
{
    uint64_t tile = ~0ull;
    uint32_t best = ~0u;
    bool neg = false;
    for (uint64_t j = 0; j < w; ++j) {
        const uint64_t at = lo + j;
        if ((at >> 11) > tile) break;
        const double v = x[j];
        if (!(v == 0.0)) continue;
        const uint32_t s = (uint32_t)at & 2047u, vl = (s & 511u) >> 1, k = vl >> 6;
        const uint32_t key = ((__brev(vl & 63u) >> 26) << 5) | ((((k & 1u) << 1) | (k >> 1)) << 3) | ((s >> 9) << 1) | (s & 1u);
        tile = at >> 11;
        if (key < best) {
            best = key;
            neg = ((uint64_t)__double_as_longlong(v) >> 63) != 0;
        }
    }
    return neg;
}

}  // namespace

// One workgroup per tile of ROLL_TILE slots of the piece: the partials of its chunks of the levels ROLL_LOW .. min(lmax,
// 11) into the pyramid.  Slots that no range covers hold whatever the scratch held: their chunks are never read.
__global__ __launch_bounds__(256) void k_roll_pyramid(const double *__restrict__ scratch, RollPart *__restrict__ pyr,
                                                      const DevRollPiece *__restrict__ pc, uint32_t lmax)
{
    __shared__ RollPart s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, t = blockIdx.x;
    const double2 *x = (const double2 *)(scratch + (uint64_t)t * ROLL_TILE + 8u * tid);
    RollPart p[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const double2 d = x[k];
        p[k] = roll_merge(roll_leaf(d.x), roll_leaf(d.y));
    }
    RollPart a = roll_merge(roll_merge(p[0], p[1]), roll_merge(p[2], p[3]));
    roll_store(pyr + pc->off[3] + 256ull * t + tid, a);
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {  // level 4 + k: lane l takes lane l + 2^k's
        const uint32_t level = 4u + k;
        if (level > lmax) return;
        a = roll_merge(a, shfl_down_part(a, 1u << k));
        if ((lane & ((2u << k) - 1u)) == 0) roll_store(pyr + pc->off[level] + (((uint64_t)t * ROLL_TILE) >> level) + (tid >> (k + 1)), a);
    }
    if (lmax < 10) return;
    if (lane == 0) s_wave[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) {
        const RollPart l = roll_merge(s_wave[0], s_wave[1]), r = roll_merge(s_wave[2], s_wave[3]);
        roll_store(pyr + pc->off[10] + 2ull * t, l);
        roll_store(pyr + pc->off[10] + 2ull * t + 1, r);
        if (lmax >= 11) roll_store(pyr + pc->off[11] + t, roll_merge(l, r));
    }
}

// One wavefront per 64 chunks of level src at a multiple of 64 in the stream's chunk index: the chunks of the levels
// src + 1 .. min(src + 6, lmax) above them.  A chunk outside the piece counts as empty; what is formed from it sticks
// out of the piece as well, and is stored (where it has a place) but never read.
__global__ __launch_bounds__(256) void k_roll_upper(RollPart *__restrict__ pyr, const DevRollPiece *__restrict__ pc, uint32_t n,
                                                    uint32_t src, uint32_t lmax)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const uint64_t a0 = pc->a0, last = pc->a1 - 1;
    const uint64_t c = (((a0 >> src) >> 6) + i) * 64u + lane;
    RollPart a = roll_none();
    if (c >= (a0 >> src) && c <= (last >> src)) a = roll_load(pyr + pc->off[src] + (c - (a0 >> src)));
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t level = src + k + 1u;
        if (level > lmax) return;
        a = roll_merge(a, shfl_down_part(a, 1u << k));
        const uint64_t j = c >> (k + 1);
        if ((lane & ((2u << k) - 1u)) == 0 && j >= (a0 >> level) && j <= (last >> level))
            roll_store(pyr + pc->off[level] + (j - (a0 >> level)), a);
    }
}

// One wavefront per DevRollTask, a lane per position: the window's canonical chunks left to right, the sum folded in
// that order, into the position's record.
__global__ __launch_bounds__(256) void k_roll_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                        const double *__restrict__ scratch, const RollPart *__restrict__ pyr,
                                                        const DevRollPiece *__restrict__ pc, uint64_t w, uint64_t stride,
                                                        RollRec *__restrict__ out)
{
    __shared__ uint64_t s_off[ROLL_MAX_LEVEL + 1];  // a lane's level is its own: the offsets are read by lane
    if (threadIdx.x <= ROLL_MAX_LEVEL) s_off[threadIdx.x] = pc->off[threadIdx.x];
    __syncthreads();
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevRollTask t = tasks[i];
    const uint64_t a0 = pc->a0;
    for (uint32_t p = lane; p < t.n; p += 64u) {
        const uint64_t lo = t.lo + (uint64_t)p * stride, hi = lo + w;
        RollPart acc = roll_none();
        for (uint64_t pos = lo; pos < hi;) {
            const uint32_t up = pos ? (uint32_t)__builtin_ctzll(pos) : 63u, fit = 63u - (uint32_t)__builtin_clzll(hi - pos);
            const uint32_t l = up < fit ? up : fit;
            const double *x = scratch + (pos - a0);
            RollPart c;
            if (l >= ROLL_LOW) {
                c = roll_load(pyr + s_off[l] + ((pos >> l) - (a0 >> l)));
            } else if (l == 0) {
                c = roll_leaf(x[0]);
            } else if (l == 1) {
                c = roll_merge(roll_leaf(x[0]), roll_leaf(x[1]));
            } else {
                c = roll_merge(roll_merge(roll_leaf(x[0]), roll_leaf(x[1])), roll_merge(roll_leaf(x[2]), roll_leaf(x[3])));
            }
            acc = roll_merge(acc, c);
            pos += 1ull << l;
        }
        const double nan = __builtin_nan("");
        RollRec r{acc.count, acc.count ? acc.mn : nan, acc.count ? acc.mx : nan, acc.count ? acc.sum : 0.0};
        if (acc.count && (acc.mn == 0.0 || acc.mx == 0.0)) {
            const bool neg = acc.zeros == 3u ? roll_zero_sign(scratch + (lo - a0), lo, w) : acc.zeros == 1u;
            if (acc.mn == 0.0) r.mn = neg ? -0.0 : 0.0;
            if (acc.mx == 0.0) r.mx = neg ? -0.0 : 0.0;
        }
        out[t.rec + p] = r;
    }
}

hipError_t launch_roll_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax,
                               hipStream_t s)
{
    if (n_tiles == 0 || lmax < ROLL_LOW) return hipSuccess;
    hipLaunchKernelGGL(k_roll_pyramid, dim3(n_tiles), dim3(256), 0, s, scratch, (RollPart *)pyr, pc, lmax);
    return hipGetLastError();
}

hipError_t launch_roll_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax, hipStream_t s)
{
    return launch_wave_tasks(k_roll_upper, n, s, (RollPart *)pyr, pc, n, src, lmax);
}

hipError_t launch_roll_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const void *pyr,
                                 const DevRollPiece *pc, uint64_t w, uint64_t stride, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_roll_positions, n, s, tasks, n, scratch, (const RollPart *)pyr, pc, w, stride, (RollRec *)out);
}

}  // namespace atsc
