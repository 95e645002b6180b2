// atsc_rolling_delta.hip -- gfx950 kernels of the windowed rolling deltas (atsc_rolling_delta_windows_dev): the deltas'
// record (atsc_window_delta) of the window [lo, lo + w) at every position of a range, from decoded samples in the call's
// scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed rolling deltas").  The leaf is a pair, not a sample: slot j
// holds the deltas' terms of the pair (x[j - 1], x[j]) (atsc_delta.hip, pair_take), or -0.0.  T(a, 0) = term(a) and
// T(a, l) = T(a, l - 1) + T(a + 2^(l-1), l - 1) for a a multiple of 2^l in the stream index; a window's three sums are
// the left-to-right fold of T over the canonical chunks of its pair slots [lo + 1, lo + w).  T does not depend on any
// window, so one pyramid of chunk partials per piece of the scratch serves every position in it, as the rolling's does
// (atsc_rolling.hip), and the three kernels are that file's:
//   pyramid    one workgroup per ROLL_TILE = 2048 aligned slots, eight consecutive ones a thread: the levels 1 .. 3 in
//              registers, 4 .. 9 across the wavefront by shuffles, 10 and 11 through LDS; the levels from ROLL_DELTA_LOW
//              = 3 up to floor(log2(w - 1)) are stored;
//   upper      one wavefront per 64 aligned chunks of level 11 (and of level 17): the six levels above by shuffles;
//   positions  one wavefront per task, a lane per position: the lane walks its window's chunks left to right, a chunk
//              below ROLL_DELTA_LOW formed from the samples by the same tree, the others read from the pyramid.
// A partial is the three sums, the two maxima and the three counts in one word: 48 bytes.  No atomics: every partial
// and every record has one writer, and a chunk's value is the same bits wherever it is formed.
//
// The sample in front of a slot: the leaf at slot j reads x[j - 1].  For slot 0 of a piece's region that sample lies in
// front of the scratch, and is not read: the slot holds "no pair".  No position reads a chunk with that slot in it:
// every chunk of a window lies in [lo + 1, lo + w), and lo is at or behind the region's first slot.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// counts: pairs, rises and falls in 21 bits each (bits 0, 21, 42): a chunk holds at most 2^20 pairs, a window fewer
struct alignas(16) RdPart {
    double up, down, after_falls, max_rise, max_fall;
    uint64_t counts;
};
static_assert(sizeof(RdPart) == ROLL_DELTA_PART, "a partial is 48 bytes");

constexpr uint32_t RD_RISES = 21, RD_FALLS = 42;
constexpr uint64_t RD_MASK = (1ull << 21) - 1;

// the record as the position kernel stores it, at the 8-byte alignment the result has
struct alignas(8) RdRec {
    uint64_t pairs, rises, falls;
    double up, down, after_falls, max_rise, max_fall;
};
static_assert(sizeof(RdRec) == sizeof(atsc_window_delta), "the record's layout");

DEVI RdPart rd_none() { return RdPart{-0.0, -0.0, -0.0, 0.0, 0.0, 0ull}; }

// the pair (a, b) at the slot of b: the deltas' terms (atsc_delta.hip, pair_take)
DEVI RdPart rd_leaf(double a, double b)
{
    const bool ok = !__builtin_isnan(a) && !__builtin_isnan(b);
    const bool rise = ok && b > a, fall = ok && b < a;
    const double r = b - a, f = a - b;
    return RdPart{rise ? r : -0.0, fall ? f : -0.0, fall ? b : -0.0, rise ? r : 0.0, fall ? f : 0.0,
                  (ok ? 1ull : 0ull) | (rise ? 1ull << RD_RISES : 0ull) | (fall ? 1ull << RD_FALLS : 0ull)};
}

// (the comparisons are the deltas': atsc_delta.hip, dlt_add)
DEVI RdPart rd_merge(RdPart a, const RdPart &b)
{
    a.up = a.up + b.up;
    a.down = a.down + b.down;
    a.after_falls = a.after_falls + b.after_falls;
    a.max_rise = b.max_rise > a.max_rise ? b.max_rise : a.max_rise;
    a.max_fall = b.max_fall > a.max_fall ? b.max_fall : a.max_fall;
    a.counts += b.counts;
    return a;
}

DEVI RdPart rd_load(const RdPart *p)
{
    const double2 a = ((const double2 *)p)[0], b = ((const double2 *)p)[1], c = ((const double2 *)p)[2];  // three 16-byte loads
    return RdPart{a.x, a.y, b.x, b.y, c.x, (uint64_t)__double_as_longlong(c.y)};
}

DEVI void rd_store(RdPart *p, const RdPart &r)
{
    ((double2 *)p)[0] = make_double2(r.up, r.down);
    ((double2 *)p)[1] = make_double2(r.after_falls, r.max_rise);
    ((double2 *)p)[2] = make_double2(r.max_fall, __longlong_as_double((long long)r.counts));
}

}  // namespace

// One workgroup per tile of ROLL_TILE slots of the piece: the partials of its chunks of the levels ROLL_DELTA_LOW ..
// min(lmax, 11) into the pyramid.  Slots that no range covers hold whatever the scratch held: their chunks are never
// read.  Slot 0 of the region holds no pair: the sample in front of it is not the scratch's.
__global__ __launch_bounds__(256) void k_rdl_pyramid(const double *__restrict__ scratch, RdPart *__restrict__ pyr,
                                                     const DevRollPiece *__restrict__ pc, uint32_t lmax)
{
    __shared__ RdPart s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, t = blockIdx.x;
    const double *xs = scratch + (uint64_t)t * ROLL_TILE + 8u * tid;
    const double2 *x = (const double2 *)xs;
    const bool first = t == 0 && tid == 0;
    double prev = first ? -0.0 : xs[-1];
    RdPart p[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const double2 d = x[k];
        p[k] = rd_merge(k == 0 && first ? rd_none() : rd_leaf(prev, d.x), rd_leaf(d.x, d.y));
        prev = d.y;
    }
    RdPart a = rd_merge(rd_merge(p[0], p[1]), rd_merge(p[2], p[3]));
    rd_store(pyr + pc->off[3] + 256ull * t + tid, a);
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {  // level 4 + k: lane l takes lane l + 2^k's
        const uint32_t level = 4u + k;
        if (level > lmax) return;
        a = rd_merge(a, shfl_down_part(a, 1u << k));
        if ((lane & ((2u << k) - 1u)) == 0) rd_store(pyr + pc->off[level] + (((uint64_t)t * ROLL_TILE) >> level) + (tid >> (k + 1)), a);
    }
    if (lmax < 10) return;
    if (lane == 0) s_wave[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) {
        const RdPart l = rd_merge(s_wave[0], s_wave[1]), r = rd_merge(s_wave[2], s_wave[3]);
        rd_store(pyr + pc->off[10] + 2ull * t, l);
        rd_store(pyr + pc->off[10] + 2ull * t + 1, r);
        if (lmax >= 11) rd_store(pyr + pc->off[11] + t, rd_merge(l, r));
    }
}

// One wavefront per 64 chunks of level src at a multiple of 64 in the stream's chunk index: the chunks of the levels
// src + 1 .. min(src + 6, lmax) above them.  A chunk outside the piece counts as empty; what is formed from it sticks
// out of the piece as well, and is stored (where it has a place) but never read.
__global__ __launch_bounds__(256) void k_rdl_upper(RdPart *__restrict__ pyr, const DevRollPiece *__restrict__ pc, uint32_t n,
                                                   uint32_t src, uint32_t lmax)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const uint64_t a0 = pc->a0, last = pc->a1 - 1;
    const uint64_t c = (((a0 >> src) >> 6) + i) * 64u + lane;
    RdPart a = rd_none();
    if (c >= (a0 >> src) && c <= (last >> src)) a = rd_load(pyr + pc->off[src] + (c - (a0 >> src)));
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t level = src + k + 1u;
        if (level > lmax) return;
        a = rd_merge(a, shfl_down_part(a, 1u << k));
        const uint64_t j = c >> (k + 1);
        if ((lane & ((2u << k) - 1u)) == 0 && j >= (a0 >> level) && j <= (last >> level))
            rd_store(pyr + pc->off[level] + (j - (a0 >> level)), a);
    }
}

// One wavefront per DevRollTask, a lane per position: the canonical chunks of the window's pair slots [lo + 1, lo + w)
// left to right, the sums folded in that order, into the position's record.
__global__ __launch_bounds__(256) void k_rdl_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                       const double *__restrict__ scratch, const RdPart *__restrict__ pyr,
                                                       const DevRollPiece *__restrict__ pc, uint64_t w, uint64_t stride,
                                                       RdRec *__restrict__ out)
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
        RdPart acc = rd_none();
        for (uint64_t pos = lo + 1; pos < hi;) {  // pos > lo >= a0: x[-1] is the region's
            const uint32_t up = (uint32_t)__builtin_ctzll(pos), fit = 63u - (uint32_t)__builtin_clzll(hi - pos);
            const uint32_t l = up < fit ? up : fit;
            const double *x = scratch + (pos - a0);
            RdPart c;
            if (l >= ROLL_DELTA_LOW) {
                c = rd_load(pyr + s_off[l] + ((pos >> l) - (a0 >> l)));
            } else if (l == 0) {
                c = rd_leaf(x[-1], x[0]);
            } else if (l == 1) {
                const double b = x[0];
                c = rd_merge(rd_leaf(x[-1], b), rd_leaf(b, x[1]));
            } else {
                const double b0 = x[0], b1 = x[1], b2 = x[2];
                c = rd_merge(rd_merge(rd_leaf(x[-1], b0), rd_leaf(b0, b1)), rd_merge(rd_leaf(b1, b2), rd_leaf(b2, x[3])));
            }
            acc = rd_merge(acc, c);
            pos += 1ull << l;
        }
        const uint64_t rises = (acc.counts >> RD_RISES) & RD_MASK, falls = acc.counts >> RD_FALLS;
        // a sum without a term is +0.0, as k_dlt_combine has it
        out[t.rec + p] = RdRec{acc.counts & RD_MASK, rises, falls, rises ? acc.up : 0.0, falls ? acc.down : 0.0,
                               falls ? acc.after_falls : 0.0, acc.max_rise, acc.max_fall};
    }
}

hipError_t launch_rdl_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax,
                              hipStream_t s)
{
    if (n_tiles == 0 || lmax < ROLL_DELTA_LOW) return hipSuccess;
    hipLaunchKernelGGL(k_rdl_pyramid, dim3(n_tiles), dim3(256), 0, s, scratch, (RdPart *)pyr, pc, lmax);
    return hipGetLastError();
}

hipError_t launch_rdl_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax, hipStream_t s)
{
    return launch_wave_tasks(k_rdl_upper, n, s, (RdPart *)pyr, pc, n, src, lmax);
}

hipError_t launch_rdl_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const void *pyr,
                                const DevRollPiece *pc, uint64_t w, uint64_t stride, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_rdl_positions, n, s, tasks, n, scratch, (const RdPart *)pyr, pc, w, stride, (RdRec *)out);
}

}  // namespace atsc
