// atsc_delta.hip -- gfx950 kernels of the windowed deltas (atsc_delta_windows_dev): per window the counted pairs of
// stream-adjacent samples, the rises and falls among them, the sums of the rises' and falls' steps and of the samples
// after a fall, and the largest single rise and fall, reduced from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed deltas").  The pair of stream index j is (a, b) =
// (x[j - 1], x[j]), for begin < j < begin + count; it is counted iff neither is NaN, a rise iff b > a and a fall iff
// b < a.  Its terms sit at slot j, the slot of b: b - a in `up` for a rise, a - b in `down` and b in `after_falls` for
// a fall; every other slot holds -0.0, and the three sums go through the tile sum's tree (tile_lane_sums,
// atsc_tile_reduce.h) side by side.  The counts and the two maxima are exact in any order.
// One wavefront reduces one tile (lane l holds the virtual lanes l, l + 64, l + 128, l + 192) or one group of 64 tile
// partials of a window.  No atomics: every partial has one writer.
//
// The sample in front of a slot: for the odd slot of a 16-byte load it is the load's own first half; for the even slot
// j it is x[j - 1], a second 8-byte load that the cache serves (the line is the one the neighbouring lane's 16-byte
// load brings in); for slot 0 of a tile it is the last sample of the tile in front, scratch[src - 1], or, where the
// tile is the first of its piece of the scratch, the sample the host carried over from the previous piece (*carry).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

__device__ __forceinline__ DevDltPart dlt_add(DevDltPart a, const DevDltPart &b)
{
    a.up = a.up + b.up;
    a.down = a.down + b.down;
    a.after_falls = a.after_falls + b.after_falls;
    a.max_rise = b.max_rise > a.max_rise ? b.max_rise : a.max_rise;
    a.max_fall = b.max_fall > a.max_fall ? b.max_fall : a.max_fall;
    a.pairs += b.pairs;
    a.rises += b.rises;
    a.falls += b.falls;
    return a;
}

// what a lane keeps beside the three sums' terms while it walks its 32 slots: the maxima and the counts
struct Side {
    double mr, mf;
    uint32_t pairs, rises, falls;
};

// the terms of the pair (a, b) at one slot; in: the pair lies in the window
__device__ __forceinline__ void pair_take(double a, double b, bool in, double &up, double &down, double &af, Side &s)
{
    const bool ok = in && !__builtin_isnan(a) && !__builtin_isnan(b);
    const bool rise = ok && b > a, fall = ok && b < a;
    const double r = b - a, f = a - b;
    up = rise ? r : -0.0;
    down = fall ? f : -0.0;
    af = fall ? b : -0.0;
    s.mr = rise && r > s.mr ? r : s.mr;
    s.mf = fall && f > s.mf ? f : s.mf;
    s.pairs += ok ? 1u : 0u;
    s.rises += rise ? 1u : 0u;
    s.falls += fall ? 1u : 0u;
}

}  // namespace

// One wavefront per DevDltTile: the pairs at the slots of [lo, hi) of the tile at scratch[src] into part[dst].  The
// pair at slot j lies in the window for lo < j < hi, and at j == lo where the window continues from the slot in front
// of the tile (DLT_CONT, lo == 0).
__global__ __launch_bounds__(256) void k_dlt_tiles(const DevDltTile *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, const double *__restrict__ carry,
                                                   DevDltPart *__restrict__ part)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevDltTile t = tasks[i];
    const double *x = scratch + t.src;
    const bool cont = (t.flags & DLT_CONT) != 0;
    Side sd{0.0, 0.0, 0, 0, 0};
    // The three tile sums in the order tile_lane_sums (atsc_tile_reduce.h) defines, written out: through that helper
    // this kernel's schedule comes out at 148 VGPRs and more instead of 126, a wave less per SIMD.  The virtual lanes
    // go two at a time, (lane, lane + 128) and then (lane + 64, lane + 192), in a loop that is not unrolled: the halving
    // tree's first step inside the lane, s[v] + s[v + 128], closes each trip, its second step joins the two trips.
    // Unrolled four times the 32 loads and their predicates take 238 VGPRs.
    double r[3] = {-0.0, -0.0, -0.0};
#pragma unroll 1
    for (uint32_t kk = 0; kk < 2; ++kk) {
        double h[3];
#pragma unroll
        for (uint32_t e = 0; e < 2; ++e) {
            double p[4][3];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t j = tile_slot(lane + 64u * kk + 128u * e, q);
                const double2 d = tile_load(x, j, t.lo, t.hi, -0.0);
                const bool in0 = j < t.hi && (j > t.lo || (cont && j == t.lo));
                const bool in1 = j + 1u < t.hi && j + 1u > t.lo;
                double a = -0.0;  // x[j - 1]: inside the tile, in front of it, or carried over from the previous piece
                if (in0) a = j ? x[j - 1u] : (t.flags & DLT_CARRY) ? *carry : x[-1];
                double u0, d0, a0, u1, d1, a1;
                pair_take(a, d.x, in0, u0, d0, a0, sd);
                pair_take(d.x, d.y, in1, u1, d1, a1, sd);
                p[q][0] = u0 + u1;
                p[q][1] = d0 + d1;
                p[q][2] = a0 + a1;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double v = (p[0][c] + p[1][c]) + (p[2][c] + p[3][c]);
                h[c] = e ? h[c] + v : v;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) r[c] = kk ? r[c] + h[c] : h[c];
    }
    const DevDltPart o{r[0], r[1], r[2], sd.mr, sd.mf, sd.pairs, sd.rises, sd.falls};
    const DevDltPart w = wave_halve(o, dlt_add);
    if (lane == 0) part[t.dst] = w;
}

// One wavefront per DevAggComb: the group's partials through comb_reduce (a missing right operand is -0.0), then, in
// the final pass, into the window's atsc_window_delta (eight 8-byte fields, one per lane): a sum without a term is +0.0.
__global__ __launch_bounds__(256) void k_dlt_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                     DevDltPart *__restrict__ part, uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const DevDltPart a = comb_reduce(c, lane, part, DevDltPart{-0.0, -0.0, -0.0, 0.0, 0.0, 0, 0, 0}, dlt_add);
    if (!c.final_) return;
    const uint64_t pairs = __shfl(a.pairs, 0, 64), rises = __shfl(a.rises, 0, 64), falls = __shfl(a.falls, 0, 64);
    const double up = __shfl(a.up, 0, 64), down = __shfl(a.down, 0, 64), af = __shfl(a.after_falls, 0, 64),
                 mr = __shfl(a.max_rise, 0, 64), mf = __shfl(a.max_fall, 0, 64);
    if (lane < 8) {
        uint64_t w;
        switch (lane) {
        case 0: w = pairs; break;
        case 1: w = rises; break;
        case 2: w = falls; break;
        case 3: w = __double_as_longlong(rises ? up : 0.0); break;
        case 4: w = __double_as_longlong(falls ? down : 0.0); break;
        case 5: w = __double_as_longlong(falls ? af : 0.0); break;
        case 6: w = __double_as_longlong(mr); break;
        default: w = __double_as_longlong(mf); break;
        }
        out[8ull * c.dst + lane] = w;
    }
}

hipError_t launch_dlt_tiles(const DevDltTile *tasks, uint32_t n, const double *scratch, const double *carry,
                            DevDltPart *part, hipStream_t s)
{
    return launch_wave_tasks(k_dlt_tiles, n, s, tasks, n, scratch, carry, part);
}

hipError_t launch_dlt_combine(const DevAggComb *tasks, uint32_t n, DevDltPart *part, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_dlt_combine, n, s, tasks, n, part, (uint64_t *)out);
}

}  // namespace atsc
