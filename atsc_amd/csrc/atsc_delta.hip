// atsc_delta.hip -- gfx950 kernels of the windowed deltas (atsc_delta_windows_dev): per window the counted pairs of
// stream-adjacent samples, the rises and falls among them, the sums of the rises' and falls' steps and of the samples
// after a fall, and the largest single rise and fall, reduced from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed deltas").  The pair of stream index j is (a, b) =
// (x[j - 1], x[j]), for begin < j < begin + count; it is counted iff neither is NaN, a rise iff b > a and a fall iff
// b < a.  Its terms sit at slot j, the slot of b: b - a in `up` for a rise, a - b in `down` and b in `after_falls` for
// a fall; every other slot holds -0.0, and the three sums go through the aggregate sum's tree (atsc_aggregate.hip)
// unchanged.  The counts and the two maxima are exact in any order.
// One wavefront reduces one tile (lane l holds the virtual lanes l, l + 64, l + 128, l + 192) or one group of 64 tile
// partials of a window.  No atomics: every partial has one writer.
//
// The sample in front of a slot: for the odd slot of a 16-byte load it is the load's own first half; for the even slot
// j it is x[j - 1], a second 8-byte load that the cache serves (the line is the one the neighbouring lane's 16-byte
// load brings in); for slot 0 of a tile it is the last sample of the tile in front, scratch[src - 1], or, where the
// tile is the first of its piece of the scratch, the sample the host carried over from the previous piece (*carry).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_device.h"

namespace atsc {

namespace {

struct Dlt {
    double up, down, af, mr, mf;
    uint64_t pairs, rises, falls;
};

__device__ __forceinline__ Dlt dlt_identity() { return Dlt{-0.0, -0.0, -0.0, 0.0, 0.0, 0, 0, 0}; }

__device__ __forceinline__ Dlt dlt_shfl_down(const Dlt &a, unsigned off)
{
    Dlt o;
    o.up = __shfl_down(a.up, off, 64);
    o.down = __shfl_down(a.down, off, 64);
    o.af = __shfl_down(a.af, off, 64);
    o.mr = __shfl_down(a.mr, off, 64);
    o.mf = __shfl_down(a.mf, off, 64);
    o.pairs = __shfl_down(a.pairs, off, 64);
    o.rises = __shfl_down(a.rises, off, 64);
    o.falls = __shfl_down(a.falls, off, 64);
    return o;
}

__device__ __forceinline__ void dlt_add(Dlt &a, const Dlt &b)
{
    a.up = a.up + b.up;
    a.down = a.down + b.down;
    a.af = a.af + b.af;
    a.mr = b.mr > a.mr ? b.mr : a.mr;
    a.mf = b.mf > a.mf ? b.mf : a.mf;
    a.pairs += b.pairs;
    a.rises += b.rises;
    a.falls += b.falls;
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
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n) return;
    const DevDltTile t = tasks[i];
    const double *x = scratch + t.src;
    const bool cont = (t.flags & DLT_CONT) != 0;
    Side sd{0.0, 0.0, 0, 0, 0};
    // The virtual lanes go two at a time, (lane, lane + 128) and then (lane + 64, lane + 192), in a loop that is not
    // unrolled: the halving tree's first step inside the lane, s[v] + s[v + 128], closes each trip, its second step
    // joins the two trips.  Unrolled four times the 32 loads and their predicates take 238 VGPRs.
    double tu = -0.0, td = -0.0, ta = -0.0;
#pragma unroll 1
    for (uint32_t kk = 0; kk < 2; ++kk) {
        double su[2], sdn[2], sa[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const uint32_t v = lane + 64u * kk + 128u * e;
            double pu[4], pd[4], pa[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = 512u * q + 2u * v;
                double2 d = make_double2(-0.0, -0.0);
                if (j < t.hi && j + 2u > t.lo) d = *(const double2 *)(x + j);  // 16-byte load; scratch tiles are 16-byte aligned
                const bool in0 = j < t.hi && (j > t.lo || (cont && j == t.lo));
                const bool in1 = j + 1u < t.hi && j + 1u > t.lo;
                double a = -0.0;  // x[j - 1]: inside the tile, in front of it, or carried over from the previous piece
                if (in0) a = j ? x[j - 1u] : (t.flags & DLT_CARRY) ? *carry : x[-1];
                double u0, d0, a0, u1, d1, a1;
                pair_take(a, d.x, in0, u0, d0, a0, sd);
                pair_take(d.x, d.y, in1, u1, d1, a1, sd);
                pu[q] = u0 + u1;
                pd[q] = d0 + d1;
                pa[q] = a0 + a1;
            }
            su[e] = (pu[0] + pu[1]) + (pu[2] + pu[3]);
            sdn[e] = (pd[0] + pd[1]) + (pd[2] + pd[3]);
            sa[e] = (pa[0] + pa[1]) + (pa[2] + pa[3]);
        }
        // halving tree over the 256 virtual lanes, h = 128 and 64: (s[l] + s[l + 128]) + (s[l + 64] + s[l + 192])
        const double hu = su[0] + su[1], hd = sdn[0] + sdn[1], ha = sa[0] + sa[1];
        tu = kk ? tu + hu : hu;
        td = kk ? td + hd : hd;
        ta = kk ? ta + ha : ha;
    }
    // then h = 32 .. 1 across the wavefront
    Dlt r{tu, td, ta, sd.mr, sd.mf, sd.pairs, sd.rises, sd.falls};
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) dlt_add(r, dlt_shfl_down(r, off));
    if (lane == 0) part[t.dst] = DevDltPart{r.up, r.down, r.af, r.mr, r.mf, r.pairs, r.rises, r.falls};
}

// One wavefront per DevAggComb: partials j = 64 g .. 64 g + 63 of a window's list (j < n; j == 0 at head, j == n - 1 at
// tail, else at mid + j) through the pairwise tree (lane l + 2^k into lane l; a missing right operand is -0.0), then
// into part[dst] or, in the final pass, the window's atsc_window_delta (eight 8-byte fields, one per lane): a sum
// without a term is +0.0.
__global__ __launch_bounds__(256) void k_dlt_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                     DevDltPart *__restrict__ part, uint64_t *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const uint64_t j = 64ull * c.g + lane;
    Dlt a = dlt_identity();
    if (j < c.n) {
        const DevDltPart p = part[j == 0 ? c.head : j == c.n - 1 ? c.tail : c.mid + j];
        a = Dlt{p.up, p.down, p.after_falls, p.max_rise, p.max_fall, p.pairs, p.rises, p.falls};
    }
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) dlt_add(a, dlt_shfl_down(a, off));
    if (!c.final_) {
        if (lane == 0) part[c.dst] = DevDltPart{a.up, a.down, a.af, a.mr, a.mf, a.pairs, a.rises, a.falls};
        return;
    }
    const uint64_t pairs = __shfl(a.pairs, 0, 64), rises = __shfl(a.rises, 0, 64), falls = __shfl(a.falls, 0, 64);
    const double up = __shfl(a.up, 0, 64), down = __shfl(a.down, 0, 64), af = __shfl(a.af, 0, 64),
                 mr = __shfl(a.mr, 0, 64), mf = __shfl(a.mf, 0, 64);
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
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dlt_tiles, dim3((n + 3) / 4), dim3(256), 0, s, tasks, n, scratch, carry, part);
    return hipGetLastError();
}

hipError_t launch_dlt_combine(const DevAggComb *tasks, uint32_t n, DevDltPart *part, void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_dlt_combine, dim3((n + 3) / 4), dim3(256), 0, s, tasks, n, part, (uint64_t *)out);
    return hipGetLastError();
}

}  // namespace atsc
