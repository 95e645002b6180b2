// atsc_tile_reduce.h -- what the window reductions over tiles share on the device (atsc_aggregate.hip,
// atsc_moments.hip, atsc_pair.hip, atsc_delta.hip, atsc_runs.hip, atsc_extremes.hip; DESIGN.md "The tile / combine
// skeleton"): the wavefront-to-task mapping and its launch, the tile's slot-to-lane mapping and masked load, the
// contract's sum tree, the shuffle trees over whole partials and the combine pass's fetch / reduce / store.
#pragma once
#include "atsc_device.h"

namespace atsc {

// One wavefront per task, four to a workgroup: the wavefront's lane and task (tasks past the list's end leave).
DEVI uint32_t wave_lane() { return threadIdx.x & 63u; }
DEVI uint32_t wave_task() { return blockIdx.x * 4u + (threadIdx.x >> 6); }

// `kernel` over n tasks; args: the kernel's own, n among them.
template <class K, class... A>
inline hipError_t launch_wave_tasks(K kernel, uint32_t n, hipStream_t s, A... args)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(kernel, dim3((n + 3) / 4), dim3(256), 0, s, args...);
    return hipGetLastError();
}

// A tile is AGG_TILE = 2048 slots; lane l holds the virtual lanes v = l + 64 k, k = 0 .. 3, and virtual lane v the slot
// pairs tile_slot(v, q), + 1 for q = 0 .. 3: the 64 lanes of one (k, q) load 128 contiguous slots, 16 bytes each.
DEVI uint32_t tile_slot(uint32_t v, uint32_t q) { return 512u * q + 2u * v; }
DEVI bool tile_in(uint32_t j, uint32_t lo, uint32_t hi) { return j >= lo && j < hi; }
// the slots j, j + 1 of the tile at x; `fill` in both where neither lies in [lo, hi)
DEVI double2 tile_load(const double *x, uint32_t j, uint32_t lo, uint32_t hi, double fill)
{
    double2 d = make_double2(fill, fill);
    if (j < hi && j + 2u > lo) d = *(const double2 *)(x + j);  // 16-byte load; scratch tiles are 16-byte aligned
    return d;
}

// A sample's key (the extremes, the value counts): its bits mapped so that unsigned integer order is value order, the
// sign bit flipped for positive values, all bits for negative ones, both zeros on +0.0's key; 0 for NaN.  No sample's
// key is 0, and none is ~0.
DEVI uint64_t sample_key(double v)
{
    uint64_t b = (uint64_t)__double_as_longlong(v);
    b = v == 0.0 ? 0ull : b;
    const uint64_t k = b ^ ((b >> 63) ? ~0ull : 0x8000000000000000ull);
    return v != v ? 0ull : k;
}

// the bits of the value of a sample's key: +0.0 for the zeros' key, every other value's own
DEVI uint64_t val_bits(uint64_t key)
{
    return (key >> 63) ? key ^ 0x8000000000000000ull : ~key;
}

// A lane's column of G keys in registers (the across quantiles, the across value counts), ascending by the bitonic
// network: G/2 compare-exchanges per step, log2 G (log2 G + 1) / 2 steps, every index a compile-time constant
template <int G>
DEVI void column_sort(uint64_t (&v)[G])
{
#pragma unroll
    for (int k = 2; k <= G; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int l = i ^ j;
                if (l < i) continue;
                const uint64_t a = v[i], b = v[l];
                const bool sw = (i & k) == 0 ? a > b : a < b;
                v[i] = sw ? b : a;
                v[l] = sw ? a : b;
            }
        }
    }
}

// THE TILE SUM of the contract (include/atsc_hip.h, DESIGN.md "Windowed aggregates"), NS sums side by side:
//   * term(k, q, p) gives p[c] = (term of slot j) + (term of slot j + 1) of sum c, j = tile_slot(lane + 64 k, q); a
//     slot without a term holds -0.0 (IEEE's exact additive identity);
//   * virtual lane v sums its pairs as (p0 + p1) + (p2 + p3);
//   * the 256 lane sums go through a halving tree, s[v] += s[v + h] for h = 128, 64, .., 1.
// This function does the tree's steps h = 128 and 64, which stay inside the lane: (s[l] + s[l + 128]) + (s[l + 64] +
// s[l + 192]) into s; the steps h = 32 .. 1 are wave_halve's, over s or over the partial that s goes into.
// The virtual lanes go two at a time, (l, l + 128) and then (l + 64, l + 192), all in line.  k_dlt_tiles and k_run_tiles
// write the same order out as a loop of two trips that is not unrolled: they would run out of registers otherwise, and
// through this function the compiler schedules them worse (profiles/tile_reduce_resources.txt).
template <int NS, class Term>
DEVI void tile_lane_sums(double (&s)[NS], Term term)
{
#pragma unroll
    for (int c = 0; c < NS; ++c) s[c] = -0.0;
#pragma unroll
    for (uint32_t kk = 0; kk < 2; ++kk) {
        double h[NS];
#pragma unroll
        for (uint32_t e = 0; e < 2; ++e) {
            double p[4][NS];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) term(kk + 2u * e, q, p[q]);
#pragma unroll
            for (int c = 0; c < NS; ++c) {
                const double t = (p[0][c] + p[1][c]) + (p[2][c] + p[3][c]);
                h[c] = e ? h[c] + t : t;
            }
        }
#pragma unroll
        for (int c = 0; c < NS; ++c) s[c] = kk ? s[c] + h[c] : h[c];
    }
}

// lane l + off's copy of a partial or node, 4-byte word by word
template <class P>
DEVI P shfl_down_part(const P &a, unsigned off)
{
    static_assert(sizeof(P) % 4 == 0, "whole words");
    struct Words {
        uint32_t w[sizeof(P) / 4];
    };
    Words s = __builtin_bit_cast(Words, a);
#pragma unroll
    for (unsigned i = 0; i < sizeof(P) / 4; ++i) s.w[i] = __shfl_down(s.w[i], off, 64);
    return __builtin_bit_cast(P, s);
}

// The halving tree's steps h = 32 .. 1 across the wavefront, merge(left, right): lane 0 ends with the whole.
template <class P, class Merge>
DEVI P wave_halve(P a, Merge merge)
{
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) a = merge(a, shfl_down_part(a, off));
    return a;
}

// The pairwise tree over the first W lanes in lane order: lane l + 2^k into lane l, the left operand first.
template <unsigned W = 64, class P, class Merge>
DEVI P wave_pairwise(P a, Merge merge)
{
#pragma unroll
    for (unsigned off = 1; off < W; off <<= 1) a = merge(a, shfl_down_part(a, off));
    return a;
}

// A combine group (DevAggComb): the lane's entry j of the window's list, and where entry j < c.n lies in part[].
DEVI uint64_t comb_entry(const DevAggComb &c, uint32_t lane) { return 64ull * c.g + lane; }
DEVI uint64_t comb_at(const DevAggComb &c, uint64_t j) { return j == 0 ? c.head : j == c.n - 1 ? c.tail : c.mid + j; }

// The group's partials, `a` (the identity) where the list has ended, through the pairwise tree; lane 0's result goes to
// part[c.dst] unless the pass is the final one, whose caller turns it into the window's record.
// (a by value and assigned under the test: a reference would have the compiler select between two address spaces.)
template <class P, class Merge>
DEVI P comb_reduce(const DevAggComb &c, uint32_t lane, P *part, P a, Merge merge)
{
    const uint64_t j = comb_entry(c, lane);
    if (j < c.n) a = part[comb_at(c, j)];
    a = wave_pairwise(a, merge);
    if (!c.final_ && lane == 0) part[c.dst] = a;
    return a;
}

}  // namespace atsc
