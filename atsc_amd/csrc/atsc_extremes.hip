// atsc_extremes.hip -- gfx950 kernels of the windowed extremes (atsc_extremes_windows_dev): per window the k largest and
// the k smallest non-NaN samples with their positions, the number of NaN samples and the window's length, selected from
// decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed extremes").  No arithmetic touches a sample: an entry is the
// sample's own bits and an integer position, so the record is bit-exact by construction.  The order of a list is (value,
// position): by value, -0.0 equal to +0.0, equal values earliest position first.  A sample's KEY is its bits mapped so
// that unsigned integer order is value order (the sign bit flipped for positive values, all bits for negative ones, both
// zeros on +0.0's key); the smallest list uses the complement.  No sample's key is 0 under either reading, so key 0 marks
// "no sample": NaN, a slot outside the window, an exhausted list.  "a ahead of b": key(a) > key(b), or equal keys and a's
// position smaller.
//
// A partial has the record's layout, 2 + 4 k eight-byte words: count, nans, k largest entries, k smallest entries, an
// entry being (value bits, position); positions are stream indices, so the partial of a shared full tile serves every
// window that shares it, and an entry that is missing holds (NaN, ~0).  The final combine pass subtracts the window's
// begin.  One wavefront selects from one tile or merges one group of 64 partials.  No atomics, no LDS: every partial has
// one writer, and the lists live one entry per lane in lanes 0 .. k - 1 (k <= 16).
//
// The tile kernel keeps the 16-byte loads and slot-to-lane mapping of atsc_tile_reduce.h and selects in three phases, per
// end:
//   1. every lane finds the entry that is ahead of all others among its own 32 slots;
//   2. a bitonic sort over the 64 lanes orders those lane-bests; lanes 0 .. k - 1 then hold the start of the list, which
//      is k members of the answer's candidates already, and lane k - 1 holds the threshold;
//   3. a second pass over the slots: one ballot per load step and half of the slots that are strictly ahead of the
//      threshold and are not their lane's best (those are in the list).  Each set bit is a candidate, read out of its
//      lane wave-uniformly and inserted into the sorted list: one compare per lane, a shift by one lane, a select.
// At most k - 1 lanes have a best ahead of the threshold, and a lane has 31 other slots: at most 31 (k - 1) insertions
// per tile and end whatever the data (an ascending counter: k - 1; k == 1: none at all).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

constexpr uint64_t EXT_NONE = ~0ull;
constexpr uint64_t EXT_NAN_BITS = 0x7ff8000000000000ull;

template <class P>
__device__ __forceinline__ bool ext_ahead(uint64_t ka, P pa, uint64_t kb, P pb)
{
    return ka > kb || (ka == kb && pa < pb);
}

__device__ __forceinline__ uint64_t ext_readlane(uint64_t v, uint32_t l)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
    return ((uint64_t)hi << 32) | lo;
}

// Bitonic sort of one (key, position) per lane over the wavefront: lane 0 ends with the entry ahead of all others.
// Entries without a sample (key 0, position ~0) are all alike and end behind every sample.
__device__ __forceinline__ void ext_sort(uint64_t &key, uint32_t &pos, uint32_t lane)
{
#pragma unroll
    for (uint32_t size = 2; size <= 64; size <<= 1) {
#pragma unroll
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            const uint64_t ok = __shfl_xor(key, stride, 64);
            const uint32_t op = __shfl_xor(pos, stride, 64);
            const bool lower = (lane & stride) == 0, desc = (lane & size) == 0;
            const bool other = ext_ahead(ok, op, key, pos);
            const bool take = lower == desc ? other : !other;
            key = take ? ok : key;
            pos = take ? op : pos;
        }
    }
}

// The candidate (ck, cp), the same in every lane, into the sorted list held one entry per lane from lane 0 on: the lanes
// whose entry it is ahead of take their left neighbour's entry, the first of them the candidate.  Lanes behind the list
// compute along; nothing reads them.
__device__ __forceinline__ void ext_insert(uint64_t &lk, uint32_t &lp, uint64_t ck, uint32_t cp, uint32_t lane)
{
    const uint64_t pk = __shfl_up(lk, 1, 64);
    const uint32_t pp = __shfl_up(lp, 1, 64);
    const bool here = ext_ahead(ck, cp, lk, lp);
    const bool left = lane != 0 && ext_ahead(ck, cp, pk, pp);
    lk = here ? (left ? pk : ck) : lk;
    lp = here ? (left ? pp : cp) : lp;
}

}  // namespace

// One wavefront per DevPosTile: the partial of the slots [lo, hi) of the tile at scratch[src], whose slot 0 is sample t0
// of the stream, into part[dst (2 + 4 k)].
__global__ __launch_bounds__(256) void k_ext_tiles(const DevPosTile *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, uint32_t k,
                                                   uint64_t *__restrict__ part)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevPosTile t = tasks[i];
    const double *x = scratch + t.src;
    // phase 1: the lane's best of each end, and its NaN samples
    uint64_t bkl = 0, bks = 0;
    uint32_t bpl = ~0u, bps = ~0u, nans = 0;
#pragma unroll 1
    for (uint32_t kk = 0; kk < 4; ++kk) {
        const uint32_t v = lane + 64u * kk;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t j = tile_slot(v, q);
            const double2 d = tile_load(x, j, t.lo, t.hi, 0.0);
#pragma unroll
            for (uint32_t e = 0; e < 2; ++e) {
                const uint32_t p = j + e;
                const double s = e ? d.y : d.x;
                const bool in = tile_in(p, t.lo, t.hi);
                const uint64_t kl = in ? sample_key(s) : 0ull, ks = kl ? ~kl : 0ull;
                nans += in && s != s ? 1u : 0u;
                if (kl && ext_ahead(kl, p, bkl, bpl)) { bkl = kl; bpl = p; }
                if (ks && ext_ahead(ks, p, bks, bps)) { bks = ks; bps = p; }
            }
        }
    }
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) nans += __shfl_down(nans, off, 64);
    // phase 2: the lane-bests in order; lanes 0 .. k - 1 start the lists, lane k - 1 is the threshold
    uint64_t lkl = bkl, lks = bks;
    uint32_t lpl = bpl, lps = bps;
    ext_sort(lkl, lpl, lane);
    ext_sort(lks, lps, lane);
    const uint64_t tkl = ext_readlane(lkl, k - 1u), tks = ext_readlane(lks, k - 1u);
    const uint32_t tpl = (uint32_t)__builtin_amdgcn_readlane((int)lpl, (int)(k - 1u));
    const uint32_t tps = (uint32_t)__builtin_amdgcn_readlane((int)lps, (int)(k - 1u));
    // phase 3: every other slot that is strictly ahead of the threshold, into the list
    if (k > 1u) {
#pragma unroll 1
        for (uint32_t kk = 0; kk < 4; ++kk) {
            const uint32_t v = lane + 64u * kk;
#pragma unroll 1
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t j = tile_slot(v, q);
                const double2 d = tile_load(x, j, t.lo, t.hi, 0.0);
#pragma unroll
                for (uint32_t e = 0; e < 2; ++e) {
                    const uint32_t p = j + e;
                    const double s = e ? d.y : d.x;
                    const bool in = tile_in(p, t.lo, t.hi);
                    const uint64_t kl = in ? sample_key(s) : 0ull, ks = kl ? ~kl : 0ull;
                    const uint32_t p0 = 512u * q + 128u * kk + e;  // lane 0's slot of this step and half
                    uint64_t m = __ballot(kl != 0 && p != bpl && ext_ahead(kl, p, tkl, tpl));
                    while (m) {
                        const uint32_t src = (uint32_t)__builtin_ctzll(m);
                        m &= m - 1;
                        ext_insert(lkl, lpl, ext_readlane(kl, src), p0 + 2u * src, lane);
                    }
                    m = __ballot(ks != 0 && p != bps && ext_ahead(ks, p, tks, tps));
                    while (m) {
                        const uint32_t src = (uint32_t)__builtin_ctzll(m);
                        m &= m - 1;
                        ext_insert(lks, lps, ext_readlane(ks, src), p0 + 2u * src, lane);
                    }
                }
            }
        }
    }
    // the partial: lane 0 the head, lane l < k entry l of either list (the sample's own bits, read at its slot)
    uint64_t *o = part + t.dst * (2ull + 4ull * k);
    if (lane == 0) {
        o[0] = t.hi - t.lo;
        o[1] = nans;
    }
    if (lane < k) {
        uint64_t vl = EXT_NAN_BITS, al = EXT_NONE, vs = EXT_NAN_BITS, as = EXT_NONE;
        if (lkl) { vl = (uint64_t)__double_as_longlong(x[lpl]); al = t.t0 + lpl; }
        if (lks) { vs = (uint64_t)__double_as_longlong(x[lps]); as = t.t0 + lps; }
        uint64_t *el = o + 2u + 2u * lane, *es = el + 2u * k;
        el[0] = vl;
        el[1] = al;
        es[0] = vs;
        es[1] = as;
    }
}

// One wavefront per DevAggComb: the group's partials (comb_entry, comb_at), one per lane, into the partial part[dst] or,
// in the final pass, the window's record out[dst] (positions counted from the window's begin[win]).  count and nans
// add.  Per end, every lane holds a cursor into its partial's list and the entry under it; k rounds pop the group's first k: the wave maximum of the heads' keys, of equal
// keys the lowest lane (partials come in stream order and a list puts equal values earliest first, so that is the
// earliest position); the winner's entry goes to lane r of the result, and the winner reads its next entry from memory.
__global__ __launch_bounds__(256) void k_ext_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks, uint32_t k,
                                                     uint64_t *__restrict__ part, const uint64_t *__restrict__ begin,
                                                     uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const uint64_t j = comb_entry(c, lane), words = 2ull + 4ull * k;
    const bool have = j < c.n;
    const uint64_t *p = part + (have ? comb_at(c, j) : 0ull) * words;
    uint64_t cnt = have ? p[0] : 0ull, nans = have ? p[1] : 0ull;
#pragma unroll
    for (unsigned off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_down(cnt, off, 64);
        nans += __shfl_down(nans, off, 64);
    }
    uint64_t *o = (c.final_ ? out : part) + c.dst * words;
    const uint64_t b0 = c.final_ && c.n ? begin[c.win] : 0ull;
    if (lane == 0) {
        o[0] = cnt;
        o[1] = nans;
    }
#pragma unroll 1
    for (uint32_t end = 0; end < 2; ++end) {
        const uint64_t *q = p + 2u + 2u * k * end;
        uint32_t cur = 0;
        uint64_t hv = EXT_NAN_BITS, ha = EXT_NONE, hk = 0;
        if (have) { hv = q[0]; ha = q[1]; }
        if (ha != EXT_NONE) { hk = sample_key(__longlong_as_double((long long)hv)); hk = end ? ~hk : hk; }
        uint64_t ov = EXT_NAN_BITS, oa = EXT_NONE;
#pragma unroll 1
        for (uint32_t r = 0; r < k; ++r) {
            uint64_t mx = hk;
#pragma unroll
            for (unsigned off = 1; off < 64; off <<= 1) {
                const uint64_t other = __shfl_xor(mx, off, 64);
                mx = other > mx ? other : mx;
            }
            if (mx == 0) break;  // (the same in every lane) every list is exhausted
            const uint32_t w = (uint32_t)__builtin_ctzll(__ballot(hk == mx));
            const uint64_t v = ext_readlane(hv, w), a = ext_readlane(ha, w);
            if (lane == r) { ov = v; oa = a; }
            if (lane == w) {
                ++cur;
                hk = 0;
                if (cur < k) {
                    hv = q[2u * cur];
                    ha = q[2u * cur + 1u];
                    if (ha != EXT_NONE) { hk = sample_key(__longlong_as_double((long long)hv)); hk = end ? ~hk : hk; }
                }
            }
        }
        if (lane < k) {
            uint64_t *e = o + 2u + 2u * k * end + 2u * lane;
            e[0] = ov;
            e[1] = oa == EXT_NONE ? EXT_NONE : oa - b0;
        }
    }
}

hipError_t launch_ext_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, uint32_t k, void *part,
                            hipStream_t s)
{
    return launch_wave_tasks(k_ext_tiles, n, s, tasks, n, scratch, k, (uint64_t *)part);
}

hipError_t launch_ext_combine(const DevAggComb *tasks, uint32_t n, uint32_t k, void *part, const uint64_t *begin,
                              void *out, hipStream_t s)
{
    return launch_wave_tasks(k_ext_combine, n, s, tasks, n, k, (uint64_t *)part, begin, (uint64_t *)out);
}

}  // namespace atsc
