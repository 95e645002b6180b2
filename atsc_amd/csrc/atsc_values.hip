// atsc_values.hip -- gfx950 kernels of the windowed value counts (atsc_values_windows_dev): per window its k smallest
// distinct values with their exact multiplicities, the number of NaN samples, the number of samples not above the call's
// `above` and the window's length, counted from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed value counts").  No arithmetic touches a sample: an entry is
// a value's bits and an integer count, so the record is bit-exact by construction.  A sample's KEY is the extremes'
// (sample_key, atsc_tile_reduce.h): unsigned integer order is value order, both zeros lie on +0.0's key, no sample's key
// is 0 and none is ~0.  `above` reaches the kernels as its key (0 for NaN): a sample is listed iff its key is greater.
// ~0 marks "no key": a slot outside the window, a NaN, a sample that is not listed, a key already counted, an exhausted
// list.
//
// A partial has the record's layout, 4 + 2 k eight-byte words: count, nans, below, (distinct, more), then k entries
// (value bits, n), an entry that is missing being (NaN, 0).  No position occurs in it, so the partial of a shared full
// tile serves every window that shares it as it is, and the final combine pass writes the window's record without a
// begin to subtract.  One wavefront counts one tile or merges one group of 64 partials.  No atomics, no LDS: every
// partial has one writer, and a list lives one entry per lane in lanes 0 .. k - 1 (k <= 32).
//
// The tile kernel keeps the 16-byte loads and slot-to-lane mapping of atsc_tile_reduce.h and the lane's 32 keys in
// registers.  A round takes the wavefront's smallest key, counts it and takes it out of every lane's keys; the rounds
// end, the same in every lane, when no key is left, and the look after the k-th round only sets `more`: at most
// min(D, k) + 1 rounds for a tile of D distinct listed values, one for a constant tile.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

constexpr uint64_t VAL_NONE = ~0ull;
constexpr uint64_t VAL_NAN_BITS = 0x7ff8000000000000ull;

__device__ __forceinline__ uint64_t val_wave_min(uint64_t v)
{
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) {
        const uint64_t other = __shfl_xor(v, off, 64);
        v = other < v ? other : v;
    }
    return v;
}

// the wavefront's sum, in every lane
template <class T>
__device__ __forceinline__ T val_wave_sum(T v)
{
#pragma unroll
    for (unsigned off = 1; off < 64; off <<= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the partial or record at o: lane 0 the head, lane l < k entry l, which is (key, n) where l < distinct
__device__ __forceinline__ void val_store(uint64_t *o, uint32_t lane, uint32_t k, uint64_t count, uint64_t nans,
                                          uint64_t below, uint32_t distinct, bool more, uint64_t key, uint64_t n)
{
    if (lane == 0) {
        o[0] = count;
        o[1] = nans;
        o[2] = below;
        o[3] = (uint64_t)distinct | ((uint64_t)(more ? 1u : 0u) << 32);
    }
    if (lane < k) {
        const bool filled = lane < distinct;
        o[4u + 2u * lane] = filled ? val_bits(key) : VAL_NAN_BITS;
        o[5u + 2u * lane] = filled ? n : 0ull;
    }
}

}  // namespace

// One wavefront per DevAggTile: the partial of the slots [lo, hi) of the tile at scratch[src] into part[dst (4 + 2 k)].
__global__ __launch_bounds__(256) void k_val_tiles(const DevAggTile *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, uint32_t k, uint64_t above,
                                                   uint64_t *__restrict__ part)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevAggTile t = tasks[i];
    const double *x = scratch + t.src;
    // the lane's 32 keys; its NaN samples and its samples that are not listed
    uint64_t key[32];
    uint32_t nans = 0, below = 0;
#pragma unroll
    for (uint32_t kk = 0; kk < 4; ++kk) {
        const uint32_t v = lane + 64u * kk;
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t j = tile_slot(v, q);
            const double2 d = tile_load(x, j, t.lo, t.hi, 0.0);
#pragma unroll
            for (uint32_t e = 0; e < 2; ++e) {
                const double s = e ? d.y : d.x;
                const bool in = tile_in(j + e, t.lo, t.hi);
                const uint64_t ks = in ? sample_key(s) : 0ull;
                const bool listed = ks > above;
                nans += in && s != s ? 1u : 0u;
                below += ks != 0 && !listed ? 1u : 0u;
                key[8u * kk + 2u * q + e] = listed ? ks : VAL_NONE;
            }
        }
    }
    nans = val_wave_sum(nans);
    below = val_wave_sum(below);
    uint64_t ek = VAL_NONE;
    uint32_t en = 0, distinct = 0;
    bool more = false;
#pragma unroll 1
    for (uint32_t r = 0; r <= k; ++r) {
        uint64_t m = key[0];
#pragma unroll
        for (uint32_t j = 1; j < 32; ++j) m = key[j] < m ? key[j] : m;
        m = val_wave_min(m);
        if (m == VAL_NONE) break;  // (the same in every lane) no key is left
        if (r == k) {
            more = true;
            break;
        }
        uint32_t c = 0;
#pragma unroll
        for (uint32_t j = 0; j < 32; ++j) {
            const bool eq = key[j] == m;
            c += eq ? 1u : 0u;
            key[j] = eq ? VAL_NONE : key[j];
        }
        c = val_wave_sum(c);
        if (lane == r) {
            ek = m;
            en = c;
        }
        distinct = r + 1u;
    }
    val_store(part + t.dst * (4ull + 2ull * k), lane, k, t.hi - t.lo, nans, below, distinct, more, ek, en);
}

// One wavefront per DevAggComb: the group's partials (comb_entry, comb_at), one per lane, into the partial part[dst] or,
// in the final pass, the window's record out[dst].  count, nans and below add.  Every lane holds a cursor into its
// partial's list and the key and n under it.  Round r takes the wave minimum of those keys; every lane that holds it adds
// its n to the wave's sum and reads its next entry; the sum goes to lane r of the result.  After the rounds, more: a lane
// still holds a key, or a partial came with more (what that hides lies above its own k-th value, which is no smaller than
// the group's).
__global__ __launch_bounds__(256) void k_val_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks, uint32_t k,
                                                     uint64_t *__restrict__ part, uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const uint64_t j = comb_entry(c, lane), words = 4ull + 2ull * k;
    const bool have = j < c.n;
    const uint64_t *p = part + (have ? comb_at(c, j) : 0ull) * words;
    uint64_t cnt = 0, nans = 0, below = 0, dm = 0;
    if (have) {
        cnt = p[0];
        nans = p[1];
        below = p[2];
        dm = p[3];
    }
    cnt = val_wave_sum(cnt);
    nans = val_wave_sum(nans);
    below = val_wave_sum(below);
    const uint32_t nd = (uint32_t)dm < k ? (uint32_t)dm : k;  // the partial's entries
    const uint64_t *q = p + 4;
    uint32_t cur = 0;
    uint64_t hk = VAL_NONE, hn = 0;
    if (cur < nd) {
        hk = sample_key(__longlong_as_double((long long)q[0]));
        hn = q[1];
    }
    uint64_t ek = VAL_NONE, en = 0;
    uint32_t distinct = 0;
#pragma unroll 1
    for (uint32_t r = 0; r < k; ++r) {
        const uint64_t m = val_wave_min(hk);
        if (m == VAL_NONE) break;  // (the same in every lane) every list is exhausted
        const bool hit = hk == m;
        const uint64_t s = val_wave_sum(hit ? hn : 0ull);
        if (lane == r) {
            ek = m;
            en = s;
        }
        distinct = r + 1u;
        if (hit) {
            ++cur;
            hk = VAL_NONE;
            hn = 0;
            if (cur < nd) {
                hk = sample_key(__longlong_as_double((long long)q[2u * cur]));
                hn = q[2u * cur + 1u];
            }
        }
    }
    const bool more = __ballot(hk != VAL_NONE || (dm >> 32) != 0) != 0;
    val_store((c.final_ ? out : part) + c.dst * words, lane, k, cnt, nans, below, distinct, more, ek, en);
}

hipError_t launch_val_tiles(const DevAggTile *tasks, uint32_t n, const double *scratch, uint32_t k, uint64_t above,
                            void *part, hipStream_t s)
{
    return launch_wave_tasks(k_val_tiles, n, s, tasks, n, scratch, k, above, (uint64_t *)part);
}

hipError_t launch_val_combine(const DevAggComb *tasks, uint32_t n, uint32_t k, void *part, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_val_combine, n, s, tasks, n, k, (uint64_t *)part, (uint64_t *)out);
}

}  // namespace atsc
