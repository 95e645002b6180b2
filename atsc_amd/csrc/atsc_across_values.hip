// atsc_across_values.hip -- gfx950 kernel of the windowed across value counts (atsc_across_values_windows_dev): at every
// position of a range, which values the call's N streams hold there and how many streams hold each -- PromQL's
// count_values: replicas per build version, members per leader id, hosts per breaker state.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across value counts"): the windowed value counts' record
// (atsc_values.hip) of the column x_0 .. x_(N-1) as if it were a window of N samples.  No arithmetic touches a sample:
// an entry is a value's bits and an integer count.  The regions, the tasks and the mapping of positions to lanes are
// atsc_across_positions.h's.
//
// A lane holds its column as keys (sample_key, atsc_tile_reduce.h: unsigned order is value order, both zeros on one
// key) in G registers, G the power of two >= N; a NaN, a sample that is not listed (key <= above's key) and the padding are AV_NONE = ~0,
// which no sample's key is and which sorts last; nans and below are counted while loading.  column_sort puts the keys
// in order; one pass over the G registers in compile-time order then reads the entries off: a register that differs
// from its predecessor closes the open entry -- the D-th distinct value with the length of its run -- which is written
// where D < k.  Every index into the column is a compile-time constant: no scratch memory, no shuffles, no atomics.
//
// Stores.  A record is 4 + 2 k words and the word an entry goes to depends on the lane's data.  The lane writes its own
// record: the head, the entries as their runs close, then (NaN, 0) from `distinct` to k -- every word of every record
// once, nothing cleared beforehand, 16 bytes a store where the result lies at a multiple of 16 bytes.  A wavefront's 64
// records are 64 (32 + 16 k) consecutive bytes, so what the lanes write piecemeal the L2 gathers into whole lines before
// it goes to memory.  The other way -- records staged in LDS at an odd pitch of 4 + 2 k + 1 words, as many rows a pass
// as 16 KB a wavefront hold, and stored by the wavefront in consecutive 8-byte words -- was built and measured beside
// this one on the MI355X (profiles/across_values_timing.txt) and is not kept: per launch it took 33 against 42 us at
// N = 8, k = 4 over 10^6 positions, the same 187 against 190 us a piece at N = 64, k = 4 (the network, not the store,
// is the time there), and more where records are long or positions few, 123 against 104 us at k = 32 (three passes a
// wavefront) and 62 against 56 us at stride 15; the calls' times did not differ beyond their spread.  The lane's store
// needs no LDS, no passes and no fences.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_across_positions.h"

namespace atsc {

namespace {

constexpr uint64_t AV_NONE = ~0ull;  // no key: NaN, not listed, padding
constexpr uint64_t AV_NAN_BITS = 0x7ff8000000000000ull;

// the column of the position whose slot is `slot` of every region: its listed samples' keys in v, ascending, AV_NONE
// behind them; the NaN samples and the others that are not listed counted
template <int G>
DEVI void av_column(const double *__restrict__ scratch, const uint64_t *__restrict__ reg, uint32_t ns, uint64_t slot,
                    uint64_t above, uint64_t (&v)[G], uint32_t &nans, uint32_t &below)
{
    nans = below = 0;
#pragma unroll
    for (int j = 0; j < G; ++j) {
        uint64_t key = AV_NONE;
        if ((uint32_t)j < ns) {
            const uint64_t ks = sample_key(scratch[reg[j] + slot]);
            const bool listed = ks > above;
            nans += ks == 0 ? 1u : 0u;
            below += ks != 0 && !listed ? 1u : 0u;
            key = listed ? ks : AV_NONE;
        }
        v[j] = key;
    }
    column_sort<G>(v);
}

// the record of a sorted column: put(w, a, b) writes its words w and w + 1, every pair of words once
template <int G, class Put>
DEVI void av_record(const uint64_t (&v)[G], uint32_t ns, uint32_t nans, uint32_t below, uint32_t k, Put put)
{
    // d: distinct listed values closed so far; (pk, pn): the open run.  The sentinel behind the column closes the last
    // run; a run of AV_NONE is never closed (nothing differs from it behind it)
    uint32_t d = 0, pn = 1;
    uint64_t pk = v[0];
#pragma unroll
    for (int j = 1; j <= G; ++j) {
        const uint64_t cur = j < G ? v[j] : AV_NONE;
        const bool start = cur != pk;
        if (start) {
            if (d < k) put(4u + 2u * d, val_bits(pk), (uint64_t)pn);
            ++d;
        }
        pn = start ? 1u : pn + 1u;
        pk = cur;
    }
    const uint32_t distinct = d < k ? d : k;
    put(0u, (uint64_t)ns, (uint64_t)nans);
    put(2u, (uint64_t)below, (uint64_t)distinct | ((uint64_t)(d > k ? 1u : 0u) << 32));
    for (uint32_t e = distinct; e < k; ++e) put(4u + 2u * e, AV_NAN_BITS, 0ull);
}

}  // namespace

// Position p's record is the 4 + 2 k words at out[(t.rec + p) (4 + 2 k) ..].  1 <= ns <= G, 1 <= k; above: the key of the
// call's `above`, 0 for NaN.  A16: the result lies at a multiple of 16 bytes (a record is 32 + 16 k bytes, so the head's
// halves and every entry of every record do).
template <int G, bool A16>
__global__ __launch_bounds__(256) void k_across_values_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                                 const double *__restrict__ scratch,
                                                                 const uint64_t *__restrict__ reg, uint32_t ns, uint64_t a0,
                                                                 uint64_t stride, uint32_t k, uint64_t above,
                                                                 uint64_t *__restrict__ out)
{
    DevRollTask t;
    uint32_t p;
    if (!slab_position(tasks, n, t, p)) return;
    uint64_t *rec = out + (t.rec + p) * (4u + 2ull * k);
    uint64_t v[G];
    uint32_t nans, below;
    av_column<G>(scratch, reg, ns, slab_slot(t, a0, p, stride), above, v, nans, below);
    av_record<G>(v, ns, nans, below, k, [rec](uint32_t x, uint64_t a, uint64_t b) { store_words<A16>(rec + x, a, b); });
}

hipError_t launch_across_values_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                          uint32_t n_streams, uint64_t a0, uint64_t stride, uint32_t k, uint64_t above,
                                          void *out, hipStream_t s)
{
    if (k == 0 || k > 32u || n_streams == 0 || ((uintptr_t)out & 7u)) return hipErrorInvalidValue;
    const bool a16 = ((uintptr_t)out & 15u) == 0;
    return pow2_dispatch<64>(n_streams, [&](auto g) {
        constexpr int G = decltype(g)::value;
        return launch_slab_tasks(a16 ? k_across_values_positions<G, true> : k_across_values_positions<G, false>, n, s, tasks, n,
                                 scratch, reg, n_streams, a0, stride, k, above, (uint64_t *)out);
    });
}

}  // namespace atsc
