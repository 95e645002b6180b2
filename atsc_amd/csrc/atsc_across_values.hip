// atsc_across_values.hip -- gfx950 kernel of the windowed across value counts (atsc_across_values_windows_dev): at every
// position of a range, which values the call's N streams hold there and how many streams hold each -- PromQL's
// count_values: replicas per build version, members per leader id, hosts per breaker state.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across value counts"): the windowed value counts' record
// (atsc_values.hip) of the column x_0 .. x_(N-1) as if it were a window of N samples.  No arithmetic touches a sample:
// an entry is a value's bits and an integer count.  The streams lie decoded in the call's scratch as the windowed across
// leaves them (atsc_across.hip): a region per stream, slot j of every region the same sample index.
//
// A lane per position, one wavefront per 64 positions of a task, as in atsc_across_quantile.hip.  A lane holds its
// column as keys (sample_key, atsc_tile_reduce.h: unsigned order is value order, both zeros on one key) in G registers,
// G the power of two >= N; a NaN, a sample that is not listed (key <= above's key) and the padding are AV_NONE = ~0,
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

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

constexpr uint64_t AV_NONE = ~0ull;  // no key: NaN, not listed, padding
constexpr uint64_t AV_NAN_BITS = 0x7ff8000000000000ull;

// A16: the result lies at a multiple of 16 bytes (a record is 32 + 16 k bytes, so the head's halves and every entry of
// every record do), and a pair of words goes out as one 16-byte store; else as two of 8 bytes
template <bool A16>
DEVI void av_store(uint64_t *p, uint64_t a, uint64_t b)
{
    if constexpr (A16) {
        *(ulonglong2 *)p = make_ulonglong2(a, b);
    } else {
        p[0] = a;
        p[1] = b;
    }
}

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

// A task's positions go 64 to a wavefront, AV_SLABS wavefronts a task, as the across quantiles' do.
constexpr uint32_t AV_SLABS = ACR_TASK / 64u;

// DevRollTask t: t.n positions, the first at sample t.lo of the streams, the others every `stride` samples behind it;
// position p's record is the 4 + 2 k words at out[(t.rec + p) (4 + 2 k) ..].  reg[s]: where stream s's region begins in
// the scratch; slot 0 of every region is sample a0 of the streams.  1 <= ns <= G, 1 <= k; above: the key of the call's
// `above`, 0 for NaN.
template <int G, bool A16>
__global__ __launch_bounds__(256) void k_across_values_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                                 const double *__restrict__ scratch,
                                                                 const uint64_t *__restrict__ reg, uint32_t ns, uint64_t a0,
                                                                 uint64_t stride, uint32_t k, uint64_t above,
                                                                 uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), w = wave_task(), i = w / AV_SLABS;
    if (i >= n) return;
    const DevRollTask t = tasks[i];
    const uint32_t p = (w % AV_SLABS) * 64u + lane;
    if (p >= t.n) return;
    uint64_t *rec = out + (t.rec + p) * (4u + 2ull * k);
    uint64_t v[G];
    uint32_t nans, below;
    av_column<G>(scratch, reg, ns, t.lo - a0 + (uint64_t)p * stride, above, v, nans, below);
    av_record<G>(v, ns, nans, below, k, [rec](uint32_t x, uint64_t a, uint64_t b) { av_store<A16>(rec + x, a, b); });
}

hipError_t launch_across_values_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                          uint32_t n_streams, uint64_t a0, uint64_t stride, uint32_t k, uint64_t above,
                                          void *out, hipStream_t s)
{
    static_assert(ACR_TASK % 64u == 0, "whole wavefronts");
    if (n > 0xFFFFFFFFu / AV_SLABS) return hipErrorInvalidValue;  // (more tasks in a piece than a grid has wavefronts)
    if (k == 0 || k > 32u || n_streams == 0 || ((uintptr_t)out & 7u)) return hipErrorInvalidValue;
    const bool a16 = ((uintptr_t)out & 15u) == 0;
#define ACROSS_VALUES_G(G)                                                                                                \
    if (n_streams <= G) {                                                                                                 \
        if (a16)                                                                                                          \
            return launch_wave_tasks(k_across_values_positions<G, true>, n * AV_SLABS, s, tasks, n, scratch, reg, n_streams, \
                                     a0, stride, k, above, (uint64_t *)out);                                              \
        return launch_wave_tasks(k_across_values_positions<G, false>, n * AV_SLABS, s, tasks, n, scratch, reg, n_streams,  \
                                 a0, stride, k, above, (uint64_t *)out);                                                  \
    }
    ACROSS_VALUES_G(1)
    ACROSS_VALUES_G(2)
    ACROSS_VALUES_G(4)
    ACROSS_VALUES_G(8)
    ACROSS_VALUES_G(16)
    ACROSS_VALUES_G(32)
    ACROSS_VALUES_G(64)
#undef ACROSS_VALUES_G
    return hipErrorInvalidValue;
}

}  // namespace atsc
