// atsc_across_extremes.hip -- gfx950 kernel of the windowed across extremes (atsc_across_extremes_windows_dev): the k
// largest and the k smallest of the N samples that the streams of a call hold at every position of a range, with the
// index of the stream that holds each.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across extremes"): the windowed extremes' record of the
// column x_0 .. x_(N-1), a sample's offset being its stream's place in the list.  The regions, the tasks and the mapping
// of positions to lanes are atsc_across_positions.h's.
//
// A lane keeps two sorted lists of KP entries (value, stream index) in registers, KP the power of two >= k.  It walks
// the streams in list order -- the loop is the same in every lane -- and puts every sample that is not NaN through a
// fully unrolled insertion step per list: entry j takes its upper neighbour where the sample belongs in front of that
// one, the sample itself where it belongs in front of entry j only.  "In front of" is a strict compare of doubles
// (`>` for the largest, `<` for the smallest), or an empty entry: walking in list order, a later equal value never
// passes an earlier one, which is the tie rule, and -0.0 == +0.0 as doubles, which is the zero rule; the value kept is
// the sample's own bits.  Where no lane's sample is in front of a list's last entry, the step is skipped for the whole
// wavefront.  Every index into a list is a compile-time constant: no scratch memory, no LDS, no shuffles, no atomics.
// The first k entries of each list go out; the lists' first j entries do not depend on KP.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_across_positions.h"

namespace atsc {

namespace {

constexpr uint32_t AEX_NONE = 0xFFFFFFFFu;  // an empty entry's stream index in a lane; ATSC_EXTREMES_NONE in the record

// a sorted list of KP (value, stream index): empty entries (NaN, AEX_NONE) behind the others
template <int KP>
struct AexList {
    double v[KP];
    uint32_t at[KP];
};

template <int KP>
DEVI void aex_clear(AexList<KP> &l)
{
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        l.v[j] = __builtin_nan("");
        l.at[j] = AEX_NONE;
    }
}

// x in front of entry e: e is empty (NaN: no compare with it holds) or x is strictly larger (LARGEST) / smaller
template <bool LARGEST>
DEVI bool aex_front(double x, double e)
{
    return LARGEST ? !(x <= e) : !(x >= e);
}

// stream k's sample x, not NaN where ok, into the list.  c[j]: x belongs in front of entry j; the list is sorted, so
// c is false .. false true .. true, and entry j moves down by one where c[j - 1]
template <bool LARGEST, int KP>
DEVI void aex_insert(AexList<KP> &l, double x, uint32_t k, bool ok)
{
    if (!__any(ok && aex_front<LARGEST>(x, l.v[KP - 1]))) return;
    bool c[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) c[j] = ok && aex_front<LARGEST>(x, l.v[j]);
#pragma unroll
    for (int j = KP - 1; j > 0; --j) {
        l.v[j] = c[j - 1] ? l.v[j - 1] : c[j] ? x : l.v[j];
        l.at[j] = c[j - 1] ? l.at[j - 1] : c[j] ? k : l.at[j];
    }
    l.v[0] = c[0] ? x : l.v[0];
    l.at[0] = c[0] ? k : l.at[0];
}

// A16: the result lies at a multiple of 16 bytes (a record is 16 + 32 k bytes, so every entry of every record does)
template <bool A16, int KP>
DEVI void aex_store_list(uint64_t *p, const AexList<KP> &l, uint32_t k)
{
#pragma unroll
    for (int j = 0; j < KP; ++j)
        if ((uint32_t)j < k)
            store_words<A16>(p + 2 * j, (uint64_t)__double_as_longlong(l.v[j]), l.at[j] == AEX_NONE ? ~0ull : (uint64_t)l.at[j]);
}

}  // namespace

// Position p's record is the 2 + 4 k words at out[(t.rec + p) (2 + 4 k) ..].  1 <= k <= KP, ns >= 1.
template <int KP, bool A16>
__global__ __launch_bounds__(256) void k_across_extremes_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                                   const double *__restrict__ scratch,
                                                                   const uint64_t *__restrict__ reg, uint32_t ns,
                                                                   uint64_t a0, uint64_t stride, uint32_t k,
                                                                   uint64_t *__restrict__ out)
{
    DevRollTask t;
    uint32_t p;
    if (!slab_position(tasks, n, t, p)) return;
    const uint64_t slot = slab_slot(t, a0, p, stride);
    AexList<KP> big, small;
    aex_clear(big);
    aex_clear(small);
    uint32_t nans = 0;
    double next = scratch[reg[0] + slot];
    for (uint32_t s = 0; s < ns; ++s) {
        const double x = next;
        if (s + 1 < ns) next = scratch[reg[s + 1] + slot];  // (the next stream's sample under way during the step)
        const bool ok = !__builtin_isnan(x);
        nans += ok ? 0u : 1u;
        aex_insert<true>(big, x, s, ok);
        aex_insert<false>(small, x, s, ok);
    }
    uint64_t *rec = out + (t.rec + p) * (2u + 4ull * k);
    store_words<A16>(rec, ns, nans);
    aex_store_list<A16>(rec + 2, big, k);
    aex_store_list<A16>(rec + 2 + 2ull * k, small, k);
}

hipError_t launch_across_extremes_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                            uint32_t n_streams, uint64_t a0, uint64_t stride, uint32_t k, void *out,
                                            hipStream_t s)
{
    if (k == 0 || n_streams == 0) return hipErrorInvalidValue;
    const bool a16 = ((uintptr_t)out & 15u) == 0;
    return pow2_dispatch<16>(k, [&](auto kp) {
        constexpr int KP = decltype(kp)::value;
        return launch_slab_tasks(a16 ? k_across_extremes_positions<KP, true> : k_across_extremes_positions<KP, false>, n, s, tasks,
                                 n, scratch, reg, n_streams, a0, stride, k, (uint64_t *)out);
    });
}

}  // namespace atsc
