// atsc_across.hip -- gfx950 kernel of the windowed across (atsc_across_windows_dev): count, min, max and sum over the N
// streams of a call at every position of a range, from the streams' decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across"); the regions, the tasks and what the across kernels
// share are atsc_across_positions.h's.  A position reads one slot per stream and folds them in list order: min and max
// keep the first of equal values, the sum is ((t_0 + t_1) + t_2) + .. with t_k the sample, or -0.0 where it is NaN.  One
// wavefront per task, a lane per position in a lane-strided loop (the fold is short); the loop over the streams is the
// same in every lane.  At stride 1 a lane takes two adjacent positions whose first slot is even (pair_split); the odd
// first and last position of a run, and every position at another stride, go one slot at a time through the same fold,
// so both give the same bytes.  No LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_across_positions.h"

namespace atsc {

namespace {

// the record as it is stored: count, min_at and max_at in the first eight bytes
struct alignas(8) AcrossRec {
    uint64_t head;
    double mn, mx, sum;
};
static_assert(sizeof(AcrossRec) == sizeof(atsc_across_record) && sizeof(AcrossRec) == 32, "the record's layout");

struct AcrossAcc {
    double mn, mx, sum;
    uint32_t count, mn_at, mx_at;
};

DEVI AcrossAcc across_none() { return AcrossAcc{0.0, 0.0, -0.0, 0u, 0xFFFFu, 0xFFFFu}; }

// stream k's sample v into the fold: the first sample that is not NaN starts both extremes, a later one replaces an
// extreme only where it is smaller (larger) as a value
DEVI void across_step(AcrossAcc &a, double v, uint32_t k)
{
    const bool ok = !__builtin_isnan(v);
    a.sum = a.sum + (ok ? v : -0.0);
    const bool first = ok && a.count == 0;
    if (first || (ok && v < a.mn)) { a.mn = v; a.mn_at = k; }
    if (first || (ok && v > a.mx)) { a.mx = v; a.mx_at = k; }
    a.count += ok ? 1u : 0u;
}

// A16: the result lies at a multiple of 16 bytes (the same for every record: a record is 32 bytes)
template <bool A16>
DEVI void across_store(AcrossRec *p, const AcrossAcc &a)
{
    const double nan = __builtin_nan("");
    const bool any = a.count != 0;
    const uint64_t head = (uint64_t)a.count | ((uint64_t)(a.mn_at & 0xFFFFu) << 32) | ((uint64_t)(a.mx_at & 0xFFFFu) << 48);
    const double mn = any ? a.mn : nan, mx = any ? a.mx : nan, sum = any ? a.sum : 0.0;
    store_words<A16>((uint64_t *)p, head, (uint64_t)__double_as_longlong(mn));
    store_words<A16>((uint64_t *)p + 2, (uint64_t)__double_as_longlong(mx), (uint64_t)__double_as_longlong(sum));
}

// the position whose slot is `slot` of every region
template <bool A16>
DEVI void across_one(const double *__restrict__ scratch, const uint64_t *__restrict__ reg, uint32_t ns, uint64_t slot,
                     AcrossRec *out)
{
    AcrossAcc a = across_none();
#pragma unroll 4
    for (uint32_t k = 0; k < ns; ++k) across_step(a, scratch[reg[k] + slot], k);
    across_store<A16>(out, a);
}

}  // namespace

// One wavefront per DevRollTask, into out[t.rec ..].
template <bool A16>
__global__ __launch_bounds__(256) void k_across_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                          const double *__restrict__ scratch,
                                                          const uint64_t *__restrict__ reg, uint32_t ns, uint64_t a0,
                                                          uint64_t stride, AcrossRec *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevRollTask t = tasks[i];
    const uint64_t s0 = t.lo - a0;
    AcrossRec *o = out + t.rec;
    if (stride != 1) {
        for (uint32_t p = lane; p < t.n; p += 64u) across_one<A16>(scratch, reg, ns, s0 + (uint64_t)p * stride, o + p);
        return;
    }
    const PairSplit sp = pair_split(s0, t.n);
    const uint32_t head = sp.head;
    for (uint32_t j = lane; j < sp.pairs; j += 64u) {
        const uint64_t slot = s0 + head + 2ull * j;
        AcrossAcc a = across_none(), b = across_none();
#pragma unroll 4
        for (uint32_t k = 0; k < ns; ++k) {
            const double2 v = *(const double2 *)(scratch + reg[k] + slot);  // one 16-byte load
            across_step(a, v.x, k);
            across_step(b, v.y, k);
        }
        across_store<A16>(o + head + 2u * j, a);
        across_store<A16>(o + head + 2u * j + 1u, b);
    }
    if (head && lane == 0) across_one<A16>(scratch, reg, ns, s0, o);
    if (sp.tail && lane == 1) across_one<A16>(scratch, reg, ns, s0 + t.n - 1u, o + (t.n - 1u));
}

hipError_t launch_across_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                   uint32_t n_streams, uint64_t a0, uint64_t stride, void *out, hipStream_t s)
{
    if (((uintptr_t)out & 15u) == 0)
        return launch_wave_tasks(k_across_positions<true>, n, s, tasks, n, scratch, reg, n_streams, a0, stride, (AcrossRec *)out);
    return launch_wave_tasks(k_across_positions<false>, n, s, tasks, n, scratch, reg, n_streams, a0, stride, (AcrossRec *)out);
}

}  // namespace atsc
