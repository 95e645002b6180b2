// atsc_across_moments.hip -- gfx950 kernel of the windowed across moments (atsc_across_moments_windows_dev): count, mean
// and M2 = sum (x - mean)^2 of the N samples that the streams of a call hold at every position of a range -- what
// `avg`, `stdvar` and `stddev by (...)` are read from.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across moments"): the x half of
// Merge(.. Merge(Merge(leaf_0, leaf_1), leaf_2) .., leaf_(N-1)), Merge being the windowed moments' rule
// (atsc_moment_rule.h, the one copy of it) and leaf_k the node of stream k's sample, empty where that is NaN.  The
// position half of a node (mt, m2t, c) is fed zeros and never stored: the compiler drops it.  The regions, the tasks and
// the mapping of positions to lanes are atsc_across_positions.h's.
//
// The loop over the streams is the same in every lane, and a lane's node and NaN count stay in registers: no LDS, no
// scratch memory.  A lane's fold is a chain of N dependent merges with a divide each.
//   stride != 1   the shared mapping; a record goes out as three 8-byte stores.
//   stride == 1   a lane takes two adjacent positions whose first slot is even (pair_split): 64 pairs to a wavefront,
//                 ACR_TASK / 128 wavefronts a task.  The two records are 48 adjacent bytes and go out as three 16-byte
//                 stores where they begin at a multiple of 16, else as 8, 16, 16 and 8 bytes.  The odd first and last
//                 position of a task go one at a time through the same fold.
// Both paths put the same samples through the same merges in the same order: the same bytes.
// 1.0 / (double)n is a divide, as the rule writes it (DESIGN.md says what a table of the 64 quotients would need).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_across_positions.h"
#include "atsc_moment_node.h"

namespace atsc {

namespace {

static_assert(sizeof(atsc_across_moments) == 24, "the record's layout");

// a position's fold so far: the node of the samples that are not NaN, and how many are
struct AmoAcc {
    Node a;
    uint32_t nans;
};

DEVI AmoAcc amo_none() { return AmoAcc{node_leaf(0.0, 0.0, false), 0u}; }

// stream k's sample x: Merge(accumulator, leaf_k)
DEVI void amo_step(AmoAcc &s, double x)
{
    const bool ok = !__builtin_isnan(x);
    s.nans += ok ? 0u : 1u;
    s.a = node_merge<false>(s.a, node_leaf(x, 0.0, ok));
}

// the record's three words: count and nans, mean, m2
struct AmoRec {
    uint64_t w[3];
};

DEVI AmoRec amo_record(const AmoAcc &s)
{
    const double nan = __builtin_nan("");
    const bool any = s.a.n != 0;
    return AmoRec{{(uint64_t)s.a.n | ((uint64_t)s.nans << 32), (uint64_t)__double_as_longlong(any ? s.a.mx : nan),
                   (uint64_t)__double_as_longlong(any ? s.a.m2x : nan)}};
}

// the position whose slot is `slot` of every region, into the three words at p
DEVI void amo_one(const double *__restrict__ scratch, const uint64_t *__restrict__ reg, uint32_t ns, uint64_t slot, uint64_t *p)
{
    AmoAcc s = amo_none();
#pragma unroll 4
    for (uint32_t k = 0; k < ns; ++k) amo_step(s, scratch[reg[k] + slot]);
    const AmoRec r = amo_record(s);
    p[0] = r.w[0];
    p[1] = r.w[1];
    p[2] = r.w[2];
}

// two adjacent records, the six words at p (8-byte aligned)
DEVI void amo_store_two(uint64_t *p, const AmoRec &a, const AmoRec &b)
{
    if (((uintptr_t)p & 15u) == 0) {
        ((ulonglong2 *)p)[0] = make_ulonglong2(a.w[0], a.w[1]);
        ((ulonglong2 *)p)[1] = make_ulonglong2(a.w[2], b.w[0]);
        ((ulonglong2 *)p)[2] = make_ulonglong2(b.w[1], b.w[2]);
    } else {
        p[0] = a.w[0];
        *(ulonglong2 *)(p + 1) = make_ulonglong2(a.w[1], a.w[2]);
        *(ulonglong2 *)(p + 3) = make_ulonglong2(b.w[0], b.w[1]);
        p[5] = b.w[2];
    }
}

}  // namespace

// wavefronts per task at stride 1: 64 pairs of positions each
constexpr uint32_t AMO_PAIR_SLABS = ACR_TASK / 128u;

// Position p's record is the three words at out[3 (t.rec + p) ..].  PAIRS: stride is 1.
template <bool PAIRS>
__global__ __launch_bounds__(256) void k_across_moments_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                                  const double *__restrict__ scratch,
                                                                  const uint64_t *__restrict__ reg, uint32_t ns, uint64_t a0,
                                                                  uint64_t stride, uint64_t *__restrict__ out)
{
    if constexpr (!PAIRS) {
        DevRollTask t;
        uint32_t p;
        if (!slab_position(tasks, n, t, p)) return;
        amo_one(scratch, reg, ns, slab_slot(t, a0, p, stride), out + 3ull * t.rec + 3ull * p);
    } else {
        uint32_t i, j;
        if (!slab_wave<AMO_PAIR_SLABS>(n, i, j)) return;
        j += wave_lane();  // the lane's pair of the task
        const DevRollTask t = tasks[i];
        const uint64_t s0 = t.lo - a0;
        uint64_t *o = out + 3ull * t.rec;
        const PairSplit sp = pair_split(s0, t.n);
        const uint32_t head = sp.head, pairs = sp.pairs, tail = sp.tail;
        if (j < pairs) {
            const uint64_t slot = s0 + head + 2ull * j;
            AmoAcc a = amo_none(), b = amo_none();
#pragma unroll 4
            for (uint32_t k = 0; k < ns; ++k) {
                const double2 v = *(const double2 *)(scratch + reg[k] + slot);  // one 16-byte load
                amo_step(a, v.x);
                amo_step(b, v.y);
            }
            amo_store_two(o + 3ull * (head + 2u * j), amo_record(a), amo_record(b));
        }
        // the two single positions go to the lanes behind the pairs: j < ACR_TASK / 2 in every wavefront of the task, and
        // pairs + head + tail <= ACR_TASK / 2 + 1, so the index wraps to lane 0 of the first wavefront only where a full
        // task begins at an odd slot
        constexpr uint32_t M = ACR_TASK / 2u - 1u;
        if (head && j == (pairs & M)) amo_one(scratch, reg, ns, s0, o);
        if (tail && j == ((pairs + head) & M)) amo_one(scratch, reg, ns, s0 + t.n - 1u, o + 3ull * (t.n - 1u));
    }
}

hipError_t launch_across_moments_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                                           uint32_t n_streams, uint64_t a0, uint64_t stride, void *out, hipStream_t s)
{
    static_assert(ACR_TASK % 128u == 0 && (ACR_TASK & (ACR_TASK - 1u)) == 0, "whole wavefronts of pairs; the index mask");
    if (n_streams == 0 || ((uintptr_t)out & 7u)) return hipErrorInvalidValue;
    if (stride == 1)
        return launch_slab_tasks<AMO_PAIR_SLABS>(k_across_moments_positions<true>, n, s, tasks, n, scratch, reg, n_streams, a0,
                                                 stride, (uint64_t *)out);
    return launch_slab_tasks(k_across_moments_positions<false>, n, s, tasks, n, scratch, reg, n_streams, a0, stride,
                             (uint64_t *)out);
}

}  // namespace atsc
