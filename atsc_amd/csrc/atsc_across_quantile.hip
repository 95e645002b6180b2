// atsc_across_quantile.hip -- gfx950 kernel of the windowed across quantiles (atsc_across_quantile_windows_dev): order
// statistics of the N samples that the streams of a call hold at every position of a range.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across quantiles").  The streams lie decoded in the call's
// scratch as the windowed across leaves them (atsc_across.hip): a region per stream, slot j of every region the same
// sample index.  A lane per position, one wavefront per 64 positions of a task, so the 64 lanes read 64 consecutive
// slots of a region at stride 1.  A lane holds its position's column in registers: G = the power of two >= N keys
// (atsc_quantile_rule.h), NaN and padding as KEY_NAN, put in order by a fully unrolled bitonic network (column_sort,
// atsc_tile_reduce.h, which the across value counts share); x[lo] and x[hi]
// of a level come out of the G registers through a binary tree of selects on the rank's bits.  Every index into the
// column is a compile-time constant: no scratch memory, no LDS, no shuffles, no atomics.  Every stride goes through
// the same code, one 8-byte load per stream and position.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_quantile_rule.h"
#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// v[e], e < G: the rank's bit b halves the candidates, G - 1 selects in all.  The selects are written on the bits (a
// mask of the rank's bit): as `odd ? v[1] : v[0]` the compiler turns the first level into a load from a selected
// address, which takes the column out of the registers.
template <int G>
DEVI uint64_t column_at(const uint64_t (&v)[G], uint32_t e)
{
    uint64_t t[G];
#pragma unroll
    for (int i = 0; i < G; ++i) t[i] = v[i];
#pragma unroll
    for (int w = G >> 1, b = 0; w > 0; w >>= 1, ++b) {
        const uint64_t odd = 0ull - (uint64_t)((e >> b) & 1u);
#pragma unroll
        for (int i = 0; i < w; ++i) t[i] = (t[2 * i + 1] & odd) | (t[2 * i] & ~odd);
    }
    return t[0];
}

// the position whose slot is `slot` of every region: its row of n_q levels
template <int G>
DEVI void across_quantile_one(const double *__restrict__ scratch, const uint64_t *__restrict__ reg, uint32_t ns,
                              uint64_t slot, const double *__restrict__ q, uint32_t n_q, int method, double *row)
{
    uint64_t v[G];
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < G; ++k) {
        uint64_t key = KEY_NAN;
        if ((uint32_t)k < ns) {
            const double d = scratch[reg[k] + slot];
            if (!__builtin_isnan(d)) { key = q_key(d); ++n; }
        }
        v[k] = key;
    }
    column_sort<G>(v);
    for (uint32_t j = 0; j < n_q; ++j) {
        double r = __builtin_nan("");
        if (n) {
            const QPick p = q_pick(n, q[j], method);
            const double a = q_unkey(column_at<G>(v, (uint32_t)p.lo));
            // (the second walk of the tree only where some lane's level lies between two ranks)
            double b = a;
            if (__any(p.hi != p.lo)) b = q_unkey(column_at<G>(v, (uint32_t)p.hi));
            r = q_interp(p, a, b);
        }
        row[j] = r;
    }
}

}  // namespace

// A task's positions go 64 to a wavefront, ACR_SLABS wavefronts a task: a position's work is long (the network, then
// the levels) and a piece has few tasks, so a wavefront per task would leave most of the GPU idle.
constexpr uint32_t ACR_SLABS = ACR_TASK / 64u;

// DevRollTask t: t.n positions, the first at sample t.lo of the streams, the others every `stride` samples behind it;
// position p's row is out[(t.rec + p) n_q ..].  reg[k]: where stream k's region begins in the scratch; slot 0 of every
// region is sample a0 of the streams.  ns <= G.
template <int G>
__global__ __launch_bounds__(256) void k_across_quantile_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                                   const double *__restrict__ scratch,
                                                                   const uint64_t *__restrict__ reg, uint32_t ns,
                                                                   uint64_t a0, uint64_t stride,
                                                                   const double *__restrict__ q, uint32_t n_q, int method,
                                                                   double *__restrict__ out)
{
    const uint32_t lane = wave_lane(), w = wave_task(), i = w / ACR_SLABS;
    if (i >= n) return;
    const DevRollTask t = tasks[i];
    const uint32_t p = (w % ACR_SLABS) * 64u + lane;
    if (p >= t.n) return;
    across_quantile_one<G>(scratch, reg, ns, t.lo - a0 + (uint64_t)p * stride, q, n_q, method, out + (t.rec + p) * n_q);
}

hipError_t launch_across_quantile_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                            const uint64_t *reg, uint32_t n_streams, uint64_t a0, uint64_t stride,
                                            const double *q, uint32_t n_q, int method, double *out, hipStream_t s)
{
    static_assert(ACR_TASK % 64u == 0, "whole wavefronts");
    if (n > 0xFFFFFFFFu / ACR_SLABS) return hipErrorInvalidValue;  // (more tasks in a piece than a grid has wavefronts)
#define ACROSS_QUANTILE_G(G)                                                                                           \
    if (n_streams <= G)                                                                                                \
        return launch_wave_tasks(k_across_quantile_positions<G>, n * ACR_SLABS, s, tasks, n, scratch, reg, n_streams, \
                                 a0, stride, q, n_q, method, out);
    ACROSS_QUANTILE_G(1)
    ACROSS_QUANTILE_G(2)
    ACROSS_QUANTILE_G(4)
    ACROSS_QUANTILE_G(8)
    ACROSS_QUANTILE_G(16)
    ACROSS_QUANTILE_G(32)
    ACROSS_QUANTILE_G(64)
#undef ACROSS_QUANTILE_G
    return hipErrorInvalidValue;
}

}  // namespace atsc
