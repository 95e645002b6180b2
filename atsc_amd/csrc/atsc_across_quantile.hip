// atsc_across_quantile.hip -- gfx950 kernel of the windowed across quantiles (atsc_across_quantile_windows_dev): order
// statistics of the N samples that the streams of a call hold at every position of a range.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed across quantiles"); the regions, the tasks and the mapping
// of positions to lanes are atsc_across_positions.h's, so the 64 lanes read 64 consecutive slots of a region at stride
// 1.  A lane holds its position's column in registers: G = the power of two >= N keys
// (atsc_quantile_rule.h), NaN and padding as KEY_NAN, put in order by a fully unrolled bitonic network (column_sort,
// atsc_tile_reduce.h, which the across value counts share); x[lo] and x[hi]
// of a level come out of the G registers through a binary tree of selects on the rank's bits.  Every index into the
// column is a compile-time constant: no scratch memory, no LDS, no shuffles, no atomics.  Every stride goes through
// the same code, one 8-byte load per stream and position.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_across_positions.h"
#include "atsc_quantile_rule.h"

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

// Position p's row is out[(t.rec + p) n_q ..].  ns <= G.
template <int G>
__global__ __launch_bounds__(256) void k_across_quantile_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                                   const double *__restrict__ scratch,
                                                                   const uint64_t *__restrict__ reg, uint32_t ns,
                                                                   uint64_t a0, uint64_t stride,
                                                                   const double *__restrict__ q, uint32_t n_q, int method,
                                                                   double *__restrict__ out)
{
    DevRollTask t;
    uint32_t p;
    if (!slab_position(tasks, n, t, p)) return;
    across_quantile_one<G>(scratch, reg, ns, slab_slot(t, a0, p, stride), q, n_q, method, out + (t.rec + p) * n_q);
}

hipError_t launch_across_quantile_positions(const DevRollTask *tasks, uint32_t n, const double *scratch,
                                            const uint64_t *reg, uint32_t n_streams, uint64_t a0, uint64_t stride,
                                            const double *q, uint32_t n_q, int method, double *out, hipStream_t s)
{
    return pow2_dispatch<64>(n_streams, [&](auto g) {
        return launch_slab_tasks(k_across_quantile_positions<decltype(g)::value>, n, s, tasks, n, scratch, reg, n_streams, a0,
                                 stride, q, n_q, method, out);
    });
}

}  // namespace atsc
