// atsc_quantile_rule.h -- the quantile rule of the contract (include/atsc_hip.h, DESIGN.md "Windowed quantiles") as the
// device evaluates it: the total-order key, the ranks of a level and the interpolation.  One copy for the kernels that
// select order statistics: along time (atsc_quantile.hip) and across streams (atsc_across_quantile.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_device.h"

namespace atsc {

constexpr uint64_t KEY_NAN = ~0ull;   // NaN sorts above every key and is not counted

// IEEE total order as an unsigned key: negative values reversed below the positive ones
__device__ __forceinline__ uint64_t q_key(double v)
{
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

__device__ __forceinline__ double q_unkey(uint64_t k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// the rank rule: level q of n >= 1 sorted samples reads x[lo] and x[hi] and interpolates at t
struct QPick {
    uint64_t lo, hi;
    double t;
};

__device__ __forceinline__ QPick q_pick(uint64_t n, double q, int method)
{
    const double v = (double)(n - 1) * q;
    const double f = __builtin_floor(v);
    QPick p;
    p.t = 0.0;
    if (method == ATSC_QUANTILE_LOWER) {
        p.lo = p.hi = (uint64_t)f;
    } else if (method == ATSC_QUANTILE_HIGHER) {
        p.lo = p.hi = (uint64_t)__builtin_ceil(v);
    } else if (method == ATSC_QUANTILE_NEAREST) {
        p.lo = p.hi = (uint64_t)__builtin_rint(v);  // ties to even, as numpy.around
    } else {
        p.lo = (uint64_t)f;
        p.hi = p.lo + 1 < n ? p.lo + 1 : n - 1;
        p.t = v - f;
    }
    return p;
}

// NumPy's _lerp without contraction (the library is built with -ffp-contract=off)
__device__ __forceinline__ double q_interp(const QPick &p, double a, double b)
{
    if (p.t == 0.0 || p.lo == p.hi) return a;
    const double d = b - a;
    return p.t >= 0.5 ? b - d * (1.0 - p.t) : a + d * p.t;
}

}  // namespace atsc
