// atsc_moment_rule.h -- Merge(a, b) of two centred co-moment nodes: THE rule of the windowed moments, the windowed pair
// moments and the windowed across moments (include/atsc_hip.h, DESIGN.md "Windowed moments"), in one copy for the
// kernels (atsc_moment_node.h, atsc_across_moments.hip) and for the host's atsc_across_moments_merge
// (atsc_windows.cpp).  Plain arithmetic only: nothing of the device's is named here, and every file that includes this
// is compiled with -ffp-contract=off, which is what makes each operation round once.
#pragma once

#if defined(__HIP__)
#define ATSC_MOMENT_RULE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define ATSC_MOMENT_RULE_FN inline
#endif

namespace atsc {

namespace {

// Merge(a, b).  EQ: the caller knows na == nb != 0 -- then w = nb / (2 nb) is 0.5 exactly and f = na * 0.5, the bits
// the divide gives; nothing else differs from the general rule.  ND: a node (n, mx, m2x, mt, m2t, c) with a count of
// any unsigned width.
template <bool EQ, class ND>
ATSC_MOMENT_RULE_FN ND node_merge(const ND &a, const ND &b)
{
    const decltype(a.n) n = a.n + b.n;
    const double w = EQ ? 0.5 : (double)b.n / (double)n;
    const double f = (double)a.n * w;
    const double dx = b.mx - a.mx, dt = b.mt - a.mt;
    ND r;
    r.mx = a.mx + dx * w;
    r.mt = a.mt + dt * w;
    r.m2x = (a.m2x + b.m2x) + (dx * dx) * f;
    r.m2t = (a.m2t + b.m2t) + (dt * dt) * f;
    r.c = (a.c + b.c) + (dx * dt) * f;
    r.n = n;
    if (EQ) return r;
    return b.n == 0 ? a : a.n == 0 ? b : r;
}

}  // namespace

}  // namespace atsc
