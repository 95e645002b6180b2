// atsc_hist_bins.h -- the value bins of the histograms, shared by the windowed histograms' kernels (atsc_histogram.hip),
// the windowed rolling histograms' (atsc_rolling_histogram.hip) and the windowed across histograms'
// (atsc_across_histogram.hip): the bin of one sample by a branch-free search over the edges in LDS, a wavefront's
// counting of its lanes' bins with LDS integer atomics, and the fence pair that orders a wavefront's LDS rows between
// its lanes.  One text, so that a row of the rolling or the across call and a row of the listed windows cannot part.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_device.h"

namespace atsc {

namespace {

constexpr uint32_t HST_NONE = ~0u;  // the bin of a lane without a sample

// the edges, from global memory into LDS (every thread of the workgroup; the caller synchronises)
__device__ __forceinline__ void load_edges(double *s_edge, const double *__restrict__ edges, uint32_t n_edges)
{
    for (uint32_t i = threadIdx.x; i < n_edges; i += blockDim.x) s_edge[i] = edges[i];
}

// The bin of one sample.  k counts the edges at or below v (RIGHT: below v): binary lifting over the ascending edges
// with `steps` = ceil(log2(n_edges + 1)) trips whatever the sample, every trip one LDS read and two selects.
template <int CLOSED>
__device__ __forceinline__ uint32_t bin_of(double v, const double *s_edge, uint32_t n_edges, uint32_t steps)
{
    uint32_t k = 0;  // (every comparison with NaN is false: k stays 0 and is replaced below)
    for (uint32_t h = 1u << (steps - 1u); h; h >>= 1) {
        const uint32_t p = k + h, at = p <= n_edges ? p : n_edges;
        const double e = s_edge[at - 1u];
        const bool below = CLOSED == ATSC_HIST_RIGHT_CLOSED ? e < v : e <= v;
        k = (p <= n_edges && below) ? p : k;
    }
    return __builtin_isnan(v) ? n_edges + 1u : k;
}

// Adds one for every lane's bin (HST_NONE: nothing) to cnt[]: a run of neighbouring lanes with the same bin adds once,
// from its first lane, the length of the run.  Every lane of the wavefront takes part.
__device__ __forceinline__ void count_bins(uint32_t *cnt, uint32_t bin, uint32_t lane)
{
    const uint32_t prev = __shfl_up(bin, 1, 64);
    const bool head = lane == 0 || prev != bin;
    const uint64_t heads = __ballot(head);
    // the next run's first lane: the lowest head above this lane, 64 when there is none
    const uint64_t above = lane == 63u ? 0ull : heads >> (lane + 1u);
    const uint32_t run = above ? (uint32_t)__ffsll((unsigned long long)above) : 64u - lane;
    if (head && bin != HST_NONE) atomicAdd(&cnt[bin], run);
}

// orders this wavefront's LDS accesses in front of the call against those behind it, whichever lanes made them
__device__ __forceinline__ void rh_row_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace

// steps of bin_of: ceil(log2(n_edges + 1)), at least 1
static inline uint32_t search_steps(uint32_t n_edges)
{
    uint32_t s = 1;
    while ((1u << s) < n_edges + 1u) ++s;
    return s;
}

}  // namespace atsc
