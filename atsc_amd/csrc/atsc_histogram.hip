// atsc_histogram.hip -- gfx950 kernels of the windowed histograms (atsc_histogram_windows_dev): per window, the counts
// of its decoded samples over value bins, from decoded samples in the call's scratch.
//
// The contract (include/atsc_hip.h, DESIGN.md "Windowed histograms"): a row of n_edges + 2 u64 counters per window;
// a non-NaN sample v goes to bin k = the number of edges <= v (left closed) or < v (right closed), compared as values;
// NaN samples are counted in the row's last counter.  Counts are integers: no order of addition to keep.
//   short  (task of at most HST_SHORT_MAX samples)  one wavefront per task, a counter row of its own in LDS;
//                                                   workgroups walk the task list in strides, so that the edges
//                                                   are loaded once per workgroup and not once per window
//   chunk  (task of at most HST_CHUNK samples)      one workgroup per task, one counter row in LDS
// Both bin with the same branch-free search of fixed length over the edges in LDS and count with LDS integer atomics;
// lanes of a wavefront that follow each other with the same bin add once, with the length of their run (a Constant or
// RLE frame puts a whole wavefront into one bin).  A task that owns its window's row (HST_OWN) stores the row whole;
// the others add their non-zero counters to a row the host call has cleared.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_device.h"
#include "atsc_hist_bins.h"

namespace atsc {

namespace {

// a task's counters into its window's row: stored whole when the task owns the row, else the non-zero ones added
__device__ __forceinline__ void flush_row(const uint32_t *cnt, uint32_t rows, bool own, uint64_t *__restrict__ row,
                                          uint32_t first, uint32_t stride)
{
    for (uint32_t i = first; i < rows; i += stride) {
        const uint32_t c = cnt[i];
        if (own) row[i] = c;
        else if (c) atomicAdd((unsigned long long *)&row[i], (unsigned long long)c);
    }
}

}  // namespace

// One wavefront per task of at most HST_SHORT_MAX samples; workgroup b takes tasks 4 b + w, 4 (b + gridDim.x) + w, ...
// LDS: the edges, then one counter row per wavefront.
template <int CLOSED>
__global__ __launch_bounds__(256) void k_hst_short(const DevHistTask *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, const double *__restrict__ edges,
                                                   uint32_t n_edges, uint32_t steps, uint64_t *__restrict__ out)
{
    extern __shared__ double s_mem[];
    double *s_edge = s_mem;
    const uint32_t rows = n_edges + 2u, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t *cnt = (uint32_t *)(s_mem + n_edges) + w * rows;
    load_edges(s_edge, edges, n_edges);
    for (uint32_t base = blockIdx.x * 4u; base < n; base += gridDim.x * 4u) {
        for (uint32_t i = lane; i < rows; i += 64u) cnt[i] = 0;
        __syncthreads();  // the edges (first trip) and the cleared rows
        const uint32_t i = base + w;
        DevHistTask t{0, 0, 0};
        if (i < n) t = tasks[i];
        const uint32_t len = t.len & ~HST_OWN;
        const double *x = scratch + t.src;
        for (uint32_t o = 0; o < len; o += 64u) {
            const uint32_t e = o + lane;
            const uint32_t bin = e < len ? bin_of<CLOSED>(x[e], s_edge, n_edges, steps) : HST_NONE;
            count_bins(cnt, bin, lane);
        }
        __syncthreads();
        if (i < n) flush_row(cnt, rows, (t.len & HST_OWN) != 0, out + (uint64_t)t.win * rows, lane, 64u);
        __syncthreads();
    }
}

// One workgroup per task of at most HST_CHUNK samples.  LDS: the edges, then one counter row.
template <int CLOSED>
__global__ __launch_bounds__(256) void k_hst_chunk(const DevHistTask *__restrict__ tasks,
                                                   const double *__restrict__ scratch, const double *__restrict__ edges,
                                                   uint32_t n_edges, uint32_t steps, uint64_t *__restrict__ out)
{
    extern __shared__ double s_mem[];
    double *s_edge = s_mem;
    const uint32_t rows = n_edges + 2u, tid = threadIdx.x, lane = tid & 63u;
    uint32_t *cnt = (uint32_t *)(s_mem + n_edges);
    const DevHistTask t = tasks[blockIdx.x];
    const uint32_t len = t.len & ~HST_OWN;
    load_edges(s_edge, edges, n_edges);
    for (uint32_t i = tid; i < rows; i += 256u) cnt[i] = 0;
    __syncthreads();
    const double *x = scratch + t.src;
    for (uint32_t base = 0; base < len; base += 1024u) {
        double d[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = base + 256u * u + tid;
            d[u] = i < len ? x[i] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t i = base + 256u * u + tid;
            const uint32_t bin = i < len ? bin_of<CLOSED>(d[u], s_edge, n_edges, steps) : HST_NONE;
            count_bins(cnt, bin, lane);
        }
    }
    __syncthreads();
    flush_row(cnt, rows, (t.len & HST_OWN) != 0, out + (uint64_t)t.win * rows, tid, 256u);
}

hipError_t launch_hst_short(const DevHistTask *tasks, uint32_t n, const double *scratch, const double *edges,
                            uint32_t n_edges, int closed, uint64_t *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t want = (n + 3u) / 4u, grid = want < HST_SHORT_GRID ? want : HST_SHORT_GRID;
    const size_t lds = (size_t)n_edges * sizeof(double) + 4u * (size_t)(n_edges + 2u) * sizeof(uint32_t);
    if (closed == ATSC_HIST_RIGHT_CLOSED)
        hipLaunchKernelGGL(k_hst_short<ATSC_HIST_RIGHT_CLOSED>, dim3(grid), dim3(256), lds, s, tasks, n, scratch, edges,
                           n_edges, search_steps(n_edges), out);
    else
        hipLaunchKernelGGL(k_hst_short<ATSC_HIST_LEFT_CLOSED>, dim3(grid), dim3(256), lds, s, tasks, n, scratch, edges,
                           n_edges, search_steps(n_edges), out);
    return hipGetLastError();
}

hipError_t launch_hst_chunk(const DevHistTask *tasks, uint32_t n, const double *scratch, const double *edges,
                            uint32_t n_edges, int closed, uint64_t *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const size_t lds = (size_t)n_edges * sizeof(double) + (size_t)(n_edges + 2u) * sizeof(uint32_t);
    if (closed == ATSC_HIST_RIGHT_CLOSED)
        hipLaunchKernelGGL(k_hst_chunk<ATSC_HIST_RIGHT_CLOSED>, dim3(n), dim3(256), lds, s, tasks, scratch, edges, n_edges,
                           search_steps(n_edges), out);
    else
        hipLaunchKernelGGL(k_hst_chunk<ATSC_HIST_LEFT_CLOSED>, dim3(n), dim3(256), lds, s, tasks, scratch, edges, n_edges,
                           search_steps(n_edges), out);
    return hipGetLastError();
}

}  // namespace atsc
