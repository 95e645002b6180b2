// atsc_pair_matrix.hip -- gfx950 kernels of the windowed pair matrix (atsc_pair_matrix_windows_dev): the pair moments
// (atsc_pair.hip) of every pair (i, j), i <= j, of N streams over the same sample windows, reduced from the decoded
// samples of all N in the call's N scratch regions.
//
// The leaf, the pairwise-complete NaN rule, the merge and the tree are the pair's (atsc_moment_node.h; the contract:
// include/atsc_hip.h, DESIGN.md "Windowed pair matrix"): pair (i, j)'s node of a tile is the node k_pair_tiles gives
// with region i as x and region j as y, bit for bit.  The partials lie pair-major: the node of pair p and partial d at
// part[p * part_n + d], so that one pair's partials are the table comb_reduce walks.  No atomics: every node has one
// writer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_moment_node.h"

namespace atsc {

// The partners a wavefront walks for its row: row i's partners j = i .. N - 1 go in chunks of PMX_CHUNK.  64, the most
// streams of a call, gives a wavefront the whole row: the row's 2048 slots are loaded once for all its partners, which
// measured 7 % below chunks of 8 at 64 streams and the same at 8 (profiles/pair_matrix_timing.txt; a build with
// -DPMX_CHUNK=8u is the other side of that table).
#ifndef PMX_CHUNK
#define PMX_CHUNK 64u
#endif

// p of pair (i, j), i <= j < n: atsc_pair_matrix_index
DEVI uint32_t pmx_index(uint32_t n, uint32_t i, uint32_t j) { return i * (2u * n - i + 1u) / 2u + (j - i); }

// the (row, partner chunk) units of n streams: a row of m partners has ceil(m / PMX_CHUNK) of them
static inline uint32_t pmx_units(uint32_t n)
{
    uint32_t u = 0;
    for (uint32_t i = 0; i < n; ++i) u += (n - i + PMX_CHUNK - 1u) / PMX_CHUNK;
    return u;
}

// One wavefront per (DevPosTile, row i, chunk of partners): blockIdx.x is the tile task, the block's four wavefronts
// take four consecutive units of it.  Stream k's tile lies at scratch + reg[k] + src (the same slots of every region;
// t0 is not read).  The wavefront loads the row's 2048 slots once (tile_slot's mapping, eight masked 16-byte loads per
// virtual lane: 32 doubles a lane) with a mask of the slots that lie in [lo, hi) and hold no NaN, then for each partner
// j loads one virtual lane's eight leaves of region j at a time and reduces them as k_pair_tiles does, the divide-free
// merges behind the same wave-uniform tests.  Lane 0 writes the node of pair (i, j) to part[p * part_n + dst].
__global__ __launch_bounds__(256) void k_pmx_tiles(const DevPosTile *__restrict__ tasks, uint32_t units,
                                                   const double *__restrict__ scratch, const uint64_t *__restrict__ reg,
                                                   uint32_t n_streams, DevMomPart *__restrict__ part, uint64_t part_n)
{
    const uint32_t lane = wave_lane();
    uint32_t u = __builtin_amdgcn_readfirstlane(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (u >= units) return;
    uint32_t i = 0;
    for (;;) {
        const uint32_t nc = (n_streams - i + PMX_CHUNK - 1u) / PMX_CHUNK;
        if (u < nc) break;
        u -= nc;
        ++i;
    }
    const uint32_t j0 = i + u * PMX_CHUNK, j1 = min(n_streams, j0 + PMX_CHUNK);
    const DevPosTile t = tasks[blockIdx.x];
    const double *x = scratch + reg[i] + t.src;
    double2 dx[4][4];
    uint32_t okx = 0;  // bit 8 k + 2 q + e: slot tile_slot(lane + 64 k, q) + e lies in the window and x is not NaN there
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t s = tile_slot(lane + 64u * k, q);
            dx[k][q] = tile_load(x, s, t.lo, t.hi, 0.0);
            if (tile_in(s, t.lo, t.hi) && !__builtin_isnan(dx[k][q].x)) okx |= 1u << (8 * k + 2 * q);
            if (tile_in(s + 1u, t.lo, t.hi) && !__builtin_isnan(dx[k][q].y)) okx |= 2u << (8 * k + 2 * q);
        }
    for (uint32_t j = j0; j < j1; ++j) {
        const double *y = scratch + reg[j] + t.src;
        bool full = true;
        Node s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            double2 dy[4];
            bool ok[8];
            bool all = true;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                dy[q] = tile_load(y, tile_slot(lane + 64u * k, q), t.lo, t.hi, 0.0);
                ok[2 * q] = ((okx >> (8 * k + 2 * q)) & 1u) && !__builtin_isnan(dy[q].x);
                ok[2 * q + 1] = ((okx >> (8 * k + 2 * q + 1)) & 1u) && !__builtin_isnan(dy[q].y);
                all = all && ok[2 * q] && ok[2 * q + 1];
            }
            auto leaf = [&](int q, int e) {
                return e ? node_leaf(dx[k][q].y, dy[q].y, ok[2 * q + 1]) : node_leaf(dx[k][q].x, dy[q].x, ok[2 * q]);
            };
            if (__all(all)) s[k] = lane_node<true>(leaf);
            else s[k] = lane_node<false>(leaf);
            full = full && all;
        }
        Node a;
        if (__all(full)) a = tile_node<true>(s);
        else a = tile_node<false>(s);
        if (lane == 0) part[pmx_index(n_streams, i, j) * part_n + t.dst] = DevMomPart{a.mx, a.m2x, a.mt, a.m2t, a.c, a.n};
    }
}

// One wavefront per (DevAggComb, pair): blockIdx.y is the pair p, whose partials are the table at part + p * part_n.
// The group through comb_reduce as in k_pair_combine; the final pass writes the six fields of record (window dst, p).
__global__ __launch_bounds__(256) void k_pmx_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                     DevMomPart *__restrict__ part, uint64_t part_n, uint32_t n_pairs,
                                                     uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task(), p = blockIdx.y;
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const DevMomPart a = comb_reduce(c, lane, part + (uint64_t)p * part_n, DevMomPart{0.0, 0.0, 0.0, 0.0, 0.0, 0},
                                     node_merge<false, DevMomPart>);
    if (!c.final_) return;
    const uint64_t cnt = __shfl(a.n, 0, 64);
    const double mx = __shfl(a.mx, 0, 64), m2x = __shfl(a.m2x, 0, 64), my = __shfl(a.mt, 0, 64),
                 m2y = __shfl(a.m2t, 0, 64), cv = __shfl(a.c, 0, 64);
    if (lane < 6) {
        double v;
        switch (lane) {
        case 1: v = mx; break;
        case 2: v = m2x; break;
        case 3: v = my; break;
        case 4: v = m2y; break;
        default: v = cv; break;
        }
        out[6ull * (c.dst * n_pairs + p) + lane] = lane == 0 ? cnt : (uint64_t)__double_as_longlong(cnt ? v : __builtin_nan(""));
    }
}

// the grids are made here from (tile tasks) x (units) and (combine groups) x (pairs): the host lists no task per pair
hipError_t launch_pmx_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, const uint64_t *reg,
                            uint32_t n_streams, DevMomPart *part, uint64_t part_n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t units = pmx_units(n_streams);
    hipLaunchKernelGGL(k_pmx_tiles, dim3(n, (units + 3) / 4), dim3(256), 0, s, tasks, units, scratch, reg, n_streams, part,
                       part_n);
    return hipGetLastError();
}

hipError_t launch_pmx_combine(const DevAggComb *tasks, uint32_t n, DevMomPart *part, uint64_t part_n, uint32_t n_streams,
                              void *out, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const uint32_t n_pairs = n_streams * (n_streams + 1) / 2;
    hipLaunchKernelGGL(k_pmx_combine, dim3((n + 3) / 4, n_pairs), dim3(256), 0, s, tasks, n, part, part_n, n_pairs,
                       (uint64_t *)out);
    return hipGetLastError();
}

}  // namespace atsc
