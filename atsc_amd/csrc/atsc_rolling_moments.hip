// atsc_rolling_moments.hip -- gfx950 kernels of the windowed rolling moments (atsc_rolling_moments_windows_dev): the
// moments' record (atsc_window_moments) of the window [lo, lo + w) at every position of a range, from decoded samples in
// the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed rolling moments").  The node, its leaf and Merge are the
// windowed moments' (atsc_moment_node.h, node_merge of atsc_moment_rule.h): the leaf of stream index j is
// (1, x[j], 0, (double)j, 0, 0), a NaN slot the empty node.  N(a, 0) = leaf(a) and N(a, l) = Merge(N(a, l - 1),
// N(a + 2^(l-1), l - 1)) for a a multiple of 2^l in the stream index; a window's node is the left-to-right fold of N over
// its canonical chunks.  A leaf's position is its stream index, so N depends on no window, and one pyramid of chunk nodes
// per piece of the scratch serves every position in it, as the rolling's does (atsc_rolling.hip); the three kernels are
// that file's:
//   pyramid    one workgroup per ROLL_TILE = 2048 aligned samples, eight consecutive ones a thread: the levels 1 .. 3 in
//              registers, 4 .. 9 across the wavefront by shuffles, 10 and 11 through LDS; the levels from
//              ROLL_MOMENTS_LOW = 3 up to floor(log2 w) are stored;
//   upper      one wavefront per 64 aligned chunks of level 11 (and of level 17): the six levels above by shuffles;
//   positions  one wavefront per task, a lane per position: the lane walks its window's chunks left to right, a chunk
//              below ROLL_MOMENTS_LOW formed from the samples by the same tree, the others read from the pyramid.
// A partial is the node's five doubles and its count in a 64-bit word: 48 bytes (atsc_rolling_node.h, which the rolling
// pair moments share: atsc_rolling_pair.hip; that call runs this file's upper kernel over its own pyramid).  No atomics: every partial and every
// record has one writer, and a chunk's node is the same bits wherever it is formed.
//
// The divide: Merge divides by the joint count.  Two nodes of the same non-zero count -- every merge of a NaN-free chunk
// -- go through node_merge<true>, which gives the divide's bits without dividing; the test is the merge's own, lane by
// lane, so the bits do not depend on what the other lanes hold.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_rolling_node.h"

namespace atsc {

namespace {

// the record as the position kernel stores it, at the 8-byte alignment the result has
struct alignas(8) RmRec {
    uint64_t count;
    double mean, m2, t_mean, t_m2, c_tx;
};
static_assert(sizeof(RmRec) == sizeof(atsc_window_moments), "the record's layout");

// the leaf of the sample v at stream index j (below 2^53: exact in f64)
DEVI Node rm_leaf(double v, uint64_t j) { return node_leaf(v, (double)j, !__builtin_isnan(v)); }

}  // namespace

// One workgroup per tile of ROLL_TILE slots of the piece: the nodes of its chunks of the levels ROLL_MOMENTS_LOW ..
// min(lmax, 11) into the pyramid.  Slots that no range covers hold whatever the scratch held: their chunks are never read.
__global__ __launch_bounds__(256) void k_rmo_pyramid(const double *__restrict__ scratch, RmPart *__restrict__ pyr,
                                                     const DevRollPiece *__restrict__ pc, uint32_t lmax)
{
    __shared__ RmPart s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, t = blockIdx.x;
    const uint64_t slot = (uint64_t)t * ROLL_TILE + 8u * tid;
    const double2 *x = (const double2 *)(scratch + slot);
    const uint64_t j0 = pc->a0 + slot;  // the stream index of the thread's first slot
    Node p[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const double2 d = x[k];
        p[k] = rm_merge(rm_leaf(d.x, j0 + 2u * k), rm_leaf(d.y, j0 + 2u * k + 1u));
    }
    Node a = rm_merge(rm_merge(p[0], p[1]), rm_merge(p[2], p[3]));
    rm_store(pyr + pc->off[3] + 256ull * t + tid, a);
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {  // level 4 + k: lane l takes lane l + 2^k's
        const uint32_t level = 4u + k;
        if (level > lmax) return;
        a = rm_merge(a, shfl_down_part(a, 1u << k));
        if ((lane & ((2u << k) - 1u)) == 0) rm_store(pyr + pc->off[level] + (((uint64_t)t * ROLL_TILE) >> level) + (tid >> (k + 1)), a);
    }
    if (lmax < 10) return;
    if (lane == 0) rm_store(s_wave + (tid >> 6), a);
    __syncthreads();
    if (tid == 0) {
        const Node l = rm_merge(rm_load(s_wave + 0), rm_load(s_wave + 1)), r = rm_merge(rm_load(s_wave + 2), rm_load(s_wave + 3));
        rm_store(pyr + pc->off[10] + 2ull * t, l);
        rm_store(pyr + pc->off[10] + 2ull * t + 1, r);
        if (lmax >= 11) rm_store(pyr + pc->off[11] + t, rm_merge(l, r));
    }
}

// One wavefront per 64 chunks of level src at a multiple of 64 in the stream's chunk index: the chunks of the levels
// src + 1 .. min(src + 6, lmax) above them.  A chunk outside the piece is the empty node; what is formed from it sticks
// out of the piece as well, and is stored (where it has a place) but never read.
__global__ __launch_bounds__(256) void k_rmo_upper(RmPart *__restrict__ pyr, const DevRollPiece *__restrict__ pc, uint32_t n,
                                                   uint32_t src, uint32_t lmax)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const uint64_t a0 = pc->a0, last = pc->a1 - 1;
    const uint64_t c = (((a0 >> src) >> 6) + i) * 64u + lane;
    Node a = rm_none();
    if (c >= (a0 >> src) && c <= (last >> src)) a = rm_load(pyr + pc->off[src] + (c - (a0 >> src)));
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t level = src + k + 1u;
        if (level > lmax) return;
        a = rm_merge(a, shfl_down_part(a, 1u << k));
        const uint64_t j = c >> (k + 1);
        if ((lane & ((2u << k) - 1u)) == 0 && j >= (a0 >> level) && j <= (last >> level))
            rm_store(pyr + pc->off[level] + (j - (a0 >> level)), a);
    }
}

// One wavefront per DevRollTask, a lane per position: the window's canonical chunks left to right, their nodes merged
// in that order from the empty node on (Merge(empty, c) is c, bit for bit), into the position's record.
__global__ __launch_bounds__(256) void k_rmo_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                       const double *__restrict__ scratch, const RmPart *__restrict__ pyr,
                                                       const DevRollPiece *__restrict__ pc, uint64_t w, uint64_t stride,
                                                       RmRec *__restrict__ out)
{
    __shared__ uint64_t s_off[ROLL_MAX_LEVEL + 1];  // a lane's level is its own: the offsets are read by lane
    if (threadIdx.x <= ROLL_MAX_LEVEL) s_off[threadIdx.x] = pc->off[threadIdx.x];
    __syncthreads();
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevRollTask t = tasks[i];
    const uint64_t a0 = pc->a0;
    for (uint32_t p = lane; p < t.n; p += 64u) {
        const uint64_t lo = t.lo + (uint64_t)p * stride, hi = lo + w;
        Node acc = rm_none();
        for (uint64_t pos = lo; pos < hi;) {
            const uint32_t up = pos ? (uint32_t)__builtin_ctzll(pos) : 63u, fit = 63u - (uint32_t)__builtin_clzll(hi - pos);
            const uint32_t l = up < fit ? up : fit;
            const double *x = scratch + (pos - a0);
            Node c;
            if (l >= ROLL_MOMENTS_LOW) {
                c = rm_load(pyr + s_off[l] + ((pos >> l) - (a0 >> l)));
            } else if (l == 0) {
                c = rm_leaf(x[0], pos);
            } else if (l == 1) {
                c = rm_merge(rm_leaf(x[0], pos), rm_leaf(x[1], pos + 1));
            } else {
                c = rm_merge(rm_merge(rm_leaf(x[0], pos), rm_leaf(x[1], pos + 1)),
                             rm_merge(rm_leaf(x[2], pos + 2), rm_leaf(x[3], pos + 3)));
            }
            acc = rm_merge(acc, c);
            pos += 1ull << l;
        }
        const double nan = __builtin_nan("");
        const bool some = acc.n != 0;
        out[t.rec + p] = RmRec{acc.n, some ? acc.mx : nan, some ? acc.m2x : nan, some ? acc.mt - (double)lo : nan,
                               some ? acc.m2t : nan, some ? acc.c : nan};
    }
}

hipError_t launch_rmo_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax,
                              hipStream_t s)
{
    if (n_tiles == 0 || lmax < ROLL_MOMENTS_LOW) return hipSuccess;
    hipLaunchKernelGGL(k_rmo_pyramid, dim3(n_tiles), dim3(256), 0, s, scratch, (RmPart *)pyr, pc, lmax);
    return hipGetLastError();
}

hipError_t launch_rmo_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax, hipStream_t s)
{
    return launch_wave_tasks(k_rmo_upper, n, s, (RmPart *)pyr, pc, n, src, lmax);
}

hipError_t launch_rmo_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const void *pyr,
                                const DevRollPiece *pc, uint64_t w, uint64_t stride, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_rmo_positions, n, s, tasks, n, scratch, (const RmPart *)pyr, pc, w, stride, (RmRec *)out);
}

}  // namespace atsc
