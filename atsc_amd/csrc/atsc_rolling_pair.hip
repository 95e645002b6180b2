// atsc_rolling_pair.hip -- gfx950 kernels of the windowed rolling pair moments (atsc_rolling_pair_windows_dev): the
// pair moments' record (atsc_window_pair) of the window [lo, lo + w) at every position of a range, from the decoded
// samples of two streams in the call's two scratch regions.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed rolling pair moments").  The node, its leaf and Merge are the
// windowed pair moments' (atsc_moment_node.h, node_merge of atsc_moment_rule.h): the leaf of stream index j is
// (1, x[j], 0, y[j], 0, 0), the empty node where x[j] or y[j] is NaN.  The order is the rolling moments'
// (atsc_rolling_moments.hip): N(a, 0) = leaf(a), N(a, l) = Merge(N(a, l - 1), N(a + 2^(l-1), l - 1)) for a a multiple of
// 2^l in the stream index, and a window's node is the left-to-right fold of N over its canonical chunks.  The partial
// and its helpers are atsc_rolling_node.h's, which that file shares; the kernels have its shapes:
//   pyramid    one workgroup per ROLL_TILE = 2048 aligned slots, eight consecutive ones a thread, the same slots of the
//              two regions: the levels 1 .. 3 in registers, 4 .. 9 across the wavefront by shuffles, 10 and 11 through
//              LDS; the levels from ROLL_MOMENTS_LOW = 3 up to floor(log2 w) are stored;
//   upper      the levels above 11 merge partials only: the host runs k_rmo_upper (launch_rmo_upper) over this pyramid;
//   positions  one wavefront per task, a lane per position: the lane walks its window's chunks left to right, a chunk
//              below ROLL_MOMENTS_LOW formed from both regions' samples by the same tree, the others read from the
//              pyramid.  No field of the record is counted from the window's begin.
// No atomics: every partial and every record has one writer, and a chunk's node is the same bits wherever it is formed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_rolling_node.h"

namespace atsc {

namespace {

// the record as the position kernel stores it, at the 8-byte alignment the result has
struct alignas(8) RpRec {
    uint64_t count;
    double mean_x, m2_x, mean_y, m2_y, c_xy;
};
static_assert(sizeof(RpRec) == sizeof(atsc_window_pair), "the record's layout");

// the leaf of the samples x and y of one stream index
DEVI Node rp_leaf(double x, double y) { return node_leaf(x, y, !__builtin_isnan(x) && !__builtin_isnan(y)); }

}  // namespace

// One workgroup per tile of ROLL_TILE slots of the piece: the nodes of its chunks of the levels ROLL_MOMENTS_LOW ..
// min(lmax, 11) into the pyramid.  Slots that no range covers hold whatever the regions held: their chunks are never read.
__global__ __launch_bounds__(256) void k_rpa_pyramid(const double *__restrict__ sx, const double *__restrict__ sy,
                                                     RmPart *__restrict__ pyr, const DevRollPiece *__restrict__ pc,
                                                     uint32_t lmax)
{
    __shared__ RmPart s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, t = blockIdx.x;
    const uint64_t slot = (uint64_t)t * ROLL_TILE + 8u * tid;
    const double2 *x = (const double2 *)(sx + slot), *y = (const double2 *)(sy + slot);
    Node p[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const double2 dx = x[k], dy = y[k];
        p[k] = rm_merge(rp_leaf(dx.x, dy.x), rp_leaf(dx.y, dy.y));
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

// One wavefront per DevRollTask, a lane per position: the window's canonical chunks left to right, their nodes merged
// in that order from the empty node on (Merge(empty, c) is c, bit for bit), into the position's record.
__global__ __launch_bounds__(256) void k_rpa_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                       const double *__restrict__ sx, const double *__restrict__ sy,
                                                       const RmPart *__restrict__ pyr, const DevRollPiece *__restrict__ pc,
                                                       uint64_t w, uint64_t stride, RpRec *__restrict__ out)
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
            const double *x = sx + (pos - a0), *y = sy + (pos - a0);
            Node c;
            if (l >= ROLL_MOMENTS_LOW) {
                c = rm_load(pyr + s_off[l] + ((pos >> l) - (a0 >> l)));
            } else if (l == 0) {
                c = rp_leaf(x[0], y[0]);
            } else if (l == 1) {
                c = rm_merge(rp_leaf(x[0], y[0]), rp_leaf(x[1], y[1]));
            } else {
                c = rm_merge(rm_merge(rp_leaf(x[0], y[0]), rp_leaf(x[1], y[1])), rm_merge(rp_leaf(x[2], y[2]), rp_leaf(x[3], y[3])));
            }
            acc = rm_merge(acc, c);
            pos += 1ull << l;
        }
        const double nan = __builtin_nan("");
        const bool some = acc.n != 0;
        out[t.rec + p] = RpRec{acc.n, some ? acc.mx : nan, some ? acc.m2x : nan, some ? acc.mt : nan, some ? acc.m2t : nan,
                               some ? acc.c : nan};
    }
}

hipError_t launch_rpa_pyramid(const double *sx, const double *sy, uint32_t n_tiles, void *pyr, const DevRollPiece *pc,
                              uint32_t lmax, hipStream_t s)
{
    if (n_tiles == 0 || lmax < ROLL_MOMENTS_LOW) return hipSuccess;
    hipLaunchKernelGGL(k_rpa_pyramid, dim3(n_tiles), dim3(256), 0, s, sx, sy, (RmPart *)pyr, pc, lmax);
    return hipGetLastError();
}

hipError_t launch_rpa_positions(const DevRollTask *tasks, uint32_t n, const double *sx, const double *sy, const void *pyr,
                                const DevRollPiece *pc, uint64_t w, uint64_t stride, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_rpa_positions, n, s, tasks, n, sx, sy, (const RmPart *)pyr, pc, w, stride, (RpRec *)out);
}

}  // namespace atsc
