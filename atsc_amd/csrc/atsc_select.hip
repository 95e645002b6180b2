// atsc_select.hip -- gfx950 kernels of the windowed select (atsc_select_windows_dev): per window the samples that meet
// a condition (x OP limit) and where they are, compacted in order from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed select").  A sample is selected iff it is not NaN and x OP
// limit holds: the three ordered comparisons of k_run_tiles (atsc_runs.hip), each false on NaN.  The size of the result
// depends on the data, so the work goes in three steps over the call's tasks (DevSelTask: at most SEL_TASK consecutive
// samples of one window in one piece of the scratch, `slot` its place in (window, position) order):
//   count   one wavefront per task: the selected samples of the task into cnt[slot];
//   scan    an exclusive 64-bit scan over cnt[] in slot order, SEL_SCAN_BLOCK values per workgroup and level by level
//           above that; the windows' offsets are read off it;
//   write   one wavefront per task over its samples again, in stream order: entry pre[slot] + (rank in the task).
// No atomics: every counter and every entry has exactly one writer, whose place the scan fixes, so the order and the
// bytes do not depend on how the wavefronts were scheduled or on which piece a task ran in.
//
// Both task kernels read 128 slots a step, 16 bytes a lane, from the even slot at or in front of the task's first
// sample (the scratch is 16-byte aligned and one slot longer than the samples it holds): lane l holds slots 2 l and
// 2 l + 1 of the step, a slot outside the task (the head of a task that begins at an odd slot, the tail) is never
// selected, and two ballots give the step's hits as wave-uniform masks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// x OP limit as the three ordered comparisons, each false on NaN
struct SelCond {
    bool gt, lt, eq;
    double limit;
};
DEVI SelCond sel_cond(int op, double limit)
{
    return SelCond{op == ATSC_RUNS_GT || op == ATSC_RUNS_GE || op == ATSC_RUNS_NE,
                   op == ATSC_RUNS_LT || op == ATSC_RUNS_LE || op == ATSC_RUNS_NE,
                   op == ATSC_RUNS_GE || op == ATSC_RUNS_LE || op == ATSC_RUNS_EQ, limit};
}
DEVI bool sel_hit(const SelCond &c, double x) { return (c.gt && x > c.limit) || (c.lt && x < c.limit) || (c.eq && x == c.limit); }

// A task as its wavefront sees it: x[lo, hi) are its samples, x 16-byte aligned, lo 0 or 1; every field wave-uniform.
struct SelSpan {
    const double *x;
    uint32_t lo, hi;
};
DEVI uint64_t uniform64(uint64_t v)
{
    return ((uint64_t)__builtin_amdgcn_readfirstlane((uint32_t)(v >> 32)) << 32) | __builtin_amdgcn_readfirstlane((uint32_t)v);
}
DEVI SelSpan sel_span(const DevSelTask &t, const double *scratch)
{
    const uint64_t src = uniform64(t.src);
    const uint32_t lo = (uint32_t)(src & 1u);
    return SelSpan{scratch + (src - lo), lo, lo + (uint32_t)__builtin_amdgcn_readfirstlane(t.len)};
}

// The slots j, j + 1 of a task (j even) and whether each is selected; the pair is loaded where either lies in the task.
struct SelPair {
    double2 d;
    bool in0, in1;
};
DEVI SelPair sel_pair(const SelSpan &p, uint32_t j, const SelCond &c)
{
    SelPair s;
    s.d = make_double2(0.0, 0.0);
    if (j < p.hi && j + 2u > p.lo) s.d = *(const double2 *)(p.x + j);  // 16-byte load
    s.in0 = j >= p.lo && j < p.hi && sel_hit(c, s.d.x);
    s.in1 = j + 1u >= p.lo && j + 1u < p.hi && sel_hit(c, s.d.y);
    return s;
}

// the set bits of a ballot below this lane
DEVI uint32_t bits_below(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// an entry as the write step stores it: 16 bytes at once, at the 8-byte alignment the block has
struct alignas(8) SelEntry {
    uint64_t bits, at;
};
static_assert(sizeof(SelEntry) == sizeof(atsc_selected), "the entry's layout");

}  // namespace

// One wavefront per task: the number of its selected samples into cnt[slot].
__global__ __launch_bounds__(256) void k_sel_count(const DevSelTask *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, int op, double limit,
                                                   uint64_t *__restrict__ cnt)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevSelTask t = tasks[i];
    const SelSpan p = sel_span(t, scratch);
    const SelCond c = sel_cond(op, limit);
    uint32_t hits = 0;
    for (uint32_t j0 = 0; j0 < p.hi; j0 += 128u) {
        const SelPair s = sel_pair(p, j0 + 2u * lane, c);
        hits += (uint32_t)__popcll(__ballot(s.in0)) + (uint32_t)__popcll(__ballot(s.in1));
    }
    if (lane == 0) cnt[t.slot] = hits;
}

// One workgroup per SEL_SCAN_BLOCK values, eight consecutive ones a thread: data[i], i < n_out, becomes the sum of the
// block's values in front of it (a value at or behind n_in counts as zero); the block's sum goes to sums[block] when
// there is more than one block.
__global__ __launch_bounds__(256) void k_sel_scan(uint64_t *__restrict__ data, uint64_t n_in, uint64_t n_out,
                                                  uint64_t *__restrict__ sums)
{
    __shared__ uint64_t s_wave[4];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint64_t first = (uint64_t)blockIdx.x * SEL_SCAN_BLOCK + 8ull * tid;
    uint64_t v[8], sum = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) v[k] = first + k < n_in ? data[first + k] : 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) {
        const uint64_t x = v[k];
        v[k] = sum;
        sum += x;
    }
    uint64_t inc = sum;  // the lanes' sums up to and including this lane's
#pragma unroll
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63u) s_wave[w] = inc;
    __syncthreads();
    uint64_t base = inc - sum, total = 0;
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
        if (u < w) base += s_wave[u];
        total += s_wave[u];
    }
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (first + k < n_out) data[first + k] = base + v[k];
    if (tid == 0 && sums) sums[blockIdx.x] = total;
}

// The level below a scanned level of block sums: every value of block b gets the sum of the blocks in front of b.
__global__ __launch_bounds__(256) void k_sel_scan_add(uint64_t *__restrict__ data, uint64_t n, const uint64_t *__restrict__ sums)
{
    const uint64_t add = sums[blockIdx.x], first = (uint64_t)blockIdx.x * SEL_SCAN_BLOCK + threadIdx.x;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k)
        if (first + 256u * k < n) data[first + 256u * k] += add;
}

// off[i] = pre[first[i]], i < n: a window's offset is the scanned count at its first task; an empty window's first task
// is the next window's, and first[n_windows] the end of the list, where the scan left the total.
__global__ __launch_bounds__(256) void k_sel_offsets(const uint64_t *__restrict__ pre, const uint32_t *__restrict__ first,
                                                     uint64_t n, uint64_t *__restrict__ off)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) off[i] = pre[first[i]];
}

// One wavefront per task, over its samples in stream order: the running base is wave-uniform, a lane's rank the hits of
// the step below it; entry r is stored iff r < cap.
__global__ __launch_bounds__(256) void k_sel_write(const DevSelTask *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, int op, double limit,
                                                   const uint64_t *__restrict__ pre, uint64_t cap,
                                                   SelEntry *__restrict__ e)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevSelTask t = tasks[i];
    const SelSpan p = sel_span(t, scratch);
    const SelCond c = sel_cond(op, limit);
    uint64_t base = uniform64(pre[t.slot]);
    const uint64_t at0 = uniform64(t.at) - p.lo;  // slot j is `at0 + j` samples behind the window's begin (modulo 2^64)
    for (uint32_t j0 = 0; j0 < p.hi && base < cap; j0 += 128u) {
        const uint32_t j = j0 + 2u * lane;
        const SelPair s = sel_pair(p, j, c);
        const uint64_t be = __ballot(s.in0), bo = __ballot(s.in1);
        const uint64_t r0 = base + bits_below(be) + bits_below(bo), r1 = r0 + (s.in0 ? 1u : 0u);
        if (s.in0 && r0 < cap) e[r0] = SelEntry{(uint64_t)__double_as_longlong(s.d.x), at0 + j};
        if (s.in1 && r1 < cap) e[r1] = SelEntry{(uint64_t)__double_as_longlong(s.d.y), at0 + j + 1u};
        base += (uint32_t)__popcll(be) + (uint32_t)__popcll(bo);
    }
}

hipError_t launch_sel_count(const DevSelTask *tasks, uint32_t n, const double *scratch, int op, double limit, uint64_t *cnt,
                            hipStream_t s)
{
    return launch_wave_tasks(k_sel_count, n, s, tasks, n, scratch, op, limit, cnt);
}

// The exclusive scan of cnt[0, n) in place, and the total into cnt[n].  sums: sel_scan_sums(n + 1) words for the levels
// above the first.
hipError_t launch_sel_scan(uint64_t *cnt, uint64_t n, uint64_t *sums, hipStream_t s)
{
    uint64_t *lv[8], m[8];
    int top = 0;
    lv[0] = cnt;
    m[0] = n + 1;
    for (;; ++top) {
        const uint64_t blocks = (m[top] + SEL_SCAN_BLOCK - 1) / SEL_SCAN_BLOCK;
        hipLaunchKernelGGL(k_sel_scan, dim3((uint32_t)blocks), dim3(256), 0, s, lv[top], top ? m[top] : n, m[top],
                           blocks > 1 ? sums : (uint64_t *)nullptr);
        if (blocks == 1) break;
        lv[top + 1] = sums;
        m[top + 1] = blocks;
        sums += blocks;
    }
    for (int l = top - 1; l >= 0; --l)
        hipLaunchKernelGGL(k_sel_scan_add, dim3((uint32_t)m[l + 1]), dim3(256), 0, s, lv[l], m[l], lv[l + 1]);
    return hipGetLastError();
}

hipError_t launch_sel_offsets(const uint64_t *pre, const uint32_t *first, uint64_t n, uint64_t *off, hipStream_t s)
{
    hipLaunchKernelGGL(k_sel_offsets, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, pre, first, n, off);
    return hipGetLastError();
}

hipError_t launch_sel_write(const DevSelTask *tasks, uint32_t n, const double *scratch, int op, double limit,
                            const uint64_t *pre, uint64_t cap, void *entries, hipStream_t s)
{
    return launch_wave_tasks(k_sel_write, n, s, tasks, n, scratch, op, limit, pre, cap, (SelEntry *)entries);
}

}  // namespace atsc
