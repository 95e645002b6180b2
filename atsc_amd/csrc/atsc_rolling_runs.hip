// atsc_rolling_runs.hip -- gfx950 kernels of the windowed rolling runs (atsc_rolling_runs_windows_dev): the runs' record
// (atsc_window_runs) of the window [lo, lo + w) at every position of a range, from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed rolling runs").  A sample is inside iff it is not NaN and
// x OP limit holds (atsc_runs.hip).  The leaf is a sample: its node is the runs' of one sample, its term fabs(x - limit)
// or -0.0.  The nine integers are an associative monoid under the runs' merge (atsc_runs.hip, run_merge), so any tree
// over a window's samples gives the same integers; excess is T(a, 0) = term(a), T(a, l) = T(a, l - 1) + T(a + 2^(l-1),
// l - 1) for a a multiple of 2^l in the stream index, folded left to right over the window's canonical chunks.  Neither
// depends on any window, so one pyramid of chunk partials per piece of the scratch serves every position in it, as the
// rolling's does (atsc_rolling.hip), and the three kernels are that file's:
//   pyramid    one workgroup per ROLL_TILE = 2048 aligned samples, eight consecutive ones a thread: the levels 1 .. 3 in
//              registers, 4 .. 9 across the wavefront by shuffles, 10 and 11 through LDS; the levels from ROLL_RUNS_LOW
//              = 3 up to floor(log2 w) are stored;
//   upper      one wavefront per 64 aligned chunks of level 11 (and of level 17): the six levels above by shuffles;
//   positions  one wavefront per task, a lane per position: the lane walks its window's chunks left to right, a chunk
//              below ROLL_RUNS_LOW formed from the samples by the same tree, the others read from the pyramid.
// The condition reaches the pyramid and the position kernels as kernel arguments; the upper kernel merges partials only.
// No atomics: every partial and every record has one writer, and a chunk's value is the same bits wherever it is formed.
//
// A chunk's length follows from its level and is not stored; its three positions count from its first sample.  A node
// without an inside sample holds 0 in first_at and last_at, one without a run 0 in longest_at: "none" is read off
// inside == 0 and runs == 0.  In the pyramid a partial is packed into 32 bytes (RrPacked); registers hold it unpacked.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// the node of a stretch of at most 2^20 samples, and the sum of its inside samples' terms
struct RrPart {
    uint32_t inside, runs, longest, head, tail, longest_at, first_at, last_at;
    double excess;
};

// a partial in the pyramid: a chunk of level l <= 20 holds at most 2^20 samples
//   a: inside (bits 0 .. 20), runs (21 .. 41), longest (42 .. 62)
//   b: head (0 .. 20), tail (21 .. 41), longest_at (42 .. 61)
//   c: first_at (0 .. 19), last_at (20 .. 39)
struct alignas(16) RrPacked {
    uint64_t a, b, c;
    double excess;
};
static_assert(sizeof(RrPacked) == ROLL_RUNS_PART, "a partial is 32 bytes");
static_assert(ROLL_MAX_LEVEL <= 20, "the packed fields hold a chunk of 2^20 samples");

constexpr uint64_t RR_M21 = (1ull << 21) - 1, RR_M20 = (1ull << 20) - 1;

// the record as the position kernel stores it, at the 8-byte alignment the result has
struct alignas(8) RrRec {
    uint64_t samples, inside, runs, longest, longest_at, first_at, last_at, head, tail;
    double excess;
};
static_assert(sizeof(RrRec) == sizeof(atsc_window_runs), "the record's layout");

// The call's condition, uniform over the launch: x OP limit from the three ordered comparisons, each false on NaN
// (k_run_tiles' form).
struct RrCond {
    bool gt, lt, eq;
    double limit;
};

DEVI RrCond rr_cond(int op, double limit)
{
    bool gt = false, lt = false, eq = false;
    switch (op) {
    case ATSC_RUNS_GT: gt = true; break;
    case ATSC_RUNS_GE: gt = eq = true; break;
    case ATSC_RUNS_LT: lt = true; break;
    case ATSC_RUNS_LE: lt = eq = true; break;
    case ATSC_RUNS_EQ: eq = true; break;
    default: gt = lt = true; break;  // ATSC_RUNS_NE (the host has checked op)
    }
    return RrCond{gt, lt, eq, limit};
}

// all outside, of any length
DEVI RrPart rr_none() { return RrPart{0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, -0.0}; }

DEVI RrPart rr_leaf(double v, const RrCond &c)
{
    const bool in = (c.gt && v > c.limit) || (c.lt && v < c.limit) || (c.eq && v == c.limit);
    const uint32_t i = in ? 1u : 0u;
    return RrPart{i, i, i, i, i, 0u, 0u, 0u, in ? __builtin_fabs(v - c.limit) : -0.0};
}

// a, of la samples, followed by b, of lb: the runs' merge rule (atsc_runs.hip, run_merge) with b's positions moved
// behind a.  The run across the seam starts tail(a) samples in front of b.  Strict comparisons: of equal runs the
// earliest stays, in any tree.  a may be the empty accumulator (la = 0).
DEVI RrPart rr_merge(const RrPart &a, uint32_t la, const RrPart &b, uint32_t lb)
{
    RrPart r;
    const bool join = a.tail != 0 && b.head != 0;
    r.inside = a.inside + b.inside;
    r.runs = a.runs + b.runs - (join ? 1u : 0u);
    r.head = a.head == la ? la + b.head : a.head;
    r.tail = b.tail == lb ? lb + a.tail : b.tail;
    r.first_at = a.inside ? a.first_at : b.inside ? la + b.first_at : 0u;
    r.last_at = b.inside ? la + b.last_at : a.last_at;
    uint32_t lg = a.longest, at = a.longest_at;
    const uint32_t jl = a.tail + b.head;
    if (join && jl > lg) { lg = jl; at = la - a.tail; }
    if (b.longest > lg) { lg = b.longest; at = la + b.longest_at; }
    r.longest = lg;
    r.longest_at = at;
    r.excess = a.excess + b.excess;
    return r;
}

DEVI RrPart rr_load(const RrPacked *p)
{
    const double2 u = ((const double2 *)p)[0], v = ((const double2 *)p)[1];  // two 16-byte loads
    const uint64_t a = (uint64_t)__double_as_longlong(u.x), b = (uint64_t)__double_as_longlong(u.y),
                   c = (uint64_t)__double_as_longlong(v.x);
    return RrPart{(uint32_t)(a & RR_M21), (uint32_t)((a >> 21) & RR_M21), (uint32_t)(a >> 42),
                  (uint32_t)(b & RR_M21), (uint32_t)((b >> 21) & RR_M21), (uint32_t)(b >> 42),
                  (uint32_t)(c & RR_M20), (uint32_t)(c >> 20), v.y};
}

DEVI void rr_store(RrPacked *p, const RrPart &r)
{
    const uint64_t a = (uint64_t)r.inside | ((uint64_t)r.runs << 21) | ((uint64_t)r.longest << 42);
    const uint64_t b = (uint64_t)r.head | ((uint64_t)r.tail << 21) | ((uint64_t)r.longest_at << 42);
    const uint64_t c = (uint64_t)r.first_at | ((uint64_t)r.last_at << 20);
    ((double2 *)p)[0] = make_double2(__longlong_as_double((long long)a), __longlong_as_double((long long)b));
    ((double2 *)p)[1] = make_double2(__longlong_as_double((long long)c), r.excess);
}

}  // namespace

// One workgroup per tile of ROLL_TILE slots of the piece: the partials of its chunks of the levels ROLL_RUNS_LOW ..
// min(lmax, 11) into the pyramid.  Slots that no range covers hold whatever the scratch held: their chunks are never read.
__global__ __launch_bounds__(256) void k_rru_pyramid(const double *__restrict__ scratch, RrPacked *__restrict__ pyr,
                                                     const DevRollPiece *__restrict__ pc, uint32_t lmax, int op, double limit)
{
    __shared__ RrPart s_wave[4];
    const RrCond cd = rr_cond(op, limit);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, t = blockIdx.x;
    const double2 *x = (const double2 *)(scratch + (uint64_t)t * ROLL_TILE + 8u * tid);
    RrPart p[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const double2 d = x[k];
        p[k] = rr_merge(rr_leaf(d.x, cd), 1u, rr_leaf(d.y, cd), 1u);
    }
    RrPart a = rr_merge(rr_merge(p[0], 2u, p[1], 2u), 4u, rr_merge(p[2], 2u, p[3], 2u), 4u);
    rr_store(pyr + pc->off[3] + 256ull * t + tid, a);
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {  // level 4 + k: lane l takes lane l + 2^k's
        const uint32_t level = 4u + k;
        if (level > lmax) return;
        a = rr_merge(a, 8u << k, shfl_down_part(a, 1u << k), 8u << k);
        if ((lane & ((2u << k) - 1u)) == 0) rr_store(pyr + pc->off[level] + (((uint64_t)t * ROLL_TILE) >> level) + (tid >> (k + 1)), a);
    }
    if (lmax < 10) return;
    if (lane == 0) s_wave[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) {
        const RrPart l = rr_merge(s_wave[0], 512u, s_wave[1], 512u), r = rr_merge(s_wave[2], 512u, s_wave[3], 512u);
        rr_store(pyr + pc->off[10] + 2ull * t, l);
        rr_store(pyr + pc->off[10] + 2ull * t + 1, r);
        if (lmax >= 11) rr_store(pyr + pc->off[11] + t, rr_merge(l, 1024u, r, 1024u));
    }
}

// One wavefront per 64 chunks of level src at a multiple of 64 in the stream's chunk index: the chunks of the levels
// src + 1 .. min(src + 6, lmax) above them.  A chunk outside the piece counts as all outside; what is formed from it
// sticks out of the piece as well, and is stored (where it has a place) but never read.
__global__ __launch_bounds__(256) void k_rru_upper(RrPacked *__restrict__ pyr, const DevRollPiece *__restrict__ pc, uint32_t n,
                                                   uint32_t src, uint32_t lmax)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const uint64_t a0 = pc->a0, last = pc->a1 - 1;
    const uint64_t c = (((a0 >> src) >> 6) + i) * 64u + lane;
    RrPart a = rr_none();
    if (c >= (a0 >> src) && c <= (last >> src)) a = rr_load(pyr + pc->off[src] + (c - (a0 >> src)));
#pragma unroll
    for (uint32_t k = 0; k < 6; ++k) {
        const uint32_t level = src + k + 1u;
        if (level > lmax) return;
        const uint32_t half = 1u << (level - 1u);  // the samples of a chunk of the level below
        a = rr_merge(a, half, shfl_down_part(a, 1u << k), half);
        const uint64_t j = c >> (k + 1);
        if ((lane & ((2u << k) - 1u)) == 0 && j >= (a0 >> level) && j <= (last >> level))
            rr_store(pyr + pc->off[level] + (j - (a0 >> level)), a);
    }
}

// One wavefront per DevRollTask, a lane per position: the window's canonical chunks left to right, merged in that order
// behind an accumulator whose length is pos - lo, into the position's record.
__global__ __launch_bounds__(256) void k_rru_positions(const DevRollTask *__restrict__ tasks, uint32_t n,
                                                       const double *__restrict__ scratch, const RrPacked *__restrict__ pyr,
                                                       const DevRollPiece *__restrict__ pc, uint64_t w, uint64_t stride, int op,
                                                       double limit, RrRec *__restrict__ out)
{
    __shared__ uint64_t s_off[ROLL_MAX_LEVEL + 1];  // a lane's level is its own: the offsets are read by lane
    if (threadIdx.x <= ROLL_MAX_LEVEL) s_off[threadIdx.x] = pc->off[threadIdx.x];
    __syncthreads();
    const RrCond cd = rr_cond(op, limit);
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevRollTask t = tasks[i];
    const uint64_t a0 = pc->a0;
    for (uint32_t p = lane; p < t.n; p += 64u) {
        const uint64_t lo = t.lo + (uint64_t)p * stride, hi = lo + w;
        RrPart acc = rr_none();  // w <= 2^20: a window's integers fit 32 bits
        for (uint64_t pos = lo; pos < hi;) {
            const uint32_t up = pos ? (uint32_t)__builtin_ctzll(pos) : 63u, fit = 63u - (uint32_t)__builtin_clzll(hi - pos);
            const uint32_t l = up < fit ? up : fit;
            const double *x = scratch + (pos - a0);
            RrPart c;
            if (l >= ROLL_RUNS_LOW) {
                c = rr_load(pyr + s_off[l] + ((pos >> l) - (a0 >> l)));
            } else if (l == 0) {
                c = rr_leaf(x[0], cd);
            } else if (l == 1) {
                c = rr_merge(rr_leaf(x[0], cd), 1u, rr_leaf(x[1], cd), 1u);
            } else {
                c = rr_merge(rr_merge(rr_leaf(x[0], cd), 1u, rr_leaf(x[1], cd), 1u), 2u,
                             rr_merge(rr_leaf(x[2], cd), 1u, rr_leaf(x[3], cd), 1u), 2u);
            }
            acc = rr_merge(acc, (uint32_t)(pos - lo), c, 1u << l);
            pos += 1ull << l;
        }
        const uint64_t none = ~0ull;
        // excess without a term is +0.0, as k_run_combine has it
        out[t.rec + p] = RrRec{w, acc.inside, acc.runs, acc.longest, acc.runs ? (uint64_t)acc.longest_at : none,
                               acc.inside ? (uint64_t)acc.first_at : none, acc.inside ? (uint64_t)acc.last_at : none,
                               acc.head, acc.tail, acc.inside ? acc.excess : 0.0};
    }
}

hipError_t launch_rru_pyramid(const double *scratch, uint32_t n_tiles, void *pyr, const DevRollPiece *pc, uint32_t lmax, int op,
                              double limit, hipStream_t s)
{
    if (n_tiles == 0 || lmax < ROLL_RUNS_LOW) return hipSuccess;
    hipLaunchKernelGGL(k_rru_pyramid, dim3(n_tiles), dim3(256), 0, s, scratch, (RrPacked *)pyr, pc, lmax, op, limit);
    return hipGetLastError();
}

hipError_t launch_rru_upper(void *pyr, const DevRollPiece *pc, uint32_t n, uint32_t src, uint32_t lmax, hipStream_t s)
{
    return launch_wave_tasks(k_rru_upper, n, s, (RrPacked *)pyr, pc, n, src, lmax);
}

hipError_t launch_rru_positions(const DevRollTask *tasks, uint32_t n, const double *scratch, const void *pyr,
                                const DevRollPiece *pc, uint64_t w, uint64_t stride, int op, double limit, void *out, hipStream_t s)
{
    return launch_wave_tasks(k_rru_positions, n, s, tasks, n, scratch, (const RrPacked *)pyr, pc, w, stride, op, limit,
                             (RrRec *)out);
}

}  // namespace atsc
