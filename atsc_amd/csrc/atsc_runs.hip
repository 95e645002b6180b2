// atsc_runs.hip -- gfx950 kernels of the windowed runs (atsc_runs_windows_dev): per window the samples that meet a
// condition (x OP limit), the maximal runs of stream-adjacent ones among them, the longest run and where it starts, the
// first and last inside sample, the runs at the window's two ends, and the sum of |x - limit| over the inside samples,
// reduced from decoded samples in the call's scratch.
//
// The contract is include/atsc_hip.h's (DESIGN.md "Windowed runs").  A sample is inside iff it is not NaN and x OP limit
// holds.  The nine integers form an associative, order-dependent monoid (run_merge below, the header's merge rule on
// absolute stream positions): a run that crosses a tile, a combine group or a piece of the scratch is joined by the merge
// itself, so no sample is carried from one piece to the next.  The term of an inside sample, fabs(x - limit), sits at the
// sample's own slot, every other slot holds -0.0, and the sum goes through the tile sum's tree (tile_lane_sums,
// atsc_tile_reduce.h) unchanged.
// One wavefront reduces one tile or one group of 64 tile partials of a window.  No atomics: every partial has one writer.
//
// The tile kernel keeps the 16-byte loads and slot-to-lane mapping of atsc_tile_reduce.h for the sum.  That mapping
// interleaves the slots, and the runs need them in stream order: the 64 lanes of one load step hold 128 contiguous
// slots, so two ballots (the loads' first halves, their second halves) give those slots' inside bits as wave-uniform
// masks; lane g < 32 keeps the halves that belong to slots [64 g, 64 g + 64), interleaves them once into a 64-bit word,
// reads the word's node off it with popcount, count-trailing / leading-zeros and six shift-and steps, and a five-step
// shuffle tree merges the 32 nodes in order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// The node of a stretch of the stream inside a tile: DevRunPart's nine integers in 32 bits, positions counted from the
// tile's slot 0, NONE = ~0u.  The empty node, here and between tiles: all zero, the three positions NONE.
struct Run {
    uint32_t samples, inside, runs, longest, longest_at, first_at, last_at, head, tail;
};
constexpr Run RUN_EMPTY{0, 0, 0, 0, ~0u, ~0u, ~0u, 0, 0};

// a followed by b.  The run that joins them starts tail(a) samples in front of b's first sample, which is b's first inside
// sample when head(b) != 0.  Strict comparisons: of equal runs the earliest stays.  Either may be the empty node.
// R: Run, or DevRunPart, whose nine integers are these with stream indices for positions.
template <class R>
__device__ __forceinline__ R run_merge(const R &a, const R &b)
{
    using T = decltype(a.samples);
    R r = a;
    const bool join = a.tail != 0 && b.head != 0;
    r.samples = a.samples + b.samples;
    r.inside = a.inside + b.inside;
    r.runs = a.runs + b.runs - (join ? 1 : 0);
    r.head = a.head == a.samples ? a.samples + b.head : a.head;
    r.tail = b.tail == b.samples ? b.samples + a.tail : b.tail;
    r.first_at = a.inside ? a.first_at : b.first_at;
    r.last_at = b.inside ? b.last_at : a.last_at;
    T lg = a.longest, at = a.longest_at;
    const T jl = a.tail + b.head;
    if (join && jl > lg) { lg = jl; at = b.first_at - a.tail; }
    if (b.longest > lg) { lg = b.longest; at = b.longest_at; }
    r.longest = lg;
    r.longest_at = at;
    return r;
}

// two partials: the nodes, and the sums' terms left operand first
__device__ __forceinline__ DevRunPart part_merge(const DevRunPart &a, const DevRunPart &b)
{
    DevRunPart r = run_merge(a, b);
    r.excess = a.excess + b.excess;
    return r;
}

// bit i of x to bit 2 i
__device__ __forceinline__ uint64_t spread_bits(uint32_t x)
{
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000ffff0000ffffull;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// The node of 64 slots whose slot 0 is slot `base` of the tile: bit i of m is set iff slot base + i lies in the window and
// is inside; the window holds the slots [vlo, vhi) of the word (vlo <= vhi <= 64), and m has no bit outside them.
__device__ __forceinline__ Run word_node(uint64_t m, uint32_t vlo, uint32_t vhi, uint32_t base)
{
    Run r = RUN_EMPTY;
    if (vhi <= vlo) return r;
    r.samples = vhi - vlo;
    if (m == 0) return r;
    r.inside = (uint32_t)__popcll(m);
    r.runs = (uint32_t)__popcll(m & ~(m << 1));
    r.first_at = base + (uint32_t)__builtin_ctzll(m);
    r.last_at = base + 63u - (uint32_t)__builtin_clzll(m);
    if (m == ~0ull) {
        r.longest = r.head = r.tail = 64;
        r.longest_at = base;
        return r;
    }
    // m has a clear bit inside the word or the window ends inside it: the complements below are not zero
    r.head = (uint32_t)__builtin_ctzll(~(m >> vlo));
    r.tail = (uint32_t)__builtin_clzll(~(m << (64u - vhi)));
    // e[i]: the bits that end a stretch of 2^i set bits (bit p: bits p - 2^i + 1 .. p are all set)
    uint64_t e[6];
    e[0] = m;
#pragma unroll
    for (int i = 1; i < 6; ++i) e[i] = e[i - 1] & (e[i - 1] << (1u << (i - 1)));
    // the longest stretch by its binary digits: `ends` holds the bits that end a stretch of `len` set bits
    uint64_t ends = ~0ull;
    uint32_t len = 0;
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        const uint64_t t = ends & (e[i] << len);
        if (t) { ends = t; len += 1u << i; }
    }
    r.longest = len;
    r.longest_at = base + (uint32_t)__builtin_ctzll(ends) + 1u - len;  // the earliest of the longest
    return r;
}

}  // namespace

// One wavefront per DevPosTile: the node of the slots [lo, hi) of the tile at scratch[src], whose slot 0 is sample t0 of
// the stream, into part[dst]; a slot outside [lo, hi) is the empty node.  op, limit: the call's condition.
__global__ __launch_bounds__(256) void k_run_tiles(const DevPosTile *__restrict__ tasks, uint32_t n,
                                                   const double *__restrict__ scratch, int op, double limit,
                                                   DevRunPart *__restrict__ part)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n) return;
    const DevPosTile t = tasks[i];
    const double *x = scratch + t.src;
    // x OP limit from the three ordered comparisons, each false on NaN
    const bool want_gt = op == ATSC_RUNS_GT || op == ATSC_RUNS_GE || op == ATSC_RUNS_NE;
    const bool want_lt = op == ATSC_RUNS_LT || op == ATSC_RUNS_LE || op == ATSC_RUNS_NE;
    const bool want_eq = op == ATSC_RUNS_GE || op == ATSC_RUNS_LE || op == ATSC_RUNS_EQ;
    uint32_t ev = 0, od = 0;  // lane g < 32: the inside bits of the even and of the odd slots of [64 g, 64 g + 64)
    // The tile sum in the order tile_lane_sums (atsc_tile_reduce.h) defines, written out: through that helper this
    // kernel comes out with either 14 % more instructions or without its wave-uniform branches on the condition.  The
    // virtual lanes go two at a time, (lane, lane + 128) and then (lane + 64, lane + 192), in a loop that is not
    // unrolled, as in k_dlt_tiles: the halving tree's first step inside the lane, s[v] + s[v + 128], closes each trip,
    // its second step joins the two trips.  Unrolled four times the 16 loads' predicates and the 32 ballots spill SGPRs.
    double ex[1] = {-0.0};
#pragma unroll 1
    for (uint32_t kk = 0; kk < 2; ++kk) {
        double s[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const uint32_t k = kk + 2u * e, v = lane + 64u * k;
            double p[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t j = tile_slot(v, q);
                const double2 d = tile_load(x, j, t.lo, t.hi, -0.0);
                const bool in0 = tile_in(j, t.lo, t.hi) &&
                                 ((want_gt && d.x > limit) || (want_lt && d.x < limit) || (want_eq && d.x == limit));
                const bool in1 = tile_in(j + 1u, t.lo, t.hi) &&
                                 ((want_gt && d.y > limit) || (want_lt && d.y < limit) || (want_eq && d.y == limit));
                const double a = in0 ? __builtin_fabs(d.x - limit) : -0.0;
                const double b = in1 ? __builtin_fabs(d.y - limit) : -0.0;
                p[q] = a + b;
                // this step's lanes hold the slots [128 w, 128 w + 128), w = 4 q + k: lane l the slots 128 w + 2 l, + 1
                const uint64_t be = __ballot(in0), bo = __ballot(in1);
                const uint32_t w = 4u * q + k;
                if ((lane >> 1) == w) {
                    ev = (lane & 1u) ? (uint32_t)(be >> 32) : (uint32_t)be;
                    od = (lane & 1u) ? (uint32_t)(bo >> 32) : (uint32_t)bo;
                }
            }
            s[e] = (p[0] + p[1]) + (p[2] + p[3]);
        }
        const double h = s[0] + s[1];
        ex[0] = kk ? ex[0] + h : h;
    }
    const double excess = wave_halve(ex[0], [](double a, double b) { return a + b; });
    // lane g < 32: the node of the slots [64 g, 64 g + 64); then lane l + 2^k into lane l, the left operand first
    Run r = RUN_EMPTY;
    if (lane < 32u) {
        const uint32_t base = 64u * lane;
        const uint32_t vlo = t.lo > base ? (t.lo - base < 64u ? t.lo - base : 64u) : 0u;
        const uint32_t vhi = t.hi > base ? (t.hi - base < 64u ? t.hi - base : 64u) : 0u;
        r = word_node(spread_bits(ev) | (spread_bits(od) << 1), vlo, vhi, base);
    }
    r = wave_pairwise<32>(r, run_merge<Run>);
    if (lane == 0) {
        const uint64_t none = ~0ull;
        DevRunPart o;
        o.samples = r.samples;
        o.inside = r.inside;
        o.runs = r.runs;
        o.longest = r.longest;
        o.longest_at = r.runs ? t.t0 + r.longest_at : none;
        o.first_at = r.inside ? t.t0 + r.first_at : none;
        o.last_at = r.inside ? t.t0 + r.last_at : none;
        o.head = r.head;
        o.tail = r.tail;
        o.excess = excess;
        part[t.dst] = o;
    }
}

// One wavefront per DevAggComb: the group's partials through comb_reduce (a missing right operand is the empty node and
// -0.0), then, in the final pass, into the window's atsc_window_runs (ten 8-byte fields, one per lane): the three
// positions counted from the window's begin[win], excess +0.0 without a term.
__global__ __launch_bounds__(256) void k_run_combine(const DevAggComb *__restrict__ tasks, uint32_t n_tasks,
                                                     DevRunPart *__restrict__ part, const uint64_t *__restrict__ begin,
                                                     uint64_t *__restrict__ out)
{
    const uint32_t lane = wave_lane(), i = wave_task();
    if (i >= n_tasks) return;
    const DevAggComb c = tasks[i];
    const uint64_t none = ~0ull;
    const DevRunPart a =
        comb_reduce(c, lane, part, DevRunPart{0, 0, 0, 0, none, none, none, 0, 0, -0.0}, part_merge);
    if (!c.final_) return;
    const uint64_t b0 = c.n ? begin[c.win] : 0;
    const uint64_t samples = __shfl(a.samples, 0, 64), inside = __shfl(a.inside, 0, 64), runs = __shfl(a.runs, 0, 64),
                   longest = __shfl(a.longest, 0, 64), longest_at = __shfl(a.longest_at, 0, 64),
                   first_at = __shfl(a.first_at, 0, 64), last_at = __shfl(a.last_at, 0, 64),
                   head = __shfl(a.head, 0, 64), tail = __shfl(a.tail, 0, 64);
    const double excess = __shfl(a.excess, 0, 64);
    if (lane < 10) {
        uint64_t w;
        switch (lane) {
        case 0: w = samples; break;
        case 1: w = inside; break;
        case 2: w = runs; break;
        case 3: w = longest; break;
        case 4: w = runs ? longest_at - b0 : none; break;
        case 5: w = inside ? first_at - b0 : none; break;
        case 6: w = inside ? last_at - b0 : none; break;
        case 7: w = head; break;
        case 8: w = tail; break;
        default: w = __double_as_longlong(inside ? excess : 0.0); break;
        }
        out[10ull * c.dst + lane] = w;
    }
}

hipError_t launch_run_tiles(const DevPosTile *tasks, uint32_t n, const double *scratch, int op, double limit,
                            DevRunPart *part, hipStream_t s)
{
    return launch_wave_tasks(k_run_tiles, n, s, tasks, n, scratch, op, limit, part);
}

hipError_t launch_run_combine(const DevAggComb *tasks, uint32_t n, DevRunPart *part, const uint64_t *begin, void *out,
                              hipStream_t s)
{
    return launch_wave_tasks(k_run_combine, n, s, tasks, n, part, begin, (uint64_t *)out);
}

}  // namespace atsc
