// atsc_across_positions.h -- what the six across kernel files share on the device (atsc_across*.hip; DESIGN.md "The
// across position skeleton"): the wavefront-to-(task, position) mapping and its launch, a task's split into pairs at
// stride 1, the two-word store and the dispatch over the powers of two.  A query's own file holds the fold of one column
// and its record.
//
// The streams of a call lie decoded in the call's scratch (across_dev, atsc_windows.cpp): a region per stream, reg[k]
// where stream k's begins (an even number of doubles), slot j of every region the same sample index, slot 0 sample a0
// (even) of the streams.  A DevRollTask t is a run of t.n <= ACR_TASK positions of one range inside one piece: the first
// at sample t.lo of the streams, the others every `stride` samples behind it; position p's record is number t.rec + p of
// the result.  No kernel here uses atomics: every record has one writer.
#pragma once
#include <type_traits>

#include "atsc_tile_reduce.h"

namespace atsc {

// A task's positions go 64 to a wavefront, a lane per position, ACR_SLABS wavefronts a task: a position's work is long
// and a piece has few tasks, so a wavefront per task would leave most of the GPU idle.  (k_across_positions, whose fold
// is short, keeps one wavefront per task and a lane-strided loop.)
constexpr uint32_t ACR_SLABS = ACR_TASK / 64u;

// The wavefront's task i and its first position p0 of that task, SLABS wavefronts of 64 a task; false past the list's end.
template <uint32_t SLABS = ACR_SLABS>
DEVI bool slab_wave(uint32_t n, uint32_t &i, uint32_t &p0)
{
    const uint32_t w = wave_task();
    i = w / SLABS;
    p0 = (w % SLABS) * 64u;
    return i < n;
}

// The lane's task t and its position p of it; false past the list's end or behind the task's last position.
DEVI bool slab_position(const DevRollTask *tasks, uint32_t n, DevRollTask &t, uint32_t &p)
{
    const uint32_t lane = wave_lane(), w = wave_task(), i = w / ACR_SLABS;
    if (i >= n) return false;
    t = tasks[i];
    p = (w % ACR_SLABS) * 64u + lane;
    return p < t.n;
}

// position p's slot of every region
DEVI uint64_t slab_slot(const DevRollTask &t, uint64_t a0, uint32_t p, uint64_t stride) { return t.lo - a0 + (uint64_t)p * stride; }

// Stride 1: n positions from slot s0 on.  An odd first slot (head) and what is left behind the pairs (tail) go one at a
// time, the rest in `pairs` pairs from the even slot s0 + head, one 16-byte load per stream and pair.
struct PairSplit {
    uint32_t head, pairs, tail;
};
DEVI PairSplit pair_split(uint64_t s0, uint32_t n)
{
    const uint32_t head = n ? (uint32_t)(s0 & 1u) : 0u;
    return PairSplit{head, (n - head) >> 1, (n - head) & 1u};
}

// Two adjacent words of a record.  A16: p lies at a multiple of 16 bytes, and they go out as one 16-byte store; else as
// two of 8 bytes, at the alignment the contract asks of a result.
template <bool A16>
DEVI void store_words(uint64_t *p, uint64_t a, uint64_t b)
{
    if constexpr (A16) {
        *(ulonglong2 *)p = make_ulonglong2(a, b);
    } else {
        p[0] = a;
        p[1] = b;
    }
}

// (more tasks in a piece than a grid has wavefronts)
inline bool slab_grid_fits(uint32_t n)
{
    static_assert(ACR_TASK % 64u == 0, "whole wavefronts");
    return n <= 0xFFFFFFFFu / ACR_SLABS;
}

// `kernel` over n tasks of SLABS wavefronts each; args: the kernel's own, n among them.
template <uint32_t SLABS = ACR_SLABS, class K, class... A>
inline hipError_t launch_slab_tasks(K kernel, uint32_t n, hipStream_t s, A... args)
{
    static_assert(SLABS >= 1 && SLABS <= ACR_SLABS, "the grid guard covers it");
    if (!slab_grid_fits(n)) return hipErrorInvalidValue;
    return launch_wave_tasks(kernel, n * SLABS, s, args...);
}

// f(std::integral_constant<int, G>()) for the smallest power of two G >= v; hipErrorInvalidValue where v > MAX.
template <int MAX, int G = 1, class F>
inline hipError_t pow2_dispatch(uint32_t v, F f)
{
    if (v <= (uint32_t)G) return f(std::integral_constant<int, G>());
    if constexpr (G < MAX)
        return pow2_dispatch<MAX, 2 * G>(v, f);
    else
        return hipErrorInvalidValue;
}

}  // namespace atsc
