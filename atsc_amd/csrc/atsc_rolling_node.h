// atsc_rolling_node.h -- the chunk partial of the rolling pyramids over the centred co-moment node (atsc_moment_node.h):
// what the windowed rolling moments (atsc_rolling_moments.hip: value x against the stream index t) and the windowed
// rolling pair moments (atsc_rolling_pair.hip: value x of one stream against value y of another, in the fields named t
// here) share.  A partial is the node's five doubles and its count in a 64-bit word: 48 bytes, read and written as three
// 16-byte words.  Merge is node_merge of atsc_moment_rule.h; the equal-count form is chosen lane by lane, so a chunk's
// bits do not depend on what the other lanes hold.  The levels above 11 merge partials only: both calls run
// k_rmo_upper (atsc_rolling_moments.hip) over their pyramids.
#pragma once
#include "atsc_moment_node.h"

namespace atsc {

namespace {

// a partial as the pyramid holds it; in registers it is a Node (a chunk holds at most 2^20 samples)
struct alignas(16) RmPart {
    double mx, m2x, mt, m2t, c;
    uint64_t n;
};
static_assert(sizeof(RmPart) == ROLL_MOMENTS_PART, "a partial is 48 bytes");

DEVI Node rm_none() { return Node{0.0, 0.0, 0.0, 0.0, 0.0, 0}; }

// Merge(a, b): equal non-zero counts skip the divide (the same bits: node_merge)
DEVI Node rm_merge(const Node &a, const Node &b)
{
    if (a.n == b.n && a.n != 0) return node_merge<true>(a, b);
    return node_merge<false>(a, b);
}

DEVI Node rm_load(const RmPart *p)
{
    const double2 a = ((const double2 *)p)[0], b = ((const double2 *)p)[1], c = ((const double2 *)p)[2];  // three 16-byte loads
    return Node{a.x, a.y, b.x, b.y, c.x, (uint32_t)(uint64_t)__double_as_longlong(c.y)};
}

DEVI void rm_store(RmPart *p, const Node &r)
{
    ((double2 *)p)[0] = make_double2(r.mx, r.m2x);
    ((double2 *)p)[1] = make_double2(r.mt, r.m2t);
    ((double2 *)p)[2] = make_double2(r.c, __longlong_as_double((long long)(uint64_t)r.n));
}

}  // namespace

}  // namespace atsc
