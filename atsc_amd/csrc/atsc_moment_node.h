// atsc_moment_node.h -- the centred co-moment node of two coordinates and its merge, shared by the windowed moments
// (atsc_moments.hip: value x against position t) and the windowed pair moments (atsc_pair.hip: value x of one stream
// against value y of another, in the fields named t here).  The merge order is part of both contracts
// (include/atsc_hip.h, DESIGN.md "Windowed moments", "Windowed pair moments"): a node is (n, mx, M2x, mt, M2t, C);
// Merge(a, b) is a when nb == 0, b when na == 0, else
//     n = na + nb; w = (double)nb / (double)n; f = (double)na * w; dx = mxb - mxa; dt = mtb - mta;
//     mx = mxa + dx * w; mt = mta + dt * w;
//     M2x = (M2xa + M2xb) + (dx * dx) * f; M2t = (M2ta + M2tb) + (dt * dt) * f; C = (Ca + Cb) + (dx * dt) * f
// (one rounding per operation: the files that include this are compiled with -ffp-contract=off).  The tree is the tile
// sum's (tile_lane_sums, atsc_tile_reduce.h) with + replaced by Merge, the left operand as a.  Merge itself is
// node_merge of atsc_moment_rule.h, which the host shares.
#pragma once
#include "atsc_moment_rule.h"
#include "atsc_tile_reduce.h"

namespace atsc {

namespace {

// the node inside a tile: DevMomPart with a 32-bit count (a tile's nodes hold at most 2048 samples)
struct Node {
    double mx, m2x, mt, m2t, c;
    uint32_t n;
};

// the leaf of the coordinates (v, t); ok: inside the window and not NaN
__device__ __forceinline__ Node node_leaf(double v, double t, bool ok)
{
    return ok ? Node{v, 0.0, t, 0.0, 0.0, 1} : Node{0.0, 0.0, 0.0, 0.0, 0.0, 0};
}

// a virtual lane's eight leaves into its node: leaf(q, e) is the leaf of slot tile_slot(v, q) + e
template <bool EQ, class Leaf>
__device__ __forceinline__ Node lane_node(Leaf leaf)
{
    Node p[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) p[q] = node_merge<EQ>(leaf(q, 0), leaf(q, 1));
    return node_merge<EQ>(node_merge<EQ>(p[0], p[1]), node_merge<EQ>(p[2], p[3]));
}

// the halving tree over the 256 virtual lanes: h = 128 and 64 inside the lane, then 32 .. 1 across the wavefront
template <bool EQ>
__device__ __forceinline__ Node tile_node(const Node (&s)[4])
{
    return wave_halve(node_merge<EQ>(node_merge<EQ>(s[0], s[2]), node_merge<EQ>(s[1], s[3])), node_merge<EQ, Node>);
}

}  // namespace

}  // namespace atsc
