// tree_refine.hpp -- topology search over the interior nodes of a small binary
// BVH, scored by the traversal cost of a recorded ray sample (tree_refine.cpp).
// Plain C++ over plain arrays: no scene, no HIP.
#pragma once
#include <cstdint>
#include <vector>

namespace frt_refine {

// A ray sample against the leaves of one tree.  Per ray and per leaf the six
// slab distances of the leaf's box are kept, so the box of any set of leaves
// costs no arithmetic beyond min / max: a union box's near (far) plane is the
// least (greatest) of its members', and the plane distance lo * (1/d) - o/d is
// monotone in the plane, so its near (far) distance is the least (greatest) of
// its members' distances, bit for bit.
struct RaySet {
    int n = 0, n_leaves = 0, n_prims = 0;   // rays, leaves, primitives over all leaves
    std::vector<float> tmin, tmax;          // per ray: the query interval (bvh_tmin, t_max)
    std::vector<uint8_t> anyhit, live;      // per ray: shadow ray; passes the root box (else no visit at all)
    std::vector<float> slab;                // [ray][leaf][6]: near x y z, then MINUS far x y z (a union is one min)
    std::vector<int> prim_first;            // [leaf], n_leaves + 1 entries: the leaf's primitives in prim_*
    std::vector<int> prim_ref;              // [prim]: device ref (FRT_PRIM_SPHERE bit for a sphere)
    std::vector<float> prim_t;              // [ray][prim]: the primitive's hit distance within the ray's interval, or -1
    std::vector<int> root;                  // [ray]: the slot the ray's traversal starts at (`live`: its box is passed);
                                            // empty: every ray starts at the tree's root
};

// Binary tree over leaves 0 .. n_leaves - 1.  A node ref is a "slot": a leaf
// index, or n_leaves + the interior node's index; n_leaves - 1 interior nodes
// -- more when a second root (RaySet::root) shares subtrees with the first, which
// tree_cost prices and refine does not take.
struct Topology {
    int n_leaves = 0, root = 0;
    std::vector<int> child;                 // [2 * interior]: the two child slots
    int depth() const;                      // levels of interior nodes (a lone leaf: 0)
};

struct Cost { double V = 0.0, T = 0.0; };   // node visits and primitive tests per ray
inline double cost_j(const Cost &c, double w) { return c.V + w * c.T; }

// V and T of the sample on the tree, by the visit rule of bvh2_step / leaf_hit
Cost tree_cost(const Topology &t, const RaySet &rays);

// Hill climb over "remove a subtree, reinsert it beside another node" (Bittner,
// Hapala & Havran 2013): a move is kept only when J = V + w T falls on `fit`,
// and never deepens the tree beyond max_depth.  Stops after max_evals move
// evaluations (or at a local minimum): no timer, no threads, so the result is
// a function of the inputs alone.  Returns the number of moves kept.
int refine(Topology &t, const RaySet &fit, double w, int max_depth, int max_evals);

}   // namespace frt_refine
