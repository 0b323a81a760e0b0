// bvh_build.hpp -- the host's two BVH builders over fp64 boxes
// (csrc/host/bvh_build.cpp): the reference's sweep-SAH rule
// (parallel_bvh_node::create_bvh, parallel_bvh.h:67-175) and a binned SAH.
// Plain arrays in, plain arrays out; csrc/host/scene.cpp installs the result.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace frt_bvh {

struct Box {
    double lo[3], hi[3];
};
inline double box_area(const Box &b)  // aabb.h:46-49 (size = max - min)
{
    const double sx = b.hi[0] - b.lo[0], sy = b.hi[1] - b.lo[1], sz = b.hi[2] - b.lo[2];
    return 2 * ((sx * sy) + (sy * sz) + (sx * sz));
}
inline Box surround(const Box &a, const Box &b)  // aabb.h:57-68
{
    Box r;
    for (int k = 0; k < 3; ++k) { r.lo[k] = std::fmin(a.lo[k], b.lo[k]); r.hi[k] = std::fmax(a.hi[k], b.hi[k]); }
    return r;
}
inline int longest_axis(const Box &b)  // aabb.h:33-43
{
    const double sx = b.hi[0] - b.lo[0], sy = b.hi[1] - b.lo[1], sz = b.hi[2] - b.lo[2];
    if (sy > sx) return 1;
    if (sz > sx) return 2;
    return 0;
}

// A tree over n >= 2 boxes: n - 1 nodes numbered in creation order, 6 doubles
// (lo, hi) and 2 children a node; a child >= 0 is a node, < 0 the leaf ~slot of
// box `slot`.  depth: what tree_depth(node_child, root) counts; the builders
// report it from their recursion.
struct Tree {
    std::vector<double> node_box;
    std::vector<int32_t> node_child;
    int32_t root = 0;
    int depth = 0;
};

// the fp64 boxes of the prim refs `refs` (FRT_PRIM_SPHERE | sphere index, or a
// triangle index) over the scene's 9-double triangles and 4-double spheres
std::vector<Box> prim_boxes(const double *tri_v, const double *sphere, const int32_t *refs, size_t n);

// boxes.size() >= 2 for both
Tree build_sweep(const std::vector<Box> &boxes);    // the reference's tree, glibc merge-sort tie order
Tree build_binned(const std::vector<Box> &boxes);   // FRT_EXP_SAH_BINS (32) centroid bins an axis

// levels of interior nodes on the longest path from `root` (the root is level 1;
// 0 for a leaf root or no nodes), or -1 where the nodes reached are not a tree
int tree_depth(const std::vector<int32_t> &node_child, int32_t root);

}  // namespace frt_bvh
