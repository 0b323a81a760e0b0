// shadow_tree.hpp -- the occluder tree of area-light shadow rays (DESIGN.md
// "Shadow tree"): which triangles no such segment can cross (classify), and the
// binary tree over the leaves that keep a primitive (build), made of the main
// tree's nodes wherever a subtree lost nothing.  Plain C++ over plain arrays,
// fp64: no scene types, no HIP (shadow_tree.cpp).
#pragma once
#include <cstdint>
#include <vector>

namespace frt_shadow {

// The geometry a shadow segment can start on, end on or cross.  Triangles and
// spheres in any one order; `lights` names them as triangle index, or
// sphere_bit | sphere index.
struct Geometry {
    int n_tris = 0, n_spheres = 0;
    const double *tri_v = nullptr;        // 9 per triangle: v0 v1 v2
    const double *tri_n = nullptr;        // 9 per triangle: vertex normals (read for smooth triangles only)
    const uint8_t *tri_smooth = nullptr;  // per triangle: shaded with the interpolated vertex normals; null = none
    const double *sphere = nullptr;       // 4 per sphere: centre, radius
    const int *lights = nullptr;
    int n_lights = 0, sphere_bit = 0;
    double cam_o[3] = {0, 0, 0}, cam_u[3] = {0, 0, 0}, cam_v[3] = {0, 0, 0}, lens_r = 0.0;   // the lens disk
    double eps = 0.0;                     // offset of a ray origin along the shading normal (absolute), and the least t_min
};

enum Why { kRan = 0, kNoLights, kTooLarge };
struct Classified {
    int why = kRan;
    std::vector<uint8_t> dropped;         // per triangle: 1 = no shadow segment can hit it
    int n_rule_a = 0, n_rule_b = 0;       // dropped by the half-space rule / the lights'-plane rule
};
// Never drops what it cannot prove; why != kRan leaves every triangle kept.
void classify(const Geometry &g, Classified &out);

// The tree.  `nodes` holds 16 floats per binary node (child 0 box lo xyz hi xyz,
// child 1 box, the two child refs as int bits, two unused): a ref >= 0 is a node,
// ~ref a leaf -- sphere_bit | k, or first triangle | (count - 1) << count_shift.
// A leaf is deleted when it holds only dropped triangles; a node left with one
// child gives way to that child; a node both of whose subtrees lost nothing is
// the main tree's own; every other node is appended to `nodes` with boxes that
// are the unions of the kept leaves' boxes below it.  Never deeper than the
// main tree.
struct Tree {
    int root = 0;                         // node index, ~leaf, or the main root when nothing was dropped
    bool empty = false;                   // no leaf kept: root is meaningless
    int added = 0, shared = 0;            // nodes appended / main-tree nodes reachable from the shadow root
    int kept_leaves = 0, dropped_leaves = 0;
};
void build(std::vector<float> &nodes, int main_root, const std::vector<uint8_t> &dropped, int sphere_bit,
           int count_shift, Tree &out);

}   // namespace frt_shadow
