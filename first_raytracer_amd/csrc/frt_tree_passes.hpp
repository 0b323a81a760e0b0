// frt_tree_passes.hpp -- the passes flatten_scene runs over the finished binary tree of an
// LDS-resident scene, and the counting hooks of the self-tests (frt_tree_passes.hip).  CPU only.
#pragma once
#include "frt_flatten.hpp"

#pragma GCC visibility push(hidden)
// The passes, in the order flatten_scene runs them.  mode: -1 = as the pass's knob says (FRT_TREE_REFINE,
// FRT_SHADOW_TREE, FRT_EXIT_TREE: default on, read at each call), 0 = off, 1 = on.  True when F.nodes
// changed: the caller makes the octant copies and BVH4Q again.
bool refine_tree(FlatScene &F, int mode);                              // topology refinement of the main tree
bool shadow_tree(const frt_scene_view *sv, FlatScene &F, int mode);    // F.shadow, meta.sroot; nodes appended
bool exit_tree(const frt_scene_view *sv, FlatScene &F, int mode);      // F.exit, the shading records' roots; nodes appended

// V, T and J of the refinement pass's validation rays, each started where the kernels start it, with
// the exit roots ignored (index 0) and used (1): over all rays, and V and T over the extension rays
// alone (per extension ray); false when the tree is not LDS-resident
struct ExitCost {
    double V_all[2] = {0, 0}, T_all[2] = {0, 0}, J_all[2] = {0, 0}, V_ext[2] = {0, 0}, T_ext[2] = {0, 0};
    int n_rays = 0, n_ext = 0;
};
bool exit_cost_host(const FlatScene &F, ExitCost &out);
// V and T of the refinement pass's validation rays that are area-light shadow rays, started at the
// main root (index 0) and at the shadow root (1); stops: how many of them miss that root's box
struct ShadowCost { double V[2] = {0, 0}, T[2] = {0, 0}; int n_rays = 0, stops[2] = {0, 0}; };
bool shadow_cost_host(const FlatScene &F, ShadowCost &out);
// the origins of those rays (3 floats each), for the segment property test
void shadow_origins_host(const FlatScene &F, std::vector<float> &origins);
// traversal cost of F's binary tree on the refinement pass's validation rays (the counting
// self-test); false when the tree is not LDS-resident, so the pass does not apply
struct TreeCost { double V = 0.0, T = 0.0, J = 0.0, w = 0.0; int depth = 0, n_rays = 0; };
bool tree_cost_host(const FlatScene &F, TreeCost &out);
#pragma GCC visibility pop
