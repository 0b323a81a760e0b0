// exit_tree.hpp -- the trees extension rays start at (DESIGN.md "Exit trees"):
// which triangles a ray that leaves triangle k on its normal's side cannot hit
// (classify), and for every leaf of the main tree the largest subtree made of
// such triangles only (classes).  The tree without that subtree is built by
// frt_shadow::build.  Plain C++ over plain arrays, fp64: no scene types, no HIP
// (exit_tree.cpp).
#pragma once
#include <cstdint>
#include <vector>

#include "shadow_tree.hpp"

namespace frt_exit {

enum Why { kRan = 0, kTooLarge };
struct Hidden {
    int why = kRan;
    int n = 0;
    std::vector<uint8_t> served;   // per triangle k: an extension ray that leaves k can be given a tree of its own
    std::vector<uint8_t> hidden;   // [k * n + j]: 1 = no such ray can report a hit on triangle j (k itself included)
};
// Geometry as the shadow pass takes it (the lights: triangles that get no root).  Never hides what
// it cannot prove; why != kRan serves no triangle.
void classify(const frt_shadow::Geometry &g, Hidden &out);

// One drop set: the subtree `sub` (a node index, or ~leaf) of the main tree, for the extension rays
// that leave the triangles `members` -- every triangle of the main-tree leaves whose largest wholly
// hidden subtree it is.
struct Class {
    int sub = 0, level = 0;            // level: the root is 0
    std::vector<int> members;          // origin triangles, ascending
    std::vector<uint8_t> dropped;      // per triangle: 1 = in `sub`
    int n_dropped = 0;
};
// `nodes` as frt_shadow::build reads them.  Classes in the order of their first leaf in a
// child-0-first walk.  A leaf with a triangle that is not served, or whose own triangles are not
// hidden from each other, is in no class; nor is one whose drop set is the whole tree.
void classes(const std::vector<float> &nodes, int main_root, int sphere_bit, int count_shift, const Hidden &h,
             std::vector<Class> &out);

}   // namespace frt_exit
