// frt_flatten.hpp -- the host image of the device scene: a frt_scene_view
// flattened into the arrays the kernels read (frt_flatten.hip).  CPU only.
#pragma once
#include <string>
#include <vector>

#include "frt.h"
#include "frt_device.hpp"
#include "frt_path.hpp"

using frt::DevScene;

#pragma GCC visibility push(hidden)
// host image of the device scene (DESIGN.md "Data layout")
struct FlatScene {
    std::vector<float4> nodes, tris, tshade, tnorm, spheres, mats, tuv;
    std::vector<float4> texels;   // image_texture texels (rgb, -), all images back to back
    std::vector<uint4> nodes4;   // 4-wide quantized BVH
    std::vector<float4> nodes_oct;   // 8 octant copies of `nodes` (DevScene::nodes_oct), LDS plan scenes only
    std::vector<double4> tris64, tshade64, tnorm64, spheres64;   // fp64 records (DevScene::tris64 ...)
    bool has4 = false;           // nodes4 / root4 usable
    int root4 = 0, depth4 = 0;
    std::vector<int> smat, lights, list;
    std::vector<int> tri_view;      // device triangle id -> scene-view triangle (DevScene::tri_view)
    DevScene meta{};     // scalars + camera; pointers filled by the consumer
    int depth = 0;
    // what the shadow-tree pass did (frt_tree_passes.hip shadow_tree): why != kShadowRan leaves
    // meta.sroot the main root and `nodes` untouched
    enum { kShadowRan = 0, kShadowOff, kShadowNoLights, kShadowTooLarge, kShadowMaterial, kShadowNotResident,
           kShadowNothing, kShadowBudget };
    struct {
        int why = kShadowOff;
        std::vector<uint8_t> dropped;   // per device triangle
        int n_dropped = 0, rule_a = 0, rule_b = 0, nodes_main = 0, added = 0, shared = 0;
        bool empty = false;
    } shadow;
    // what the exit-tree pass did (frt_tree_passes.hip exit_tree): why != kExitRan leaves `nodes` and the
    // shading records untouched (every exit root 0 = the main root)
    enum { kExitRan = 0, kExitOff, kExitMaterial, kExitNotResident, kExitTooLarge, kExitNothing, kExitBudget };
    struct ExitClass { int sub, root, members, dropped, added, shared; double gain; };   // sub: the dropped subtree (node, or ~leaf)
    struct {
        int why = kExitOff;
        int classes = 0;                // distinct drop sets found
        std::vector<ExitClass> taken;   // those given a tree, in the order taken
        std::vector<int> root;          // per device triangle: the node its extension rays start at, 0 = the main root
        int nodes_before = 0, added = 0;
        bool budget_refused = false;    // a drop set with a gain was left out for the LDS budget
    } exit;
};

// f64: also build the fp64 records of the fp64 kernels (DESIGN.md "Precision")
// refine, shadow, exit: the modes of the passes over the finished tree (frt_tree_passes.hpp)
int flatten_scene(const frt_scene_view *sv, FlatScene &F, std::string &err, bool f64, int refine = -1, int shadow = -1,
                  int exit = -1);
// frt_set_env_image / the self-test: validate the image and convert it
int env_texels_of(const frt_image *img, std::vector<float4> &out, std::string &err);
// host image of the flattened scene as the kernels see it (HBM strides)
frt::DevScene host_scene(const FlatScene &F);
#pragma GCC visibility pop
