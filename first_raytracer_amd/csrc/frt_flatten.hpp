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
};

// f64: also build the fp64 records of the fp64 kernels (DESIGN.md "Precision")
// refine: the topology refinement of LDS-resident binary trees; -1 = as FRT_TREE_REFINE says
// (default on, read at each call), 0 = off, 1 = on
int flatten_scene(const frt_scene_view *sv, FlatScene &F, std::string &err, bool f64, int refine = -1);
// traversal cost of F's binary tree on the refinement pass's validation rays (the counting
// self-test); false when the tree is not LDS-resident, so the pass does not apply
struct TreeCost { double V = 0.0, T = 0.0, J = 0.0, w = 0.0; int depth = 0, n_rays = 0; };
bool tree_cost_host(const FlatScene &F, TreeCost &out);
// frt_set_env_image / the self-test: validate the image and convert it
int env_texels_of(const frt_image *img, std::vector<float4> &out, std::string &err);
// host image of the flattened scene as the kernels see it (HBM strides)
frt::DevScene host_scene(const FlatScene &F);
#pragma GCC visibility pop
