// scene_host_check.cpp -- the host scene pipeline (csrc/host/obj_import.cpp, bvh_build.cpp, scene.cpp,
// tessellate.cpp) with a stand-alone main, for the address and undefined-behaviour sanitizers
// (make scene_host_asan).  No device: frt_internal_lbvh is a stub.
//   scene_host_check [--tess-dir DIR] FILE.obj ...
//     each file through frt_scene_create as obj_geo and as obj_smooth, then frt_scene_build_bvh_sah, and
//     through frt_write_tessellated_obj (k = 2) into DIR; one line a file:
//       FILE: create=<geo rc>/<smooth rc> n_tris= n_nodes= depth= sah=<rc> sah_nodes= sah_depth= tess=<rc>
//             geom=<FNV-1a of tri_v, tri_n> uv_zero=<1: every uv is 0>
//     Exit status 0 whatever the codes are: they are the result.
//   scene_host_check
//     both builders on synthetic boxes at the sizes where they branch; exit status 1 if a check fails.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "frt.h"
#include "host/bvh_build.hpp"

extern "C" int frt_internal_lbvh(frt_ctx *, int, const float *, int32_t *, float *, int32_t *, double *, int)
{
    return FRT_E_UNSUPPORTED;
}

namespace {

using namespace frt_bvh;

int g_bad = 0;
std::string g_what;
#define CHECK(x) ((x) ? 0 : (std::printf("line %d (%s): %s does not hold\n", __LINE__, g_what.c_str(), #x), ++g_bad))

// levels of interior nodes below and with `node`, counted the way the builders descend (root = 1);
// marks every leaf slot it meets and checks that a node's box contains its children's
int walk(const Tree &t, const std::vector<Box> &boxes, int32_t node, int level, std::vector<int> &seen)
{
    int deepest = level;
    const double *nb = &t.node_box[6 * (size_t)node];
    for (int side = 0; side < 2; ++side) {
        const int32_t c = t.node_child[2 * (size_t)node + side];
        double cb[6];
        for (int k = 0; k < 3; ++k) {
            cb[k] = c < 0 ? boxes[~c].lo[k] : t.node_box[6 * (size_t)c + k];
            cb[3 + k] = c < 0 ? boxes[~c].hi[k] : t.node_box[6 * (size_t)c + 3 + k];
        }
        if (c < 0) ++seen[~c];
        for (int k = 0; k < 3; ++k) CHECK(nb[k] <= cb[k] && nb[3 + k] >= cb[3 + k]);
        if (c >= 0) deepest = std::max(deepest, walk(t, boxes, c, level + 1, seen));
    }
    return deepest;
}

void check_tree(const char *builder, const char *what, const std::vector<Box> &boxes, const Tree &t)
{
    g_what = std::string(builder) + ", " + what;
    const size_t n = boxes.size();
    CHECK(t.node_child.size() == 2 * (n - 1) && t.node_box.size() == 6 * (n - 1) && t.root >= 0);
    if (t.root < 0 || t.node_child.size() != 2 * (n - 1)) return;
    std::vector<int> seen(n, 0);
    const int levels = walk(t, boxes, t.root, 1, seen);
    for (size_t i = 0; i < n; ++i) CHECK(seen[i] == 1);
    CHECK(tree_depth(t.node_child, t.root) == levels && t.depth == levels);
}

int self_checks()
{
    auto line = [](int n, double step) {   // unit boxes along x, `step` apart (0: identical)
        std::vector<Box> b(n);
        for (int i = 0; i < n; ++i) b[i] = Box{{i * step, 0, 0}, {i * step + 1, 1, 1}};
        return b;
    };
    const struct { const char *what; std::vector<Box> boxes; } cases[] = {
        {"2 boxes", line(2, 2.0)}, {"3 boxes", line(3, 2.0)},
        {"5 identical boxes", line(5, 0.0)},            // every sort key tied; one centroid bin: the median split
        {"33 boxes on a line", line(33, 1.5)},          // more boxes than bins
    };
    for (const auto &c : cases) {
        check_tree("sweep", c.what, c.boxes, build_sweep(c.boxes));
        check_tree("binned", c.what, c.boxes, build_binned(c.boxes));
    }
    // tree_depth on what the builders never make: a leaf root, no nodes, a cycle
    g_what = "tree_depth";
    CHECK(tree_depth({}, ~0) == 0 && tree_depth({}, 0) == 0);
    CHECK(tree_depth({~0, ~1}, 0) == 1 && tree_depth({1, ~0, 0, ~1}, 0) == -1 && tree_depth({5, ~0}, 0) == -1);
    // one prim and none go through the scene (install_tree): spheres, no file
    g_what = "one sphere";
    for (int n = 0; n <= 3; ++n) {
        frt_host_scene *s = nullptr;
        frt_material m{};
        m.type = FRT_MAT_LAMBERTIAN;
        CHECK(frt_scene_new(&s) == FRT_OK);
        for (int i = 0; i < n; ++i) {
            const double c[3] = {3.0 * i, 0, 0};
            CHECK(frt_scene_add_sphere(s, c, 1.0, &m, FRT_SPHERE_WORLD) == FRT_OK);
        }
        frt_host_scene_info info{};
        if (n == 0) {
            CHECK(frt_scene_finish(s, FRT_WORLD_BVH) == FRT_E_INVALID);
        } else {
            CHECK(frt_scene_finish(s, FRT_WORLD_LIST) == FRT_OK && frt_scene_build_bvh_sah(s) == FRT_OK);
            frt_scene_view v{};
            CHECK(frt_scene_info(s, &info) == FRT_OK && frt_scene_view_get(s, &v) == FRT_OK);
            CHECK(info.n_nodes == n - 1 && info.bvh_depth == (n > 1 ? n - 1 : 0) && info.n_list == 0);
            CHECK(info.world_kind == FRT_WORLD_BVH && (n > 1 ? v.root == 0 : v.root == ~(FRT_PRIM_SPHERE | 0)));
            CHECK(frt_scene_build_bvh_gpu(s, reinterpret_cast<frt_ctx *>(s), nullptr) ==
                  (n > 1 ? FRT_E_UNSUPPORTED : FRT_OK));   // the stub refuses; one prim needs no device
        }
        frt_scene_destroy(s);
    }
    std::printf("scene_host_check: %d checks failed\n", g_bad);
    return g_bad ? 1 : 0;
}

unsigned long long fnv(unsigned long long h, const void *p, size_t bytes)
{
    const unsigned char *b = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < bytes; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

void one_file(const char *path, const std::string &tess_dir, int index)
{
    frt_host_scene *geo = nullptr, *smooth = nullptr;
    const int rc_geo = frt_scene_create("obj_geo", path, 1.0, &geo);
    const int rc_smooth = frt_scene_create("obj_smooth", path, 1.0, &smooth);
    frt_host_scene_info a{}, b{};
    int sah = FRT_E_INVALID, uv_zero = 1;
    unsigned long long h = 14695981039346656037ull;
    if (geo) {
        frt_scene_info(geo, &a);
        frt_scene_view v{};
        frt_scene_view_get(geo, &v);
        h = fnv(fnv(h, v.tri_v, sizeof(double) * 9 * (size_t)v.n_tris), v.tri_n, sizeof(double) * 9 * (size_t)v.n_tris);
        for (size_t i = 0; v.tri_uv && i < 6 * (size_t)v.n_tris; ++i) uv_zero &= (v.tri_uv[i] == 0.0);
        sah = frt_scene_build_bvh_sah(geo);
        frt_scene_info(geo, &b);
    }
    int tess = FRT_E_INVALID;
    if (!tess_dir.empty())
        tess = frt_write_tessellated_obj(path, 2, (tess_dir + "/tess_" + std::to_string(index) + ".obj").c_str());
    std::printf("%s: create=%d/%d n_tris=%d n_nodes=%d depth=%d sah=%d sah_nodes=%d sah_depth=%d tess=%d geom=%016llx uv_zero=%d\n",
                path, rc_geo, rc_smooth, a.n_tris, a.n_nodes, a.bvh_depth, sah, b.n_nodes, b.bvh_depth, tess, h, uv_zero);
    frt_scene_destroy(geo);
    frt_scene_destroy(smooth);
}

}  // namespace

int main(int argc, char **argv)
{
    std::string tess_dir;
    int files = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--tess-dir") && i + 1 < argc) tess_dir = argv[++i];
        else one_file(argv[i], tess_dir, files++);
    }
    return files ? 0 : self_checks();
}
