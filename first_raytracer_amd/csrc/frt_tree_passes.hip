// frt_tree_passes.hip -- what scene upload does to the flattened binary tree of an LDS-resident
// scene once flatten_scene (frt_flatten.hip) has finished it: the topology refinement (refine_tree),
// the occluder tree of area-light shadow rays (shadow_tree) and the trees extension rays start at
// (exit_tree), each judged on a host replay of the scene's own path integrator (sample_rays), and
// the counting hooks the self-tests read.  The searches and proofs themselves are plain C++ under
// host/.  No kernel and no HIP runtime call; built with the kernel units' compiler and flags, since
// the replay runs path_begin / path_shade / trace / trav_begin and must round as the kernels do.
#include "frt_tree_passes.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <unordered_map>

#include "frt_kernels.hpp"   // the LDS footprint rule (lds_*_bytes, lds_*_fits, kLdsMaxDepth)
#include "host/exit_tree.hpp"
#include "host/shadow_tree.hpp"
#include "host/tree_refine.hpp"

using namespace frt;

// ---- what the passes share ----
// a pass's knob: on unless the variable is set to 0 (a tuning knob of this library, not part of the C-ABI)
static bool knob(const char *name)
{
    const char *e = std::getenv(name);
    return !(e && std::atoi(e) == 0);
}
static bool pass_on(int mode, const char *name) { return mode < 0 ? knob(name) : mode != 0; }

// dielectric and the specular lobes leave from p - eps n: the shadow and exit proofs hold for
// lambertian / diffuse_light scenes only
static bool lambertian_only(const frt_scene_view *sv)
{
    for (int i = 0; i < sv->n_materials; ++i)
        if (sv->materials[i].type != FRT_MAT_LAMBERTIAN && sv->materials[i].type != FRT_MAT_DIFFUSE_LIGHT) return false;
    return true;
}

// does the residency rule (frt_ctx.hpp residency) put this scene's binary tree in LDS?
static bool tree_in_lds(const FlatScene &F)
{
    if (F.meta.world_kind != FRT_WORLD_BVH || F.meta.root < 0 || F.depth >= kLdsMaxDepth) return false;
    return lds_planar_fits(lds_planar_bytes(F.nodes.size() / 4, lds_rest(F))) || !F.nodes_oct.empty();
}

// Blocks of the LDS plans that a CU holds: a block's LDS -- the traversal stack and the item state
// of its 256 lanes, then the scene -- is allocated in granules of 1280 B out of 160 KiB.  Measured
// on the Cornell octant plan (8-entry stack: 18432 B before the scene), profiles/exittree/
// exit_cap.jsonl: a scene of 13328 B (31760 B a block, 25 granules, 5 blocks) runs the path kernel
// in 186.6 ms and AO in 25.0 ms, one of 13712 B (32144 B, 26 granules, 4 blocks) in 209.3 ms and
// 28.3 ms -- inside kLdsOctBytes, which the residency rule keeps.  The exit trees are worth less
// than a block, so their nodes must leave this count where it is.
constexpr size_t kLdsGranule = 1280, kLdsCuBytes = 160 * 1024;
static int lds_blocks_per_cu(const FlatScene &F, size_t scene_bytes)
{
    const size_t block = lds_block_bytes(F.depth < 8 ? 8 : 16, scene_bytes);   // the LDS plans' stack classes (frt_plans.hpp)
    return (int)(kLdsCuBytes / ((block + kLdsGranule - 1) / kLdsGranule * kLdsGranule));
}
// Do nn1 nodes instead of nn0 leave the scene on the plan it has (residency() reads these sizes)?
// same_blocks: ... and with as many blocks on a CU.
static bool keeps_plan(const FlatScene &F, int nn0, int nn1, bool same_blocks)
{
    const size_t rest = lds_rest(F);
    const size_t p0 = lds_planar_bytes(nn0, rest), p1 = lds_planar_bytes(nn1, rest);
    const size_t o0 = lds_octant_bytes(nn0, rest), o1 = lds_octant_bytes(nn1, rest);
    const bool lds0 = lds_planar_fits(p0), oct0 = !F.nodes_oct.empty();
    if (lds0 != lds_planar_fits(p1) || oct0 != lds_octant_fits(o1)) return false;
    if (!same_blocks) return true;
    if (lds0 && lds_blocks_per_cu(F, p1) != lds_blocks_per_cu(F, p0)) return false;
    return !oct0 || lds_blocks_per_cu(F, o1) == lds_blocks_per_cu(F, o0);
}

// F.nodes in the form host/ takes (16 floats per node), and such nodes adopted as the scene's: the
// nodes that were there stay in front, the octant copies are sized for the caller to fill again
static std::vector<float> node_floats(const std::vector<float4> &nodes)
{
    std::vector<float> v(4 * nodes.size());
    memcpy(v.data(), nodes.data(), sizeof(float4) * nodes.size());
    return v;
}
static std::vector<float4> node_records(const std::vector<float> &v)
{
    std::vector<float4> nodes(v.size() / 4);
    memcpy(nodes.data(), v.data(), sizeof(float) * v.size());
    return nodes;
}
static void adopt_nodes(FlatScene &F, const std::vector<float> &v)
{
    F.nodes = node_records(v);
    if (!F.nodes_oct.empty()) F.nodes_oct.resize(8 * F.nodes.size());
}

struct RefineLeaf { float box[6]; int ref; };   // lo xyz, hi xyz; the child ref as stored (~leaf)

// Every node of a node array -- the main tree and what the shadow and exit passes appended -- as one
// topology over the distinct leaves, numbered in (node, side) order of their first use; interior node
// i = slot n_leaves + i.  A tree that shares no leaf has nn + 1 of them and the root at slot n_leaves.
struct TreeView {
    frt_refine::Topology t;
    std::vector<RefineLeaf> leaves;
    std::unordered_map<int, int> leaf_of;   // leaf ref -> leaf

    explicit TreeView(const std::vector<float4> &nodes)
    {
        const int nn = (int)(nodes.size() / 4);
        t.child.assign(2 * (size_t)nn, 0);
        for (int i = 0; i < nn; ++i) {
            const float4 *n = &nodes[4 * i];
            const float b[2][6] = {{n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y}, {n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w}};
            for (int side = 0; side < 2; ++side) {
                const int c = f2i(side ? n[3].y : n[3].x);
                if (c >= 0) { t.child[2 * i + side] = ~c; continue; }   // a node: its slot once the leaves are counted
                const auto [it, fresh] = leaf_of.emplace(c, (int)leaves.size());
                if (fresh) {
                    RefineLeaf l;
                    for (int k = 0; k < 6; ++k) l.box[k] = b[side][k];
                    l.ref = c;
                    leaves.push_back(l);
                }
                t.child[2 * i + side] = it->second;
            }
        }
        t.n_leaves = (int)leaves.size();
        t.root = t.n_leaves;
        for (int &c : t.child)
            if (c < 0) c = t.n_leaves + ~c;
    }
    // the slot of a child ref or a root: a node index, or ~leaf
    int slot(int ref) const { return ref >= 0 ? t.n_leaves + ref : leaf_of.at(ref); }
    std::vector<int> leaves_under(int s) const
    {
        std::vector<int> under, st{s};
        while (!st.empty()) {
            const int x = st.back();
            st.pop_back();
            if (x < t.n_leaves) { under.push_back(x); continue; }
            st.push_back(t.child[2 * (x - t.n_leaves)]);
            st.push_back(t.child[2 * (x - t.n_leaves) + 1]);
        }
        return under;
    }
    bool same_leaves(const TreeView &o) const
    {
        return leaves.size() == o.leaves.size() &&
               std::equal(leaves.begin(), leaves.end(), o.leaves.begin(),
                          [](const RefineLeaf &a, const RefineLeaf &b) { return a.ref == b.ref; });
    }
};

// ---- the replay ----
// kRefineW, the price of a primitive test in node visits: the VALU instructions
// of one trip of leaf_hit's triangle loop over those of one node visit, both
// read from the disassembly of the octant plan's path kernel (path_megakernel
// <8, kWorldBvh2Oct, ...> of frt_render_lds.hip, the two innermost loops of
// its step loop).  A node visit is 31: the record and ref addresses (2), 12
// v_fma_f32, 8 v_maximum3 / v_minimum3, 4 compares, the select and store of
// the far child (3), the select of the near one (1) and the loop test (1).  A
// leaf trip whose triangle passes every stage of the Moller-Trumbore test --
// in a wave, a trip where any lane does -- is 56: the determinant (12), u (11),
// v (14), t and its interval (7), the hit update (8) and the loop count (4).
// 56 / 31 = 1.8.
constexpr double kRefineW = 1.8;
// The ray samples: host replays of path::Li (path_begin / path_shade, the code the
// kernel runs per lane) on a small frame of the scene's camera, one sample per
// pixel, fixed seeds.  The search fits on the first and the result is judged on
// the second, larger one, which it never saw.
constexpr int kRefineFitFrame = 24, kRefineValFrame = 40;
constexpr uint32_t kRefineFitSeed = 0x7ee5eed1u, kRefineValSeed = 0x7ee5eed2u;
constexpr int kRefineMaxDepth = 33;      // the renders' default max_depth
// Move evaluations per flatten, the pass's whole budget (no timer).  On Cornell
// (19 leaves) the first sweep over every (subtree, place) pair takes ~600 and
// finds all but a percent of the gain; 700 keep the pass under a frame's time
// (0.17 s on one core against 0.23 s for the 1080p, 512 spp frame).
constexpr int kRefineMaxEvals = 700;

// The rays of one replayed frame against the leaves.  Every ray is traced from the main root,
// whatever shadow and exit roots F holds: the sample is the same with those passes on and off.
struct Replay {
    frt_refine::RaySet R;
    std::vector<uint8_t> occl;    // per ray of R: 1 = an area-light shadow ray (light_shadow_ray)
    std::vector<int> from;        // per ray of R: the device triangle an extension ray leaves (the closest hit before
                                  // it), -1 for a camera ray, a shadow ray and a ray that leaves a sphere
    std::vector<float> origins;   // of the rays marked in occl, in R's order: 3 floats each
};
static Replay sample_rays(const FlatScene &F, const std::vector<RefineLeaf> &leaves, int frame, uint32_t seed)
{
    const DevScene S = host_scene(F);
    struct Ray { f3 o, d; float tmax; bool shadow, occl; int from; };
    std::vector<Ray> rays;
    std::vector<int> stack(std::max(F.depth + 1, 1));
    for (int pix = 0; pix < frame * frame; ++pix) {
        PathState<float> P;
        path_begin<kMatsAll>(P, S, pix % frame, pix / frame, frame, frame, seed, (uint32_t)pix, 0u);
        int last = -1;   // the primitive the path stands on
        for (;;) {
            rays.push_back(Ray{P.ro, P.rd, P.rtmax, P.shadow, light_shadow_ray(P),
                               (P.shadow || last < 0 || (last & FRT_PRIM_SPHERE)) ? -1 : last});
            const Hit<float> h = trace<FRT_WORLD_BVH, 1>(S, P.ro, P.rd, P.rtmax, P.shadow, stack.data(), light_shadow_ray(P));
            if (!P.shadow) last = h.prim;
            uint32_t n_ext = 0, n_sh = 0;
            if (path_shade<kMatsAll>(P, S, h, kRefineMaxDepth, n_ext, n_sh)) break;
        }
    }
    const int n = (int)rays.size(), nl = (int)leaves.size();
    Replay out;
    frt_refine::RaySet &R = out.R;
    R.n = n;
    R.n_leaves = nl;
    R.prim_first.assign(nl + 1, 0);
    for (int l = 0; l < nl; ++l) {
        const int lref = ~leaves[l].ref;
        const bool sph = (lref & FRT_PRIM_SPHERE) != 0;
        const int first = sph ? lref : (lref & kLeafIndexMask), count = sph ? 1 : (lref >> kLeafCountShift) + 1;
        for (int k = 0; k < count; ++k) R.prim_ref.push_back(first + k);
        R.prim_first[l + 1] = (int)R.prim_ref.size();
    }
    R.n_prims = (int)R.prim_ref.size();
    R.tmin.resize(n); R.tmax.resize(n); R.anyhit.resize(n); R.live.resize(n);
    out.occl.assign(n, 0);
    out.from.assign(n, -1);
    R.slab.resize((size_t)nl * n * 6);
    R.prim_t.resize((size_t)n * R.n_prims);
    // rays in a scattered order (a stride coprime to n), so that every chunk of the
    // sample holds every part of the frame and every bounce
    int stride = (int)(0.618 * n) | 1;
    auto gcd = [](int a, int b) { while (b) { const int c = a % b; a = b; b = c; } return a; };
    while (n > 1 && gcd(stride, n) != 1) stride += 2;
    for (int i = 0; i < n; ++i) {
        const Ray &q = rays[(int)(((int64_t)i * stride) % std::max(n, 1))];
        Trav<float> T;
        R.live[i] = trav_begin(T, S, S.root, q.o, q.d, q.tmax) ? 1 : 0;
        R.tmin[i] = T.tmin;
        R.tmax[i] = q.tmax;
        R.anyhit[i] = q.shadow ? 1 : 0;
        out.occl[i] = q.occl ? 1 : 0;
        out.from[i] = q.from;
        if (q.occl) out.origins.insert(out.origins.end(), {q.o.x, q.o.y, q.o.z});
        const float inv[3] = {T.sr.invd.x, T.sr.invd.y, T.sr.invd.z}, oi[3] = {T.sr.oinv.x, T.sr.oinv.y, T.sr.oinv.z};
        for (int l = 0; l < nl; ++l) {
            float *s = &R.slab[((size_t)i * nl + l) * 6];
            for (int a = 0; a < 3; ++a) {
                const bool neg = inv[a] < 0.0f;
                s[a] = vfma(leaves[l].box[neg ? 3 + a : a], inv[a], oi[a]);
                s[3 + a] = -vfma(leaves[l].box[neg ? a : 3 + a], inv[a], oi[a]);
            }
        }
        for (int k = 0; k < R.n_prims; ++k) {
            float u, v;
            R.prim_t[(size_t)i * R.n_prims + k] = prim_t(S, R.prim_ref[k], q.o, q.d, T.tmin, q.tmax, u, v);
        }
    }
    return out;
}

// ---- topology refinement of LDS-resident binary trees (DESIGN.md "Tree refinement") ----
// The interior nodes above the leaves of collapse_leaves are rearranged to
// lower the traversal cost J = V + w T (node visits and primitive tests per
// ray) of the rays the scene's own path integrator traces: the surface area
// heuristic prices rays uniform over the box, while these start on surfaces
// inside the scene and a third of them are shadow rays to the lights.  Leaves,
// their boxes and the device triangle ids (the DFS rank of the input tree) stay;
// an interior box becomes the union of its children's padded fp32 boxes, which
// bounds them.  The closest hit is the minimum of (t, device id) whatever the
// visit order and a shadow ray asks only whether a hit exists (collapse_leaves,
// trace_bvh), so every hit, film and ray count is unchanged -- only visits drop.

// F.nodes rewritten for topology t in pre-order: leaf boxes as they were, an
// interior child's box the union of its children's
static void write_topology(FlatScene &F, const frt_refine::Topology &t, const std::vector<RefineLeaf> &leaves)
{
    const int L = t.n_leaves, nn = L - 1;
    std::vector<float> box(6 * (size_t)(L + nn));
    std::function<void(int)> bound = [&](int s) {
        float *b = &box[6 * (size_t)s];
        if (s < L) { for (int k = 0; k < 6; ++k) b[k] = leaves[s].box[k]; return; }
        const int c0 = t.child[2 * (s - L)], c1 = t.child[2 * (s - L) + 1];
        bound(c0);
        bound(c1);
        for (int k = 0; k < 3; ++k) {
            b[k] = std::min(box[6 * (size_t)c0 + k], box[6 * (size_t)c1 + k]);
            b[3 + k] = std::max(box[6 * (size_t)c0 + 3 + k], box[6 * (size_t)c1 + 3 + k]);
        }
    };
    bound(t.root);
    std::vector<float4> out(4 * (size_t)nn);
    int next = 0;
    std::function<int(int)> emit = [&](int s) {   // returns the child ref of slot s
        if (s < L) return leaves[s].ref;
        const int me = next++;
        const int c[2] = {t.child[2 * (s - L)], t.child[2 * (s - L) + 1]};
        const float *a = &box[6 * (size_t)c[0]], *b = &box[6 * (size_t)c[1]];
        out[4 * me + 0] = make_float4(a[0], a[1], a[2], a[3]);
        out[4 * me + 1] = make_float4(a[4], a[5], b[0], b[1]);
        out[4 * me + 2] = make_float4(b[2], b[3], b[4], b[5]);
        const int r0 = emit(c[0]), r1 = emit(c[1]);
        out[4 * me + 3] = make_float4(i2f(r0), i2f(r1), 0.0f, 0.0f);
        return me;
    };
    emit(t.root);
    F.nodes.swap(out);
}

bool tree_cost_host(const FlatScene &F, TreeCost &out)
{
    out = TreeCost{};
    out.w = kRefineW;
    if (!tree_in_lds(F) || F.nodes.empty()) return false;
    const TreeView v(F.nodes);
    const Replay val = sample_rays(F, v.leaves, kRefineValFrame, kRefineValSeed);
    const frt_refine::Cost c = frt_refine::tree_cost(v.t, val.R);
    out.V = c.V; out.T = c.T; out.J = frt_refine::cost_j(c, kRefineW);
    out.depth = v.t.depth();
    out.n_rays = val.R.n;
    return true;
}

// The pass itself, on a finished FlatScene.  F.depth stays the input tree's: the
// refined tree is never deeper, and the stack class and launch plan chosen from
// it stay what they were.
bool refine_tree(FlatScene &F, int mode)
{
    const int nn = (int)(F.nodes.size() / 4);
    if (!pass_on(mode, "FRT_TREE_REFINE") || !tree_in_lds(F) || nn < 3) return false;
    const TreeView v(F.nodes);
    if (v.t.n_leaves != nn + 1) return false;   // a leaf named twice: write_topology numbers a tree
    frt_refine::Topology t = v.t;
    const Replay fit = sample_rays(F, v.leaves, kRefineFitFrame, kRefineFitSeed);
    if (frt_refine::refine(t, fit.R, kRefineW, v.t.depth(), kRefineMaxEvals) == 0) return false;
    // keep it only if the rays it was not fitted on agree
    const Replay val = sample_rays(F, v.leaves, kRefineValFrame, kRefineValSeed);
    const double j0 = frt_refine::cost_j(frt_refine::tree_cost(v.t, val.R), kRefineW);
    const double j1 = frt_refine::cost_j(frt_refine::tree_cost(t, val.R), kRefineW);
    if (!(j1 < j0)) return false;
    write_topology(F, t, v.leaves);
    return true;
}

// ---- the occluder tree of area-light shadow rays (DESIGN.md "Shadow tree") ----
// path::Li's and pssmlt::Li's shadow rays to a light are segments from a surface
// point to a point on a light.  host/shadow_tree.cpp proves for each triangle
// whether any such segment can report a hit on it (in a closed room: the walls no
// segment crosses, the light's own plane); the leaves that keep a primitive get a
// binary tree of their own, built from the main tree's nodes where a subtree lost
// nothing and appended behind them in F.nodes otherwise, and trav_begin starts
// those rays at its root.  Every other ray, and BVH4Q, keep the main root.  A
// shadow ray asks only whether a hit exists, so films and ray counts are
// unchanged -- only visits drop.

// sv's triangles in device order (tri_view) for the proofs of the shadow-tree and exit-tree passes,
// which name triangles as the leaves do
struct ProofGeometry {
    std::vector<double> tv, tn;
    std::vector<uint8_t> smooth;
    frt_shadow::Geometry g;
};
static void proof_geometry(const frt_scene_view *sv, const FlatScene &F, ProofGeometry &pg)
{
    const int nt = sv->n_tris;
    pg.tv.resize(9 * (size_t)nt);
    pg.smooth.assign(nt, 0);
    bool any_smooth = false;
    for (int d = 0; d < nt; ++d) {
        const int i = F.tri_view[d];
        std::copy(&sv->tri_v[9 * (size_t)i], &sv->tri_v[9 * (size_t)i] + 9, &pg.tv[9 * (size_t)d]);
        pg.smooth[d] = sv->tri_geometry_normal && !sv->tri_geometry_normal[i];
        any_smooth |= pg.smooth[d] != 0;
    }
    if (any_smooth) {
        pg.tn.resize(9 * (size_t)nt);
        for (int d = 0; d < nt; ++d)
            std::copy(&sv->tri_n[9 * (size_t)F.tri_view[d]], &sv->tri_n[9 * (size_t)F.tri_view[d]] + 9, &pg.tn[9 * (size_t)d]);
    }
    frt_shadow::Geometry &g = pg.g;
    g.n_tris = nt; g.n_spheres = sv->n_spheres;
    g.tri_v = pg.tv.data(); g.tri_n = any_smooth ? pg.tn.data() : nullptr; g.tri_smooth = pg.smooth.data();
    g.sphere = sv->sphere;
    g.lights = F.lights.data(); g.n_lights = (int)F.lights.size(); g.sphere_bit = FRT_PRIM_SPHERE;
    for (int k = 0; k < 3; ++k) { g.cam_o[k] = sv->cam_origin[k]; g.cam_u[k] = sv->cam_u[k]; g.cam_v[k] = sv->cam_v[k]; }
    g.lens_r = sv->cam_lens_radius;
    g.eps = (double)Cst<float>::eps;
}

bool shadow_tree(const frt_scene_view *sv, FlatScene &F, int mode)
{
    if (!pass_on(mode, "FRT_SHADOW_TREE")) return false;
    auto &I = F.shadow;
    DevScene &S = F.meta;
    auto why = [&](int w) { I.why = w; return w == FlatScene::kShadowRan; };
    I.nodes_main = (int)(F.nodes.size() / 4);
    if (sv->n_lights <= 0) return why(FlatScene::kShadowNoLights);
    if (!lambertian_only(sv)) return why(FlatScene::kShadowMaterial);
    if (!tree_in_lds(F) || F.nodes.empty()) return why(FlatScene::kShadowNotResident);
    ProofGeometry pg;
    proof_geometry(sv, F, pg);
    frt_shadow::Classified c;
    frt_shadow::classify(pg.g, c);
    if (c.why != frt_shadow::kRan)
        return why(c.why == frt_shadow::kNoLights ? FlatScene::kShadowNoLights : FlatScene::kShadowTooLarge);
    // triangles outside the tree (trailing device ids) are in no leaf; count those in one
    int n_dropped = 0;
    for (int d = 0; d < sv->n_tris; ++d) n_dropped += c.dropped[d];
    if (n_dropped == 0) return why(FlatScene::kShadowNothing);
    std::vector<float> nodes = node_floats(F.nodes);
    frt_shadow::Tree t;
    frt_shadow::build(nodes, S.root, c.dropped, FRT_PRIM_SPHERE, kLeafCountShift, t);
    if (t.dropped_leaves == 0) return why(FlatScene::kShadowNothing);
    if (!keeps_plan(F, I.nodes_main, (int)(nodes.size() / 16), false)) return why(FlatScene::kShadowBudget);
    adopt_nodes(F, nodes);
    S.sroot = t.empty ? kSentinel : t.root;   // nothing can occlude: the traversal ends at its first step
    I.dropped = c.dropped;
    I.n_dropped = n_dropped; I.rule_a = c.n_rule_a; I.rule_b = c.n_rule_b;
    I.added = t.added; I.shared = t.shared; I.empty = t.empty;
    return why(FlatScene::kShadowRan);
}

bool shadow_cost_host(const FlatScene &F, ShadowCost &out)
{
    out = ShadowCost{};
    if (F.shadow.why != FlatScene::kShadowRan) return false;
    const TreeView v(F.nodes);
    Replay val = sample_rays(F, v.leaves, kRefineValFrame, kRefineValSeed);
    frt_refine::RaySet &R = val.R;
    const std::vector<uint8_t> &occl = val.occl;
    int n_occl = 0;
    for (int i = 0; i < R.n; ++i) n_occl += occl[i];
    out.n_rays = n_occl;
    if (n_occl == 0) return true;
    auto price = [&](int which) {   // V and T of the rays marked live, per area-light shadow ray
        const frt_refine::Cost c = frt_refine::tree_cost(v.t, R);
        out.V[which] = c.V * R.n / n_occl;
        out.T[which] = c.T * R.n / n_occl;
    };
    // from the main root: the area-light shadow rays alone, those that miss the scene's box stopped there
    for (int i = 0; i < R.n; ++i) {
        R.live[i] = R.live[i] && occl[i];
        if (occl[i] && !R.live[i]) ++out.stops[0];
    }
    price(0);
    // from the shadow root.  trav_begin tests no box there, so every such ray is live; a ray that would
    // miss the box of the shadow tree's leaves costs its one visit and is reported as a stop
    if (F.shadow.empty) {   // kSentinel: done at the first step
        out.stops[1] = n_occl;
        return true;
    }
    const int sroot = v.slot(F.meta.sroot);
    const std::vector<int> under = v.leaves_under(sroot);
    auto misses_box = [&](int i) {   // the union of the leaves' slab records against trav_begin's interval
        float u[6];
        for (int k = 0; k < 6; ++k) u[k] = __builtin_inff();
        for (int l : under)
            for (int k = 0; k < 6; ++k) u[k] = std::min(u[k], R.slab[((size_t)i * R.n_leaves + l) * 6 + k]);
        const float tn = std::max(std::max(u[0], u[1]), std::max(u[2], Cst<float>::eps));
        const float tf = std::min(std::min(-u[3], -u[4]), std::min(-u[5], R.tmax[i]));
        return !(tn <= tf);
    };
    R.root.assign(R.n, sroot);
    for (int i = 0; i < R.n; ++i) {
        R.live[i] = occl[i];
        if (occl[i] && misses_box(i)) ++out.stops[1];
    }
    price(1);
    return true;
}

void shadow_origins_host(const FlatScene &F, std::vector<float> &origins)
{
    origins.clear();
    if (F.meta.world_kind != FRT_WORLD_BVH || F.nodes.empty()) return;
    origins = sample_rays(F, TreeView(F.nodes).leaves, kRefineValFrame, kRefineValSeed).origins;
}

// ---- the trees extension rays start at (DESIGN.md "Exit trees") ----
// An extension ray of a lambertian vertex leaves its triangle on the stored normal's side and
// climbs from there; its origin lies inside the box of the leaf it leaves and of every ancestor, so
// from the main root the first leaf it reaches is its own, two triangles in the plane it has just
// left.  host/exit_tree.cpp proves per origin triangle which triangles such a ray cannot report a
// hit on; per main-tree leaf the largest subtree made of those alone is its drop set (a wall: its
// own leaf; a face of a box: the box's subtree where the tree groups the box), and the main tree
// without it -- frt_shadow::build's rules, the copied ancestors appended behind the main and shadow
// nodes -- is where trav_begin starts those rays.  The root's node index goes into the third word of
// the triangle's second shading record (0 = the main root).  Closest hits are unchanged, so films
// and ray counts are; only visits and triangle tests drop.  Among the distinct drop sets the pass
// takes, greedily, those with the largest fall of J = V + kRefineW T on the refinement pass's
// fitting replay per appended node, while the appended nodes leave the scene on the LDS plan it has
// and the CU its blocks (keeps_plan).
constexpr int kExitMaxRoot = 1 << 10;   // node indices the kernels carry above PathState::depth (kExitShift)

bool exit_tree(const frt_scene_view *sv, FlatScene &F, int mode)
{
    if (!pass_on(mode, "FRT_EXIT_TREE")) return false;
    auto &I = F.exit;
    DevScene &S = F.meta;
    auto why = [&](int w) { I.why = w; return w == FlatScene::kExitRan; };
    I.nodes_before = (int)(F.nodes.size() / 4);
    I.root.assign((size_t)std::max(sv->n_tris, 0), 0);
    if (!lambertian_only(sv)) return why(FlatScene::kExitMaterial);
    if (!tree_in_lds(F) || F.nodes.empty() || S.root != 0) return why(FlatScene::kExitNotResident);
    ProofGeometry pg;
    proof_geometry(sv, F, pg);
    frt_exit::Hidden hid;
    frt_exit::classify(pg.g, hid);
    if (hid.why != frt_exit::kRan) return why(FlatScene::kExitTooLarge);
    std::vector<float> nodes = node_floats(F.nodes);
    std::vector<frt_exit::Class> cls;
    frt_exit::classes(nodes, S.root, FRT_PRIM_SPHERE, kLeafCountShift, hid, cls);
    I.classes = (int)cls.size();
    if (cls.empty()) return why(FlatScene::kExitNothing);

    // the fitting replay against the leaves, with the triangle every extension ray leaves
    const TreeView v0(F.nodes);
    Replay fit = sample_rays(F, v0.leaves, kRefineFitFrame, kRefineFitSeed);
    frt_refine::RaySet &R = fit.R;
    const std::vector<uint8_t> live0 = R.live;

    // each class alone: its tree on a copy of the nodes, the nodes it appends and the fall of J
    struct Cand { int cls, added; double gain; };
    std::vector<Cand> cand;
    for (int c = 0; c < (int)cls.size(); ++c) {
        std::vector<float> trial = nodes;
        frt_shadow::Tree t;
        frt_shadow::build(trial, S.root, cls[c].dropped, FRT_PRIM_SPHERE, kLeafCountShift, t);
        if (t.empty || t.root <= 0 || t.root >= kExitMaxRoot || t.dropped_leaves == 0) continue;
        const TreeView v(node_records(trial));
        if (!v.same_leaves(v0)) continue;   // (appended nodes name the main tree's leaves only)
        bool any = false;
        for (int i = 0; i < R.n; ++i) {
            const int from = fit.from[i];
            const bool mine = from >= 0 && std::binary_search(cls[c].members.begin(), cls[c].members.end(), from);
            R.live[i] = live0[i] && mine;
            any |= R.live[i] != 0;
        }
        if (!any) continue;
        R.root.clear();
        const double j0 = frt_refine::cost_j(frt_refine::tree_cost(v.t, R), kRefineW);
        R.root.assign(R.n, v.slot(t.root));
        const double j1 = frt_refine::cost_j(frt_refine::tree_cost(v.t, R), kRefineW);
        if (j1 < j0) cand.push_back(Cand{c, t.added, j0 - j1});
    }
    if (cand.empty()) return why(FlatScene::kExitNothing);
    // by gain per appended node (a tree that appends nothing first), then gain, then class order
    std::stable_sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) {
        if ((a.added == 0) != (b.added == 0)) return a.added == 0;
        const double ra = a.gain / std::max(a.added, 1), rb = b.gain / std::max(b.added, 1);
        if (ra != rb) return ra > rb;
        return a.gain > b.gain;
    });
    bool refused = false;
    for (const Cand &k : cand) {
        const frt_exit::Class &c = cls[k.cls];
        std::vector<float> next = nodes;
        frt_shadow::Tree t;
        frt_shadow::build(next, S.root, c.dropped, FRT_PRIM_SPHERE, kLeafCountShift, t);
        if (!keeps_plan(F, I.nodes_before, (int)(next.size() / 16), true) || t.root >= kExitMaxRoot) { refused = true; continue; }
        nodes.swap(next);
        for (int d : c.members) I.root[d] = t.root;
        I.taken.push_back({c.sub, t.root, (int)c.members.size(), c.n_dropped, t.added, t.shared, k.gain});
        I.added += t.added;
    }
    if (I.taken.empty()) return why(refused ? FlatScene::kExitBudget : FlatScene::kExitNothing);
    I.budget_refused = refused;
    adopt_nodes(F, nodes);
    for (size_t d = 0; d < I.root.size(); ++d)
        if (I.root[d]) F.tshade[2 * d + 1].z = i2f(I.root[d]);
    return why(FlatScene::kExitRan);
}

bool exit_cost_host(const FlatScene &F, ExitCost &out)
{
    out = ExitCost{};
    if (!tree_in_lds(F) || F.nodes.empty()) return false;
    const TreeView v(F.nodes);
    Replay val = sample_rays(F, v.leaves, kRefineValFrame, kRefineValSeed);
    frt_refine::RaySet &R = val.R;
    const std::vector<uint8_t> &occl = val.occl;
    const std::vector<int> &from = val.from;
    const DevScene &S = F.meta;
    const std::vector<uint8_t> live0 = R.live;
    out.n_rays = R.n;
    for (int i = 0; i < R.n; ++i) out.n_ext += from[i] >= 0;
    for (int on = 0; on < 2; ++on) {
        // every ray where the kernels start it: area-light shadow rays at the shadow root (trav_begin
        // tests no box there; an empty shadow tree ends them at once), extension rays at their exit root
        R.root.assign(R.n, v.t.root);
        R.live = live0;
        for (int i = 0; i < R.n; ++i) {
            if (occl[i] && S.sroot != S.root) {
                if (S.sroot == kSentinel) R.live[i] = 0;
                else { R.root[i] = v.slot(S.sroot); R.live[i] = 1; }
            } else if (on && from[i] >= 0 && from[i] < (int)F.exit.root.size() && F.exit.root[from[i]]) {
                R.root[i] = v.slot(F.exit.root[from[i]]);
            }
        }
        const frt_refine::Cost all = frt_refine::tree_cost(v.t, R);
        out.V_all[on] = all.V; out.T_all[on] = all.T; out.J_all[on] = frt_refine::cost_j(all, kRefineW);
        for (int i = 0; i < R.n; ++i) R.live[i] = R.live[i] && from[i] >= 0;
        const frt_refine::Cost ext = frt_refine::tree_cost(v.t, R);
        if (out.n_ext > 0) { out.V_ext[on] = ext.V * R.n / out.n_ext; out.T_ext[on] = ext.T * R.n / out.n_ext; }
    }
    return true;
}
