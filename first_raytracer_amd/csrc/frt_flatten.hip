// frt_flatten.hip -- scene flattening on the host: DFS order, fp32 conversion
// with outward-rounded boxes, multi-triangle leaves, the 4-wide quantized tree
// (BVH4Q), the octant node copies, the texel conversion and the topology
// refinement of LDS-resident trees (refine_tree).  No kernel and no
// HIP runtime call; built with the kernel units' compiler and flags so that
// its floating-point results do not depend on which unit holds it.  Also the
// shadow-tree pass (shadow_tree): the occluder tree of area-light shadow rays
// appended behind the main nodes, and the exit-tree pass (exit_tree): the
// trees extension rays start at, behind those.
#include "frt_flatten.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>

#include "frt_kernels.hpp"   // the LDS budgets (kLdsSceneBytes, kLdsOctBytes, kLdsMaxDepth, oct_lds_node_slots)
#include "host/exit_tree.hpp"
#include "host/shadow_tree.hpp"
#include "host/tree_refine.hpp"

using namespace frt;

// ---- scene flattening: DFS order, fp32 conversion with outward-rounded boxes ----
static inline float round_down(double x)
{
    float f = (float)x;
    if ((double)f > x) f = std::nextafter(f, -INFINITY);
    return f;
}
static inline float round_up(double x)
{
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
}

// Triangles per leaf: FRT_LEAF_SIZE overrides (1 = the reference's one-prim
// leaves), else 0 = by plan (see flatten_scene).  A tuning knob of this
// library, not part of the C-ABI.
static int leaf_size_override()
{
    const char *e = std::getenv("FRT_LEAF_SIZE");
    return e ? std::min(std::max(std::atoi(e), 1), kLeafMax) : 0;
}

// Multi-triangle leaves: every subtree of the DFS-ordered binary tree holding
// only triangles, at most `leaf_max` of them, becomes one leaf.  Its triangles
// are the contiguous device ids [first, first + count) (device id = DFS rank).
// The closest hit over triangles is the lexicographic minimum of (t, DFS rank)
// whatever the visit order (the tie rule in trace_bvh), and the parent's box
// already bounds the subtree, so hits are unchanged -- only node visits drop.
static void collapse_leaves(FlatScene &F, int leaf_max)
{
    const int nn = (int)(F.nodes.size() / 4);
    if (leaf_max <= 1 || nn == 0) return;
    auto child = [&](int i, int side) { return f2i(side ? F.nodes[4 * i + 3].y : F.nodes[4 * i + 3].x); };
    // subtree triangle count / first device id / holds a sphere; children follow parents in pre-order
    std::vector<int> cnt(nn, 0), first(nn, INT32_MAX);
    std::vector<char> sph(nn, 0);
    for (int i = nn - 1; i >= 0; --i)
        for (int side = 0; side < 2; ++side) {
            const int c = child(i, side);
            if (c >= 0) {
                cnt[i] += cnt[c]; first[i] = std::min(first[i], first[c]); sph[i] |= sph[c];
            } else if (~c & FRT_PRIM_SPHERE) {
                sph[i] = 1;
            } else {
                cnt[i] += 1; first[i] = std::min(first[i], ~c);
            }
        }
    std::vector<float4> out;
    out.reserve(F.nodes.size());
    int depth = 0;
    // pre-order rebuild; (old node, slot in `out` of the parent's child ref or -1, level)
    struct Item { int old, parent_slot, side, lvl; };
    std::vector<Item> st{{0, -1, 0, 1}};
    while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        const int me = (int)(out.size() / 4);
        if (it.parent_slot >= 0) {
            float4 &r = out[it.parent_slot];
            (it.side ? r.y : r.x) = i2f(me);
        }
        depth = std::max(depth, it.lvl);
        for (int k = 0; k < 4; ++k) out.push_back(F.nodes[4 * it.old + k]);
        const int slot = 4 * me + 3;
        for (int side = 1; side >= 0; --side) {
            const int c = child(it.old, side);
            if (c < 0) continue;                                  // leaf ref kept as is
            if (!sph[c] && cnt[c] <= leaf_max) {
                float4 &r = out[slot];
                (side ? r.y : r.x) = i2f(~(first[c] | ((cnt[c] - 1) << kLeafCountShift)));
            } else {
                st.push_back({c, slot, side, it.lvl + 1});
            }
        }
    }
    F.nodes.swap(out);
    F.depth = depth;
}

// 4-wide quantized BVH (DESIGN.md "BVH4Q") from the binary tree after
// collapse_leaves: each 4-wide node takes the descendants of its binary node
// that minimise the summed box area of the 4-wide nodes below it (an exact
// dynamic programme over the binary tree, after Ylitie, Karras & Laine 2017;
// round 5, replacing "open the interior child of largest area until four":
// cornell_1m +0.4 %, 23 % fewer nodes).  Child boxes are the binary tree's padded fp32 boxes quantized to 8
// bits per plane on a per-node power-of-two grid, rounded outward.  Nodes in
// depth-first pre-order (a node's first interior child follows it; sibling
// blocks and a breadth-first order measured the same).
// Returns false (no BVH4; the binary tree is used) when a node's grid would
// overflow the slab arithmetic.
static bool build_bvh4(FlatScene &F, int root_ref)
{
    F.nodes4.clear();
    F.depth4 = 0;
    F.root4 = root_ref;
    const int nn = (int)(F.nodes.size() / 4);
    if (nn == 0 || root_ref < 0) return true;
    struct Child { float lo[3], hi[3]; int ref; };
    auto kids = [&](int i, Child *out) {
        const float4 a = F.nodes[4 * i], b = F.nodes[4 * i + 1], c = F.nodes[4 * i + 2], r = F.nodes[4 * i + 3];
        out[0] = Child{{a.x, a.y, a.z}, {a.w, b.x, b.y}, f2i(r.x)};
        out[1] = Child{{b.z, b.w, c.x}, {c.y, c.z, c.w}, f2i(r.y)};
    };
    auto area = [](const Child &c) {
        const double dx = (double)c.hi[0] - c.lo[0], dy = (double)c.hi[1] - c.lo[1], dz = (double)c.hi[2] - c.lo[2];
        return dx * dy + dy * dz + dz * dx;
    };
    // empty slots: the inverted box q_lo = 255 > q_hi = 0 on every axis,
    // which the near / far slab test rejects -- except on a node so small
    // against its distance from the ray origin that each axis' planes round
    // to one value (then a real child's hit has tn == tf and must stay a hit,
    // so the test cannot reject it either; ADVICE r2,
    // test_bvh4_tiny_far_nodes).  Their ref is a one-primitive leaf of the
    // scene's first primitive: a spurious visit re-tests a real primitive,
    // which cannot change a closest hit (same t, same DFS rank) or an any-hit
    // answer, and needs no per-child ref compare in the node loop (that
    // compare cost 2 % on cornell_1m).
    const uint32_t empty_ref = (uint32_t)~(F.tris.empty() ? FRT_PRIM_SPHERE : 0);
    // Area-optimal collapse: per binary node n, T[n] = the summed box area of the
    // 4-wide nodes that represent n's subtree when n takes one slot (n becomes a
    // node), D[n][j] the least such sum when n's subtree fills at most j slots of
    // its parent (n opened); the leaves are fixed, so the sum of node areas is
    // the whole SAH difference between two collapses.  Children follow parents
    // in pre-order, so one backward sweep fills the tables.
    std::vector<double> T(nn, 0.0), D(5 * (size_t)nn, 0.0);
    std::vector<signed char> split(5 * (size_t)nn, 1);
    auto slot_cost = [&](const Child &c, int k) {   // c in at most k slots
        if (c.ref < 0) return 0.0;
        return k >= 2 ? std::min(T[c.ref], D[5 * (size_t)c.ref + k]) : T[c.ref];
    };
    {
        std::vector<double> own(nn, 0.0);   // a node's own box area, from its parent's record
        for (int i = 0; i < nn; ++i) {
            Child two[2];
            kids(i, two);
            for (int s = 0; s < 2; ++s) if (two[s].ref >= 0) own[two[s].ref] = area(two[s]);
        }
        for (int i = nn - 1; i >= 0; --i) {
            Child two[2];
            kids(i, two);
            for (int j = 2; j <= 4; ++j) {
                double best = 1e300;
                for (int k = 1; k < j; ++k) {
                    const double v = slot_cost(two[0], k) + slot_cost(two[1], j - k);
                    if (v < best) { best = v; split[5 * (size_t)i + j] = (signed char)k; }
                }
                D[5 * (size_t)i + j] = best;
            }
            T[i] = own[i] + D[5 * (size_t)i + 4];
        }
    }
    std::function<void(const Child &, int, Child *, int &)> gather = [&](const Child &c, int k, Child *out, int &n) {
        if (c.ref < 0 || k < 2 || !(D[5 * (size_t)c.ref + k] < T[c.ref])) { out[n++] = c; return; }
        Child two[2];
        kids(c.ref, two);
        const int kl = split[5 * (size_t)c.ref + k];
        gather(two[0], kl, out, n);
        gather(two[1], k - kl, out, n);
    };
    struct Item { int bin, parent, slot, lvl; };   // binary node, wide parent (-1 root), child slot, level
    std::vector<Item> st{{root_ref, -1, 0, 1}};
    while (!st.empty()) {
        const Item it = st.back();
        st.pop_back();
        const int me = (int)(F.nodes4.size() / kNode4Parts);
        if (it.parent >= 0) {
            uint4 &r = F.nodes4[(size_t)kNode4Parts * it.parent + 1];
            (it.slot == 0 ? r.x : it.slot == 1 ? r.y : it.slot == 2 ? r.z : r.w) = (uint32_t)me;
        }
        F.depth4 = std::max(F.depth4, it.lvl);
        Child ch[4], two[2];   // slots in left-to-right order
        int n = 0;
        kids(it.bin, two);
        const int kl = split[5 * (size_t)it.bin + 4];
        gather(two[0], kl, ch, n);
        gather(two[1], 4 - kl, ch, n);
        // per-axis grid: origin = min child lo, step 2^e with every plane within 255 steps
        float org[3];
        int ex[3];
        uint32_t qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
        for (int a = 0; a < 3; ++a) {
            float lo = ch[0].lo[a], hi = ch[0].hi[a];
            for (int k = 1; k < n; ++k) { lo = std::min(lo, ch[k].lo[a]); hi = std::max(hi, ch[k].hi[a]); }
            org[a] = lo;
            const double ext = (double)hi - (double)lo;
            int e = -126;
            if (ext > 0.0) {
                std::frexp(ext / 255.0, &e);            // ext / 255 <= 2^e
                e = std::max(e, -126);
                while (e > -126 && std::ldexp(255.0, e - 1) >= ext) --e;
            }
            if (e > 20) return false;                  // 2^e / |d| must stay finite (|1/d| <= 1e30)
            if (e < -100) return false;                // 2^e / |d| must stay a normal float for the empty-slot
                                                       // test (padded boxes are never this thin)
            ex[a] = e;
            for (int s = 0; s < 4; ++s) {
                double ql = 255.0, qh = 0.0;           // empty slot: the inverted box
                if (s < n) {
                    const Child &c = ch[s];
                    ql = std::floor(((double)c.lo[a] - lo) / std::ldexp(1.0, e));
                    qh = std::ceil(((double)c.hi[a] - lo) / std::ldexp(1.0, e));
                    ql = std::min(std::max(ql, 0.0), 255.0);
                    qh = std::min(std::max(qh, 0.0), 255.0);
                    // outward: the decoded plane must enclose the fp32 box (exact in double)
                    while (ql > 0.0 && (double)lo + ql * std::ldexp(1.0, e) > (double)c.lo[a]) ql -= 1.0;
                    while (qh < 255.0 && (double)lo + qh * std::ldexp(1.0, e) < (double)c.hi[a]) qh += 1.0;
                }
                qlo[a] |= (uint32_t)ql << (8 * s);
                qhi[a] |= (uint32_t)qh << (8 * s);
            }
        }
        uint32_t refs[4];
        for (int s = 0; s < 4; ++s) refs[s] = s < n ? (uint32_t)ch[s].ref : empty_ref;
        F.nodes4.resize((size_t)(me + 1) * kNode4Parts);
        uint4 *out = F.nodes4.data() + (size_t)me * kNode4Parts;
        out[0] = make_uint4((uint32_t)f2i(org[0]), (uint32_t)f2i(org[1]), (uint32_t)f2i(org[2]),
                            ((uint32_t)ex[0] & 0xffu) | (((uint32_t)ex[1] & 0xffu) << 8) | (((uint32_t)ex[2] & 0xffu) << 16));
        out[1] = make_uint4(refs[0], refs[1], refs[2], refs[3]);
        out[2] = make_uint4(qlo[0], qhi[0], qlo[1], qhi[1]);
        out[3] = make_uint4(qlo[2], qhi[2], 0u, 0u);
        for (int s = n - 1; s >= 0; --s)               // pre-order: the first slot next
            if (ch[s].ref >= 0) st.push_back({ch[s].ref, me, s, it.lvl + 1});
    }
    F.root4 = 0;
    return true;
}

// f64: also build the fp64 records of the fp64 kernels (DESIGN.md "Precision")
// image_texture texels: the reference's value per texel (texture.h:76-87: the float of an
// HDR image, FromSrgb(byte / 255.0) in double otherwise, util.h:62-66) rounded to fp32,
// appended to `out` (scene textures and the environment image)
static void append_texels(const frt_image &im, std::vector<float4> &out)
{
    const size_t n = (size_t)im.nx * im.ny;
    auto srgb = [](double v) { return v <= 0.04045 ? v * (1.0 / 12.92) : std::pow((v + 0.055) * (1.0 / 1.055), 2.4); };
    for (size_t q = 0; q < n; ++q) {
        double c[3];
        for (int ch = 0; ch < 3; ++ch)
            c[ch] = im.format == FRT_IMAGE_F32 ? (double)static_cast<const float *>(im.data)[3 * q + ch]
                                               : srgb(static_cast<const uint8_t *>(im.data)[3 * q + ch] / 255.0);
        out.push_back(make_float4((float)c[0], (float)c[1], (float)c[2], 0.0f));
    }
}
// frt_set_env_image / the self-test: validate the image and convert it.  PSS-MLT's
// splats assume contributions >= 0, so negative and non-finite texels are refused.
int env_texels_of(const frt_image *img, std::vector<float4> &out, std::string &err)
{
    if (img->nx <= 0 || img->ny <= 0) { err = "environment image: nx and ny must be positive"; return FRT_E_INVALID; }
    if (!img->data) { err = "environment image: null data"; return FRT_E_INVALID; }
    if (img->format != FRT_IMAGE_SRGB8 && img->format != FRT_IMAGE_F32) {
        err = "environment image: format must be FRT_IMAGE_SRGB8 or FRT_IMAGE_F32";
        return FRT_E_INVALID;
    }
    if ((size_t)img->nx * img->ny > (size_t)INT32_MAX) { err = "environment image larger than 2^31 texels"; return FRT_E_UNSUPPORTED; }
    out.clear();
    out.reserve((size_t)img->nx * img->ny);
    append_texels(*img, out);
    for (size_t q = 0; q < out.size(); ++q) {
        const float v[3] = {out[q].x, out[q].y, out[q].z};
        for (int ch = 0; ch < 3; ++ch)
            if (!(v[ch] >= 0.0f && v[ch] <= FLT_MAX)) {
                err = "environment image: texel (" + std::to_string(q % img->nx) + ", " + std::to_string(q / img->nx) +
                      ") is negative or not finite";
                return FRT_E_INVALID;
            }
    }
    return FRT_OK;
}

// octant copies of the binary nodes (when flatten_scene sized them): child boxes as (near xyz, far xyz)
static void fill_octants(FlatScene &F)
{
    for (int o = 0; o < 8 && !F.nodes_oct.empty(); ++o)
        for (size_t i = 0; i < F.nodes.size() / 4; ++i) {
            const float4 *n = &F.nodes[4 * i];
            const float b0[6] = {n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y};
            const float b1[6] = {n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w};
            float q[12];
            for (int a = 0; a < 3; ++a) {
                const bool neg = (o >> a) & 1;
                q[a] = neg ? b0[3 + a] : b0[a];
                q[3 + a] = neg ? b0[a] : b0[3 + a];
                q[6 + a] = neg ? b1[3 + a] : b1[a];
                q[9 + a] = neg ? b1[a] : b1[3 + a];
            }
            float4 *d = &F.nodes_oct[(size_t)o * F.nodes.size() + 4 * i];
            d[0] = make_float4(q[0], q[1], q[2], q[3]);
            d[1] = make_float4(q[4], q[5], q[6], q[7]);
            d[2] = make_float4(q[8], q[9], q[10], q[11]);
            d[3] = n[3];
        }
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
//
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

static bool tree_refine_knob()
{
    const char *e = std::getenv("FRT_TREE_REFINE");
    return !(e && std::atoi(e) == 0);
}

// does the residency rule (frt_ctx.hpp pick_*) put this scene's binary tree in LDS?
static bool tree_in_lds(const FlatScene &F)
{
    if (F.meta.world_kind != FRT_WORLD_BVH || F.meta.root < 0 || F.depth >= kLdsMaxDepth) return false;
    const size_t bytes = sizeof(float4) * (F.nodes.size() + F.tris.size() + F.tshade.size() + F.mats.size());
    return bytes <= kLdsSceneBytes || !F.nodes_oct.empty();
}

struct RefineLeaf { float box[6]; int ref; };   // lo xyz, hi xyz; the child ref as stored (~leaf)

// the binary nodes as a topology over their leaves (interior node i = slot n_leaves + i)
static void topology_of(const std::vector<float4> &nodes, frt_refine::Topology &t, std::vector<RefineLeaf> &leaves)
{
    const int nn = (int)(nodes.size() / 4);
    leaves.clear();
    t.child.assign(2 * (size_t)nn, 0);
    t.n_leaves = nn + 1;
    t.root = t.n_leaves;
    for (int i = 0; i < nn; ++i) {
        const float4 *n = &nodes[4 * i];
        const float b[2][6] = {{n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y}, {n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w}};
        for (int side = 0; side < 2; ++side) {
            const int c = f2i(side ? n[3].y : n[3].x);
            if (c >= 0) { t.child[2 * i + side] = t.n_leaves + c; continue; }
            RefineLeaf l;
            for (int k = 0; k < 6; ++k) l.box[k] = b[side][k];
            l.ref = c;
            t.child[2 * i + side] = (int)leaves.size();
            leaves.push_back(l);
        }
    }
}

// the rays of one replayed frame against the leaves
// occl (optional): per ray of R, 1 = an area-light shadow ray (light_shadow_ray)
// from (optional): per ray of R, the device triangle an extension ray leaves (the closest hit before
// it), -1 for a camera ray, a shadow ray and a ray that leaves a sphere.  Every ray is traced from
// the main root here, whatever exit roots F holds: the sample is the same with the pass on and off.
static void sample_rays(const FlatScene &F, const std::vector<RefineLeaf> &leaves, int frame, uint32_t seed,
                        frt_refine::RaySet &R, std::vector<uint8_t> *occl = nullptr, std::vector<float> *origins = nullptr,
                        std::vector<int> *from = nullptr)
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
    R = frt_refine::RaySet{};
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
    if (occl) occl->assign(n, 0);
    if (from) from->assign(n, -1);
    if (origins) origins->clear();
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
        if (occl) (*occl)[i] = q.occl ? 1 : 0;
        if (from) (*from)[i] = q.from;
        if (origins && q.occl) { origins->push_back(q.o.x); origins->push_back(q.o.y); origins->push_back(q.o.z); }
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
}

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
    frt_refine::Topology t;
    std::vector<RefineLeaf> leaves;
    topology_of(F.nodes, t, leaves);
    frt_refine::RaySet val;
    sample_rays(F, leaves, kRefineValFrame, kRefineValSeed, val);
    const frt_refine::Cost c = frt_refine::tree_cost(t, val);
    out.V = c.V; out.T = c.T; out.J = frt_refine::cost_j(c, kRefineW);
    out.depth = t.depth();
    out.n_rays = val.n;
    return true;
}

// The pass itself, on a finished FlatScene.  True when F.nodes changed (the
// caller makes the octant copies and BVH4Q again).  F.depth stays the input
// tree's: the refined tree is never deeper, and the stack class and launch plan
// chosen from it stay what they were.
static bool refine_tree(FlatScene &F)
{
    if (!tree_in_lds(F) || F.nodes.size() / 4 < 3) return false;
    frt_refine::Topology t;
    std::vector<RefineLeaf> leaves;
    topology_of(F.nodes, t, leaves);
    const frt_refine::Topology input = t;
    frt_refine::RaySet fit;
    sample_rays(F, leaves, kRefineFitFrame, kRefineFitSeed, fit);
    if (frt_refine::refine(t, fit, kRefineW, input.depth(), kRefineMaxEvals) == 0) return false;
    // keep it only if the rays it was not fitted on agree
    frt_refine::RaySet val;
    sample_rays(F, leaves, kRefineValFrame, kRefineValSeed, val);
    const double j0 = frt_refine::cost_j(frt_refine::tree_cost(input, val), kRefineW);
    const double j1 = frt_refine::cost_j(frt_refine::tree_cost(t, val), kRefineW);
    if (!(j1 < j0)) return false;
    write_topology(F, t, leaves);
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
static bool shadow_tree_knob()
{
    const char *e = std::getenv("FRT_SHADOW_TREE");
    return !(e && std::atoi(e) == 0);
}

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

// sv's triangles in device order (tri_view) for the proof, which names triangles as the leaves do
static void shadow_tree(const frt_scene_view *sv, FlatScene &F)
{
    auto &I = F.shadow;
    DevScene &S = F.meta;
    I.nodes_main = (int)(F.nodes.size() / 4);
    if (sv->n_lights <= 0) { I.why = FlatScene::kShadowNoLights; return; }
    // dielectric and the specular lobes leave from p - eps n: only lambertian / diffuse_light scenes
    for (int i = 0; i < sv->n_materials; ++i)
        if (sv->materials[i].type != FRT_MAT_LAMBERTIAN && sv->materials[i].type != FRT_MAT_DIFFUSE_LIGHT) {
            I.why = FlatScene::kShadowMaterial;
            return;
        }
    if (!tree_in_lds(F) || F.nodes.empty()) { I.why = FlatScene::kShadowNotResident; return; }
    const int nt = sv->n_tris;
    ProofGeometry pg;
    proof_geometry(sv, F, pg);
    const frt_shadow::Geometry &g = pg.g;
    frt_shadow::Classified c;
    frt_shadow::classify(g, c);
    if (c.why != frt_shadow::kRan) {
        I.why = c.why == frt_shadow::kNoLights ? FlatScene::kShadowNoLights : FlatScene::kShadowTooLarge;
        return;
    }
    // triangles outside the tree (trailing device ids) are in no leaf; count those in one
    int n_dropped = 0;
    for (int d = 0; d < nt; ++d) n_dropped += c.dropped[d];
    if (n_dropped == 0) { I.why = FlatScene::kShadowNothing; return; }
    std::vector<float> nodes(4 * F.nodes.size());
    memcpy(nodes.data(), F.nodes.data(), sizeof(float4) * F.nodes.size());
    frt_shadow::Tree t;
    frt_shadow::build(nodes, S.root, c.dropped, FRT_PRIM_SPHERE, kLeafCountShift, t);
    if (t.dropped_leaves == 0) { I.why = FlatScene::kShadowNothing; return; }
    // the appended nodes must leave the scene on the plan it has (pick_launcher_t reads these sizes)
    const size_t rest = F.tris.size() + F.tshade.size() + F.mats.size();
    const int nn0 = I.nodes_main, nn1 = (int)(nodes.size() / 16);
    const bool lds0 = sizeof(float4) * (4 * (size_t)nn0 + rest) <= kLdsSceneBytes;
    const bool lds1 = sizeof(float4) * (4 * (size_t)nn1 + rest) <= kLdsSceneBytes;
    const bool oct0 = !F.nodes_oct.empty();
    const bool oct1 = sizeof(float4) * (oct_lds_node_slots(nn1) + rest) <= kLdsOctBytes;
    if (lds0 != lds1 || oct0 != oct1) { I.why = FlatScene::kShadowBudget; return; }
    F.nodes.resize((size_t)4 * nn1);
    memcpy(F.nodes.data(), nodes.data(), sizeof(float) * nodes.size());
    if (oct0) F.nodes_oct.resize(8 * F.nodes.size());
    S.sroot = t.empty ? kSentinel : t.root;   // nothing can occlude: the traversal ends at its first step
    I.why = FlatScene::kShadowRan;
    I.dropped = c.dropped;
    I.n_dropped = n_dropped; I.rule_a = c.n_rule_a; I.rule_b = c.n_rule_b;
    I.added = t.added; I.shared = t.shared; I.empty = t.empty;
}

// every node of F.nodes -- the main tree and the shadow tree's own -- as one topology over the
// distinct leaves; slot_of_ref(ref) names a root
static void topology_all(const std::vector<float4> &nodes, frt_refine::Topology &t, std::vector<RefineLeaf> &leaves,
                         std::vector<int> &leaf_refs)
{
    const int nn = (int)(nodes.size() / 4);
    leaves.clear();
    leaf_refs.clear();
    for (int i = 0; i < nn; ++i)
        for (int side = 0; side < 2; ++side) {
            const float4 *n = &nodes[4 * i];
            const int c = f2i(side ? n[3].y : n[3].x);
            if (c >= 0 || std::find(leaf_refs.begin(), leaf_refs.end(), c) != leaf_refs.end()) continue;
            const float b[2][6] = {{n[0].x, n[0].y, n[0].z, n[0].w, n[1].x, n[1].y}, {n[1].z, n[1].w, n[2].x, n[2].y, n[2].z, n[2].w}};
            RefineLeaf l;
            for (int k = 0; k < 6; ++k) l.box[k] = b[side][k];
            l.ref = c;
            leaves.push_back(l);
            leaf_refs.push_back(c);
        }
    t.n_leaves = (int)leaves.size();
    t.root = t.n_leaves;
    t.child.assign(2 * (size_t)nn, 0);
    for (int i = 0; i < nn; ++i)
        for (int side = 0; side < 2; ++side) {
            const int c = f2i(side ? nodes[4 * i + 3].y : nodes[4 * i + 3].x);
            t.child[2 * i + side] = c >= 0 ? t.n_leaves + c
                                           : (int)(std::find(leaf_refs.begin(), leaf_refs.end(), c) - leaf_refs.begin());
        }
}

bool shadow_cost_host(const FlatScene &F, ShadowCost &out)
{
    out = ShadowCost{};
    if (F.shadow.why != FlatScene::kShadowRan) return false;
    frt_refine::Topology t;
    std::vector<RefineLeaf> leaves;
    std::vector<int> leaf_refs;
    topology_all(F.nodes, t, leaves, leaf_refs);
    frt_refine::RaySet R;
    std::vector<uint8_t> occl;
    sample_rays(F, leaves, kRefineValFrame, kRefineValSeed, R, &occl);
    const DevScene S = host_scene(F);
    int n_occl = 0;
    for (int i = 0; i < R.n; ++i) n_occl += occl[i];
    out.n_rays = n_occl;
    if (n_occl == 0) return true;
    auto price = [&](int which) {   // V and T of the rays marked live, per area-light shadow ray
        const frt_refine::Cost c = frt_refine::tree_cost(t, R);
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
    const int sroot = S.sroot >= 0 ? t.n_leaves + S.sroot
                                   : (int)(std::find(leaf_refs.begin(), leaf_refs.end(), S.sroot) - leaf_refs.begin());
    std::vector<int> under, st{sroot};   // the leaves under the shadow root
    while (!st.empty()) {
        const int s = st.back();
        st.pop_back();
        if (s < t.n_leaves) { under.push_back(s); continue; }
        st.push_back(t.child[2 * (s - t.n_leaves)]);
        st.push_back(t.child[2 * (s - t.n_leaves) + 1]);
    }
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
    frt_refine::Topology t;
    std::vector<RefineLeaf> leaves;
    std::vector<int> leaf_refs;
    topology_all(F.nodes, t, leaves, leaf_refs);
    frt_refine::RaySet R;
    std::vector<uint8_t> occl;
    sample_rays(F, leaves, kRefineValFrame, kRefineValSeed, R, &occl, &origins);
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
// fitting replay per appended node, while the appended nodes leave the scene on the LDS plan it has.
static bool exit_tree_knob()
{
    const char *e = std::getenv("FRT_EXIT_TREE");
    return !(e && std::atoi(e) == 0);
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
    const size_t stack = F.depth < 8 ? 8 : 16;   // the LDS plans' stack classes (frt_plans.hpp)
    const size_t block = (stack + kItemWords) * kBlock * sizeof(int) + scene_bytes;
    return (int)(kLdsCuBytes / ((block + kLdsGranule - 1) / kLdsGranule * kLdsGranule));
}
constexpr int kExitMaxRoot = 1 << 10;   // node indices the kernels carry above PathState::depth (kExitShift)

static void exit_tree(const frt_scene_view *sv, FlatScene &F)
{
    auto &I = F.exit;
    DevScene &S = F.meta;
    I.nodes_before = (int)(F.nodes.size() / 4);
    I.root.assign((size_t)std::max(sv->n_tris, 0), 0);
    // dielectric and the specular lobes leave from p - eps n: only lambertian / diffuse_light scenes
    for (int i = 0; i < sv->n_materials; ++i)
        if (sv->materials[i].type != FRT_MAT_LAMBERTIAN && sv->materials[i].type != FRT_MAT_DIFFUSE_LIGHT) {
            I.why = FlatScene::kExitMaterial;
            return;
        }
    if (!tree_in_lds(F) || F.nodes.empty() || S.root != 0) { I.why = FlatScene::kExitNotResident; return; }
    ProofGeometry pg;
    proof_geometry(sv, F, pg);
    frt_exit::Hidden hid;
    frt_exit::classify(pg.g, hid);
    if (hid.why != frt_exit::kRan) { I.why = FlatScene::kExitTooLarge; return; }
    std::vector<float> nodes(4 * F.nodes.size());
    memcpy(nodes.data(), F.nodes.data(), sizeof(float4) * F.nodes.size());
    std::vector<frt_exit::Class> cls;
    frt_exit::classes(nodes, S.root, FRT_PRIM_SPHERE, kLeafCountShift, hid, cls);
    I.classes = (int)cls.size();
    if (cls.empty()) { I.why = FlatScene::kExitNothing; return; }

    // the fitting replay against the leaves, with the triangle every extension ray leaves
    frt_refine::Topology t0;
    std::vector<RefineLeaf> leaves;
    std::vector<int> leaf_refs;
    topology_all(F.nodes, t0, leaves, leaf_refs);
    frt_refine::RaySet R;
    std::vector<int> from;
    sample_rays(F, leaves, kRefineFitFrame, kRefineFitSeed, R, nullptr, nullptr, &from);
    const std::vector<uint8_t> live0 = R.live;

    // each class alone: its tree on a copy of the nodes, the nodes it appends and the fall of J
    struct Cand { int cls, added; double gain; };
    std::vector<Cand> cand;
    auto as_float4 = [](const std::vector<float> &v) {
        std::vector<float4> o(v.size() / 4);
        memcpy(o.data(), v.data(), sizeof(float) * v.size());
        return o;
    };
    for (int c = 0; c < (int)cls.size(); ++c) {
        std::vector<float> trial = nodes;
        frt_shadow::Tree t;
        frt_shadow::build(trial, S.root, cls[c].dropped, FRT_PRIM_SPHERE, kLeafCountShift, t);
        if (t.empty || t.root <= 0 || t.root >= kExitMaxRoot || t.dropped_leaves == 0) continue;
        frt_refine::Topology tt;
        std::vector<RefineLeaf> l2;
        std::vector<int> r2;
        topology_all(as_float4(trial), tt, l2, r2);
        if (r2 != leaf_refs) continue;   // (appended nodes name the main tree's leaves only)
        bool any = false;
        for (int i = 0; i < R.n; ++i) {
            const bool mine = from[i] >= 0 && std::binary_search(cls[c].members.begin(), cls[c].members.end(), from[i]);
            R.live[i] = live0[i] && mine;
            any |= R.live[i] != 0;
        }
        if (!any) continue;
        R.root.clear();
        const double j0 = frt_refine::cost_j(frt_refine::tree_cost(tt, R), kRefineW);
        R.root.assign(R.n, tt.n_leaves + t.root);
        const double j1 = frt_refine::cost_j(frt_refine::tree_cost(tt, R), kRefineW);
        if (j1 < j0) cand.push_back(Cand{c, t.added, j0 - j1});
    }
    if (cand.empty()) { I.why = FlatScene::kExitNothing; return; }
    // by gain per appended node (a tree that appends nothing first), then gain, then class order
    std::stable_sort(cand.begin(), cand.end(), [](const Cand &a, const Cand &b) {
        if ((a.added == 0) != (b.added == 0)) return a.added == 0;
        const double ra = a.gain / std::max(a.added, 1), rb = b.gain / std::max(b.added, 1);
        if (ra != rb) return ra > rb;
        return a.gain > b.gain;
    });
    // the appended nodes must leave the scene on the plan it has (pick_launcher_t reads these sizes)
    const size_t rest = F.tris.size() + F.tshade.size() + F.mats.size();
    const int nn0 = I.nodes_before;
    const bool lds0 = sizeof(float4) * (4 * (size_t)nn0 + rest) <= kLdsSceneBytes;
    const bool oct0 = !F.nodes_oct.empty();
    auto planar = [&](int nn) { return sizeof(float4) * (4 * (size_t)nn + rest); };
    auto octant = [&](int nn) { return sizeof(float4) * (oct_lds_node_slots(nn) + rest); };
    auto fits = [&](int nn1) {
        const bool lds1 = planar(nn1) <= kLdsSceneBytes;
        const bool oct1 = octant(nn1) <= kLdsOctBytes;
        if (lds0 != lds1 || oct0 != oct1) return false;
        // ... and with as many blocks on a CU (lds_blocks_per_cu)
        if (lds0 && lds_blocks_per_cu(F, planar(nn1)) != lds_blocks_per_cu(F, planar(nn0))) return false;
        return !oct0 || lds_blocks_per_cu(F, octant(nn1)) == lds_blocks_per_cu(F, octant(nn0));
    };
    bool refused = false;
    for (const Cand &k : cand) {
        const frt_exit::Class &c = cls[k.cls];
        std::vector<float> next = nodes;
        frt_shadow::Tree t;
        frt_shadow::build(next, S.root, c.dropped, FRT_PRIM_SPHERE, kLeafCountShift, t);
        if (!fits((int)(next.size() / 16)) || t.root >= kExitMaxRoot) { refused = true; continue; }
        nodes.swap(next);
        for (int d : c.members) I.root[d] = t.root;
        I.taken.push_back({c.sub, t.root, (int)c.members.size(), c.n_dropped, t.added, t.shared, k.gain});
        I.added += t.added;
    }
    if (I.taken.empty()) { I.why = refused ? FlatScene::kExitBudget : FlatScene::kExitNothing; return; }
    I.budget_refused = refused;
    F.nodes.resize(nodes.size() / 4);
    memcpy(F.nodes.data(), nodes.data(), sizeof(float) * nodes.size());
    if (oct0) F.nodes_oct.resize(8 * F.nodes.size());
    for (size_t d = 0; d < I.root.size(); ++d)
        if (I.root[d]) F.tshade[2 * d + 1].z = i2f(I.root[d]);
    I.why = FlatScene::kExitRan;
}

bool exit_cost_host(const FlatScene &F, ExitCost &out)
{
    out = ExitCost{};
    if (!tree_in_lds(F) || F.nodes.empty()) return false;
    frt_refine::Topology t;
    std::vector<RefineLeaf> leaves;
    std::vector<int> leaf_refs;
    topology_all(F.nodes, t, leaves, leaf_refs);
    frt_refine::RaySet R;
    std::vector<uint8_t> occl;
    std::vector<int> from;
    sample_rays(F, leaves, kRefineValFrame, kRefineValSeed, R, &occl, nullptr, &from);
    const DevScene S = host_scene(F);
    auto slot = [&](int ref) {
        return ref >= 0 ? t.n_leaves + ref : (int)(std::find(leaf_refs.begin(), leaf_refs.end(), ref) - leaf_refs.begin());
    };
    const std::vector<uint8_t> live0 = R.live;
    out.n_rays = R.n;
    for (int i = 0; i < R.n; ++i) out.n_ext += from[i] >= 0;
    for (int on = 0; on < 2; ++on) {
        // every ray where the kernels start it: area-light shadow rays at the shadow root (trav_begin
        // tests no box there; an empty shadow tree ends them at once), extension rays at their exit root
        R.root.assign(R.n, t.root);
        R.live = live0;
        for (int i = 0; i < R.n; ++i) {
            if (occl[i] && S.sroot != S.root) {
                if (S.sroot == kSentinel) R.live[i] = 0;
                else { R.root[i] = slot(S.sroot); R.live[i] = 1; }
            } else if (on && from[i] >= 0 && from[i] < (int)F.exit.root.size() && F.exit.root[from[i]]) {
                R.root[i] = slot(F.exit.root[from[i]]);
            }
        }
        const frt_refine::Cost all = frt_refine::tree_cost(t, R);
        out.V_all[on] = all.V; out.T_all[on] = all.T; out.J_all[on] = frt_refine::cost_j(all, kRefineW);
        for (int i = 0; i < R.n; ++i) R.live[i] = R.live[i] && from[i] >= 0;
        const frt_refine::Cost ext = frt_refine::tree_cost(t, R);
        if (out.n_ext > 0) { out.V_ext[on] = ext.V * R.n / out.n_ext; out.T_ext[on] = ext.T * R.n / out.n_ext; }
    }
    return true;
}

int flatten_scene(const frt_scene_view *sv, FlatScene &F, std::string &err, bool f64, int refine, int shadow, int exit)
{
    auto fail = [&](int code, const std::string &m) { err = m; return code; };
    const int nt = sv->n_tris, ns = sv->n_spheres, nm = sv->n_materials;
    if (nt < 0 || ns < 0 || nm <= 0 || !sv->materials || (nt > 0 && (!sv->tri_v || !sv->tri_material || !sv->tri_inv_area)))
        return fail(FRT_E_INVALID, "scene view: missing triangle arrays or materials");
    if (ns > 0 && (!sv->sphere || !sv->sphere_material)) return fail(FRT_E_INVALID, "scene view: missing sphere arrays");
    for (int i = 0; i < nm; ++i) {
        const int t = sv->materials[i].type;
        if (t != FRT_MAT_LAMBERTIAN && t != FRT_MAT_DIFFUSE_LIGHT && t != FRT_MAT_MODIFIED_PHONG &&
            t != FRT_MAT_METAL && t != FRT_MAT_DIELECTRIC && t != FRT_MAT_ROUGH_CONDUCTOR)
            return fail(FRT_E_UNSUPPORTED, "material type " + std::to_string(t) + " is not supported");
        const int tex = sv->materials[i].texture;
        if (tex != FRT_TEX_CONSTANT && tex != FRT_TEX_CHECKER && tex != FRT_TEX_IMAGE)
            return fail(FRT_E_INVALID, "material texture must be FRT_TEX_CONSTANT, FRT_TEX_CHECKER or FRT_TEX_IMAGE");
        if (tex != FRT_TEX_CONSTANT && (t == FRT_MAT_DIFFUSE_LIGHT || t == FRT_MAT_METAL))
            return fail(FRT_E_UNSUPPORTED, "checker / image textures apply to lambertian / modified_phong / dielectric / "
                                           "rough_conductor colours");
        if (tex == FRT_TEX_IMAGE) {
            const int k = sv->materials[i].image;
            if (k < 0 || k >= sv->n_images || !sv->images)
                return fail(FRT_E_INVALID, "material image index out of range");
            const frt_image &im = sv->images[k];
            if (im.nx <= 0 || im.ny <= 0 || !im.data || (im.format != FRT_IMAGE_SRGB8 && im.format != FRT_IMAGE_F32))
                return fail(FRT_E_INVALID, "scene view: bad image");
        }
        if (t == FRT_MAT_ROUGH_CONDUCTOR &&
            (!(sv->materials[i].alpha > 0.0) || (sv->materials[i].distribution != FRT_DIST_GGX &&
                                                  sv->materials[i].distribution != FRT_DIST_BECKMANN)))
            return fail(FRT_E_INVALID, "rough_conductor needs alpha > 0 and a GGX / Beckmann distribution");
    }
    auto valid_ref = [&](int ref) {
        if (ref < 0) return false;
        if (ref & FRT_PRIM_SPHERE) return (ref & ~FRT_PRIM_SPHERE) < ns;
        return ref < nt;
    };
    auto prim_box = [&](int ref, double *lo, double *hi) {
        if (ref & FRT_PRIM_SPHERE) {
            const double *q = &sv->sphere[4 * (ref & ~FRT_PRIM_SPHERE)];
            for (int k = 0; k < 3; ++k) { lo[k] = q[k] - q[3]; hi[k] = q[k] + q[3]; }
        } else {
            const double *v = &sv->tri_v[9 * ref];
            for (int k = 0; k < 3; ++k) {
                lo[k] = std::min(std::min(v[k], v[3 + k]), v[6 + k]);
                hi[k] = std::max(std::max(v[k], v[3 + k]), v[6 + k]);
            }
        }
    };
    std::vector<int> tri_order;            // device id -> view triangle
    std::vector<int> tri_dev(nt, -1);      // view triangle -> device id
    DevScene &S = F.meta;
    S = DevScene{};
    if (sv->world_kind == FRT_WORLD_BVH) {
        const int nn = sv->n_nodes;
        if (nn < 0 || (nn > 0 && (!sv->node_box || !sv->node_child)))
            return fail(FRT_E_INVALID, "scene view: missing BVH arrays");
        if (sv->root >= nn || (sv->root >= 0 && nn == 0)) return fail(FRT_E_INVALID, "scene view: bad root");
        double rlo[3], rhi[3];
        if (sv->root < 0) {
            if (!valid_ref(~sv->root)) return fail(FRT_E_INVALID, "scene view: bad root prim");
            prim_box(~sv->root, rlo, rhi);
        } else {
            for (int k = 0; k < 3; ++k) { rlo[k] = sv->node_box[6 * sv->root + k]; rhi[k] = sv->node_box[6 * sv->root + 3 + k]; }
        }
        double scale = 1.0;   // conservative box padding relative to the scene extent
        for (int k = 0; k < 3; ++k) scale = std::max(scale, std::max(std::fabs(rlo[k]), std::fabs(rhi[k])));
        const double pad = 4e-6 * scale;
        auto padded = [&](const double *lo, const double *hi, float *flo, float *fhi) {
            for (int k = 0; k < 3; ++k) { flo[k] = round_down(lo[k] - pad); fhi[k] = round_up(hi[k] + pad); }
        };
        padded(rlo, rhi, S.root_lo, S.root_hi);
        S.ao_tmax = (float)((rhi[1] - rlo[1]) * 0.50f);   // ao.cpp:19-21 (unpadded root box, fp64)
        std::vector<int> new_id(std::max(nn, 1), -1), order;
        order.reserve(nn);
        // left-first DFS: node ids in pre-order, triangle leaves numbered in visit order
        std::vector<std::pair<int, int>> st;   // (child ref, level)
        st.push_back({sv->root, 1});
        while (!st.empty()) {
            const auto [x, lvl] = st.back();
            st.pop_back();
            if (x >= 0) {
                if (x >= nn || new_id[x] >= 0) return fail(FRT_E_INVALID, "scene view: BVH is not a tree");
                new_id[x] = (int)order.size();
                order.push_back(x);
                F.depth = std::max(F.depth, lvl);
                st.push_back({sv->node_child[2 * x + 1], lvl + 1});
                st.push_back({sv->node_child[2 * x], lvl + 1});
            } else {
                const int ref = ~x;
                if (!valid_ref(ref)) return fail(FRT_E_INVALID, "scene view: bad leaf prim");
                if (!(ref & FRT_PRIM_SPHERE)) {
                    if (tri_dev[ref] >= 0) return fail(FRT_E_INVALID, "scene view: triangle in two leaves");
                    tri_dev[ref] = (int)tri_order.size();
                    tri_order.push_back(ref);
                }
            }
        }
        F.nodes.resize(4 * order.size());
        for (size_t i = 0; i < order.size(); ++i) {
            const int x = order[i];
            float cb[2][6];
            int cref[2];
            for (int side = 0; side < 2; ++side) {
                const int ch = sv->node_child[2 * x + side];
                double lo[3], hi[3];
                if (ch >= 0) {
                    for (int k = 0; k < 3; ++k) { lo[k] = sv->node_box[6 * ch + k]; hi[k] = sv->node_box[6 * ch + 3 + k]; }
                    cref[side] = new_id[ch];
                } else {
                    const int ref = ~ch;
                    prim_box(ref, lo, hi);
                    cref[side] = ~((ref & FRT_PRIM_SPHERE) ? ref : tri_dev[ref]);
                }
                padded(lo, hi, &cb[side][0], &cb[side][3]);
            }
            F.nodes[4 * i + 0] = make_float4(cb[0][0], cb[0][1], cb[0][2], cb[0][3]);
            F.nodes[4 * i + 1] = make_float4(cb[0][4], cb[0][5], cb[1][0], cb[1][1]);
            F.nodes[4 * i + 2] = make_float4(cb[1][2], cb[1][3], cb[1][4], cb[1][5]);
            F.nodes[4 * i + 3] = make_float4(i2f(cref[0]), i2f(cref[1]), 0.0f, 0.0f);
        }
        if (nt >= kLeafIndexLimit) return fail(FRT_E_INVALID, "scene view: too many triangles");
        // leaf size by plan (profiles/r01_leaf_ab.txt; re-checked at 512 spp in
        // profiles/r02/r02z_ab_leaf_512spp.txt): 2 triangles when the scene
        // fits the LDS plan (Cornell +6 % over 4), else 4 (cornell_1m: +11 % over 2)
        const int forced = leaf_size_override();
        if (forced) {
            collapse_leaves(F, forced);
        } else {
            const std::vector<float4> binary = F.nodes;
            const int depth = F.depth;
            collapse_leaves(F, kLeafSmallScene);
            const size_t bytes = sizeof(float4) * (F.nodes.size() + 5 * (size_t)nt + 2 * (size_t)nm);
            if (bytes > kLdsSceneBytes || F.depth >= kLdsMaxDepth) {
                F.nodes = binary;
                F.depth = depth;
                collapse_leaves(F, kLeafDefault);
            }
        }
        for (int i = 0; i < nt; ++i)   // triangles outside the tree: trailing ids, never intersected
            if (tri_dev[i] < 0) { tri_dev[i] = (int)tri_order.size(); tri_order.push_back(i); }
    } else if (sv->world_kind == FRT_WORLD_LIST) {
        S.ao_spheres_only = 1;                              // ao.cpp:21 t_max is NaN (ao_shade)
        if (sv->n_list < 0 || (sv->n_list > 0 && !sv->list)) return fail(FRT_E_INVALID, "scene view: bad list");
        for (int i = 0; i < nt; ++i) { tri_dev[i] = i; tri_order.push_back(i); }
        for (int i = 0; i < sv->n_list; ++i)
            if (!valid_ref(sv->list[i])) return fail(FRT_E_INVALID, "scene view: bad list entry");
    } else {
        return fail(FRT_E_INVALID, "scene view: unknown world kind");
    }
    auto dev_ref = [&](int ref) { return (ref & FRT_PRIM_SPHERE) ? ref : tri_dev[ref]; };
    F.tri_view = tri_order;

    // triangles in device order: v0 | e1 | e2 with the edges taken in fp64 (triangle.h:58-60)
    bool any_smooth = false;
    for (int i = 0; i < nt; ++i)
        if (sv->tri_geometry_normal && !sv->tri_geometry_normal[i]) any_smooth = true;
    if (any_smooth && !sv->tri_n) return fail(FRT_E_INVALID, "scene view: smooth triangles without normals");
    F.tris.resize(3 * (size_t)nt);
    F.tshade.resize(2 * (size_t)nt);
    if (any_smooth) F.tnorm.resize(3 * (size_t)nt);
    if (f64) {
        F.tris64.resize(3 * (size_t)nt);
        F.tshade64.resize(nt);
        if (any_smooth) F.tnorm64.resize(3 * (size_t)nt);
    }
    for (int d = 0; d < nt; ++d) {
        const int i = tri_order[d];
        const double *v = &sv->tri_v[9 * i];
        const double e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]};
        const double e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
        double ng[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double l = std::sqrt(ng[0] * ng[0] + ng[1] * ng[1] + ng[2] * ng[2]);
        for (int k = 0; k < 3; ++k) ng[k] = ng[k] / l;   // unit_vector(cross(e1, e2)), triangle.h:101
        F.tris[3 * d + 0] = make_float4((float)v[0], (float)v[1], (float)v[2], 0.0f);
        F.tris[3 * d + 1] = make_float4((float)e1[0], (float)e1[1], (float)e1[2], 0.0f);
        F.tris[3 * d + 2] = make_float4((float)e2[0], (float)e2[1], (float)e2[2], 0.0f);
        const int mat = sv->tri_material[i];
        if (mat < 0 || mat >= nm) return fail(FRT_E_INVALID, "scene view: bad triangle material");
        const int geo = sv->tri_geometry_normal ? (sv->tri_geometry_normal[i] ? 1 : 0) : 1;
        F.tshade[2 * d + 0] = make_float4((float)ng[0], (float)ng[1], (float)ng[2], (float)sv->tri_inv_area[i]);
        F.tshade[2 * d + 1] = make_float4(i2f(mat), i2f(geo), 0.0f, 0.0f);
        if (any_smooth)
            for (int k = 0; k < 3; ++k)
                F.tnorm[3 * d + k] = make_float4((float)sv->tri_n[9 * i + 3 * k], (float)sv->tri_n[9 * i + 3 * k + 1],
                                                 (float)sv->tri_n[9 * i + 3 * k + 2], 0.0f);
        if (f64) {
            F.tris64[3 * d + 0] = make_double4(v[0], v[1], v[2], 0.0);
            F.tris64[3 * d + 1] = make_double4(e1[0], e1[1], e1[2], 0.0);
            F.tris64[3 * d + 2] = make_double4(e2[0], e2[1], e2[2], 0.0);
            F.tshade64[d] = make_double4(ng[0], ng[1], ng[2], sv->tri_inv_area[i]);
            if (any_smooth)
                for (int k = 0; k < 3; ++k)
                    F.tnorm64[3 * d + k] = make_double4(sv->tri_n[9 * i + 3 * k], sv->tri_n[9 * i + 3 * k + 1],
                                                        sv->tri_n[9 * i + 3 * k + 2], 0.0);
        }
    }
    // texture coordinates, only when a material is textured (in HBM; read at textured hits)
    bool any_tex = false;
    for (int i = 0; i < nm; ++i) any_tex |= sv->materials[i].texture != FRT_TEX_CONSTANT;
    if (any_tex) {
        F.tuv.assign(2 * (size_t)std::max(nt, 1), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
        if (sv->tri_uv)
            for (int d = 0; d < nt; ++d) {
                const double *q = &sv->tri_uv[6 * tri_order[d]];
                F.tuv[2 * d] = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
                F.tuv[2 * d + 1] = make_float4((float)q[4], (float)q[5], 0.0f, 0.0f);
            }
    }
    F.spheres.resize(ns);
    F.smat.resize(ns);
    if (f64) F.spheres64.resize(ns);
    for (int k = 0; k < ns; ++k) {
        const double *q = &sv->sphere[4 * k];
        F.spheres[k] = make_float4((float)q[0], (float)q[1], (float)q[2], (float)q[3]);
        if (f64) F.spheres64[k] = make_double4(q[0], q[1], q[2], q[3]);
        F.smat[k] = sv->sphere_material[k];
        if (F.smat[k] < 0 || F.smat[k] >= nm) return fail(FRT_E_INVALID, "scene view: bad sphere material");
    }
    // image_texture texels (append_texels)
    std::vector<int> image_off(std::max(sv->n_images, 0), -1);
    for (int i = 0; i < nm; ++i) {
        if (sv->materials[i].texture != FRT_TEX_IMAGE) continue;
        const int k = sv->materials[i].image;
        if (image_off[k] >= 0) continue;
        const frt_image &im = sv->images[k];
        const size_t n = (size_t)im.nx * im.ny;
        if (F.texels.size() + n > (size_t)INT32_MAX) return fail(FRT_E_UNSUPPORTED, "images larger than 2^31 texels");
        image_off[k] = (int)F.texels.size();
        append_texels(im, F.texels);
    }
    F.mats.assign(kMatStride * (size_t)nm, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (int i = 0; i < nm; ++i) {
        const frt_material &m = sv->materials[i];
        float4 *d = &F.mats[kMatStride * i];
        auto f4 = [](const double *v, float w) { return make_float4((float)v[0], (float)v[1], (float)v[2], w); };
        // m0 = (albedo | kd | metal albedo | rough eta, type); m1 = (emit, -) for lights,
        // (ks, exponent | ior | alpha) otherwise; m2 = (rough k, distribution)
        d[0] = f4(m.type == FRT_MAT_ROUGH_CONDUCTOR ? m.eta : m.albedo, i2f(m.type));
        if (m.type == FRT_MAT_DIFFUSE_LIGHT) d[1] = f4(m.emit, 0.0f);
        else d[1] = f4(m.specular, (float)(m.type == FRT_MAT_MODIFIED_PHONG ? m.exponent
                                           : m.type == FRT_MAT_DIELECTRIC ? m.ior : m.alpha));
        d[2] = f4(m.k, i2f(m.distribution));
        d[3] = f4(m.tex_odd, i2f(m.texture));
        d[4] = make_float4((float)m.tex_scale[0], (float)m.tex_scale[1], 0.0f, 0.0f);
        if (m.texture == FRT_TEX_IMAGE)   // (nx, ny, first texel)
            d[4] = make_float4(i2f(sv->images[m.image].nx), i2f(sv->images[m.image].ny), i2f(image_off[m.image]), 0.0f);
    }
    if (sv->n_lights < 0 || (sv->n_lights > 0 && !sv->lights)) return fail(FRT_E_INVALID, "scene view: bad lights");
    F.lights.resize(sv->n_lights);
    for (int i = 0; i < sv->n_lights; ++i) {
        if (!valid_ref(sv->lights[i])) return fail(FRT_E_INVALID, "scene view: bad light");
        F.lights[i] = dev_ref(sv->lights[i]);
    }
    F.list.resize(sv->world_kind == FRT_WORLD_LIST ? sv->n_list : 0);
    for (size_t i = 0; i < F.list.size(); ++i) F.list[i] = dev_ref(sv->list[i]);

    // octant copies of the binary nodes: child boxes as (near xyz, far xyz).
    // Only the LDS binary plan reads them, and only when they fit its budget
    // (pick_launcher_t): larger scenes get none (8x the node array otherwise).
    const size_t oct_bytes = sizeof(float4) * (oct_lds_node_slots((int)(F.nodes.size() / 4)) + F.tris.size() +
                                               F.tshade.size() + F.mats.size());
    if (sv->world_kind == FRT_WORLD_BVH && F.depth < kLdsMaxDepth && oct_bytes <= kLdsOctBytes)
        F.nodes_oct.resize(8 * F.nodes.size());
    S.root = (sv->world_kind == FRT_WORLD_BVH) ? ((sv->root >= 0) ? 0 : ~dev_ref(~sv->root)) : 0;
    S.sroot = S.root;   // until the shadow-tree pass finds one
    // the trees derived from the binary nodes: the octant copies and BVH4Q
    auto derive_trees = [&]() {
        fill_octants(F);
        F.has4 = sv->world_kind == FRT_WORLD_BVH && build_bvh4(F, S.root);
        if (!F.has4) F.nodes4.clear();
        S.root4 = F.has4 ? F.root4 : S.root;
        S.n_nodes4 = (int)(F.nodes4.size() / kNode4Parts);
    };
    derive_trees();
    S.n_lights = sv->n_lights;
    S.n_list = (int)F.list.size();
    S.n_nodes = (int)(F.nodes.size() / 4);
    S.n_tris = nt;
    S.n_mats = nm;
    S.n_nodes4 = (int)(F.nodes4.size() / kNode4Parts);
    S.node_es = 4; S.node_ps = 1;
    S.node4_es = kNode4Parts; S.node4_ps = 1;
    S.tri_es = 3; S.tri_ps = 1;
    S.sh_es = 2; S.sh_ps = 1;
    S.world_kind = sv->world_kind;
    auto f3d = [](const double *x) { return mk3((float)x[0], (float)x[1], (float)x[2]); };
    S.cam_o = f3d(sv->cam_origin); S.cam_llc = f3d(sv->cam_lower_left);
    S.cam_h = f3d(sv->cam_horizontal); S.cam_v = f3d(sv->cam_vertical);
    S.cam_u = f3d(sv->cam_u); S.cam_vv = f3d(sv->cam_v);
    S.lens_r = (float)sv->cam_lens_radius;
    S.cam_w = f3d(sv->cam_w);
    S.cam_half_height = (float)sv->cam_half_height;
    S.env = f3d(sv->env_color);
    auto d3d = [](const double *x) { return d3{x[0], x[1], x[2]}; };
    S.cam64_o = d3d(sv->cam_origin); S.cam64_llc = d3d(sv->cam_lower_left);
    S.cam64_h = d3d(sv->cam_horizontal); S.cam64_v = d3d(sv->cam_vertical);
    S.cam64_u = d3d(sv->cam_u); S.cam64_vv = d3d(sv->cam_v);
    S.lens_r64 = sv->cam_lens_radius;
    // topology refinement (refine_tree): needs the finished scene for its ray sample, so the
    // derived trees are made again from the nodes it rewrote
    bool again = (refine < 0 ? tree_refine_knob() : refine != 0) && refine_tree(F);
    // the shadow tree over the tree the main rays will walk: its nodes go behind the main ones
    if (shadow < 0 ? shadow_tree_knob() : shadow != 0) {
        shadow_tree(sv, F);
        again |= F.shadow.why == FlatScene::kShadowRan;
    }
    // the exit trees over the same tree: their nodes go behind the shadow tree's
    if (exit < 0 ? exit_tree_knob() : exit != 0) {
        exit_tree(sv, F);
        again |= F.exit.why == FlatScene::kExitRan;
    }
    if (again) derive_trees();
    S.n_nodes = (int)(F.nodes.size() / 4);
    return FRT_OK;
}

// host image of the flattened scene as the kernels see it (HBM strides)
DevScene host_scene(const FlatScene &F)
{
    DevScene S = F.meta;
    S.nodes = F.nodes.data(); S.nodes4 = F.nodes4.data(); S.nodes_oct = F.nodes_oct.data();
    S.tris = F.tris.data(); S.tshade = F.tshade.data(); S.tnorm = F.tnorm.data();
    S.tuv = F.tuv.data(); S.texels = F.texels.data();
    S.spheres = F.spheres.data(); S.sphere_mat = F.smat.data(); S.mats = F.mats.data();
    S.lights = F.lights.data(); S.list = F.list.data(); S.tri_view = F.tri_view.data();
    S.tris64 = F.tris64.data(); S.tshade64 = F.tshade64.data(); S.tnorm64 = F.tnorm64.data();
    S.spheres64 = F.spheres64.data();
    return S;
}
