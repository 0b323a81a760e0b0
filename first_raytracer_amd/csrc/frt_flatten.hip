// frt_flatten.hip -- scene flattening on the host: DFS order, fp32 conversion
// with outward-rounded boxes, multi-triangle leaves, the 4-wide quantized tree
// (BVH4Q), the octant node copies and the texel conversion.  The passes over
// the finished tree (refinement, shadow tree, exit trees) are frt_tree_passes.hip's;
// flatten_scene ends by calling them.  No kernel and no HIP runtime call; built
// with the kernel units' compiler and flags so that its floating-point results
// do not depend on which unit holds it.
#include "frt_flatten.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <functional>

#include "frt_kernels.hpp"   // the LDS footprint rule (lds_*_bytes, lds_*_fits, kLdsMaxDepth)
#include "frt_tree_passes.hpp"

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
            // (2 float4s per material undercounts them: kMatStride is 5.  Counting them right changes
            // which scenes get two-triangle leaves, so it is a change of its own.)
            if (!lds_planar_fits(lds_planar_bytes(F.nodes.size() / 4, 5 * (size_t)nt + 2 * (size_t)nm)) || F.depth >= kLdsMaxDepth) {
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
    if (sv->world_kind == FRT_WORLD_BVH && F.depth < kLdsMaxDepth &&
        lds_octant_fits(lds_octant_bytes(F.nodes.size() / 4, lds_rest(F))))
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
    // The passes over the tree (frt_tree_passes.hip) need the finished scene for their ray samples, so
    // the derived trees are made again from the nodes they rewrote: the refinement of the main tree,
    // the shadow tree over the tree the main rays will walk, its nodes behind the main ones, and the
    // exit trees over the same tree, their nodes behind the shadow tree's.
    bool again = refine_tree(F, refine);
    again |= shadow_tree(sv, F, shadow);
    again |= exit_tree(sv, F, exit);
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
