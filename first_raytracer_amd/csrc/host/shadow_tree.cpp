// shadow_tree.cpp -- see shadow_tree.hpp.
//
// What is proven before a triangle P is dropped.  A shadow segment runs from an
// origin o = fl(x + eps n(x)), x a computed hit point on some primitive and n its
// stored shading normal, to an end y sampled on a light, and asks tri_intersect
// for a hit with t in (t_min, 1 - shadow_eps], t_min >= eps.  Write s(.) for the
// signed distance to P's plane pi, positive on the side the scene occupies.
// tri_intersect forms t = N / a, where in exact arithmetic N = 2A s(o) and
// a = 2A (s(o) - s(y)), A the triangle's area.  In fp32 the two triple products
// carry absolute errors of at most 8 u |o - v0| |e1| |e2| and 8 u |y - o| |e1| |e2|
// (u = 2^-24: three products and two sums per cross component, three and two per
// dot), which in units of distance is 8 u rho Dm with rho = |e1| |e2| / 2A the
// triangle's aspect and Dm the scene's diameter.  The fp32 copies of o, y and of
// P's vertices sit within 2 u Dm of the fp64 ones, and a hit point is the closest
// hit along its ray, so it lies beyond pi -- where P or a coplanar neighbour
// would have been hit first -- by no more than the rounding of that hit's own t
// and of the fma that forms the point, 16 u rho Dm.  All of it is covered by
//     E = kNoise u rho Dm,  kNoise = 32:
// the computed t is (s_o + e1) / (s_o - s_y + e2) with |e1|, |e2| <= E, for true
// distances s_o >= -E and s_y.
//
// Rule (a), the half-space rule.  Let every light keep s_y >= D = 4 E / eps.
//  - s_o <= 2 E: |numerator| <= 3 E and the denominator is below 3 E - D, so
//    |t| <= 3 E / (D - 3 E) < eps <= t_min: no hit.
//  - s_o > 2 E: the numerator is positive.  A negative denominator gives t < 0;
//    a positive one needs s_o > s_y - E >= D - E, and then
//    t >= (s_o - E) / (s_o - D + E) > 1 because D > 2 E: beyond the segment.
// That origins keep s_o >= -E needs the scene on one side of pi (the tolerance
// kOnPlane u M below, M the largest coordinate: the fp32 conversion moves a
// coordinate by at most u M, so 8 u M covers a point against a plane through
// three such vertices; at Cornell's size that is 2 % of eps) and no origin pushed
// through pi by its own eps n.  The terms above leave E / 4 of the budget, and both
// cases hold as they stand for s_o >= -2 E, so a push of up to E is let through: a
// geometric normal that leans to the far side by at most E / eps (a ceiling against
// a wall that is a degree off the vertical).  A primitive whose stored normal leans
// further must stay 2 eps clear of pi.  P itself is one of those primitives, so its
// own normal has to point to the occupied side.
//
// Rule (b), the lights' plane.  Only for a plane of constant coordinate k = c:
// P's vertices and every light vertex hold the same double c there, so e1_k =
// e2_k = 0 exactly, every sampled end has y_k = (float)c (prim_sample: v0 + b0 e1
// + b1 e2) and d_k = fl(y_k - o_k) = -fl(o_k - v0_k).  With the zero components
// both triple products collapse to that one coordinate times the triangle's
// doubled area, each within 4 u rho relatively, so t = 1 + O(10 u rho): above
// 1 - shadow_eps for any origin whatever, given rho <= kMaxAspect.  (o_k = c makes
// a = 0, a miss.)  A slanted plane has no such argument -- near it s_o and s_y are
// both rounding noise -- and keeps its triangles.
//
// The pass is off (kTooLarge) when kNoise u Dm > eps / 4: the offset eps no
// longer dominates the rounding of a hit point, and D would pass the size of the
// scene.  Cornell (Dm = 5.2, eps = 1e-4) has 1.0e-5 against 2.5e-5.
#include "shadow_tree.hpp"

#include <algorithm>
#include <cmath>

namespace frt_shadow {
namespace {

constexpr double kU = 1.0 / 16777216.0;   // 2^-24
constexpr double kNoise = 32.0, kOnPlane = 8.0, kMaxAspect = 8.0;

struct V { double x, y, z; };
inline V sub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V cross(V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double len(V a) { return std::sqrt(dot(a, a)); }
inline V at(const double *p) { return V{p[0], p[1], p[2]}; }

}   // namespace

void classify(const Geometry &g, Classified &out)
{
    out = Classified{};
    out.dropped.assign((size_t)std::max(g.n_tris, 0), 0);
    if (g.n_lights <= 0) { out.why = kNoLights; return; }
    // size of the scene: the box of every vertex, sphere and lens point
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    auto grow = [&](const double *p, double r) {
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k] - r); hi[k] = std::max(hi[k], p[k] + r); }
    };
    for (int i = 0; i < 3 * g.n_tris; ++i) grow(&g.tri_v[3 * i], 0.0);
    for (int i = 0; i < g.n_spheres; ++i) grow(&g.sphere[4 * i], g.sphere[4 * i + 3]);
    grow(g.cam_o, std::fabs(g.lens_r));
    double M = 0.0, Dm = 0.0;
    for (int k = 0; k < 3; ++k) {
        M = std::max(M, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
        Dm += (hi[k] - lo[k]) * (hi[k] - lo[k]);
    }
    Dm = std::sqrt(Dm);
    if (!(kNoise * kU * Dm <= 0.25 * g.eps) || !(M < 1e30)) { out.why = kTooLarge; return; }
    const double tol = kOnPlane * kU * M;
    const double lens = std::fabs(g.lens_r);

    // unit geometric normals; a degenerate triangle has none and takes part in no proof
    std::vector<V> ng((size_t)g.n_tris);
    std::vector<uint8_t> flat((size_t)g.n_tris, 0);
    for (int i = 0; i < g.n_tris; ++i) {
        const double *v = &g.tri_v[9 * i];
        const V c = cross(sub(at(v + 3), at(v)), sub(at(v + 6), at(v)));
        const double l = len(c);
        if (l > 0.0) ng[i] = V{c.x / l, c.y / l, c.z / l};
        else { ng[i] = V{0, 0, 0}; flat[i] = 1; }
    }
    auto smooth = [&](int i) { return g.tri_smooth && g.tri_smooth[i]; };
    auto light_is_sphere = [&](int ref) { return (ref & g.sphere_bit) != 0; };

    for (int p = 0; p < g.n_tris; ++p) {
        if (flat[p]) continue;
        const double *pv = &g.tri_v[9 * p];
        const V v0 = at(pv), e1 = sub(at(pv + 3), v0), e2 = sub(at(pv + 6), v0), m = ng[p];
        const double rho = len(e1) * len(e2) / len(cross(e1, e2));
        if (!(rho <= kMaxAspect)) continue;
        const double E = kNoise * kU * rho * Dm, D = 4.0 * E / g.eps;
        auto s = [&](const double *x) { return dot(m, sub(at(x), v0)); };

        // ---- rule (b): P and every light in one plane of constant coordinate ----
        bool rule_b = false;
        for (int k = 0; k < 3 && !rule_b; ++k) {
            const double c = pv[k];
            bool ok = pv[3 + k] == c && pv[6 + k] == c;
            for (int l = 0; l < g.n_lights && ok; ++l) {
                const int ref = g.lights[l];
                if (light_is_sphere(ref)) { ok = false; break; }
                const double *lv = &g.tri_v[9 * ref];
                ok = lv[k] == c && lv[3 + k] == c && lv[6 + k] == c;
            }
            rule_b = ok;
        }
        if (rule_b) { out.dropped[p] = 1; ++out.n_rule_b; continue; }

        // ---- rule (a): the scene in one closed half-space of pi ----
        for (int side = 1; side >= -1 && !out.dropped[p]; side -= 2) {
            const double sg = (double)side;
            bool ok = true;
            // every vertex, sphere and lens point on the occupied side
            for (int i = 0; i < 3 * g.n_tris && ok; ++i) ok = sg * s(&g.tri_v[3 * i]) >= -tol;
            for (int i = 0; i < g.n_spheres && ok; ++i) ok = sg * s(&g.sphere[4 * i]) - g.sphere[4 * i + 3] >= -tol;
            if (ok) {   // the lens disk's extent along m
                const double a = dot(m, at(g.cam_u)), b = dot(m, at(g.cam_v));
                ok = sg * s(g.cam_o) - lens * std::sqrt(a * a + b * b) >= -tol;
            }
            // no origin pushed through pi: a normal that leans to the far side needs 2 eps of room
            for (int q = 0; q < g.n_tris && ok; ++q) {
                const double *qv = &g.tri_v[9 * q];
                bool leans;
                if (smooth(q)) {   // the interpolated normal stays on the side all three vertex normals are on
                    leans = false;
                    for (int j = 0; j < 3; ++j) leans |= !(sg * dot(m, at(&g.tri_n[9 * q + 3 * j])) >= 0.0);
                } else {
                    leans = flat[q] || !(-sg * dot(m, ng[q]) * g.eps <= E);
                }
                if (leans) ok = std::min(std::min(sg * s(qv), sg * s(qv + 3)), sg * s(qv + 6)) >= 2.0 * g.eps;
            }
            for (int i = 0; i < g.n_spheres && ok; ++i)   // a sphere's normals point every way
                ok = sg * s(&g.sphere[4 * i]) - g.sphere[4 * i + 3] >= 2.0 * g.eps;
            // every end at least D from pi
            for (int l = 0; l < g.n_lights && ok; ++l) {
                const int ref = g.lights[l];
                if (light_is_sphere(ref)) {
                    const double *q = &g.sphere[4 * (ref & ~g.sphere_bit)];
                    ok = sg * s(q) - q[3] >= D;
                } else {
                    const double *lv = &g.tri_v[9 * ref];
                    ok = std::min(std::min(sg * s(lv), sg * s(lv + 3)), sg * s(lv + 6)) >= D;
                }
            }
            if (ok) { out.dropped[p] = 1; ++out.n_rule_a; }
        }
    }
}

void build(std::vector<float> &nodes, int main_root, const std::vector<uint8_t> &dropped, int sphere_bit,
           int count_shift, Tree &out)
{
    out = Tree{};
    auto ref_of = [&](int i, int side) {
        int r;
        const float f = nodes[16 * (size_t)i + 12 + side];
        static_assert(sizeof(r) == sizeof(f), "refs are stored as int bits");
        std::copy(reinterpret_cast<const char *>(&f), reinterpret_cast<const char *>(&f) + sizeof(f), reinterpret_cast<char *>(&r));
        return r;
    };
    auto leaf_kept = [&](int lref) {   // lref = ~ref
        if (lref & sphere_bit) return true;
        const int first = lref & ((1 << count_shift) - 1), count = (lref >> count_shift) + 1;
        for (int k = 0; k < count; ++k)
            if (first + k >= (int)dropped.size() || !dropped[first + k]) return true;
        return false;
    };
    struct Sub { bool empty, same; int ref; float box[6]; int n_nodes; };   // n_nodes: main-tree nodes in it, not yet counted
    // children follow parents nowhere in particular after the refinement pass: plain recursion
    // (the trees this pass sees are LDS-resident, at most kLdsMaxDepth levels)
    struct Rec {
        std::vector<float> &nodes;
        decltype(ref_of) &ref;
        decltype(leaf_kept) &kept;
        Tree &out;
        Sub visit(int r, const float *box)
        {
            Sub s{};
            for (int k = 0; k < 6; ++k) s.box[k] = box[k];
            s.ref = r;
            if (r < 0) {
                s.same = true;
                s.empty = !kept(~r);
                ++(s.empty ? out.dropped_leaves : out.kept_leaves);
                return s;
            }
            float b0[6], b1[6];
            for (int k = 0; k < 6; ++k) { b0[k] = nodes[16 * (size_t)r + k]; b1[k] = nodes[16 * (size_t)r + 6 + k]; }
            const Sub a = visit(ref(r, 0), b0), b = visit(ref(r, 1), b1);
            if (a.empty && b.empty) { s.empty = true; return s; }
            if (a.empty || b.empty) { Sub c = a.empty ? b : a; c.same = false; return c; }   // contracted
            if (a.same && b.same) { s.same = true; s.n_nodes = 1 + a.n_nodes + b.n_nodes; return s; }
            // a new node over the two results
            out.shared += a.n_nodes + b.n_nodes;
            s.ref = (int)(nodes.size() / 16);
            float rec[16] = {0};
            for (int k = 0; k < 6; ++k) { rec[k] = a.box[k]; rec[6 + k] = b.box[k]; }
            const int refs[2] = {a.ref, b.ref};
            std::copy(reinterpret_cast<const char *>(refs), reinterpret_cast<const char *>(refs) + sizeof(refs),
                      reinterpret_cast<char *>(&rec[12]));
            nodes.insert(nodes.end(), rec, rec + 16);
            ++out.added;
            for (int k = 0; k < 3; ++k) { s.box[k] = std::min(a.box[k], b.box[k]); s.box[3 + k] = std::max(a.box[3 + k], b.box[3 + k]); }
            return s;
        }
    } rec{nodes, ref_of, leaf_kept, out};
    const float no_box[6] = {0, 0, 0, 0, 0, 0};   // the root's own box is in no record
    const Sub r = rec.visit(main_root, no_box);
    out.shared += r.n_nodes;
    out.empty = r.empty;
    out.root = r.empty ? main_root : r.ref;
}

}   // namespace frt_shadow
