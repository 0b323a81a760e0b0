// exit_tree.cpp -- see exit_tree.hpp.
//
// What is proven before triangle j is hidden from the rays that leave triangle k.
// path_shade starts the extension ray of a lambertian vertex on k at
// o = fl(p + eps n), p = fl(ro + t rd) the computed hit point and n the stored
// geometric normal of k (prim_shade does not turn it toward the incoming ray, so
// whichever side the path arrived from, it leaves on n's side), along a direction
// wo of the cosine lobe around n with n . wo >= 2^-12 |wo| (the comment in
// path_shade: z = sqrt(1 - r0), r0 < 1 - 2^-24; the basis and the sum that form
// wo carry a few u = 2^-24 of relative error, four orders below that).  Write
// s(.) for the signed distance to k's plane, positive on n's side, M for the
// largest coordinate and Dm for the diameter of the scene, rho = |e1| |e2| / 2A
// for a triangle's aspect, and E(rho) = kNoise u rho Dm, kNoise = 32, for the
// shadow pass's bound on what fp32 tri_intersect and the fma that forms a hit
// point can be off by, in units of distance (shadow_tree.cpp derives it).
//  - The hit point: p is a closest hit on k, so |s(p)| <= E(rho_k).
//  - The offset: eps n moves p up by eps (1 - 2 u) at least (n is the fp32 copy
//    of a unit vector), and the product and sum round each coordinate by at most
//    2 u M, under kRound u M = 4 u M of distance.  So
//        s(o) >= eps - delta,   delta = E(rho_k) + kRound u M.
//  - The ray: s(o + t wo) >= s(o) for every t >= 0, because n . wo > 0.
//  - A reported hit: a t >= t_min > 0 that tri_intersect reports for triangle j
//    puts the computed point o + t wo within E(rho_j) of j.  Every point of j
//    has s <= tau, tau = kOnPlane u M = 8 u M (the shadow pass's allowance for
//    vertices that were meant to lie in the plane: the fp32 conversion moves a
//    coordinate by at most u M).
// So   eps - delta - tau > E(rho_j)   rules a reported hit out.  k itself and its
// coplanar neighbours are the case s = 0 of it.  Both aspects are capped at
// kMaxAspect, where E's derivation stops holding.
//
// The pass is off (kTooLarge) when the inequality fails even for rho = 1:
// 2 E(1) + (kRound + kOnPlane) u M >= eps.  Cornell (Dm = 5.2, M = 2.8, eps = 1e-4)
// has 2.0e-5 + 2.0e-6 against 1e-4; at a thousand times the size it fails.
//
// What is not proven stays: spheres are never hidden (a sphere leaf is in no drop
// set), a triangle shaded with vertex normals or one of zero area serves no ray,
// a light serves none either (no path scatters there).
#include "exit_tree.hpp"

#include <algorithm>
#include <cmath>

namespace frt_exit {
namespace {

constexpr double kU = 1.0 / 16777216.0;   // 2^-24
constexpr double kNoise = 32.0, kOnPlane = 8.0, kRound = 4.0, kMaxAspect = 8.0;

struct V { double x, y, z; };
inline V sub(V a, V b) { return V{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline double dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V cross(V a, V b) { return V{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double len(V a) { return std::sqrt(dot(a, a)); }
inline V at(const double *p) { return V{p[0], p[1], p[2]}; }

}   // namespace

void classify(const frt_shadow::Geometry &g, Hidden &out)
{
    out = Hidden{};
    const int n = std::max(g.n_tris, 0);
    out.n = n;
    out.served.assign((size_t)n, 0);
    out.hidden.assign((size_t)n * n, 0);
    // size of the scene, as the shadow pass takes it: every vertex, sphere and lens point
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    auto grow = [&](const double *p, double r) {
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], p[k] - r); hi[k] = std::max(hi[k], p[k] + r); }
    };
    for (int i = 0; i < 3 * n; ++i) grow(&g.tri_v[3 * i], 0.0);
    for (int i = 0; i < g.n_spheres; ++i) grow(&g.sphere[4 * i], g.sphere[4 * i + 3]);
    grow(g.cam_o, std::fabs(g.lens_r));
    double M = 0.0, Dm = 0.0;
    for (int k = 0; k < 3; ++k) {
        M = std::max(M, std::max(std::fabs(lo[k]), std::fabs(hi[k])));
        Dm += (hi[k] - lo[k]) * (hi[k] - lo[k]);
    }
    Dm = std::sqrt(Dm);
    const double E1 = kNoise * kU * Dm, tau = kOnPlane * kU * M, rnd = kRound * kU * M;
    if (!(2.0 * E1 + rnd + tau < g.eps) || !(M < 1e30)) { out.why = kTooLarge; return; }

    // unit normals and aspects; a degenerate triangle has neither and takes part in no proof
    std::vector<V> ng((size_t)n);
    std::vector<double> rho((size_t)n, 0.0);
    std::vector<uint8_t> usable((size_t)n, 0);
    for (int i = 0; i < n; ++i) {
        const double *v = &g.tri_v[9 * i];
        const V e1 = sub(at(v + 3), at(v)), e2 = sub(at(v + 6), at(v)), c = cross(e1, e2);
        const double l = len(c);
        ng[i] = V{0, 0, 0};
        if (!(l > 0.0)) continue;
        ng[i] = V{c.x / l, c.y / l, c.z / l};
        rho[i] = len(e1) * len(e2) / l;
        usable[i] = rho[i] <= kMaxAspect;
    }
    std::vector<uint8_t> light((size_t)n, 0);
    for (int l = 0; l < g.n_lights; ++l)
        if (!(g.lights[l] & g.sphere_bit) && g.lights[l] >= 0 && g.lights[l] < n) light[g.lights[l]] = 1;

    for (int k = 0; k < n; ++k) {
        if (!usable[k] || light[k] || (g.tri_smooth && g.tri_smooth[k])) continue;
        out.served[k] = 1;
        const V v0 = at(&g.tri_v[9 * k]), m = ng[k];
        const double room = g.eps - (kNoise * kU * rho[k] * Dm + rnd) - tau;   // eps - delta - tau
        for (int j = 0; j < n; ++j) {
            if (!usable[j] || !(room > kNoise * kU * rho[j] * Dm)) continue;
            const double *q = &g.tri_v[9 * j];
            bool under = true;
            for (int c = 0; c < 3 && under; ++c) under = dot(m, sub(at(q + 3 * c), v0)) <= tau;
            out.hidden[(size_t)k * n + j] = under ? 1 : 0;
        }
        if (!out.hidden[(size_t)k * n + k]) out.served[k] = 0;   // (its own inequality failed)
    }
}

void classes(const std::vector<float> &nodes, int main_root, int sphere_bit, int count_shift, const Hidden &h,
             std::vector<Class> &out)
{
    out.clear();
    if (h.why != kRan || main_root < 0) return;
    const int n = h.n, nn = (int)(nodes.size() / 16);
    auto ref_of = [&](int i, int side) {
        int r;
        const float f = nodes[16 * (size_t)i + 12 + side];
        static_assert(sizeof(r) == sizeof(f), "refs are stored as int bits");
        std::copy(reinterpret_cast<const char *>(&f), reinterpret_cast<const char *>(&f) + sizeof(f), reinterpret_cast<char *>(&r));
        return r;
    };
    // every subtree on the way down, with its triangles: the main tree is LDS-resident (a few dozen leaves)
    struct Sub { int ref, level; bool sphere; std::vector<int> tris; };
    struct Leaf { std::vector<int> path; };   // indices into subs, root first, the leaf itself last
    std::vector<Sub> subs;
    std::vector<Leaf> leaves;
    struct Rec {
        decltype(ref_of) &ref;
        std::vector<Sub> &subs;
        std::vector<Leaf> &leaves;
        int sphere_bit, count_shift, n, nn;
        std::vector<int> path;
        bool bad = false;
        int visit(int r, int level)   // returns the index into subs
        {
            const int me = (int)subs.size();
            subs.push_back(Sub{r, level, false, {}});
            path.push_back(me);
            if (r < 0) {
                const int lref = ~r;
                if (lref & sphere_bit) {
                    subs[me].sphere = true;
                } else {
                    const int first = lref & ((1 << count_shift) - 1), count = (lref >> count_shift) + 1;
                    for (int k = 0; k < count; ++k) {
                        if (first + k >= n) { bad = true; break; }
                        subs[me].tris.push_back(first + k);
                    }
                    leaves.push_back(Leaf{path});
                }
            } else if (r >= nn || level > 64) {
                bad = true;
            } else {
                for (int side = 0; side < 2 && !bad; ++side) {
                    const int c = visit(ref(r, side), level + 1);
                    subs[me].sphere |= subs[c].sphere;
                    subs[me].tris.insert(subs[me].tris.end(), subs[c].tris.begin(), subs[c].tris.end());
                }
            }
            path.pop_back();
            return me;
        }
    } rec{ref_of, subs, leaves, sphere_bit, count_shift, n, nn, {}, false};
    rec.visit(main_root, 0);
    if (rec.bad) return;

    for (const Leaf &lf : leaves) {
        const Sub &own = subs[lf.path.back()];
        bool ok = !own.tris.empty();
        for (int k : own.tris) ok = ok && h.served[k];
        if (!ok) continue;
        auto in_d = [&](int j) {   // D(leaf): hidden from every triangle of the leaf
            for (int k : own.tris)
                if (!h.hidden[(size_t)k * n + j]) return false;
            return true;
        };
        int pick = -1;
        for (int s : lf.path) {   // the largest first
            bool all = !subs[s].sphere;
            for (size_t i = 0; i < subs[s].tris.size() && all; ++i) all = in_d(subs[s].tris[i]);
            if (all) { pick = s; break; }
        }
        if (pick < 0 || subs[pick].level == 0) continue;   // its own triangles see each other / nothing would be left
        auto it = std::find_if(out.begin(), out.end(), [&](const Class &c) { return c.sub == subs[pick].ref; });
        if (it == out.end()) {
            Class c;
            c.sub = subs[pick].ref; c.level = subs[pick].level;
            c.dropped.assign((size_t)n, 0);
            for (int j : subs[pick].tris) c.dropped[j] = 1;
            c.n_dropped = (int)subs[pick].tris.size();
            out.push_back(c);
            it = out.end() - 1;
        }
        it->members.insert(it->members.end(), own.tris.begin(), own.tris.end());
    }
    for (Class &c : out) std::sort(c.members.begin(), c.members.end());
}

}   // namespace frt_exit
