// shadow_tree_check.cpp -- csrc/host/shadow_tree.cpp and the per-ray roots of
// csrc/host/tree_refine.cpp's counter with a stand-alone main, for the address and
// undefined-behaviour sanitizers (make shadow_tree_asan): small rooms
// (tests/shadow_tree_scenes.py builds the same ones; its dielectric room is
// refused by flatten_scene's material test before this code is reached) through
// classify and build, and a tree with a second root that shares subtrees through
// tree_cost, with the answers checked.  Exit status 0 when every check holds.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "host/shadow_tree.hpp"
#include "host/tree_refine.hpp"

namespace {

constexpr int kSphereBit = 1 << 30, kCountShift = 27;

struct Room {
    std::vector<double> tri_v, sphere;
    std::vector<int> lights;
    double cam[3] = {0.0, 1.0, 3.9};
    void quad(const double p[4][3], bool flip = false)
    {
        const int order[2][3] = {{0, 1, 2}, {0, 2, 3}};
        for (const auto &t : order)
            for (int k = 0; k < 3; ++k) {
                const double *v = p[flip ? 3 - t[k] : t[k]];
                tri_v.insert(tri_v.end(), v, v + 3);
            }
    }
    int n_tris() const { return (int)(tri_v.size() / 9); }
};

// room open to +z, normals inward; quads in the order floor, ceiling, back, left, right, lamp
Room make_room(double s, bool ceiling, bool flip_back)
{
    Room r;
    const double fl[4][3] = {{-s, 0, s}, {s, 0, s}, {s, 0, -s}, {-s, 0, -s}};
    const double ce[4][3] = {{-s, 2 * s, -s}, {s, 2 * s, -s}, {s, 2 * s, s}, {-s, 2 * s, s}};
    const double ba[4][3] = {{-s, 0, -s}, {s, 0, -s}, {s, 2 * s, -s}, {-s, 2 * s, -s}};
    const double le[4][3] = {{-s, 0, s}, {-s, 0, -s}, {-s, 2 * s, -s}, {-s, 2 * s, s}};
    const double ri[4][3] = {{s, 0, -s}, {s, 0, s}, {s, 2 * s, s}, {s, 2 * s, -s}};
    const double y = 1.98 * s, h = 0.25 * s;
    const double la[4][3] = {{-h, y, -h}, {h, y, -h}, {h, y, h}, {-h, y, h}};
    r.quad(fl);
    if (ceiling) r.quad(ce);
    r.quad(ba, flip_back);
    r.quad(le);
    r.quad(ri);
    r.lights = {r.n_tris(), r.n_tris() + 1};
    r.quad(la);
    for (double &c : r.cam) c *= s;
    return r;
}

int failures = 0;
void check(bool ok, const std::string &what)
{
    if (!ok) { std::printf("FAILED: %s\n", what.c_str()); ++failures; }
}

// classify, then a left-deep tree with one two-triangle leaf per quad through build
void run(const std::string &name, const Room &r, int want_why, const std::vector<int> &want_dropped_quads)
{
    frt_shadow::Geometry g;
    g.n_tris = r.n_tris(); g.tri_v = r.tri_v.data();
    g.n_spheres = (int)(r.sphere.size() / 4); g.sphere = r.sphere.data();
    g.lights = r.lights.data(); g.n_lights = (int)r.lights.size(); g.sphere_bit = kSphereBit;
    for (int k = 0; k < 3; ++k) g.cam_o[k] = r.cam[k];
    g.cam_u[0] = 1.0; g.cam_v[1] = 1.0;
    g.eps = 1e-4;
    frt_shadow::Classified c;
    frt_shadow::classify(g, c);
    check(c.why == want_why, name + ": why");
    const int nq = g.n_tris / 2;
    std::vector<int> got;
    for (int q = 0; q < nq; ++q) {
        check(c.dropped[2 * q] == c.dropped[2 * q + 1], name + ": a quad's triangles agree");
        if (c.dropped[2 * q]) got.push_back(q);
    }
    check(got == want_dropped_quads, name + ": dropped quads");
    // node i: child 0 = leaf of quad i, child 1 = node i + 1 (the last: the last quad's leaf)
    std::vector<float> nodes(16 * (size_t)(nq - 1), 0.0f);
    auto put = [&](int i, int side, int ref) { std::memcpy(&nodes[16 * (size_t)i + 12 + side], &ref, sizeof(ref)); };
    auto leaf = [&](int q) { return ~((2 * q) | (1 << kCountShift)); };
    for (int i = 0; i < nq - 1; ++i) {
        for (int k = 0; k < 3; ++k) { nodes[16 * i + k] = nodes[16 * i + 6 + k] = -3.0f; nodes[16 * i + 3 + k] = nodes[16 * i + 9 + k] = 3.0f; }
        put(i, 0, leaf(i));
        put(i, 1, i + 1 < nq - 1 ? i + 1 : leaf(nq - 1));
    }
    frt_shadow::Tree t;
    frt_shadow::build(nodes, 0, c.dropped, kSphereBit, kCountShift, t);
    check(t.kept_leaves + t.dropped_leaves == nq, name + ": every leaf is kept or dropped");
    check(t.dropped_leaves == (int)got.size(), name + ": dropped leaves");
    check(t.empty == (t.kept_leaves == 0), name + ": empty");
    check((int)(nodes.size() / 16) == nq - 1 + t.added, name + ": appended nodes");
    check(t.empty || t.root < (int)(nodes.size() / 16), name + ": root in range");
    std::printf("%-16s why %d dropped %zu of %d quads, +%d nodes, %d shared, root %d%s\n", name.c_str(), c.why, got.size(), nq,
                t.added, t.shared, t.root, t.empty ? " (empty)" : "");
}

// tree_cost with a root per ray: leaves 0..3; main tree n0 = (l0, n1), n1 = (l1, n2), n2 = (l2, l3); a
// second tree behind it, n3 = (l1, n2) sharing n2 and n4 = (l0, n3); rays start at n0, n4, n3 or at leaf l2
void counter_roots()
{
    using namespace frt_refine;
    const int L = 4, n = 64;
    Topology t;
    t.n_leaves = L; t.root = L;
    t.child = {0, L + 1, 1, L + 2, 2, 3, 1, L + 2, 0, L + 3};
    RaySet R;
    R.n = n; R.n_leaves = L; R.n_prims = L;
    R.prim_first = {0, 1, 2, 3, 4};
    R.prim_ref = {0, 1, 2, 3};
    R.tmin.assign(n, 1e-4f); R.tmax.assign(n, 1.0f); R.anyhit.assign(n, 1); R.live.assign(n, 1);
    R.slab.resize((size_t)n * L * 6);
    R.prim_t.resize((size_t)n * L);
    uint32_t x = 12345u;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (float)(x >> 8) / 16777216.0f; };
    for (int r = 0; r < n; ++r)
        for (int l = 0; l < L; ++l) {
            float *q = &R.slab[((size_t)r * L + l) * 6];
            for (int k = 0; k < 3; ++k) { q[k] = rnd() * 0.6f - 0.2f; q[3 + k] = -(q[k] + rnd() * 0.8f); }   // near, minus far
            R.prim_t[(size_t)r * L + l] = rnd() < 0.3f ? 0.1f + 0.8f * rnd() : -1.0f;
        }
    const Cost main_cost = tree_cost(t, R);
    R.root.assign(n, t.root);
    const Cost same = tree_cost(t, R);
    check(same.V == main_cost.V && same.T == main_cost.T, "counter: every ray at the root is the plain count");
    R.root.assign(n, 2);   // a leaf root: no node visit, at most one test a ray
    const Cost leaf = tree_cost(t, R);
    check(leaf.V == 0.0 && leaf.T == 1.0, "counter: a leaf root");
    const int roots[4] = {L + 0, L + 4, L + 3, 2};
    for (int r = 0; r < n; ++r) R.root[r] = roots[r % 4];
    const Cost mixed = tree_cost(t, R);
    check(mixed.V > 0.0 && mixed.V <= 3.0 && mixed.T <= 4.0, "counter: mixed roots");
    R.root.assign(n, L + 3);   // n3 = (l1, n2): at most two visits, never leaf 0
    const Cost sub = tree_cost(t, R);
    check(sub.V >= 1.0 && sub.V <= 2.0 && sub.T <= 3.0, "counter: the second root's subtree");
    std::printf("%-16s main V %.3f T %.3f, second root V %.3f T %.3f, mixed V %.3f T %.3f\n", "counter_roots", main_cost.V,
                main_cost.T, sub.V, sub.T, mixed.V, mixed.T);
}

}   // namespace

int main()
{
    run("room", make_room(1.0, true, false), frt_shadow::kRan, {0, 2, 3, 4, 5});
    run("outward_normal", make_room(1.0, true, true), frt_shadow::kRan, {0, 3, 4, 5});
    run("empty_room", make_room(1.0, false, false), frt_shadow::kRan, {0, 1, 2, 3, 4});
    run("scaled", make_room(1000.0, true, false), frt_shadow::kTooLarge, {});
    Room behind = make_room(1.0, true, false);
    behind.cam[2] = -3.9;
    run("outside_camera", behind, frt_shadow::kRan, {0, 3, 4, 5});
    Room balls = make_room(1.0, true, false);
    balls.sphere = {0.4, 0.0, 0.3, 0.3, 0.0, 1.0, -1.0, 0.2};
    balls.lights.push_back(kSphereBit | 1);
    run("spheres", balls, frt_shadow::kRan, {3, 4});
    Room dark = make_room(1.0, true, false);
    dark.lights.clear();
    run("no_lights", dark, frt_shadow::kNoLights, {});
    // a ramp whose lower edge lies in the floor's plane and whose normal points down: the floor stays
    Room ramp = make_room(1.0, true, false);
    const double rp[4][3] = {{-0.5, 0.0, -0.5}, {-0.5, 0.6, 0.1}, {0.5, 0.6, 0.1}, {0.5, 0.0, -0.5}};
    ramp.quad(rp, true);
    run("ramp", ramp, frt_shadow::kRan, {2, 3, 4, 5});
    // a second light in the plane x = 0.98: no lights' plane, and the right wall is too near it
    Room two = make_room(1.0, true, false);
    const double sd[4][3] = {{0.98, 0.8, -0.2}, {0.98, 0.8, 0.2}, {0.98, 1.2, 0.2}, {0.98, 1.2, -0.2}};
    two.lights.push_back(two.n_tris());
    two.lights.push_back(two.n_tris() + 1);
    two.quad(sd);
    run("two_lights", two, frt_shadow::kRan, {0, 2, 3});
    counter_roots();
    std::printf(failures ? "%d checks failed\n" : "all checks hold\n", failures);
    return failures ? 1 : 0;
}
