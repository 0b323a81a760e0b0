// exit_tree_check.cpp -- csrc/host/exit_tree.cpp with a stand-alone main, for the address and
// undefined-behaviour sanitizers (make exit_tree_asan), and the property its proof claims, put to
// the fp32 code the kernels run: for every served triangle k, extension rays made the way
// path_shade makes them -- an incoming ray to a point of k (corners and edges included), the hit
// point p = ro + t rd and the origin p + eps n in fp32, a direction of the cosine lobe around the
// stored normal down to its grazing limit -- go through frt::tri_intersect of every triangle the
// pass hides from k, with leaf_hit's interval (eps, t_max].  No hit may be reported.  The hidden
// set holds every drop set a tree can make of it, so the check needs no tree; the drop sets of a
// left-deep tree go through frt_exit::classes and frt_shadow::build for the sanitizers.
//   exit_tree_check [rays per triangle, default 100000] [an OBJ of triangles / quads, e.g. CornellBox-Original.obj]
// Exit status 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "frt_path.hpp"
#include "host/exit_tree.hpp"

using namespace frt;

namespace {

constexpr int kSphereBit = 1 << 30, kCountShift = 27;

struct Room {
    std::string name;
    std::vector<double> tri_v;
    std::vector<int> lights;
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

// room open to +z, normals inward: floor, ceiling, back, left, right, lamp (tests/shadow_tree_scenes.py)
Room make_room(const std::string &name, bool flip_back)
{
    Room r;
    r.name = name;
    const double s = 1.0;
    const double fl[4][3] = {{-s, 0, s}, {s, 0, s}, {s, 0, -s}, {-s, 0, -s}};
    const double ce[4][3] = {{-s, 2 * s, -s}, {s, 2 * s, -s}, {s, 2 * s, s}, {-s, 2 * s, s}};
    const double ba[4][3] = {{-s, 0, -s}, {s, 0, -s}, {s, 2 * s, -s}, {-s, 2 * s, -s}};
    const double le[4][3] = {{-s, 0, s}, {-s, 0, -s}, {-s, 2 * s, -s}, {-s, 2 * s, s}};
    const double ri[4][3] = {{s, 0, -s}, {s, 0, s}, {s, 2 * s, s}, {s, 2 * s, -s}};
    const double la[4][3] = {{-0.25, 1.98, -0.25}, {0.25, 1.98, -0.25}, {0.25, 1.98, 0.25}, {-0.25, 1.98, 0.25}};
    r.quad(fl);
    r.quad(ce);
    r.quad(ba, flip_back);
    r.quad(le);
    r.quad(ri);
    r.lights = {r.n_tris(), r.n_tris() + 1};
    r.quad(la);
    return r;
}

// v / f lines only (triangles and quads, any of the index forms); the material named "light" emits
bool load_obj(const std::string &path, Room &r)
{
    std::ifstream in(path);
    if (!in) return false;
    std::vector<double> v;
    std::string line, mtl;
    while (std::getline(in, line)) {
        std::istringstream ss(line);
        std::string tag;
        ss >> tag;
        if (tag == "v") { double x, y, z; ss >> x >> y >> z; v.insert(v.end(), {x, y, z}); }
        else if (tag == "usemtl") ss >> mtl;
        else if (tag == "f") {
            std::vector<int> idx;
            std::string w;
            while (ss >> w) {
                const int i = std::atoi(w.c_str());
                idx.push_back(i < 0 ? (int)(v.size() / 3) + i : i - 1);
            }
            for (size_t k = 2; k < idx.size(); ++k) {
                const int t[3] = {idx[0], idx[k - 1], idx[k]};
                if (mtl == "light") r.lights.push_back(r.n_tris());
                for (int c : t) {
                    if (c < 0 || 3 * (size_t)c + 2 >= v.size()) return false;
                    r.tri_v.insert(r.tri_v.end(), &v[3 * (size_t)c], &v[3 * (size_t)c] + 3);
                }
            }
        }
    }
    r.name = path.substr(path.find_last_of('/') + 1);
    return r.n_tris() > 0;
}

int failures = 0;
void check(bool ok, const std::string &what)
{
    if (!ok) { std::printf("FAILED: %s\n", what.c_str()); ++failures; }
}

struct Rng {
    uint32_t x;
    float next() { x = x * 1664525u + 1013904223u; return (float)(x >> 8) / 16777216.0f; }
};

void run(const Room &r, int rays_per_tri)
{
    const int n = r.n_tris();
    frt_shadow::Geometry g;
    g.n_tris = n; g.tri_v = r.tri_v.data();
    g.lights = r.lights.data(); g.n_lights = (int)r.lights.size(); g.sphere_bit = kSphereBit;
    g.cam_o[1] = 1.0; g.cam_o[2] = 3.9; g.cam_u[0] = 1.0; g.cam_v[1] = 1.0;
    g.eps = (double)Cst<float>::eps;
    frt_exit::Hidden h;
    frt_exit::classify(g, h);
    check(h.why == frt_exit::kRan, r.name + ": the proof applies");
    if (h.why != frt_exit::kRan) return;

    // the fp32 records as flatten_scene writes them: v0, e1, e2 and the unit normal, rounded from fp64
    std::vector<f3> v0(n), e1(n), e2(n), nn(n);
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int i = 0; i < n; ++i) {
        const double *v = &r.tri_v[9 * i];
        double a[3], b[3], c[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = v[3 + k] - v[k]; b[k] = v[6 + k] - v[k];
            for (int q = 0; q < 3; ++q) { lo[k] = std::min(lo[k], v[3 * q + k]); hi[k] = std::max(hi[k], v[3 * q + k]); }
        }
        c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
        const double l = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        v0[i] = mk3((float)v[0], (float)v[1], (float)v[2]);
        e1[i] = mk3((float)a[0], (float)a[1], (float)a[2]);
        e2[i] = mk3((float)b[0], (float)b[1], (float)b[2]);
        nn[i] = l > 0.0 ? mk3((float)(c[0] / l), (float)(c[1] / l), (float)(c[2] / l)) : mk3(0.0f, 0.0f, 0.0f);
    }
    long long rays = 0, tests = 0, hits = 0;
    int served = 0, pairs = 0;
    Rng rng{12345u};
    for (int k = 0; k < n; ++k) {
        if (!h.served[k]) continue;
        ++served;
        std::vector<int> hid;
        for (int j = 0; j < n; ++j)
            if (h.hidden[(size_t)k * n + j]) hid.push_back(j);
        pairs += (int)hid.size();
        for (int i = 0; i < rays_per_tri; ++i) {
            // a point of k: corners, edges and the interior in turn
            float b0 = rng.next(), b1 = rng.next();
            if (b0 + b1 > 1.0f) { b0 = 1.0f - b0; b1 = 1.0f - b1; }
            switch (i % 8) {
            case 0: b0 = 0.0f; break;
            case 1: b1 = 0.0f; break;
            case 2: b1 = 1.0f - b0; break;
            case 3: b0 = (float)((i / 8) % 3 == 1); b1 = (float)((i / 8) % 3 == 2); break;
            default: break;
            }
            const f3 target = v0[k] + b0 * e1[k] + b1 * e2[k];
            // the incoming ray, from anywhere in the scene's box on either side of k
            const f3 ro = mk3((float)(lo[0] + (hi[0] - lo[0]) * rng.next()), (float)(lo[1] + (hi[1] - lo[1]) * rng.next()),
                              (float)(lo[2] + (hi[2] - lo[2]) * rng.next()));
            const f3 rd = target - ro;
            float u, v;
            const float t = tri_intersect(ro, rd, v0[k], e1[k], e2[k], Cst<float>::eps, Cst<float>::tmax, u, v);
            const f3 p = t > 0.0f ? ro + t * rd : target;   // (a grazing incoming ray may miss: start on the point itself)
            const f3 o = p + Cst<float>::eps * nn[k];
            // the cosine lobe; every fourth ray at its grazing limit r0 = 1 - 2^-24
            const float r0 = (i % 4 == 3) ? 1.0f - 1.0f / 16777216.0f : rng.next(), r1 = rng.next();
            const f3 wo = onb_local(onb_from_w(nn[k]), cosine_direction(r0, r1));
            ++rays;
            for (int j : hid) {
                ++tests;
                if (tri_intersect(o, wo, v0[j], e1[j], e2[j], Cst<float>::eps, Cst<float>::tmax, u, v) > 0.0f) ++hits;
            }
        }
    }
    check(hits == 0, r.name + ": no hidden triangle reports a hit");
    check(served > 0 && pairs >= served, r.name + ": triangles are served, each hides itself");

    // the drop sets of a left-deep tree with one leaf per pair of triangles, each through build
    const int nl = n / 2;
    int n_classes = 0, added = 0;
    if (nl >= 2) {
        std::vector<float> nodes(16 * (size_t)(nl - 1), 0.0f);
        auto put = [&](int i, int side, int ref) { std::memcpy(&nodes[16 * (size_t)i + 12 + side], &ref, sizeof(ref)); };
        auto leaf = [&](int q) { return ~((2 * q) | (1 << kCountShift)); };
        for (int i = 0; i < nl - 1; ++i) {
            for (int k = 0; k < 3; ++k) { nodes[16 * i + k] = nodes[16 * i + 6 + k] = (float)lo[k]; nodes[16 * i + 3 + k] = nodes[16 * i + 9 + k] = (float)hi[k]; }
            put(i, 0, leaf(i));
            put(i, 1, i + 1 < nl - 1 ? i + 1 : leaf(nl - 1));
        }
        std::vector<frt_exit::Class> cls;
        frt_exit::classes(nodes, 0, kSphereBit, kCountShift, h, cls);
        n_classes = (int)cls.size();
        for (const auto &c : cls) {
            std::vector<float> trial = nodes;
            frt_shadow::Tree t;
            frt_shadow::build(trial, 0, c.dropped, kSphereBit, kCountShift, t);
            check(!t.empty && t.dropped_leaves > 0, r.name + ": a drop set leaves a tree");
            check(t.root < (int)(trial.size() / 16), r.name + ": root in range");
            for (int m : c.members) check(c.dropped[m] != 0, r.name + ": a member's own leaf is dropped");
            added += t.added;
        }
    }
    std::printf("%-28s %3d triangles, %3d served, %4d hidden pairs, %lld rays, %lld tests, %lld hits; %d drop sets, +%d nodes\n",
                r.name.c_str(), n, served, pairs, rays, tests, hits, n_classes, added);
}

}   // namespace

int main(int argc, char **argv)
{
    const int rays = argc > 1 ? std::atoi(argv[1]) : 100000;
    run(make_room("room", false), rays);
    run(make_room("outward_wall", true), rays);
    for (double a : {5e-7, 1e-3}) {   // a quad under the floor whose upper edge stands a above it
        Room r = make_room(a < 1e-6 ? "straddle_less" : "straddle_more", false);
        const double q[4][3] = {{-0.3, -0.5, 0.1}, {0.3, -0.5, 0.1}, {0.3, a, 0.1}, {-0.3, a, 0.1}};
        r.quad(q);
        run(r, rays);
    }
    {   // a box on the floor, its bottom in the floor's plane
        Room r = make_room("box_on_floor", false);
        const double x0 = -0.5, x1 = 0.1, y0 = 0.0, y1 = 0.7, z0 = -0.4, z1 = 0.2;
        const double f[6][4][3] = {
            {{x0, y0, z0}, {x1, y0, z0}, {x1, y0, z1}, {x0, y0, z1}}, {{x0, y1, z0}, {x0, y1, z1}, {x1, y1, z1}, {x1, y1, z0}},
            {{x0, y0, z0}, {x0, y0, z1}, {x0, y1, z1}, {x0, y1, z0}}, {{x1, y0, z0}, {x1, y1, z0}, {x1, y1, z1}, {x1, y0, z1}},
            {{x0, y0, z0}, {x0, y1, z0}, {x1, y1, z0}, {x1, y0, z0}}, {{x0, y0, z1}, {x1, y0, z1}, {x1, y1, z1}, {x0, y1, z1}}};
        for (const auto &q : f) r.quad(q);
        run(r, rays);
    }
    {   // a folded quad (normals up, each triangle above the other's plane) and a slanted wall
        Room r = make_room("fold_and_slant", false);
        const double fo[4][3] = {{-0.4, 0.3, -0.4}, {-0.4, 0.9, 0.4}, {0.4, 0.3, 0.4}, {0.4, 0.3, -0.4}};
        const double sl[4][3] = {{-1, 0, -0.2}, {1, 0, -0.2}, {1, 2, -1}, {-1, 2, -1}};
        r.quad(fo);
        r.quad(sl);
        run(r, rays);
    }
    if (argc > 2) {
        Room r;
        check(load_obj(argv[2], r), std::string("read ") + argv[2]);
        if (r.n_tris() > 0) run(r, rays);
    }
    std::printf(failures ? "%d checks failed\n" : "all checks hold\n", failures);
    return failures ? 1 : 0;
}
