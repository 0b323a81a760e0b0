// obj_import.cpp -- OBJ/MTL ingest with the semantics of mesh_loader::load_obj
// (first_ray/mesh_loader.cpp:5-162) on top of Assimp 5.0.1's OBJ import
// (object/material mesh split, fast_atoreal_move parsing, quad triangulation,
// GenSmoothNormals) -- Assimp is absent from this image, its behaviour is
// restated ("unpinned at the Assimp boundary").  Where Assimp throws
// "index out of range" and the reference reports a failed import, parse_obj
// refuses the file (obj_import.hpp: the index rule).
#include "obj_import.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <unordered_map>

#include "frt.h"

namespace frt_obj {

namespace {

constexpr double kPi = 3.14159265358979323846;

inline void fdivs(float *v, float f)  // aiVector3t::operator/=
{
    if (f == 1.0f) return;
    const float inv = 1.0f / f;
    v[0] *= inv; v[1] *= inv; v[2] *= inv;
}

// TriangulateProcess: a quad is fanned from its concave vertex (or vertex 0)
int quad_start(const ObjData &od, const Corner *c)
{
    for (int i = 0; i < 4; ++i) {
        const float *v0 = &od.v[3 * c[(i + 3) % 4].v], *v1 = &od.v[3 * c[(i + 2) % 4].v];
        const float *v2 = &od.v[3 * c[(i + 1) % 4].v], *v = &od.v[3 * c[i].v];
        float l[3] = {v0[0] - v[0], v0[1] - v[1], v0[2] - v[2]};
        float dg[3] = {v1[0] - v[0], v1[1] - v[1], v1[2] - v[2]};
        float r[3] = {v2[0] - v[0], v2[1] - v[1], v2[2] - v[2]};
        fdivs(l, std::sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]));
        fdivs(dg, std::sqrt(dg[0] * dg[0] + dg[1] * dg[1] + dg[2] * dg[2]));
        fdivs(r, std::sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
        const float angle = std::acos(l[0] * dg[0] + l[1] * dg[1] + l[2] * dg[2]) +
                            std::acos(r[0] * dg[0] + r[1] * dg[1] + r[2] * dg[2]);
        if (angle > (float)kPi) return i;
    }
    return 0;
}

// One index of a face corner at `q`.  *idx: its 0-based position among `count`
// elements, -1 where no number stands at q, -2 for a number that names none of
// them (0, out of range, not representable).  Returns the first character after it.
// A corner ends at white space (ObjFileParser::getFace): "1/ 2" is two corners, and
// strtol must not skip ahead and take the next corner's vertex for this one's vt.
const char *face_index(const char *q, size_t count, int *idx)
{
    if (*q == ' ' || *q == '\t') return *idx = -1, q;
    char *e;
    const long a = strtol(q, &e, 10);   // (LONG_MAX / LONG_MIN for what a long cannot hold: out of range below)
    const long n = (long)std::min(count, (size_t)INT_MAX);
    if (e == q) *idx = -1;
    else if (a == 0 || a > n || a < -n) *idx = -2;
    else *idx = (int)(a < 0 ? n + a : a - 1);
    return e;
}

}  // namespace

std::string dir_of(const std::string &path)
{
    const size_t s = path.find_last_of('/');
    return s == std::string::npos ? std::string() : path.substr(0, s + 1);
}
std::string rstrip(std::string s)
{
    while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ' || s.back() == '\t')) s.pop_back();
    return s;
}

bool load_mtl(const std::string &path, ObjData &od)
{
    std::ifstream f(path);
    if (!f) return false;
    std::string line;
    Mtl *cur = nullptr;
    while (std::getline(f, line)) {
        line = rstrip(line);
        const char *p = skip_ws(line.c_str());
        if (!strncmp(p, "newmtl", 6)) {
            od.mats.emplace_back();
            cur = &od.mats.back();
            cur->name = skip_ws(p + 6);
            continue;
        }
        if (!cur) continue;
        float *dst = nullptr;
        int n = 1;
        const char *q = nullptr;
        if (p[0] == 'K' && p[1] && (p[2] == ' ' || p[2] == '\t')) {
            if (p[1] == 'd') dst = cur->kd;
            else if (p[1] == 's') dst = cur->ks;
            else if (p[1] == 'e') dst = cur->ke;
            n = 3;
            q = p + 2;
        } else if (p[0] == 'd' && (p[1] == ' ' || p[1] == '\t')) {
            dst = &cur->d; q = p + 1;
        } else if (p[0] == 'N' && p[1] == 'i') {
            dst = &cur->ni; q = p + 2;
        } else if (p[0] == 'N' && p[1] == 's') {
            dst = &cur->ns; q = p + 2;
        } else if (p[0] == 'T' && p[1] == 'r') {
            float tr;
            parse_float(skip_ws(p + 2), tr);
            cur->d = 1.0f - tr;
            continue;
        }
        if (!dst) continue;
        for (int k = 0; k < n; ++k) q = parse_float(skip_ws(q), dst[k]);
    }
    return true;
}

int face_corners(const char *q, size_t nv, size_t nt, size_t nn, Corner *out)
{
    int n = 0;
    while (*q && n < kFaceMax) {
        q = skip_ws(q);
        if (!*q || *q == '\r' || *q == '\n') break;
        Corner c{-1, -1, -1};
        q = face_index(q, nv, &c.v);
        if (c.v < 0) return -1;
        if (*q == '/') {
            ++q;
            if (*q != '/') q = face_index(q, nt, &c.vt);
            if (*q == '/') q = face_index(q + 1, nn, &c.vn);
        }
        if (c.vn == -2) return -1;
        if (c.vt == -2) c.vt = -1;
        while (*q && *q != ' ' && *q != '\t') ++q;
        out[n++] = c;
    }
    return n;
}

int parse_obj(const std::string &path, ObjData &od)
{
    std::ifstream f(path);
    if (!f) return FRT_E_IO;
    std::string line, group;
    ObjMesh *cur = nullptr;
    int cur_mtl = -2;
    bool any_group = false;
    auto new_mesh = [&](int m) {
        od.meshes.emplace_back();
        od.meshes.back().mtl = m;
        return &od.meshes.back();
    };
    while (std::getline(f, line)) {
        const char *p = skip_ws(line.c_str());
        if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
            const char *q = p + 1;
            for (int k = 0; k < 3; ++k) {
                float x;
                q = parse_float(skip_ws(q), x);
                od.v.push_back(x);
            }
        } else if (p[0] == 'v' && p[1] == 'n') {
            const char *q = p + 2;
            for (int k = 0; k < 3; ++k) {
                float x;
                q = parse_float(skip_ws(q), x);
                od.vn.push_back(x);
            }
        } else if (p[0] == 'v' && p[1] == 't') {
            const char *q = p + 2;
            for (int k = 0; k < 2; ++k) {       // u, v (Assimp keeps a third component; uv uses two)
                float x;
                q = parse_float(skip_ws(q), x);
                od.vt.push_back(x);
            }
        } else if (!strncmp(p, "mtllib", 6)) {
            load_mtl(dir_of(path) + rstrip(skip_ws(p + 6)), od);
        } else if ((p[0] == 'g' || p[0] == 'o') && (p[1] == ' ' || p[1] == '\t' || p[1] == 0 || p[1] == '\r')) {
            // ObjFileParser: a new group name starts a new object whose first mesh inherits the material
            const std::string nm = rstrip(skip_ws(p + 1));
            if (cur && any_group && nm == group) continue;
            group = nm;
            any_group = true;
            cur = new_mesh(cur_mtl);
        } else if (!strncmp(p, "usemtl", 6)) {
            const std::string nm = rstrip(skip_ws(p + 6));
            int idx = -1;
            for (size_t i = 0; i < od.mats.size(); ++i)
                if (od.mats[i].name == nm) idx = (int)i;
            if (idx < 0) {  // unknown: a named default material
                od.mats.emplace_back();
                od.mats.back().name = nm;
                idx = (int)od.mats.size() - 1;
            }
            if (idx == cur_mtl && cur) continue;
            cur_mtl = idx;
            if (!cur) {
                cur = new_mesh(cur_mtl);
                continue;
            }
            if (cur->mtl != -2 && cur->mtl != idx && !cur->v.empty()) cur = new_mesh(cur_mtl);  // needsNewMesh
            else cur->mtl = idx;
        } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
            if (!cur) cur = new_mesh(cur_mtl);
            Corner c[kFaceMax];
            const int nv = face_corners(p + 1, od.v.size() / 3, od.vt.size() / 2, od.vn.size() / 3, c);
            if (nv < 0) return FRT_E_INVALID;
            auto push = [&](int a, int b, int d) {
                cur->v.insert(cur->v.end(), {c[a].v, c[b].v, c[d].v});
                cur->vn.insert(cur->vn.end(), {c[a].vn, c[b].vn, c[d].vn});
                cur->vt.insert(cur->vt.end(), {c[a].vt, c[b].vt, c[d].vt});
            };
            if (nv == 3) {
                push(0, 1, 2);
            } else if (nv == 4) {
                const int s = quad_start(od, c);
                push(s, (s + 1) % 4, (s + 2) % 4);
                push(s, (s + 2) % 4, (s + 3) % 4);
            } else if (nv > 4) {
                for (int k = 1; k + 1 < nv; ++k) push(0, k, k + 1);
            }
        }
    }
    return FRT_OK;
}

// GenVertexNormalsProcess, default 175 degree limit: every corner gets the
// normalised sum of the face normals of all corners within epsilon of it.
void smooth_normals(const ObjData &od, const ObjMesh &m, std::vector<float> &cn)
{
    const size_t nf = m.v.size() / 3, nc = m.v.size();
    std::vector<float> fn(3 * nf);
    float lo[3] = {1e30f, 1e30f, 1e30f}, hi[3] = {-1e30f, -1e30f, -1e30f};
    for (size_t f = 0; f < nf; ++f) {
        const float *a = &od.v[3 * m.v[3 * f]], *b = &od.v[3 * m.v[3 * f + 1]], *c = &od.v[3 * m.v[3 * f + 2]];
        const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
        const float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        float n[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const float l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        if (l > 0.0f) fdivs(n, l);
        memcpy(&fn[3 * f], n, sizeof n);
        for (int k = 0; k < 3; ++k) {
            const float *v = &od.v[3 * m.v[3 * f + k]];
            for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], v[d]); hi[d] = std::max(hi[d], v[d]); }
        }
    }
    const float dd[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    const float eps = std::sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]) * 1e-4f;
    const float eps2 = eps * eps;
    // grid hashing with cell = eps (neighbour cells searched)
    const float cell = eps > 0.0f ? eps : 1.0f;
    auto key = [&](int64_t ix, int64_t iy, int64_t iz) {
        return (uint64_t)(ix * 73856093LL) ^ (uint64_t)(iy * 19349663LL) ^ (uint64_t)(iz * 83492791LL);
    };
    std::unordered_multimap<uint64_t, size_t> grid;
    grid.reserve(nc * 2);
    auto cell_of = [&](const float *v, int64_t *c3) {
        for (int d = 0; d < 3; ++d) c3[d] = (int64_t)std::floor((v[d] - lo[d]) / cell);
    };
    for (size_t i = 0; i < nc; ++i) {
        int64_t c3[3];
        cell_of(&od.v[3 * m.v[i]], c3);
        grid.emplace(key(c3[0], c3[1], c3[2]), i);
    }
    cn.assign(3 * nc, 0.0f);
    std::vector<size_t> found;
    for (size_t i = 0; i < nc; ++i) {
        const float *pi = &od.v[3 * m.v[i]];
        int64_t c3[3];
        cell_of(pi, c3);
        found.clear();
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    auto r = grid.equal_range(key(c3[0] + dx, c3[1] + dy, c3[2] + dz));
                    for (auto it = r.first; it != r.second; ++it) {
                        const float *pj = &od.v[3 * m.v[it->second]];
                        const float d3[3] = {pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2]};
                        if (d3[0] * d3[0] + d3[1] * d3[1] + d3[2] * d3[2] < eps2) found.push_back(it->second);
                    }
                }
        std::sort(found.begin(), found.end());
        found.erase(std::unique(found.begin(), found.end()), found.end());
        float acc[3] = {0, 0, 0};
        for (size_t j : found) {
            acc[0] += fn[3 * (j / 3)];
            acc[1] += fn[3 * (j / 3) + 1];
            acc[2] += fn[3 * (j / 3) + 2];
        }
        const float l = std::sqrt(acc[0] * acc[0] + acc[1] * acc[1] + acc[2] * acc[2]);
        if (l > 0.0f) fdivs(acc, l);
        memcpy(&cn[3 * i], acc, sizeof acc);
    }
}

double from_srgb(double v)
{
    if (v <= 0.04045) return v * (1.0 / 12.92);
    return std::pow((v + 0.055) * (1.0 / 1.055), 2.4);
}

}  // namespace frt_obj
