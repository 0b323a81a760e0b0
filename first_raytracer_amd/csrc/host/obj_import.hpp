// obj_import.hpp -- OBJ/MTL text to ObjData (csrc/host/obj_import.cpp), with the
// semantics of Assimp 5.0.1's OBJ import as mesh_loader::load_obj uses it.
// Knows nothing of frt_host_scene: csrc/host/scene.cpp turns ObjData into
// triangles, csrc/host/tessellate.cpp reads faces and materials through it.
//
// The index rule (face_corners): an index is 1-based, or negative = relative to
// the elements read so far; it is resolved and checked in `long`, before any
// narrowing.  A vertex index that is missing, not a number, 0, outside
// [1, count], below -count or not representable refuses the file, and so does
// such a normal index where one is written (a corner without one has no
// normal).  A texture index that is missing or out of range is no error: the
// mesh then has no uv.  A corner ends at white space.  A face keeps its first
// kFaceMax corners -- for the importer as always, for the tessellator since it
// shares this tokenizer.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

namespace frt_obj {

struct Mtl {
    std::string name;
    float kd[3] = {0.6f, 0.6f, 0.6f}, ks[3] = {0, 0, 0}, ke[3] = {0, 0, 0};
    float d = 1.0f, ni = 1.0f, ns = 0.0f;
};
struct ObjMesh {
    int mtl = -2;  // -2: no material
    std::vector<int> v;   // 3 per face
    std::vector<int> vn;  // 3 per face (-1 = none)
    std::vector<int> vt;  // 3 per face (-1 = none)
};
struct ObjData {
    std::vector<float> v, vn, vt;   // vt: 2 per texture vertex (u, v)
    std::vector<Mtl> mats;
    std::vector<ObjMesh> meshes;
};

inline const char *skip_ws(const char *p)
{
    while (*p == ' ' || *p == '\t') ++p;
    return p;
}
std::string dir_of(const std::string &path);
std::string rstrip(std::string s);

// ---------------------------------------------------------------------------
// Assimp fast_atoreal_move<float> (restated): integer part -> float, up to 15
// fractional digits as an integer scaled by a double table, added in float.
// parse_float returns the first character it did not consume.  Inline here: a
// position-independent build does not inline an exported function, and the
// import calls it three times a vertex line.
// ---------------------------------------------------------------------------
inline constexpr double kAtofTable[16] = {0.0, 0.1, 0.01, 0.001, 0.0001, 0.00001, 0.000001, 0.0000001, 0.00000001, 0.000000001,
                               0.0000000001, 0.00000000001, 0.000000000001, 0.0000000000001, 0.00000000000001,
                               0.000000000000001};
inline uint64_t strtoul10_64(const char *in, const char **out, unsigned *max_inout)
{
    unsigned cur = 0;
    uint64_t value = 0;
    while (*in >= '0' && *in <= '9') {
        const uint64_t nv = value * 10 + (uint64_t)(*in - '0');
        if (nv < value) break;
        value = nv;
        ++in;
        ++cur;
        if (max_inout && *max_inout == cur) {
            while (*in >= '0' && *in <= '9') ++in;
            break;
        }
    }
    if (out) *out = in;
    if (max_inout) *max_inout = cur;
    return value;
}

inline const char *parse_float(const char *c, float &out)
{
    float f = 0.0f;
    const bool inv = (*c == '-');
    if (inv || *c == '+') ++c;
    if (!((*c >= '0' && *c <= '9') || ((*c == '.' || *c == ',') && c[1] >= '0' && c[1] <= '9'))) {
        out = 0.0f;
        return c;
    }
    if (!(*c == '.' || *c == ',')) f = (float)strtoul10_64(c, &c, nullptr);
    if ((*c == '.' || *c == ',') && c[1] >= '0' && c[1] <= '9') {
        ++c;
        unsigned diff = 15;
        double pl = (double)strtoul10_64(c, &c, &diff);
        pl *= kAtofTable[diff];
        f += (float)pl;
    } else if (*c == '.') {
        ++c;
    }
    if (*c == 'e' || *c == 'E') {
        ++c;
        const bool einv = (*c == '-');
        if (einv || *c == '+') ++c;
        float ex = (float)strtoul10_64(c, &c, nullptr);
        if (einv) ex = -ex;
        f *= std::pow(10.0f, ex);
    }
    out = inv ? -f : f;
    return c;
}

bool load_mtl(const std::string &path, ObjData &od);   // false: unreadable (not fatal to an import)

constexpr int kFaceMax = 64;
struct Corner {
    int v, vt, vn;   // 0-based into the elements read so far; vt, vn: -1 = none
};
// the corners of the face line whose text after "f" is `q`, against `nv` vertices,
// `nt` texture vertices and `nn` normals: their number (0 .. kFaceMax), or -1 for
// a line the index rule refuses
int face_corners(const char *q, size_t nv, size_t nt, size_t nn, Corner *out);

// FRT_OK, FRT_E_IO (unreadable file) or FRT_E_INVALID (a face the index rule refuses)
int parse_obj(const std::string &path, ObjData &od);

// GenVertexNormalsProcess: 3 floats per corner of `m` into `cn`
void smooth_normals(const ObjData &od, const ObjMesh &m, std::vector<float> &cn);

double from_srgb(double v);  // util.h:62-66

}  // namespace frt_obj
