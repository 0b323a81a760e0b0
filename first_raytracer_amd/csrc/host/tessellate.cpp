// tessellate.cpp -- the cornell_1m generator: non-emissive
// quads -> k x k cells.  Faces are read by the importer's tokenizer
// (csrc/host/obj_import.hpp), so its index rule holds here too: a bad index or a
// token that is no number gives FRT_E_INVALID, and a face keeps its first 64
// corners.  The output is closed on every path; after an error its content is
// unspecified.
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "frt.h"
#include "obj_import.hpp"

namespace {

using namespace frt_obj;

int tessellate(const char *src_obj, int k, const char *dst_obj)
{
    std::ifstream in(src_obj);
    if (!in) return FRT_E_IO;
    std::string dst = dst_obj;
    std::string mtl_dst = dst.substr(0, dst.size() >= 4 ? dst.size() - 4 : dst.size()) + ".mtl";
    // find and copy the material library next to the output
    std::vector<std::string> lines;
    std::string line, mtllib;
    while (std::getline(in, line)) {
        lines.push_back(line);
        const char *p = skip_ws(line.c_str());
        if (!strncmp(p, "mtllib", 6)) mtllib = rstrip(skip_ws(p + 6));
    }
    std::map<std::string, bool> emissive;
    if (!mtllib.empty()) {
        ObjData od;
        load_mtl(dir_of(src_obj) + mtllib, od);
        for (auto &m : od.mats) emissive[m.name] = (m.ke[0] != 0 || m.ke[1] != 0 || m.ke[2] != 0);
        std::ifstream mi(dir_of(src_obj) + mtllib, std::ios::binary);
        std::ofstream mo(mtl_dst, std::ios::binary);
        if (!mi || !mo) return FRT_E_IO;
        mo << mi.rdbuf();
    }
    const std::unique_ptr<FILE, int (*)(FILE *)> out(fopen(dst_obj, "w"), fclose);
    FILE *f = out.get();
    if (!f) return FRT_E_IO;
    const size_t slash = mtl_dst.find_last_of('/');
    fprintf(f, "# cornell-shaped tessellation (k=%d) of %s\nmtllib %s\n", k, src_obj,
            (slash == std::string::npos ? mtl_dst : mtl_dst.substr(slash + 1)).c_str());
    std::vector<std::string> vtok;  // raw vertex tokens of the source (positions)
    size_t n_vt = 0, n_vn = 0;
    std::string cur_mtl;
    for (const std::string &ln : lines) {
        const char *p = skip_ws(ln.c_str());
        if (p[0] == 'v' && (p[1] == ' ' || p[1] == '\t')) {
            vtok.push_back(rstrip(skip_ws(p + 1)));
        } else if (p[0] == 'v' && (p[1] == 't' || p[1] == 'n')) {
            ++(p[1] == 't' ? n_vt : n_vn);
        } else if (!strncmp(p, "usemtl", 6)) {
            cur_mtl = rstrip(skip_ws(p + 6));
            fprintf(f, "%s\n", rstrip(p).c_str());
        } else if ((p[0] == 'g' || p[0] == 'o') && (p[1] == ' ' || p[1] == '\t')) {
            fprintf(f, "%s\n", rstrip(p).c_str());
        } else if (p[0] == 'f' && (p[1] == ' ' || p[1] == '\t')) {
            Corner c[kFaceMax];
            const int nc = face_corners(p + 1, vtok.size(), n_vt, n_vn, c);
            if (nc < 0) return FRT_E_INVALID;
            std::vector<std::array<double, 3>> P;
            for (int i = 0; i < nc; ++i) {
                float x, y, z;
                const char *q = vtok[c[i].v].c_str();
                q = parse_float(skip_ws(q), x);
                q = parse_float(skip_ws(q), y);
                parse_float(skip_ws(q), z);
                P.push_back({x, y, z});
            }
            const bool keep = emissive.count(cur_mtl) && emissive[cur_mtl];
            if (P.size() != 4 || keep || k == 1) {  // lights (and non-quads) stay as they are
                for (auto &pt : P) fprintf(f, "v %.9g %.9g %.9g\n", pt[0], pt[1], pt[2]);
                fprintf(f, "f");
                for (size_t i = 0; i < P.size(); ++i) fprintf(f, " %ld", (long)i - (long)P.size());
                fprintf(f, "\n");
                continue;
            }
            // bilinear grid (k+1)^2 over p0..p3, cells as quads (fanned like the source quads)
            for (int j = 0; j <= k; ++j)
                for (int i = 0; i <= k; ++i) {
                    const double s = (double)i / k, tt = (double)j / k;
                    double q[3];
                    for (int d = 0; d < 3; ++d)
                        q[d] = (1 - s) * (1 - tt) * P[0][d] + s * (1 - tt) * P[1][d] + s * tt * P[2][d] + (1 - s) * tt * P[3][d];
                    fprintf(f, "v %.9g %.9g %.9g\n", q[0], q[1], q[2]);
                }
            const long nvert = (long)(k + 1) * (k + 1);
            for (int j = 0; j < k; ++j)
                for (int i = 0; i < k; ++i) {
                    const long a = j * (k + 1) + i, b = a + 1, c4 = a + (k + 1) + 1, d = a + (k + 1);
                    fprintf(f, "f %ld %ld %ld %ld\n", a - nvert, b - nvert, c4 - nvert, d - nvert);
                }
        }
    }
    return FRT_OK;
}

}  // namespace

extern "C" int frt_write_tessellated_obj(const char *src_obj, int k, const char *dst_obj)
{
    if (!src_obj || !dst_obj || k < 1) return FRT_E_INVALID;
    return frt_guard([&] { return tessellate(src_obj, k, dst_obj); });
}
