// scene.cpp -- the frt_host_scene object behind include/frt.h and its C entry points:
//   * create_triangle_mesh (triangle.cpp:9-23): one triangle per face of what
//     csrc/host/obj_import.cpp read, emissive meshes feed Scene::lights;
//   * scene constructors cornell_box_obj (main.cpp:222-252) and veach_mis
//     (main.cpp:281-314), camera (camera.h:10-28);
//   * the world's tree: the builders of csrc/host/bvh_build.cpp or the GPU's
//     (csrc/frt_lbvh.hip), installed by install_tree.
// No exception leaves an entry point that allocates (csrc/host/abi_guard.hpp).
#include <chrono>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "abi_guard.hpp"
#include "bvh_build.hpp"
#include "frt.h"
#include "obj_import.hpp"

namespace {

constexpr double kPi = 3.14159265358979323846;

struct V3 {
    double x = 0, y = 0, z = 0;
};
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator*(double t, V3 v) { return {t * v.x, t * v.y, t * v.z}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double length(V3 v) { return std::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }
inline V3 unit(V3 v)
{
    const double l = length(v);
    return {v.x / l, v.y / l, v.z / l};
}

double ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

// ---------------------------------------------------------------------------
// host scene
// ---------------------------------------------------------------------------
struct frt_host_scene {
    std::vector<double> tri_v, tri_n, tri_inv_area, tri_uv;
    std::vector<int32_t> tri_mat;
    std::vector<uint8_t> tri_geo;
    std::vector<double> sphere;
    std::vector<int32_t> sphere_mat;
    std::vector<frt_material> mats;
    std::vector<double> node_box;
    std::vector<int32_t> node_child;
    int32_t root = 0;
    int32_t world_kind = FRT_WORLD_BVH;
    std::vector<int32_t> list, lights;
    std::vector<int32_t> world;   // world prims in insertion order (frt_scene_add_*)
    double cam[7][3] = {};   // origin, llc, horizontal, vertical, u, v, w
    double lens_radius = 0, half_height = 0;
    double env[3] = {0, 0, 0};
    std::vector<frt_image> images;                    // data points into image_data
    std::vector<std::vector<uint8_t>> image_data;
    int env_image = -1;      // frt_scene_set_env_image: index into images, -1 = the constant env
    int bvh_depth = 0;
    double load_ms = 0, build_ms = 0;
    bool finished = true;    // false between frt_scene_new and frt_scene_finish

    int add_material(int type, V3 albedo, V3 emit, V3 specular = {}, double exponent = 0, double ior = 0)
    {
        frt_material m{};
        m.type = type;
        m.albedo[0] = albedo.x; m.albedo[1] = albedo.y; m.albedo[2] = albedo.z;
        m.emit[0] = emit.x; m.emit[1] = emit.y; m.emit[2] = emit.z;
        m.specular[0] = specular.x; m.specular[1] = specular.y; m.specular[2] = specular.z;
        m.exponent = exponent;
        m.ior = ior;
        mats.push_back(m);
        return (int)mats.size() - 1;
    }
    int add_sphere(V3 c, double r, int mat)
    {
        sphere.insert(sphere.end(), {c.x, c.y, c.z, r});
        sphere_mat.push_back(mat);
        return (int)sphere_mat.size() - 1;
    }
    void set_camera(V3 lookfrom, V3 lookat, V3 vup, double vfov, double aspect, double aperture, double focus)
    {
        // camera.h:10-28 (fp64, same operation order)
        lens_radius = aperture / 2;
        const double theta = vfov * kPi / 180.0;
        const double hh = std::tan(theta / 2);
        const double hw = aspect * hh;
        const V3 w = unit(lookfrom - lookat);
        const V3 u = unit(cross(vup, w));
        const V3 v = cross(w, u);
        const V3 llc = ((lookfrom - (hw * focus) * u) - (hh * focus) * v) - focus * w;
        const V3 h = (2 * hw * focus) * u;
        const V3 vv = (2 * hh * focus) * v;
        const V3 all[7] = {lookfrom, llc, h, vv, u, v, w};
        for (int i = 0; i < 7; ++i) { cam[i][0] = all[i].x; cam[i][1] = all[i].y; cam[i][2] = all[i].z; }
        half_height = hh;
    }
};

namespace {

using frt_obj::from_srgb;

// Matrix4x4 (geometry.h:919-1065), row-major double[16]: point transform with
// the w divide (:966-983), Gauss-Jordan inverse with full pivoting
// (Matrix::invert, :857-907), normal_transform = inverse-transpose product (:830-838)
V3 mat4_point(const double *m, const double *v)
{
    const double x = m[0] * v[0] + m[1] * v[1] + m[2] * v[2] + m[3];
    const double y = m[4] * v[0] + m[5] * v[1] + m[6] * v[2] + m[7];
    const double z = m[8] * v[0] + m[9] * v[1] + m[10] * v[2] + m[11];
    const double w = m[12] * v[0] + m[13] * v[1] + m[14] * v[2] + m[15];
    if (w == 1.0) return {x, y, z};
    return {x / w, y / w, z / w};
}
V3 mat4_normal(const double *inv, const double *v)
{
    return {inv[0] * v[0] + inv[4] * v[1] + inv[8] * v[2], inv[1] * v[0] + inv[5] * v[1] + inv[9] * v[2],
            inv[2] * v[0] + inv[6] * v[1] + inv[10] * v[2]};
}
bool mat4_invert(const double *src, double *t)
{
    int indxc[4], indxr[4], ipiv[4] = {0, 0, 0, 0};
    memcpy(t, src, 16 * sizeof(double));
    for (int i = 0; i < 4; i++) {
        int irow = -1, icol = -1;
        double big = 0;
        for (int j = 0; j < 4; j++) {
            if (ipiv[j] == 1) continue;
            for (int k = 0; k < 4; k++) {
                if (ipiv[k] == 0) {
                    if (std::fabs(t[4 * j + k]) >= big) { big = std::fabs(t[4 * j + k]); irow = j; icol = k; }
                } else if (ipiv[k] > 1) {
                    return false;
                }
            }
        }
        ++ipiv[icol];
        if (irow != icol)
            for (int k = 0; k < 4; ++k) std::swap(t[4 * irow + k], t[4 * icol + k]);
        indxr[i] = irow;
        indxc[i] = icol;
        if (t[4 * icol + icol] == 0) return false;
        const double pivinv = 1.0 / t[4 * icol + icol];
        t[4 * icol + icol] = 1.0;
        for (int j = 0; j < 4; j++) t[4 * icol + j] *= pivinv;
        for (int j = 0; j < 4; j++) {
            if (j == icol) continue;
            const double save = t[4 * j + icol];
            t[4 * j + icol] = 0;
            for (int k = 0; k < 4; k++) t[4 * j + k] -= t[4 * icol + k] * save;
        }
    }
    for (int j = 3; j >= 0; j--)
        if (indxr[j] != indxc[j])
            for (int k = 0; k < 4; k++) std::swap(t[4 * k + indxr[j]], t[4 * k + indxc[j]]);
    return true;
}

// mesh_loader::load_obj + create_triangle_mesh (triangle.cpp:9-23), and its
// (file, toWorld, bsdf) overload (triangle.cpp:26-60): every mesh of the file
// takes `bsdf` when given (one material object for all of them), vertices go
// through toWorld and normals through its inverse transpose.  Emissive meshes
// join Scene::lights.  Returns FRT_OK, FRT_E_IO or FRT_E_INVALID (singular matrix,
// a face index the file does not have); the scene is touched only once the whole
// file has been read, so a refused file leaves it as it was.
int add_obj(frt_host_scene &s, const std::string &path, bool geo, const double *to_world = nullptr,
            const frt_material *bsdf = nullptr)
{
    using namespace frt_obj;
    double inv[16];
    if (to_world && !mat4_invert(to_world, inv)) return FRT_E_INVALID;
    ObjData od;
    if (const int rc = parse_obj(path, od)) return rc;
    int shared_mat = -1;
    for (const ObjMesh &m : od.meshes) {
        const size_t nf = m.v.size() / 3;
        if (nf == 0) continue;  // Assimp drops empty meshes
        const Mtl *mt = (m.mtl >= 0) ? &od.mats[m.mtl] : nullptr;
        int type;
        V3 albedo, emit, spec;
        double exponent = 0, ior = 0;
        if (!mt) {  // DefaultMaterial -> lambertian 0.5 (mesh_loader.cpp:107-111)
            type = FRT_MAT_LAMBERTIAN;
            albedo = {0.5, 0.5, 0.5};
        } else if (mt->ke[0] != 0 || mt->ke[1] != 0 || mt->ke[2] != 0) {
            type = FRT_MAT_DIFFUSE_LIGHT;
            emit = {mt->ke[0], mt->ke[1], mt->ke[2]};
        } else if (mt->ks[0] != 0 || mt->ks[1] != 0 || mt->ks[2] != 0) {
            // opacity < 1: dielectric(Ni, FromSrgb(Ks), 1); else modified_phong(FromSrgb(Kd), FromSrgb(Ks), Ns)
            // (mesh_loader.cpp:78-100)
            type = (mt->d < 1.0f) ? FRT_MAT_DIELECTRIC : FRT_MAT_MODIFIED_PHONG;
            albedo = {from_srgb(mt->kd[0]), from_srgb(mt->kd[1]), from_srgb(mt->kd[2])};
            spec = {from_srgb(mt->ks[0]), from_srgb(mt->ks[1]), from_srgb(mt->ks[2])};
            exponent = mt->ns;
            ior = mt->ni;
        } else {
            type = FRT_MAT_LAMBERTIAN;
            albedo = {from_srgb(mt->kd[0]), from_srgb(mt->kd[1]), from_srgb(mt->kd[2])};
        }
        int mat;
        if (bsdf) {                                   // mesh->mat.reset(bsdf)
            if (shared_mat < 0) {
                s.mats.push_back(*bsdf);
                shared_mat = (int)s.mats.size() - 1;
            }
            mat = shared_mat;
            type = bsdf->type;
        } else {
            mat = s.add_material(type, albedo, emit, spec, exponent, ior);
        }
        bool has_vn = true;
        for (int x : m.vn) if (x < 0) { has_vn = false; break; }
        std::vector<float> cn;
        if (has_vn) {
            cn.resize(3 * m.vn.size());
            for (size_t i = 0; i < m.vn.size(); ++i) memcpy(&cn[3 * i], &od.vn[3 * m.vn[i]], 3 * sizeof(float));
        } else if (!geo) {
            smooth_normals(od, m, cn);
        } else {
            cn.assign(3 * m.v.size(), 0.0f);
        }
        // texture coordinates (mesh_loader.cpp:34-38) when every corner has a vt;
        // without them the reference leaves uv uninitialised -- here 0
        bool has_vt = !od.vt.empty();
        for (int x : m.vt) if (x < 0) { has_vt = false; break; }
        const int base = (int)s.tri_mat.size();
        for (size_t f = 0; f < nf; ++f) {
            for (int k = 0; k < 3; ++k)
                for (int d = 0; d < 2; ++d) s.tri_uv.push_back(has_vt ? (double)od.vt[2 * m.vt[3 * f + k] + d] : 0.0);
            double v[9], n[9];
            for (int k = 0; k < 3; ++k)
                for (int d = 0; d < 3; ++d) {
                    v[3 * k + d] = od.v[3 * m.v[3 * f + k] + d];
                    n[3 * k + d] = cn[3 * (3 * f + k) + d];
                }
            if (to_world) {
                for (int k = 0; k < 3; ++k) {
                    const V3 pv = mat4_point(to_world, v + 3 * k), nv = mat4_normal(inv, n + 3 * k);
                    v[3 * k] = pv.x; v[3 * k + 1] = pv.y; v[3 * k + 2] = pv.z;
                    n[3 * k] = nv.x; n[3 * k + 1] = nv.y; n[3 * k + 2] = nv.z;
                }
            }
            s.tri_v.insert(s.tri_v.end(), v, v + 9);
            s.tri_n.insert(s.tri_n.end(), n, n + 9);
            const V3 e1{v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2{v[6] - v[0], v[7] - v[1], v[8] - v[2]};
            s.tri_inv_area.push_back(1 / (0.5 * length(cross(e1, e2)) * (double)nf));  // triangle.h:65
            s.tri_mat.push_back(mat);
            s.tri_geo.push_back(geo ? 1 : 0);
            if (type == FRT_MAT_DIFFUSE_LIGHT) s.lights.push_back(base + (int)f);
            s.world.push_back(base + (int)f);
        }
    }
    return FRT_OK;
}

// The world of `s` becomes a BVH over `prims` (which may be s.list or s.world):
// no nodes and root 0 over none, a leaf root over one, otherwise the tree that
// make(boxes, tree) builds over their fp64 boxes, its leaves ~slot mapped back to
// prim refs here.  A make that fails leaves the scene as it was.
template <class Make>
int install_tree(frt_host_scene &s, const std::vector<int32_t> &prims, Make make)
{
    const size_t n = prims.size();
    frt_bvh::Tree t;
    if (n == 1) t.root = ~0;
    if (n >= 2)
        if (const int rc = make(frt_bvh::prim_boxes(s.tri_v.data(), s.sphere.data(), prims.data(), n), t)) return rc;
    for (auto &c : t.node_child)
        if (c < 0) c = ~prims[~c];
    s.root = t.root < 0 ? ~prims[~t.root] : t.root;
    s.node_box = std::move(t.node_box);
    s.node_child = std::move(t.node_child);
    s.bvh_depth = t.depth;
    s.world_kind = FRT_WORLD_BVH;
    s.list.clear();
    return FRT_OK;
}
int install_sweep(frt_host_scene &s, const std::vector<int32_t> &prims)   // parallel_bvh_node::create_bvh
{
    return install_tree(s, prims, [](const std::vector<frt_bvh::Box> &b, frt_bvh::Tree &t) {
        t = frt_bvh::build_sweep(b);
        return FRT_OK;
    });
}

bool material_ok(const frt_material *m, const frt_host_scene *s = nullptr)
{
    if (!m) return false;
    if (m->texture == FRT_TEX_IMAGE) {
        if (m->image < 0 || (s && m->image >= (int)s->images.size())) return false;
    } else if (m->texture != FRT_TEX_CONSTANT && m->texture != FRT_TEX_CHECKER) {
        return false;
    }
    switch (m->type) {
    case FRT_MAT_LAMBERTIAN: case FRT_MAT_DIFFUSE_LIGHT: case FRT_MAT_MODIFIED_PHONG: case FRT_MAT_METAL:
    case FRT_MAT_DIELECTRIC: return true;
    case FRT_MAT_ROUGH_CONDUCTOR:
        return m->alpha > 0.0 && (m->distribution == FRT_DIST_GGX || m->distribution == FRT_DIST_BECKMANN);
    default: return false;
    }
}

// the world prims a rebuilt tree covers
const std::vector<int32_t> &world_prims(const frt_host_scene &s)
{
    return s.world_kind == FRT_WORLD_LIST ? s.list : s.world;
}

inline float f_down(double x)
{
    float f = (float)x;
    if ((double)f > x) f = std::nextafter(f, -INFINITY);
    return f;
}
inline float f_up(double x)
{
    float f = (float)x;
    if ((double)f < x) f = std::nextafter(f, INFINITY);
    return f;
}

}  // namespace

extern "C" int frt_scene_create(const char *kind, const char *obj_path, double aspect, frt_host_scene **out)
{
    if (!kind || !obj_path || !out) return FRT_E_INVALID;
    *out = nullptr;
    return frt_guard([&] {
        auto s = std::make_unique<frt_host_scene>();
        const std::string k = kind;
        const auto t0 = std::chrono::steady_clock::now();
        if (k == "cornell_box_obj" || k == "obj_geo" || k == "obj_smooth") {
            if (const int rc = add_obj(*s, obj_path, k != "obj_smooth")) return rc;
            s->world_kind = FRT_WORLD_BVH;
            s->set_camera({0, 1, (double)3.9f}, {0, 1, 0}, {0, 1, 0}, 40.0, aspect, 0.0, 10.0);  // main.cpp:236-242
        } else if (k == "veach_mis") {
            if (const int rc = add_obj(*s, obj_path, false)) return rc;
            // main.cpp:292-302: five emissive spheres in the world list, and five
            // separate identical sphere objects in Scene::lights
            const double cx[5] = {10, (double)-1.25f, (double)-3.75f, (double)1.25f, (double)3.75f};
            const double cy[5] = {10, 0, 0, 0, 0}, cz[5] = {4, 0, 0, 0, 0};
            const double rad[5] = {0.5, (double)0.1f, (double)0.03333f, (double)0.3f, (double)0.9f};
            const double em[5] = {800, 100, (double)901.803f, (double)11.1111f, 1.23457};
            s->world_kind = FRT_WORLD_LIST;
            for (int i = 0; i < (int)s->tri_mat.size(); ++i) s->list.push_back(i);
            for (int j = 0; j < 5; ++j) {
                const int m = s->add_material(FRT_MAT_DIFFUSE_LIGHT, {}, {em[j], em[j], em[j]});
                s->list.push_back(FRT_PRIM_SPHERE | s->add_sphere({cx[j], cy[j], cz[j]}, rad[j], m));
            }
            for (int j = 0; j < 5; ++j) {
                const int m = s->add_material(FRT_MAT_DIFFUSE_LIGHT, {}, {em[j], em[j], em[j]});
                s->lights.push_back(FRT_PRIM_SPHERE | s->add_sphere({cx[j], cy[j], cz[j]}, rad[j], m));
            }
            s->set_camera({0, 2, 15}, {0, -2, 2.5}, {0, 1, 0}, 28.0, aspect, 0.0, 50.0);
        } else {
            return (int)FRT_E_INVALID;
        }
        s->load_ms = ms_since(t0);
        const auto t1 = std::chrono::steady_clock::now();
        if (s->world_kind == FRT_WORLD_BVH) {
            std::vector<int32_t> prims(s->tri_mat.size());
            for (size_t i = 0; i < prims.size(); ++i) prims[i] = (int32_t)i;
            install_sweep(*s, prims);
        }
        s->build_ms = ms_since(t1);
        *out = s.release();
        return (int)FRT_OK;
    });
}

// ---- incremental construction (what main.cpp's scene functions do) ----
extern "C" int frt_scene_new(frt_host_scene **out)
{
    if (!out) return FRT_E_INVALID;
    *out = new (std::nothrow) frt_host_scene();
    if (!*out) return FRT_E_INVALID;
    (*out)->finished = false;
    return FRT_OK;
}

extern "C" int frt_scene_add_obj(frt_host_scene *s, const char *obj_path, const double *to_world16,
                                 const frt_material *bsdf, int use_geometry_normals)
{
    if (!s || !obj_path || s->finished || (bsdf && !material_ok(bsdf, s))) return FRT_E_INVALID;
    const auto t0 = std::chrono::steady_clock::now();
    const int rc = frt_guard([&] { return add_obj(*s, obj_path, use_geometry_normals != 0, to_world16, bsdf); });
    s->load_ms += ms_since(t0);
    return rc;
}

extern "C" int frt_scene_add_sphere(frt_host_scene *s, const double *center, double radius, const frt_material *m,
                                    int where)
{
    if (!s || !center || s->finished || !material_ok(m, s) || !(where & FRT_SPHERE_BOTH)) return FRT_E_INVALID;
    return frt_guard([&] {
        s->mats.push_back(*m);
        const int id = s->add_sphere({center[0], center[1], center[2]}, radius, (int)s->mats.size() - 1);
        if (where & FRT_SPHERE_WORLD) s->world.push_back(FRT_PRIM_SPHERE | id);
        if (where & FRT_SPHERE_LIGHTS) s->lights.push_back(FRT_PRIM_SPHERE | id);
        return (int)FRT_OK;
    });
}

extern "C" int frt_scene_set_camera(frt_host_scene *s, const double *lookfrom, const double *lookat, const double *vup,
                                    double vfov, double aspect, double aperture, double focus_dist)
{
    if (!s || !lookfrom || !lookat || !vup) return FRT_E_INVALID;
    s->set_camera({lookfrom[0], lookfrom[1], lookfrom[2]}, {lookat[0], lookat[1], lookat[2]}, {vup[0], vup[1], vup[2]},
                  vfov, aspect, aperture, focus_dist);
    return FRT_OK;
}

extern "C" int frt_scene_set_env(frt_host_scene *s, const double *rgb)
{
    if (!s || !rgb) return FRT_E_INVALID;
    for (int k = 0; k < 3; ++k) s->env[k] = rgb[k];
    return FRT_OK;
}

// image_texture's image (texture.h:51-95), copied: stb's decoded rows as given
extern "C" int frt_scene_add_image(frt_host_scene *s, const frt_image *img, int *index)
{
    if (!s || !img || !index || s->finished || img->nx <= 0 || img->ny <= 0 || !img->data ||
        (img->format != FRT_IMAGE_SRGB8 && img->format != FRT_IMAGE_F32))
        return FRT_E_INVALID;
    return frt_guard([&] {
        const size_t n = (size_t)img->nx * img->ny * 3 * (img->format == FRT_IMAGE_F32 ? sizeof(float) : 1);
        const uint8_t *src = static_cast<const uint8_t *>(img->data);
        s->image_data.emplace_back(src, src + n);
        frt_image c = *img;
        c.data = s->image_data.back().data();
        s->images.push_back(c);
        *index = (int)s->images.size() - 1;
        return (int)FRT_OK;
    });
}

// Scene::env_map over image `index` (material.h:206-244); the context takes it
// through frt_scene_env_image + frt_set_env_image, the scene view is unchanged
extern "C" int frt_scene_set_env_image(frt_host_scene *s, int index)
{
    if (!s || index < -1 || index >= (int)s->images.size()) return FRT_E_INVALID;
    s->env_image = index;
    return FRT_OK;
}
extern "C" int frt_scene_env_image(const frt_host_scene *s, frt_image *out)
{
    if (!s || !out) return FRT_E_INVALID;
    if (s->env_image < 0) return 0;
    *out = s->images[s->env_image];
    return 1;
}

extern "C" int frt_scene_finish(frt_host_scene *s, int world_kind)
{
    if (!s || s->finished || (world_kind != FRT_WORLD_BVH && world_kind != FRT_WORLD_LIST) || s->world.empty())
        return FRT_E_INVALID;
    return frt_guard([&] {
        const auto t0 = std::chrono::steady_clock::now();
        if (world_kind == FRT_WORLD_BVH) install_sweep(*s, s->world);
        else s->list = s->world;
        s->world_kind = world_kind;
        s->finished = true;
        s->build_ms = ms_since(t0);
        return (int)FRT_OK;
    });
}

extern "C" int frt_scene_build_bvh_sah(frt_host_scene *s)
{
    if (!s || !s->finished || world_prims(*s).empty()) return FRT_E_INVALID;
    return frt_guard([&] {
        const auto t0 = std::chrono::steady_clock::now();
        install_tree(*s, world_prims(*s), [](const std::vector<frt_bvh::Box> &b, frt_bvh::Tree &t) {
            t = frt_bvh::build_binned(b);
            return FRT_OK;
        });
        s->build_ms = ms_since(t0);
        return (int)FRT_OK;
    });
}

// ---- GPU BVH build (frt_lbvh.hip through the context's device) ----
extern "C" int frt_internal_lbvh(frt_ctx *c, int n, const float *box6, int32_t *child2, float *node_box6,
                                 int32_t *order, double *ms, int algo);

extern "C" int frt_scene_build_bvh_gpu(frt_host_scene *s, frt_ctx *ctx, double *device_ms)
{
    return frt_scene_build_bvh_gpu_algo(s, ctx, FRT_GPU_BVH_SAH, device_ms);
}

extern "C" int frt_scene_build_bvh_gpu_algo(frt_host_scene *s, frt_ctx *ctx, int algo, double *device_ms)
{
    if (!s || !ctx || !s->finished || world_prims(*s).empty()) return FRT_E_INVALID;
    return frt_guard([&] {
        const auto t0 = std::chrono::steady_clock::now();
        double ms = 0.0;
        const int rc = install_tree(*s, world_prims(*s), [&](const std::vector<frt_bvh::Box> &b, frt_bvh::Tree &t) {
            // fp32 boxes rounded outward: they contain the fp64 primitives, so the
            // tree's boxes do too (flatten_scene pads them again for the fp32 rays)
            const int n = (int)b.size();
            std::vector<float> box6(6 * (size_t)n);
            for (int i = 0; i < n; ++i)
                for (int k = 0; k < 3; ++k) { box6[6 * i + k] = f_down(b[i].lo[k]); box6[6 * i + 3 + k] = f_up(b[i].hi[k]); }
            std::vector<int32_t> child2(2 * (size_t)(n - 1)), order(n);
            std::vector<float> nb6(6 * (size_t)(n - 1));
            const int rc = frt_internal_lbvh(ctx, n, box6.data(), child2.data(), nb6.data(), order.data(), &ms, algo);
            if (rc != FRT_OK) return rc;
            t.node_box.assign(nb6.begin(), nb6.end());
            t.node_child.resize(child2.size());
            for (size_t i = 0; i < child2.size(); ++i) {   // leaf ~i of the device names box order[i]
                const int c = child2[i];
                if (c < 0 && (~c >= n || order[~c] < 0 || order[~c] >= n)) return (int)FRT_E_HIP;
                if (c >= n - 1) return (int)FRT_E_HIP;
                t.node_child[i] = c >= 0 ? c : ~order[~c];
            }
            t.depth = frt_bvh::tree_depth(t.node_child, t.root);
            return t.depth < 0 ? (int)FRT_E_HIP : (int)FRT_OK;   // not a tree
        });
        if (rc != FRT_OK) return rc;
        s->build_ms = ms_since(t0);
        if (device_ms) *device_ms = ms;
        return (int)FRT_OK;
    });
}

extern "C" int frt_scene_view_get(const frt_host_scene *s, frt_scene_view *v)
{
    if (!s || !v || !s->finished) return FRT_E_INVALID;
    memset(v, 0, sizeof(*v));
    v->world_kind = s->world_kind;
    v->n_tris = (int32_t)s->tri_mat.size();
    v->tri_v = s->tri_v.data();
    v->tri_n = s->tri_n.data();
    v->tri_material = s->tri_mat.data();
    v->tri_geometry_normal = s->tri_geo.data();
    v->tri_inv_area = s->tri_inv_area.data();
    v->tri_uv = s->tri_uv.empty() ? nullptr : s->tri_uv.data();
    v->n_spheres = (int32_t)s->sphere_mat.size();
    v->sphere = s->sphere.data();
    v->sphere_material = s->sphere_mat.data();
    v->n_materials = (int32_t)s->mats.size();
    v->materials = s->mats.data();
    v->n_nodes = (int32_t)(s->node_child.size() / 2);
    v->root = s->root;
    v->node_box = s->node_box.data();
    v->node_child = s->node_child.data();
    v->n_list = (int32_t)s->list.size();
    v->list = s->list.data();
    v->n_lights = (int32_t)s->lights.size();
    v->lights = s->lights.data();
    for (int k = 0; k < 3; ++k) {
        v->cam_origin[k] = s->cam[0][k];
        v->cam_lower_left[k] = s->cam[1][k];
        v->cam_horizontal[k] = s->cam[2][k];
        v->cam_vertical[k] = s->cam[3][k];
        v->cam_u[k] = s->cam[4][k];
        v->cam_v[k] = s->cam[5][k];
        v->cam_w[k] = s->cam[6][k];
        v->env_color[k] = s->env[k];
    }
    v->cam_lens_radius = s->lens_radius;
    v->cam_half_height = s->half_height;
    v->n_images = (int32_t)s->images.size();
    v->images = s->images.empty() ? nullptr : s->images.data();
    return FRT_OK;
}

extern "C" int frt_scene_info(const frt_host_scene *s, frt_host_scene_info *info)
{
    if (!s || !info) return FRT_E_INVALID;
    info->n_tris = (int32_t)s->tri_mat.size();
    info->n_spheres = (int32_t)s->sphere_mat.size();
    info->n_materials = (int32_t)s->mats.size();
    info->n_lights = (int32_t)s->lights.size();
    info->n_nodes = (int32_t)(s->node_child.size() / 2);
    info->world_kind = s->world_kind;
    info->n_list = (int32_t)s->list.size();
    info->bvh_depth = s->bvh_depth;
    info->load_ms = s->load_ms;
    info->build_ms = s->build_ms;
    return FRT_OK;
}

extern "C" void frt_scene_destroy(frt_host_scene *s) { delete s; }
