// frt_render.hip -- the library's main kernel unit: the lambertian path, AO,
// normals, ray-query and PSS-MLT kernels (frt_kernels.hpp, frt_plans.hpp), the
// film reductions, and the C-ABI of include/frt.h that launches them.
#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "frt_kernels.hpp"
#include "frt_plans.hpp"
#include "frt_rays.hpp"
#include "frt_flatten.hpp"
#include "frt_lbvh.hpp"
#include "host/envdist.hpp"

namespace {

// film: slot mean = sum over chunks (fixed order) * (1/spp)  (viewer.cpp:111)
__global__ void film_reduce(const float *__restrict__ partial, float *__restrict__ out, uint32_t n_slots,
                            int n_chunks, int spp, int tile, int ntx, int shard_index, int shard_count, int nx, int ny)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const int T2 = tile * tile;
    const int t_ord = (int)(s / (uint32_t)T2), sl = (int)(s % (uint32_t)T2);
    const int tile_id = shard_index + t_ord * shard_count;
    int lx, ly;
    slot_to_local(sl, tile, lx, ly);
    const int px = (tile_id % ntx) * tile + lx, py = (tile_id / ntx) * tile + ly;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (px < nx && py < ny) {
        for (int c = 0; c < n_chunks; ++c) {
            const float *q = partial + 3ull * ((size_t)c * n_slots + s);
            r += q[0]; g += q[1]; b += q[2];
        }
        const float k = 1.0f / (float)spp;
        r *= k; g *= k; b *= k;
    }
    out[3ull * s + 0] = r;
    out[3ull * s + 1] = g;
    out[3ull * s + 2] = b;
}

// ... of the feature integrators (albedo, depth): sum / spp, so that a pixel whose every
// sample added exactly 1 (depth's coverage, a white albedo) is exactly 1.0f at any spp,
// which spp * (1 / spp) is not.  moments: the depth film, whose second moment keeps
// y k >= x^2 (depth_moment_floor).
__global__ void film_reduce_mean(const float *__restrict__ partial, float *__restrict__ out, uint32_t n_slots,
                                 int n_chunks, int spp, int tile, int ntx, int shard_index, int shard_count, int nx, int ny,
                                 int moments)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const int T2 = tile * tile;
    const int t_ord = (int)(s / (uint32_t)T2), sl = (int)(s % (uint32_t)T2);
    const int tile_id = shard_index + t_ord * shard_count;
    int lx, ly;
    slot_to_local(sl, tile, lx, ly);
    const int px = (tile_id % ntx) * tile + lx, py = (tile_id / ntx) * tile + ly;
    float r = 0.0f, g = 0.0f, b = 0.0f;
    if (px < nx && py < ny) {
        for (int c = 0; c < n_chunks; ++c) {
            const float *q = partial + 3ull * ((size_t)c * n_slots + s);
            r += q[0]; g += q[1]; b += q[2];
        }
        const float n = (float)spp;
        r /= n; g /= n; b /= n;
        if (moments) g = depth_moment_floor(r, g, b);
    }
    out[3ull * s + 0] = r;
    out[3ull * s + 1] = g;
    out[3ull * s + 2] = b;
}

__global__ void mlt_film_to_float(const unsigned long long *__restrict__ acc, float *__restrict__ film, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) film[i] = (float)((double)(long long)acc[i] * (1.0 / (double)(1ull << kSplatFix)));
}

}  // namespace

#if defined(FRT_DIAG)
__device__ unsigned long long *frt::frt_diag;
#endif

// ==========================================================================
// host side
// ==========================================================================
extern "C" int frt_get_abi_version(void) { return FRT_ABI_VERSION; }

extern "C" int frt_create(int hip_device, frt_ctx **out)
{
    if (!out) return FRT_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return FRT_E_NO_DEVICE;
    if (hip_device < 0 || hip_device >= n) return FRT_E_NO_DEVICE;
    frt_ctx *c = new frt_ctx();
    c->device = hip_device;
    if (hipSetDevice(hip_device) != hipSuccess) { delete c; return FRT_E_HIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, hip_device) != hipSuccess) { delete c; return FRT_E_HIP; }
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) {
        fprintf(stderr, "frt: device %d is %s, not gfx950\n", hip_device, prop.gcnArchName);
        delete c;
        return FRT_E_NO_DEVICE;
    }
    c->n_cu = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&c->ev0) != hipSuccess || hipEventCreate(&c->ev1) != hipSuccess ||
        hipMalloc(&c->counter, kCounterBytes) != hipSuccess) {
        delete c;
        return FRT_E_HIP;
    }
    *out = c;
    return FRT_OK;
}

static void free_scene(frt_ctx *c)
{
    for (void *p : c->scene_bufs) (void)hipFree(p);
    c->scene_bufs.clear();
    c->have_scene = false;
}

extern "C" int frt_destroy(frt_ctx *c)
{
    if (!c) return FRT_E_INVALID;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    free_scene(c);
    if (c->counter) (void)hipFree(c->counter);
    if (c->env_texels) (void)hipFree(c->env_texels);
    free_comms(c);
    for (DevBufAny *b : c->bufs) b->release();
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return FRT_OK;
}

// without a context: the last refusal of a frtx_*_rays call made without one (frt_rays.hpp), if any
std::string &frt::null_ctx_err()
{
    static thread_local std::string e;
    return e;
}
extern "C" const char *frt_last_error(const frt_ctx *c)
{
    if (c) return c->err.c_str();
    return frt::null_ctx_err().empty() ? "null context" : frt::null_ctx_err().c_str();
}

// Precision of the context's kernels (DESIGN.md "Precision"): read by the
// next frt_upload_scene (which then also uploads the fp64 records) and by
// every render.
extern "C" int frt_set_precision(frt_ctx *c, int precision)
{
    if (!c) return FRT_E_INVALID;
    if (precision != FRT_PRECISION_AUTO && precision != FRT_PRECISION_FP32 && precision != FRT_PRECISION_FP64)
        return set_err(c, FRT_E_INVALID, "precision must be FRT_PRECISION_AUTO, _FP32 or _FP64");
    c->precision = precision;
    return FRT_OK;
}

// GPU BVH build on this context's device and stream (frt_lbvh.hip); called
// by frt_scene_build_bvh_gpu (csrc/host/scene.cpp).  Internal to libfrt.so.
extern "C" int frt_internal_lbvh(frt_ctx *c, int n, const float *box6, int32_t *child2, float *node_box6,
                                 int32_t *order, double *ms, int algo)
{
    if (!c || n < 2 || !box6 || !child2 || !node_box6 || !order) return FRT_E_INVALID;
    if (algo != FRT_GPU_BVH_PLOC && algo != FRT_GPU_BVH_LBVH && algo != FRT_GPU_BVH_SAH)
        return set_err(c, FRT_E_INVALID, "unknown GPU BVH builder");
    HIPCHK(c, hipSetDevice(c->device));
    float dev_ms = 0.0f;
    std::string err;
    if (frt::lbvh_build(c->stream, n, box6, child2, node_box6, order, &dev_ms, err,
                        algo == FRT_GPU_BVH_LBVH ? frt::kGpuBvhLbvh
                        : algo == FRT_GPU_BVH_SAH ? frt::kGpuBvhSah : frt::kGpuBvhPloc) != 0)
        return set_err(c, FRT_E_HIP, err);
    if (ms) *ms = dev_ms;
    return FRT_OK;
}

// Shading starts when at most this many lanes of a wave still traverse
// (0 = every ray of the wave finishes first).  Per plan and integrator, at the
// bench's 1080p / 512 spp (same call, profiles/r02/r02_ab_trav_min_512spp.txt):
// path 28 from LDS (Cornell 308.0 -> 301.4 ms; 12 was round 1's 64-spp
// optimum, profiles/r01_ab_perf6.jsonl) and 40 from HBM (cornell_1m 863.5 ->
// 857.3 ms); PSS-MLT and AO keep 12 / 32 (28 costs them 4-5 %).  Round 4's
// cheaper LDS node loop moved the LDS path optimum to 20 (Cornell 245.3 ->
// 242.5 ms; 16 / 24: 243.4 / 243.7; profiles/r04/r04{h,i}/ab_*.jsonl).
// FRT_TRAV_MIN overrides (tuning knob of this library, not part of the C-ABI).
int trav_min(bool lds_scene, bool path)
{
    const char *e = std::getenv("FRT_TRAV_MIN");
    const int v = e ? std::atoi(e)
                    : path ? (lds_scene ? kTravMinLdsPath : kTravMinHbmPath) : (lds_scene ? kTravMinLds : kTravMinHbm);
    return std::min(std::max(v, 0), 63);
}

// Leaf postponing (bvh2_step): a wave's descent stops once fewer than this
// many of its lanes still descend.  0 = every lane reaches its leaf first.
// HBM plans 12 since round 4 (cornell_1m 512 spp 767.5 -> 760.9 ms over 8, 16:
// 761.6, same call, profiles/r04/r04n; confirmed 765.4 -> 759.2 in r04o).
// FRT_MIN_DESC overrides (tuning knob, not part of the C-ABI).
int min_desc(bool lds_scene)
{
    const char *e = std::getenv("FRT_MIN_DESC");
    const int v = e ? std::atoi(e) : (lds_scene ? kMinDescLds : kMinDescHbm);
    return std::min(std::max(v, 0), 64);
}

template <typename T, typename P>
static int upload_vec(frt_ctx *c, const std::vector<T> &v, P *dst)
{
    void *p = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    HIPCHK(c, hipMalloc(&p, bytes));
    c->scene_bufs.push_back(p);
    if (!v.empty()) HIPCHK(c, hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = (P)p;
    return FRT_OK;
}

// Scene::env_map as environment_map(image_texture): state of the context like
// the precision.  The texels go to a device buffer of their own (the LDS scene
// copy is not touched); renders after this call run the kernels compiled with
// the lookup (kMatsEnv: frt_mats::pick, frt_mats::mlt), NULL returns to the
// uploaded view's env_color and to the kernels the scene ran before.
// The buffer has room behind the texels for the sampling tables of
// FRT_FLAG_ENV_SAMPLING (env_tables): a new image starts without them.
extern "C" int frt_set_env_image(frt_ctx *c, const frt_image *img)
{
    if (!c) return FRT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    float4 *dev = nullptr;
    int nx = 0, ny = 0;
    uint64_t hash = 0;
    if (img) {
        std::vector<float4> tex;
        std::string err;
        const int rc = env_texels_of(img, tex, err);
        if (rc != FRT_OK) return set_err(c, rc, err);
        HIPCHK(c, hipMalloc((void **)&dev, (tex.size() + env_table_records(img->nx, img->ny)) * sizeof(float4)));
        if (hipMemcpy(dev, tex.data(), tex.size() * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipFree(dev);
            return set_err(c, FRT_E_HIP, "frt_set_env_image: copy to the device failed");
        }
        nx = img->nx; ny = img->ny;
        hash = 1469598103934665603ull;   // FNV-1a over the converted texels
        const unsigned char *b = reinterpret_cast<const unsigned char *>(tex.data());
        for (size_t i = 0; i < tex.size() * sizeof(float4); ++i) hash = (hash ^ b[i]) * 1099511628211ull;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));   // no render of this context still reads the old buffer
    if (c->env_texels) (void)hipFree(c->env_texels);
    c->env_texels = dev; c->env_nx = nx; c->env_ny = ny; c->env_hash = hash;
    c->env_tab = frt_ctx::kEnvTabNone;
    c->S.env_texels = dev; c->S.env_nx = nx; c->S.env_ny = ny;
    return FRT_OK;
}

// FRT_FLAG_ENV_SAMPLING: the context's image has its sampling tables behind the
// texels.  Built here, on the host from the texels the kernels read, at the first
// render that wants them; no render in flight reads that part of the buffer.
int env_tables(frt_ctx *c)
{
    if (c->env_tab != frt_ctx::kEnvTabNone) return FRT_OK;
    const size_t n = (size_t)c->env_nx * c->env_ny;
    std::vector<float4> tex(n);
    HIPCHK(c, hipMemcpy(tex.data(), c->env_texels, n * sizeof(float4), hipMemcpyDeviceToHost));
    std::vector<float> tab;
    const bool lit = env_tables_of(&tex[0].x, c->env_nx, c->env_ny, tab);
    HIPCHK(c, hipMemcpy(c->env_texels + n, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice));
    c->env_tab = lit ? frt_ctx::kEnvTabBuilt : frt_ctx::kEnvTabDark;
    return FRT_OK;
}

extern "C" int frt_upload_scene(frt_ctx *c, const frt_scene_view *sv)
{
    if (!c || !sv) return FRT_E_INVALID;
    HIPCHK(c, hipSetDevice(c->device));
    FlatScene F;
    std::string err;
    // fp64 records when this context's precision can pick the fp64 kernels for the scene
    const bool want_f64 = c->precision == FRT_PRECISION_FP64 ||
                          (c->precision == FRT_PRECISION_AUTO && sv->world_kind == FRT_WORLD_LIST);
    const int frc = flatten_scene(sv, F, err, want_f64);
    if (frc != FRT_OK) return set_err(c, frc, err);
    free_scene(c);
    c->S = F.meta;
    DevScene &S = c->S;
    S.env_texels = c->env_texels; S.env_nx = c->env_nx; S.env_ny = c->env_ny;   // context state, kept across uploads
    int rc;
    if ((rc = upload_vec(c, F.nodes, &S.nodes)) || (rc = upload_vec(c, F.nodes4, &S.nodes4)) ||
        (rc = upload_vec(c, F.nodes_oct, &S.nodes_oct)) ||
        (rc = upload_vec(c, F.tris, &S.tris)) ||
        (rc = upload_vec(c, F.tshade, &S.tshade)) || (rc = upload_vec(c, F.tnorm, &S.tnorm)) ||
        (rc = upload_vec(c, F.tuv, &S.tuv)) || (rc = upload_vec(c, F.texels, &S.texels)) ||
        (rc = upload_vec(c, F.spheres, &S.spheres)) || (rc = upload_vec(c, F.smat, &S.sphere_mat)) ||
        (rc = upload_vec(c, F.mats, &S.mats)) || (rc = upload_vec(c, F.lights, &S.lights)) ||
        (rc = upload_vec(c, F.list, &S.list)) || (rc = upload_vec(c, F.tri_view, &S.tri_view)))
        return rc;
    S.tris64 = nullptr; S.tshade64 = nullptr; S.tnorm64 = nullptr; S.spheres64 = nullptr;
    if (want_f64 && ((rc = upload_vec(c, F.tris64, &S.tris64)) || (rc = upload_vec(c, F.tshade64, &S.tshade64)) ||
                     (rc = upload_vec(c, F.tnorm64, &S.tnorm64)) || (rc = upload_vec(c, F.spheres64, &S.spheres64))))
        return rc;
    c->world_kind = S.world_kind;
    c->stack_needed = F.depth;
    c->has_bvh4 = F.has4;
    c->n_tris = S.n_tris;
    c->n_spheres = (int)F.spheres.size();
    c->n_list = S.n_list;
    c->has_spec_mats = false;
    c->has_metal = false;
    c->mats = kMatsNone;
    for (int i = 0; i < sv->n_materials; ++i) {
        const int t = sv->materials[i].type;
        if (t == FRT_MAT_MODIFIED_PHONG || t == FRT_MAT_METAL || t == FRT_MAT_DIELECTRIC) c->mats |= kMatsSpec;
        if (t == FRT_MAT_ROUGH_CONDUCTOR) c->mats |= kMatsRough;
        if (sv->materials[i].texture != FRT_TEX_CONSTANT) c->mats |= kMatsTex;
        if (t == FRT_MAT_METAL) c->has_metal = true;
    }
    c->has_spec_mats = c->mats != kMatsNone;
    c->depth4 = F.depth4;
    c->scene_lds_bytes = lds_planar_bytes(S.n_nodes, lds_rest(F));
    c->scene_lds_bytes_oct = F.nodes_oct.empty() ? SIZE_MAX : lds_octant_bytes(S.n_nodes, lds_rest(F));
    c->has_f64 = want_f64;
    c->have_scene = true;
    return FRT_OK;
}

// ---- shard geometry ----
int eff_tile(const frt_render_params *p) { return p->tile_size > 0 ? p->tile_size : 32; }
constexpr int kRetiredFlags = 32 | 64 | 128;   // frt.h: the round-4 plans measured slower and removed
bool params_ok(const frt_render_params *p)
{
    const int T = eff_tile(p);
    if (!(p && p->nx > 0 && p->ny > 0 && p->spp > 0 && (T % 8) == 0 && T <= 256 && p->shard_count >= 1 &&
          p->shard_index >= 0 && p->shard_index < p->shard_count && p->max_depth >= -1 && p->max_depth < 100000))
        return false;
    if (p->sample_offset < 0 || (int64_t)p->sample_offset + p->spp > (int64_t)0xffffffffLL) return false;
    if ((int64_t)p->nx * p->ny > (int64_t)INT32_MAX) return false;   // pixel indices are int32 (frt_shard_slots)
    if (p->flags & kRetiredFlags) return false;         // removed A/B plans: fail loudly, not silently
    if (p->integrator == FRT_INTEGRATOR_PATH || p->integrator == FRT_INTEGRATOR_AO ||
        p->integrator == FRT_INTEGRATOR_NORMALS || p->integrator == FRT_INTEGRATOR_ALBEDO ||
        p->integrator == FRT_INTEGRATOR_DEPTH || p->integrator == FRT_INTEGRATOR_ERROR)   // ERROR: the geometry of path
        return true;
    if (p->integrator == FRT_INTEGRATOR_DENOISE) return p->shard_count == 1;   // the stencil crosses tiles
    return p->integrator == FRT_INTEGRATOR_PSSMLT && p->mlt_chains > 0 && p->mlt_bootstrap > 0 &&
           p->sample_offset == 0;
}
static int my_tiles(const frt_render_params *p)
{
    const int T = eff_tile(p);
    const int ntiles = ((p->nx + T - 1) / T) * ((p->ny + T - 1) / T);
    if (p->shard_index >= ntiles) return 0;
    return (ntiles - 1 - p->shard_index) / p->shard_count + 1;
}
extern "C" int64_t frt_shard_slot_count(const frt_render_params *p)
{
    if (!params_ok(p)) return FRT_E_INVALID;
    if (p->integrator == FRT_INTEGRATOR_PSSMLT) return (int64_t)p->nx * p->ny;   // whole film per shard
    const int T = eff_tile(p);
    return (int64_t)my_tiles(p) * T * T;
}
extern "C" int frt_shard_slots(const frt_render_params *p, int32_t *slot_pixel)
{
    if (!params_ok(p) || !slot_pixel) return FRT_E_INVALID;
    if (p->integrator == FRT_INTEGRATOR_PSSMLT) {
        for (int64_t i = 0; i < (int64_t)p->nx * p->ny; ++i) slot_pixel[i] = (int32_t)i;
        return FRT_OK;
    }
    const int T = eff_tile(p), ntx = (p->nx + T - 1) / T;
    const int nmt = my_tiles(p);
    for (int t = 0; t < nmt; ++t) {
        const int tile_id = p->shard_index + t * p->shard_count;
        for (int s = 0; s < T * T; ++s) {
            int lx, ly;
            slot_to_local(s, T, lx, ly);
            const int px = (tile_id % ntx) * T + lx, py = (tile_id / ntx) * T + ly;
            slot_pixel[(size_t)t * T * T + s] = (px < p->nx && py < p->ny) ? py * p->nx + px : -1;
        }
    }
    return FRT_OK;
}


// does this render run the fp64 kernels?  FRT_FLAG_FP64 / _FP32 override the
// context's precision for one call (A/B)
bool use_f64(const frt_ctx *c, const frt_render_params *p)
{
    if (p->integrator != FRT_INTEGRATOR_PATH || (p->flags & FRT_FLAG_FP32)) return false;
    if (p->flags & FRT_FLAG_FP64) return true;
    return c->precision == FRT_PRECISION_FP64 || (c->precision == FRT_PRECISION_AUTO && c->world_kind == FRT_WORLD_LIST);
}
// The plan of a render: integrator and flags -> material set and unit -> ladder (frt_plans.hpp)
static int pick_launcher(const frt_ctx *c, int integrator, int flags, Launcher &L, bool f64, bool env_sampling)
{
    if (f64 && !c->has_f64) return FRT_E_INVALID;
    if (integrator == FRT_INTEGRATOR_ALBEDO || integrator == FRT_INTEGRATOR_DEPTH)   // no estimator flag, no image
        return frt_feat::pick(c, integrator, flags, L);
    // FRT_FLAG_ROULETTE, FRT_FLAG_SOBOL (path): the kernels compiled with these kMatsFeatures bits
    const int features = integrator != FRT_INTEGRATOR_PATH ? 0 : ((flags & FRT_FLAG_ROULETTE) ? kMatsRoulette : 0) |
                                                                     ((flags & FRT_FLAG_SOBOL) ? kMatsSobol : 0);
    // the material unit holds every kernel with a material set: an image's lookup, AO, the scene's
    // materials, and the fp64 kernels of BVH worlds (they carry every material)
    if (env_sampling || c->env_texels ||
        (integrator != FRT_INTEGRATOR_NORMALS && (integrator == FRT_INTEGRATOR_AO || c->mats != kMatsNone ||
                                                  (f64 && c->world_kind != FRT_WORLD_LIST))))
        return frt_mats::pick(c, integrator, flags, f64, env_sampling, features, L);
    // a lambertian scene without an image (fp64: a list world)
    if (integrator == FRT_INTEGRATOR_NORMALS) return plan_fixed<kMatsNone, FRT_INTEGRATOR_NORMALS, 5, 6, 6>(c, flags, L);
    if (features)   // the sibling plans' caps: 5 waves from LDS, 6 from HBM, 7 on the 4-wide tree
        return with_features(features, [&](auto x) -> int {
            constexpr int M = decltype(x)::value;
            return f64 ? plan_f64<M, false>(c, L) : plan_fixed<M, FRT_INTEGRATOR_PATH, 5, FRT_EXP_W6, FRT_EXP_W7>(c, flags, L);
        });
    return f64 ? plan_f64<kMatsNone, false>(c, L) : pick_launcher_t<kMatsNone>(c, flags, L);
}


int render_preamble(frt_ctx *c, const frt_render_params *p, bool *env_sampling, bool *f64)
{
    // FRT_FLAG_ENV_SAMPLING: path renders of a context with an image that has any luminance
    *env_sampling = false;
    if ((p->flags & FRT_FLAG_ENV_SAMPLING) && p->integrator == FRT_INTEGRATOR_PATH && c->env_texels) {
        if (const int trc = env_tables(c)) return trc;
        *env_sampling = c->env_tab == frt_ctx::kEnvTabBuilt;
    }
    if (p->integrator == FRT_INTEGRATOR_AO && c->has_metal)   // ao::Li -> constant_pdf::generate throws (pdf.h:195-198)
        return set_err(c, FRT_E_UNSUPPORTED, "ao integrator: metal has no sampling pdf (constant_pdf::generate)");
    *f64 = use_f64(c, p);
    if (*f64 && !c->has_f64)
        return set_err(c, FRT_E_INVALID, "fp64 render of a scene uploaded without fp64 records: frt_set_precision(FRT_PRECISION_FP64) "
                                         "before frt_upload_scene");
    return FRT_OK;
}

// ---- ray queries: trace_kernel plans (the path plans' residency rules) ----
template <int STACK, int WORLD, bool LDS, int WAVES>
static Launcher make_trace(size_t scene_bytes)
{
    Launcher L;
    L.stack = WORLD != FRT_WORLD_LIST ? STACK : 0;   // a list world has none
    L.wide = WORLD == kWorldBvh4;
    L.fn = reinterpret_cast<const void *>(&trace_kernel<STACK, WORLD, LDS, WAVES>);
    L.lds = (WORLD != FRT_WORLD_LIST ? (size_t)STACK * kBlock * sizeof(int) : 0) + (LDS ? scene_bytes : 0);
    L.scene_lds = LDS ? scene_bytes : 0;
    L.waves = WAVES;
    L.lds_scene = LDS;
    return L;
}
// register cap of the ray-query kernel: FRT_TRACE_WAVES (6 / 8 / 10; A/B knob, not part of the C-ABI)
template <int STACK, int WORLD, bool LDS>
static Launcher trace_waves(size_t sb)
{
    const char *e = std::getenv("FRT_TRACE_WAVES");
    const int w = e ? std::atoi(e) : 8;
    if (w == 6) return make_trace<STACK, WORLD, LDS, 6>(sb);
    if (w == 10) return make_trace<STACK, WORLD, LDS, 10>(sb);
    return make_trace<STACK, WORLD, LDS, 8>(sb);
}
static int pick_trace(const frt_ctx *c, int flags, Launcher &L)
{
    return walk_plan(c, flags, [&](auto r, size_t scene_bytes) -> int {
        using R = decltype(r);
        if constexpr (R::world == kWorldBvh2Oct || R::world == kWorldBvh4) L = trace_waves<R::stack, R::world, R::lds>(scene_bytes);
        else L = make_trace<R::stack, R::world, R::lds, R::stack == 64 ? 1 : 8>(scene_bytes);
        return FRT_OK;
    });
}

// Batched Scene::world->hit (include/frt.h frt_trace_device)
extern "C" int frt_trace_device(frt_ctx *c, const float *rays, int64_t n, float *hits, int flags, void *hip_stream,
                                frt_stats *st)
{
    Persist P;
    if (!c || n < 0 || (n > 0 && (!rays || !hits))) return FRT_E_INVALID;
    if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
    Launcher L;
    if (pick_trace(c, flags, L) != FRT_OK) return set_err(c, FRT_E_UNSUPPORTED, "BVH deeper than 63 levels");
    if (const int rc = persist_plan(c, L.fn, L.lds, std::max<int64_t>(1, (n + kBlock - 1) / kBlock), nullptr, P)) return rc;
    // the ray-queue head runs past n by up to one chunk per wave
    if (const int rc = queue_headroom(c, P, (uint64_t)n, kTraceChunk,
                                      "frt_trace_device: too many rays for one call (2^32 - 1 less the queue headroom)"))
        return rc;
    DevRays R{};
    R.ray = reinterpret_cast<const float4 *>(rays);
    R.hit = reinterpret_cast<float4 *>(hits);
    R.n = (uint32_t)n;
    R.min_desc = min_desc(L.lds_scene);
    // its own queue word, a cache line away from the render queue's: a trace and
    // a render of one context on two streams do not share a queue head
    R.counter = c->counter + kTraceCounterWord;
    DevScene Sarg = c->S;
    void *args[] = {&Sarg, &R};
    if (const int rc = persist_launch(c, P, "trace_kernel", L.fn, L.lds, args, R.counter, sizeof(unsigned), stream, n > 0)) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, stream));
    if (const int rc = persist_finish(c, P, nullptr, stream, st)) return rc;   // the kernel keeps no ray counters
    if (st) st->camera_rays = (uint64_t)n;
    fill_plan_stats(st, c, L);
    return FRT_OK;
}

// ---- PSS-MLT render: bootstrap b, then the chain megakernel splatting into dev_film ----

#if defined(FRT_DIAG)
// diagnostic builds only: the per-phase counters of the last path or PSS-MLT
// render, one kDiagSlots row per wave on the device, summed over waves here
static unsigned long long g_diag_sum[kDiagSlots];
static unsigned long long *g_diag_buf = nullptr;
static size_t g_diag_n = 0;
static int diag_begin(frt_ctx *c, size_t n_waves, hipStream_t st)
{
    if (g_diag_n < n_waves * kDiagSlots) {
        if (g_diag_buf) HIPCHK(c, hipFree(g_diag_buf));
        g_diag_n = n_waves * kDiagSlots;
        HIPCHK(c, hipMalloc(&g_diag_buf, g_diag_n * sizeof(unsigned long long)));
    }
    HIPCHK(c, hipMemsetAsync(g_diag_buf, 0, g_diag_n * sizeof(unsigned long long), st));
    HIPCHK(c, hipMemcpyToSymbolAsync(HIP_SYMBOL(frt::frt_diag), &g_diag_buf, sizeof(g_diag_buf), 0,
                                     hipMemcpyHostToDevice, st));
    return FRT_OK;
}
static int diag_end(frt_ctx *c, size_t n_waves)
{
    std::vector<unsigned long long> dv(n_waves * kDiagSlots);
    HIPCHK(c, hipMemcpy(dv.data(), g_diag_buf, dv.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int k = 0; k < kDiagSlots; ++k) g_diag_sum[k] = 0;
    for (size_t w = 0; w < n_waves; ++w)
        for (int k = 0; k < kDiagSlots; ++k) g_diag_sum[k] += dv[w * kDiagSlots + k];
    return FRT_OK;
}
extern "C" int frt_diag_read(unsigned long long *out)
{
    for (int k = 0; k < kDiagSlots; ++k) out[k] = g_diag_sum[k];
    return kDiagSlots;
}
#endif

// ---- one launch of a persistent kernel (frt_ctx.hpp) ----
int persist_plan(frt_ctx *c, const void *fn, size_t lds, int64_t max_blocks, DevBuf<unsigned long long> *counters, Persist &P)
{
    int bpc = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, fn, kBlock, lds) != hipSuccess || bpc <= 0) bpc = 1;
    P.grid = (int)std::min<int64_t>((int64_t)c->n_cu * bpc, max_blocks);
    P.n_waves = (size_t)P.grid * kBlock / 64;
    return counters ? counters->reserve(c, P.n_waves * 4 * sizeof(unsigned long long)) : FRT_OK;
}
int queue_headroom(frt_ctx *c, const Persist &P, uint64_t n_items, uint64_t per_wave, const std::string &msg)
{
    return n_items + (uint64_t)P.n_waves * per_wave >= 0xffffffffULL ? set_err(c, FRT_E_UNSUPPORTED, msg) : FRT_OK;
}
int persist_launch(frt_ctx *c, const Persist &P, const char *name, const void *fn, size_t lds, void **args, unsigned *queue,
                   size_t queue_bytes, hipStream_t st, bool run)
{
    HIPCHK(c, hipMemsetAsync(queue, 0, queue_bytes, st));
#if defined(FRT_DIAG)
    if (const int drc = P.diag ? diag_begin(c, P.n_waves, st) : FRT_OK) return drc;
#endif
    HIPCHK(c, hipEventRecord(c->ev0, st));
    const hipError_t le = run ? hipLaunchKernel(fn, dim3(P.grid), dim3(kBlock), args, lds, st) : hipSuccess;
    return le == hipSuccess ? FRT_OK : set_err(c, FRT_E_HIP, std::string(name) + " launch: " + hipGetErrorString(le));
}
int persist_finish(frt_ctx *c, const Persist &P, const unsigned long long *counters, hipStream_t st, frt_stats *stats)
{
    std::vector<unsigned long long> wr(counters ? P.n_waves * 4 : 0);
    if (counters) HIPCHK(c, hipMemcpyAsync(wr.data(), counters, wr.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
#if defined(FRT_DIAG)
    if (const int drc = P.diag ? diag_end(c, P.n_waves) : FRT_OK) return drc;
#endif
    if (!stats) return FRT_OK;
    memset(stats, 0, sizeof(*stats));
    for (size_t w = 0; w < wr.size(); w += 4) {
        stats->camera_rays += wr[w]; stats->extension_rays += wr[w + 1];
        stats->shadow_rays += wr[w + 2]; stats->samples += wr[w + 3];
    }
    stats->kernel_ms = ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - P.t_start).count();
    return FRT_OK;
}
void fill_plan_stats(frt_stats *stats, const frt_ctx *c, const Launcher &L)
{
    if (!stats) return;
    stats->scene_in_lds = L.lds_scene ? 1u : 0u;
    stats->waves_cap = (uint32_t)L.waves;
    stats->stack_entries = (uint32_t)L.stack;
    stats->bvh_depth = (uint32_t)(L.wide ? c->depth4 : c->stack_needed);
    stats->scene_bytes = L.lds_scene ? L.scene_lds : c->scene_lds_bytes;   // what this plan reads
    stats->fp64 = L.f64 ? 1u : 0u;
}

// The PSS-MLT plan of a context: the bootstrap and chain kernels, the traversal stack and the
// LDS bytes of the two launches.  No device call: frtx_selftest_plan asks it too.
struct MltPlan {
    const void *boot = nullptr, *chain = nullptr;
    int stack = 0;
    size_t lds_boot = 0, lds = 0;
    bool lds_scene = false, oct = false;
};
static int pick_mlt(frt_ctx *c, int flags, MltPlan &P)
{
    const bool env = c->env_texels != nullptr;   // the chain kernels with the environment lookup
    bool rung = false;
    size_t scene_lds = 0;
    // the octant node copies when they fit, as the path kernels (round 5: the chain kernel used the planar tree)
    const int krc = walk_plan(c, flags, [&](auto r, size_t scene_bytes) -> int {
        using R = decltype(r);
        rung = true;
        P.stack = R::world == FRT_WORLD_LIST ? 0 : R::stack;
        P.lds_scene = R::lds; P.oct = R::world == kWorldBvh2Oct;
        scene_lds = scene_bytes;
        // the material branch and the image's lookup from the material unit, the lambertian octant kernels from frt_lds
        if (c->has_spec_mats || env) return frt_mats::mlt(c, flags, env, &P.boot, &P.chain);
        if constexpr (R::world == kWorldBvh2Oct && kSplitLds) {
            return frt_lds::mlt_oct(c, flags, &P.boot, &P.chain);
        } else {
            mlt_kernels_t<R::stack, R::world, R::lds, false>(&P.boot, &P.chain);
            return FRT_OK;
        }
    });
    if (!rung) return set_err(c, FRT_E_UNSUPPORTED, "BVH deeper than 63 levels");
    if (krc != FRT_OK || !P.boot || !P.chain) return set_err(c, FRT_E_UNSUPPORTED, "pssmlt: no kernels for this plan in this build");
    P.lds_boot = (size_t)P.stack * kBlock * sizeof(int);
    P.lds = P.lds_boot + (size_t)kChainWords * kBlock * sizeof(int) + scene_lds;
    return FRT_OK;
}

static int render_mlt(frt_ctx *c, const frt_render_params *p, float *dev_film, hipStream_t st, frt_stats *stats)
{
    Persist PL;
    MltPlan P;
    if (const int prc = pick_mlt(c, p->flags, P)) return prc;
    const uint32_t n_chains = (uint32_t)p->mlt_chains;
    const uint32_t n_local = (n_chains > (uint32_t)p->shard_index)
                                 ? (n_chains - 1 - (uint32_t)p->shard_index) / (uint32_t)p->shard_count + 1 : 0;
    const uint64_t total = (uint64_t)p->spp * (uint64_t)p->nx * (uint64_t)p->ny;   // viewer ns
    const uint64_t steps = total / n_chains;                                       // samples_per_thread
    if (steps >= 0xffffffffULL) return set_err(c, FRT_E_UNSUPPORTED, "pssmlt: more than 2^32 - 1 mutations per chain");
    // bootstrap normaliser (identical on every shard: same streams, fixed-order host sum)
    const int n_init = p->mlt_bootstrap;
    const size_t need = std::max<size_t>((size_t)n_init * sizeof(float), (size_t)kMltRow * n_local * sizeof(float));
    if (const int rc = c->partial.reserve(c, need)) return rc;
#if defined(FRT_DIAG)
    // the bootstrap's traversal ticks too: a diagnostic buffer for its grid (zeroed again before the chains)
    if (const int drc = diag_begin(c, (size_t)(n_init + kBlock - 1) / kBlock * (kBlock / 64), st)) return drc;
#endif
    {
        int nx = p->nx, ny = p->ny, ni = n_init;
        uint32_t seed = p->seed;
        float *sc = c->partial;
        DevScene Sarg = c->S;
        void *args[] = {&Sarg, &nx, &ny, &seed, &ni, &sc};
        HIPCHK(c, hipLaunchKernel(P.boot, dim3((n_init + kBlock - 1) / kBlock), dim3(kBlock), args, P.lds_boot, st));
    }
    std::vector<float> sc(n_init);
    HIPCHK(c, hipMemcpyAsync(sc.data(), c->partial, n_init * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    double b = 0.0;
    for (float v : sc) b += v;
    b /= n_init;
    if (const int rc = persist_plan(c, P.chain, P.lds, std::max<int64_t>(1, (n_local + kBlock - 1) / kBlock), &c->wave_rays, PL)) return rc;
    PL.diag = true;
    MltWork W{};
    W.nx = p->nx; W.ny = p->ny; W.seed = p->seed;
    W.shard_index = p->shard_index; W.shard_count = p->shard_count;
    W.n_local = n_local; W.steps = steps;
    W.b = (float)b;
    W.scale = (float)((double)p->nx * p->ny / ((double)steps * (double)n_chains));   // AccumulatePathContribution
    W.s2p = 0.1f;
    W.logp = (float)std::log((double)0.1f / (2.0 / (double)(p->nx + p->ny)));
    const size_t n_film = (size_t)p->nx * p->ny * 3;
    if (const int rc = c->splat.reserve(c, n_film * sizeof(unsigned long long))) return rc;
    W.U = c->partial; W.film = c->splat; W.counter = c->counter; W.wave_rays = c->wave_rays;
    W.trav_min = trav_min(P.lds_scene);
    W.min_desc = min_desc(P.lds_scene);
    HIPCHK(c, hipMemsetAsync(c->splat, 0, n_film * sizeof(unsigned long long), st));
    const bool run = n_local > 0 && steps > 0;
    DevScene Sarg = c->S;
    void *args[] = {&Sarg, &W};
    if (const int rc = persist_launch(c, PL, "mlt_megakernel", P.chain, P.lds, args, c->counter, 64, st, run)) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, st));
    mlt_film_to_float<<<dim3((unsigned)((n_film + kBlock - 1) / kBlock)), dim3(kBlock), 0, st>>>(c->splat.get(), dev_film, n_film);
    HIPCHK(c, hipGetLastError());
    if (const int rc = persist_finish(c, PL, run ? c->wave_rays.get() : nullptr, st, stats)) return rc;
    if (stats) {
        stats->pixels = (uint64_t)p->nx * p->ny;
        stats->work_items = n_local;
        stats->scene_in_lds = P.lds_scene ? 1u : 0u;
        stats->stack_entries = (uint32_t)P.stack;
        stats->bvh_depth = (uint32_t)c->stack_needed;
        // the LDS copy the chain kernel loads (the octant node copies on that plan)
        stats->scene_bytes = P.oct ? c->scene_lds_bytes_oct : c->scene_lds_bytes;
    }
    c->last_mlt_b = b;
    c->mlt_rows = run ? n_local : 0;
    return FRT_OK;
}

// The chain states of the last PSS-MLT render (test / diagnostic read-back):
// local chains [first, first + n) of that render's shard, chain c = shard_index
// + j * shard_count.  u_out (n x 92): final primary samples; fp_out (n x 2): the
// trajectory fingerprint (accepted proposals, sum of the accepted steps' 1-based
// indices mod 2^32), which ora_mlt_render_shard computes the same way.
extern "C" int frt_mlt_chain_state(frt_ctx *c, uint64_t first, uint64_t n, float *u_out, uint32_t *fp_out)
{
    if (!c) return FRT_E_INVALID;
    if (c->mlt_rows == 0 || first + n > c->mlt_rows || first + n < first)
        return set_err(c, FRT_E_INVALID, "frt_mlt_chain_state: no such chains in the last PSS-MLT render");
    if (n == 0) return FRT_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<float> rows(n * kMltRow);
    HIPCHK(c, hipMemcpy(rows.data(), c->partial + first * kMltRow, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (uint64_t k = 0; k < n; ++k) {
        if (u_out) memcpy(u_out + k * kMltDims, rows.data() + k * kMltRow, kMltDims * sizeof(float));
        if (fp_out) memcpy(fp_out + 2 * k, rows.data() + k * kMltRow + kMltFp, 2 * sizeof(uint32_t));
    }
    return FRT_OK;
}


// Work granule of a path / AO / normals render: the frame's samples cut into
// n_chunks chunks of spi samples (the last one shorter), k = n_chunks chosen
// for at least about 40 items per resident lane and at most `target` samples
// an item (about 150 rays: path 24, AO 96, normals 128).  With one queue
// atomic per refill the first rule alone was best (Cornell 512 spp at 5-6
// chunks, profiles/r03/samecall/spi_*.jsonl); with 64-item grabs smaller items
// pay: Cornell 512 spp 289.7 ms at 6 chunks, 281.9 at 23 (flat from 16 to 64
// chunks), cornell_1m 824.1 -> 810.0 ms, while AO stays best at 6 chunks (1.5
// rays a sample; profiles/r03/samecall/grab64_spi_*.jsonl).  The target rule
// grows k with spp, so it is capped at kMaxItemsPerLane items per resident
// lane: the (chunk, slot) partial sums, 12 B an item, stay below
// kMaxItemsPerLane x the resident lanes x 12 B (~1.8 GB on MI355X) at any spp,
// and frames of any spp fit the 32-bit queue.  FRT_SPI_TARGET overrides the target (0:
// the first rule alone; A/B knob).  spi_req > 0: the caller's samples per item.
// Round 4: the chunks are the whole frame's for every shard count (films
// identical at any N), so at N = 8 a shard has an eighth of the items.  Path
// items of 8 samples under a cap of 384 items per lane (1080p 512 spp: 57 / 64
// chunks, partial sums 1.4 / 1.6 GB) keep ~40 items per lane in an eighth:
// predicted 8-way speedup of the render Cornell 6.79 -> 7.37, cornell_1m
// 6.64 -> 7.20 (shards timed alone, tools/shard_balance.py); at N = 1 Cornell
// +0.5 %, cornell_1m -0.4 % time (profiles/r04/r04g).
constexpr double kMaxItemsPerLane = 384.0;
static void work_granule(int integrator, int spp, uint64_t n_slots, long long lanes, int spi_req, int &spi,
                         int &n_chunks)
{
    spi = spi_req;
    if (spi <= 0) {
        const char *tgt = std::getenv("FRT_SPI_TARGET");
        const int target = tgt ? std::atoi(tgt)
                               : integrator == FRT_INTEGRATOR_PATH ? 8 : integrator == FRT_INTEGRATOR_AO ? 96 : 128;
        const double slots = std::max((double)n_slots, 1.0);
        const double k_lanes = std::max(1.0, std::round(40.0 * (double)lanes / slots));
        double k = k_lanes;
        if (target > 0) {
            const double k_cap = std::max(k_lanes, std::floor(kMaxItemsPerLane * (double)lanes / slots));
            k = std::max(k, std::min(std::ceil((double)spp / (double)target), k_cap));
        }
        spi = (int)std::ceil((double)spp / k);
    }
    spi = std::max(1, std::min(spi, spp));
    n_chunks = (spp + spi - 1) / spi;
}
// the granule rule for host tests (CPU): internal to libfrt.so, not in include/frt.h
extern "C" int frt_internal_work_granule(int integrator, int spp, int64_t n_slots, int64_t lanes, int spi_req,
                                         int *spi, int *n_chunks)
{
    if (spp <= 0 || n_slots < 0 || lanes <= 0 || !spi || !n_chunks) return FRT_E_INVALID;
    work_granule(integrator, spp, (uint64_t)n_slots, (long long)lanes, spi_req, *spi, *n_chunks);
    return FRT_OK;
}

// FRT_INTEGRATOR_DENOISE: dev_slots holds the colour of the whole frame in slot
// order.  The three feature films are the public renders of the same parameters
// (this function again, one integrator each), into the context's feature
// buffer; then the filter (frt_denoise.hip) rewrites the colour in place.
static int render_denoise(frt_ctx *c, const frt_render_params *p, float *dev_slots, hipStream_t st, frt_stats *stats)
{
    const auto t_start = std::chrono::steady_clock::now();
    const int T = eff_tile(p);
    const uint64_t n_slots64 = (uint64_t)(((p->nx + T - 1) / T) * (uint64_t)((p->ny + T - 1) / T)) * T * T;
    if (n_slots64 >= 0xffffffffULL) return set_err(c, FRT_E_UNSUPPORTED, "frame too large for one call");
    const uint32_t n_slots = (uint32_t)n_slots64;
    const size_t plane = (size_t)n_slots * 3;
    if (const int rc = c->dn_feat.reserve(c, 3 * plane * sizeof(float))) return rc;
    const int kinds[3] = {FRT_INTEGRATOR_NORMALS, FRT_INTEGRATOR_DEPTH, FRT_INTEGRATOR_ALBEDO};   // albedo last: its plan fields stay
    float *films[3] = {c->dn_feat, c->dn_feat + 2 * plane, c->dn_feat + plane};
    frt_stats sum{};
    for (int k = 0; k < 3; ++k) {
        frt_render_params q = *p;
        q.integrator = kinds[k];
        frt_stats s{};
        const int rc = render_impl(c, &q, films[k], st, &s);
        if (rc != FRT_OK) return rc;
        const frt_stats prev = sum;
        sum = s;
        sum.camera_rays += prev.camera_rays; sum.extension_rays += prev.extension_rays;
        sum.shadow_rays += prev.shadow_rays; sum.samples += prev.samples; sum.work_items += prev.work_items;
        sum.kernel_ms += prev.kernel_ms;
    }
    float ms = 0.0f;
    const int rc = frt_denoise::run(c, p, dev_slots, films[0], films[2], films[1], n_slots, st, &ms);
    if (rc != FRT_OK) return rc;
    if (stats) {
        *stats = sum;
        stats->kernel_ms += ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return FRT_OK;
}

// pixels of the frame that this shard's tiles hold
static uint64_t shard_pixels(const frt_render_params *p)
{
    const int T = eff_tile(p), ntx = (p->nx + T - 1) / T, nmt = my_tiles(p);
    uint64_t px = 0;
    for (int t = 0; t < nmt; ++t) {
        const int tile_id = p->shard_index + t * p->shard_count;
        const int tx = tile_id % ntx, ty = tile_id / ntx;
        px += (uint64_t)std::max(0, std::min(T, p->nx - tx * T)) * std::max(0, std::min(T, p->ny - ty * T));
    }
    return px;
}

// FRT_INTEGRATOR_ERROR: no ray is traced; the chunk sums that this context's last render left in
// `partial` (c->last_render) are reduced to the variance film (frt_error.hip).  The record stays.
static int render_error(frt_ctx *c, const frt_render_params *p, float *dev_slots, hipStream_t st, frt_stats *stats)
{
    const auto t_start = std::chrono::steady_clock::now();
    const auto &r = c->last_render;
    if (!r.valid)
        return set_err(c, FRT_E_INVALID, "error film: this context holds no chunk sums -- render path, ao, normals, albedo or "
                                         "depth first (a pssmlt render, a denoise call and a failed render leave none)");
    if (p->nx != r.nx || p->ny != r.ny || p->spp != r.spp || eff_tile(p) != r.tile || p->shard_index != r.shard_index ||
        p->shard_count != r.shard_count)
        return set_err(c, FRT_E_INVALID, "error film: nx, ny, spp, tile_size, shard_index and shard_count must be those of the "
                                         "context's last render (" + std::to_string(r.nx) + " x " + std::to_string(r.ny) + ", " +
                                         std::to_string(r.spp) + " spp, tile " + std::to_string(r.tile) + ", shard " +
                                         std::to_string(r.shard_index) + " of " + std::to_string(r.shard_count) + ")");
    if (r.n_chunks < 2)
        return set_err(c, FRT_E_INVALID, "error film: the last render cut each pixel's samples into one chunk, which has no "
                                         "spread; render with samples_per_item < spp (e.g. spp / 2) for more chunks");
    float ms = 0.0f;
    const int rc = frt_error::run(c, p, dev_slots, r.n_slots, r.n_chunks, r.spi, st, &ms);
    if (rc != FRT_OK) return rc;
    if (stats) {
        memset(stats, 0, sizeof(*stats));
        stats->pixels = shard_pixels(p);
        stats->kernel_ms = ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return FRT_OK;
}

// render_impl proper; the wrapper below keeps c->last_render
static int render_impl_body(frt_ctx *c, const frt_render_params *p, float *dev_slots, hipStream_t st, frt_stats *stats)
{
    Persist P;
    if (!params_ok(p)) {
        if (p->integrator == FRT_INTEGRATOR_DENOISE && p->shard_count != 1)
            return set_err(c, FRT_E_INVALID, "denoise: shard_count must be 1 (the filter's stencil crosses tiles); "
                                             "filter the assembled frame");
        return set_err(c, FRT_E_INVALID, "bad render params");
    }
    if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
    HIPCHK(c, hipSetDevice(c->device));
    if (p->integrator == FRT_INTEGRATOR_DENOISE) return render_denoise(c, p, dev_slots, st, stats);
    if (p->integrator == FRT_INTEGRATOR_ERROR) return render_error(c, p, dev_slots, st, stats);
    c->mlt_rows = 0;                                   // `partial` is about to be reused
    if (p->integrator == FRT_INTEGRATOR_PSSMLT) {
        if (p->flags & FRT_FLAG_SOBOL)
            return set_err(c, FRT_E_INVALID, "FRT_FLAG_SOBOL: pssmlt draws its primary samples from the hash stream "
                                             "(its sample layout and mutations are the reference's); render without the flag");
        if (p->flags & FRT_FLAG_ROULETTE)
            return set_err(c, FRT_E_INVALID, "FRT_FLAG_ROULETTE: pssmlt plays no Russian roulette "
                                             "(its primary-sample layout is the reference's); render without the flag");
        if (p->flags & FRT_FLAG_ENV_SAMPLING)
            return set_err(c, FRT_E_INVALID, "FRT_FLAG_ENV_SAMPLING: pssmlt does not sample the environment image "
                                             "(its primary-sample layout is the reference's); render without the flag");
        return render_mlt(c, p, dev_slots, st, stats);
    }
    bool env_sampling = false, f64 = false;
    if (const int rc = render_preamble(c, p, &env_sampling, &f64)) return rc;
    const int T = eff_tile(p);
    const int nmt = my_tiles(p);
    // 32-bit slot indices: params_ok caps the frame at 2^31 - 1 pixels, so a shard's padded
    // slots stay below 2^32 (checked, not assumed: a wrap would render nothing)
    const uint64_t n_slots64 = (uint64_t)nmt * T * T;
    if (n_slots64 >= 0xffffffffULL) return set_err(c, FRT_E_UNSUPPORTED, "frame too large for one call: shard it");
    const uint32_t n_slots = (uint32_t)n_slots64;
    // kernel variant: stack depth, world kind, LDS-resident scene
    Launcher L;
    if (pick_launcher(c, p->integrator, p->flags, L, f64, env_sampling) != FRT_OK)
        return set_err(c, FRT_E_UNSUPPORTED, "BVH deeper than 63 levels");
    if (const int rc = persist_plan(c, L.fn, L.lds, INT32_MAX, &c->wave_rays, P)) return rc;
    P.diag = true;
    const long long lanes = (long long)P.grid * kBlock;
    // the granule follows the whole frame's slots, not the shard's: every
    // shard cuts its pixels' samples into the same chunks, so the per-pixel
    // sums (and the film) are byte-identical for any shard count
    // (tools/shard_balance.py: N = 8 of the bench frame still balances)
    const int n_tiles_frame = ((p->nx + T - 1) / T) * ((p->ny + T - 1) / T);
    int spi = 0, n_chunks = 0;
    work_granule(p->integrator, p->spp, (uint64_t)n_tiles_frame * T * T, lanes, p->samples_per_item, spi, n_chunks);
    const unsigned long long n_items = (unsigned long long)n_slots * n_chunks;
    // queue grab: items a wave takes per atomic (FRT_GRAB: A/B knob, not part of the C-ABI)
    const char *gb = std::getenv("FRT_GRAB");
    const uint32_t grab = (uint32_t)std::min(std::max(gb ? std::atoi(gb) : kQueueGrab, 1), 4096);
    // the counter runs past n_items by at most one grab per wave
    if (const int rc = queue_headroom(c, P, n_items, grab + 64, "frame too large for one call: shard it")) return rc;
    if (const int rc = c->partial.reserve(c, (size_t)n_chunks * n_slots * 3 * sizeof(float))) return rc;
    DevWork W{};
    W.nx = p->nx; W.ny = p->ny; W.spp = p->spp; W.max_depth = p->max_depth; W.seed = p->seed;
    W.s_off = (uint32_t)p->sample_offset;
    W.tile = T; W.ntx = (p->nx + T - 1) / T; W.shard_index = p->shard_index; W.shard_count = p->shard_count;
    W.spi = spi; W.n_chunks = n_chunks; W.n_items = (uint32_t)n_items; W.n_slots = n_slots;
    W.grab = grab;
    W.partial = c->partial; W.counter = c->counter; W.wave_rays = c->wave_rays;
    W.trav_min = trav_min(L.lds_scene, p->integrator == FRT_INTEGRATOR_PATH);
    W.min_desc = min_desc(L.lds_scene);

    DevScene Sarg = c->S;
    void *args[] = {&Sarg, &W};
    if (const int rc = persist_launch(c, P, "path_megakernel", L.fn, L.lds, args, c->counter, 64, st)) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, st));   // kernel_ms: the render without its film reduction
    if (n_slots > 0) {
        if (p->integrator == FRT_INTEGRATOR_ALBEDO || p->integrator == FRT_INTEGRATOR_DEPTH)
            hipLaunchKernelGGL(film_reduce_mean, dim3((n_slots + 255) / 256), dim3(256), 0, st, c->partial.get(), dev_slots,
                               n_slots, n_chunks, p->spp, T, W.ntx, p->shard_index, p->shard_count, p->nx, p->ny,
                               p->integrator == FRT_INTEGRATOR_DEPTH ? 1 : 0);
        else
            hipLaunchKernelGGL(film_reduce, dim3((n_slots + 255) / 256), dim3(256), 0, st, c->partial.get(), dev_slots, n_slots,
                               n_chunks, p->spp, T, W.ntx, p->shard_index, p->shard_count, p->nx, p->ny);
        HIPCHK(c, hipGetLastError());
    }
    if (const int rc = persist_finish(c, P, c->wave_rays, st, stats)) return rc;
    if (stats) {
        stats->pixels = shard_pixels(p);
        stats->work_items = n_items;
    }
    fill_plan_stats(stats, c, L);
    // the chunk sums of this render stay in `partial`: FRT_INTEGRATOR_ERROR reduces them
    auto &r = c->last_render;
    r.nx = p->nx; r.ny = p->ny; r.spp = p->spp; r.tile = T; r.shard_index = p->shard_index; r.shard_count = p->shard_count;
    r.spi = spi; r.n_chunks = n_chunks; r.n_slots = n_slots;
    r.valid = true;
    return FRT_OK;
}

// The record of FRT_INTEGRATOR_ERROR: every call but an ERROR call drops it first, so that a
// failure, a pssmlt render (which reuses `partial`) and a denoise call (whose feature passes fill
// it with other films) leave none; a render that fills `partial` sets it as its last step.
int render_impl(frt_ctx *c, const frt_render_params *p, float *dev_slots, hipStream_t st, frt_stats *stats)
{
    if (!c || !p) return FRT_E_INVALID;
    if (p->integrator != FRT_INTEGRATOR_ERROR) c->last_render.valid = false;
    const int rc = render_impl_body(c, p, dev_slots, st, stats);
    if (p->integrator == FRT_INTEGRATOR_DENOISE) c->last_render.valid = false;
    return rc;
}

extern "C" int frt_render_device(frt_ctx *c, const frt_render_params *p, float *slots_rgb, void *hip_stream, frt_stats *st)
{
    if (c && p && p->integrator != FRT_INTEGRATOR_ERROR) c->last_render.valid = false;   // also where the call is refused below
    if (!c || !slots_rgb) return FRT_E_INVALID;
    return render_impl(c, p, slots_rgb, hip_stream ? (hipStream_t)hip_stream : c->stream, st);
}

extern "C" int frt_render(frt_ctx *c, const frt_render_params *p, float *film_rgb, frt_stats *st)
{
    if (c && p && p->integrator != FRT_INTEGRATOR_ERROR) c->last_render.valid = false;   // also where the call fails before render_impl
    if (!c || !film_rgb) return FRT_E_INVALID;
    if (!params_ok(p)) return render_impl(c, p, nullptr, c->stream, st);   // its text for the refusal
    const bool denoise = p->integrator == FRT_INTEGRATOR_DENOISE;
    if (denoise) {   // the film is the input: refuse what the filter's weights are not defined for
        if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
        const size_t n = (size_t)p->nx * p->ny * 3;
        for (size_t i = 0; i < n; ++i)
            if (!(film_rgb[i] >= 0.0f && film_rgb[i] <= FLT_MAX))
                return set_err(c, FRT_E_INVALID, "denoise: film value " + std::to_string(film_rgb[i]) + " at pixel " +
                                                     std::to_string(i / 3) + ": the colour must be finite and >= 0");
    }
    const int64_t ns = frt_shard_slot_count(p);
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = c->slots_out.reserve(c, (size_t)ns * 3 * sizeof(float))) return rc;
    std::vector<float> host((size_t)ns * 3);
    std::vector<int32_t> map((size_t)ns);
    if (denoise) {   // the colour, in slot order (padding slots: 0)
        frt_shard_slots(p, map.data());
        for (int64_t s = 0; s < ns; ++s)
            for (int k = 0; k < 3; ++k) host[3 * s + k] = map[s] < 0 ? 0.0f : film_rgb[3 * (size_t)map[s] + k];
        HIPCHK(c, hipMemcpy(c->slots_out, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    const int rc = render_impl(c, p, c->slots_out, c->stream, st);
    if (rc != FRT_OK) return rc;
    HIPCHK(c, hipMemcpy(host.data(), c->slots_out, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    if (p->integrator == FRT_INTEGRATOR_PSSMLT) {   // splat film of this shard: accumulate
        for (size_t i = 0; i < host.size(); ++i) film_rgb[i] += host[i];
        return FRT_OK;
    }
    frt_shard_slots(p, map.data());
    for (int64_t s = 0; s < ns; ++s) {
        const int32_t px = map[s];
        if (px < 0) continue;
        film_rgb[3 * (size_t)px + 0] = host[3 * s + 0];
        film_rgb[3 * (size_t)px + 1] = host[3 * s + 1];
        film_rgb[3 * (size_t)px + 2] = host[3 * s + 2];
    }
    return FRT_OK;
}

// The launch plan of a call on a context with the queried scene properties (include/frt.h): the
// dispatch above over a context built here, which needs no device.  A kernel is answered as the
// offset of its host-side handle in the library; the handle's symbol carries the kernel's name.
extern "C" int frtx_selftest_plan(const frt_plan_query *q, frt_plan_answer *a)
{
    if (!q || !a) return FRT_E_INVALID;
    memset(a, 0, sizeof(*a));
    static float4 texel;   // an image: the dispatch reads only that the pointer is set
    frt_ctx c;
    c.world_kind = q->world_kind; c.stack_needed = q->stack_needed;
    c.scene_lds_bytes = (size_t)q->scene_lds_bytes; c.scene_lds_bytes_oct = (size_t)q->scene_lds_bytes_oct;
    c.has_bvh4 = q->has_bvh4 != 0; c.depth4 = q->depth4;
    c.mats = q->mats; c.has_spec_mats = q->has_spec_mats != 0;
    c.env_texels = q->env_image ? &texel : nullptr;
    c.has_f64 = q->has_f64 != 0; c.precision = q->precision;
    auto handle = [](const void *fn) -> uint64_t {
        Dl_info info;
        return fn && dladdr(fn, &info) ? (uint64_t)((const char *)fn - (const char *)info.dli_fbase) : 0;
    };
    if (q->kind == 1) {
        Launcher L;
        a->rc = pick_trace(&c, q->flags, L);
        a->lds = (int64_t)L.lds; a->waves = L.waves; a->lds_scene = L.lds_scene; a->scene_lds = (int64_t)L.scene_lds;
        a->kernel = handle(L.fn);
    } else if (q->integrator == FRT_INTEGRATOR_PSSMLT) {
        MltPlan P;
        a->rc = pick_mlt(&c, q->flags, P);
        a->stack = P.stack; a->lds = (int64_t)P.lds; a->lds_boot = (int64_t)P.lds_boot; a->lds_scene = P.lds_scene;
        a->scene_lds = (int64_t)(P.oct ? c.scene_lds_bytes_oct : P.lds_scene ? c.scene_lds_bytes : 0);
        a->kernel = handle(P.chain); a->kernel_boot = handle(P.boot);
    } else {
        frt_render_params p{};
        p.integrator = q->integrator; p.flags = q->flags;
        Launcher L;
        a->rc = pick_launcher(&c, q->integrator, q->flags, L, use_f64(&c, &p), q->env_sampling != 0);
        a->lds = (int64_t)L.lds; a->stack = L.stack; a->waves = L.waves; a->lds_scene = L.lds_scene; a->wide = L.wide;
        a->f64 = L.f64; a->scene_lds = (int64_t)L.scene_lds;
        a->kernel = handle(L.fn);
    }
    return FRT_OK;
}
