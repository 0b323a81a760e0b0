// frt_render_sparse.hip -- frtx_render_pixels / frtx_render_pixels_device (frt.h): a list of
// pixels rendered by a persistent kernel of its own, and the reduction of its chunk sums to the
// mean and the batch-means variance (frt_error.hpp).  The per-lane code is the megakernel's
// (path_begin, trav_begin_world / trav_step_world, shade_kind / path_after_shadow) with the
// megakernel's RNG streams, so a listed pixel gets the samples frt_render draws for it.  No
// existing kernel, DevWork or plan is touched: the adaptive drivers (render_until) spend their
// later passes through this unit.
//
// Kernels.  Rungs: walk_plan with HBM residency forced -- the list world, the binary tree at
// stacks 16 / 32 / 64, the 4-wide tree; fp64 as plan_f64 has it (list, binary 32 / 64).  The scene
// is always read from HBM: a sparse pass is small and an LDS copy is a fixed cost per block.
// Material sets: collapsed to {none, all} as the host replay (frt_selftest.hip) collapses them --
// the sets of the full dispatch times these rungs would be over 150 kernels.  A path render takes
//   kMatsNone                          a lambertian scene, no image, no estimator flag
//   kMatsAll [| kMatsEnv [| kMatsEnvNee]] | feature bits     every other case
// and AO kMatsAll [| kMatsEnv], as in the full render: 114 kernels.  No register cap (the
// compiler's own allocation).  The whole unit is built with the basic SGPR register allocator,
// like frt_render_mats.hip (Makefile; DESIGN.md "Register-cap hazard").
//
// The unit compiles in parts (FRT_SPARSE_PART, Makefile) so that the parts build side by side:
// 0 = the C-ABI, the reduce kernel, the lambertian and AO kernels; 1, 2, 3 = the path kernels of
// kMatsAll, kMatsAll | kMatsEnv, and the sampled image.  Without the macro it is one unit.
//
// frtx_radiance_rays / frtx_radiance_rays_device / frtx_camera_rays_device (frt.h):
// the same loop over a list of caller-supplied first rays.  The list's kind is a compile-time
// parameter of the loop (SRC), so the pixel kernels compile to what they were; the ray kernels
// (sparse_kernel<..., kSrcRays>, the same 114 rungs x material sets) are parts 4 .. 7, cut as 0 .. 3 are.
// Their C-ABI and the camera-ray kernel stand in part 0 beside the pixel list's, whose request
// check, buffers, queue word and reduce kernel they share.
#undef FRT_DIAG
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "frt_kernels.hpp"
#include "frt_plans.hpp"
#include "frt_error.hpp"
#include "frt_rays.hpp"

// part 4 * SRC + k holds piece k of the kernels of source SRC
#ifdef FRT_SPARSE_PART
#define FRT_SPARSE_HAS(src, k) (FRT_SPARSE_PART == 4 * (src) + (k))
#else
#define FRT_SPARSE_HAS(src, k) 1
#endif

#pragma GCC visibility push(hidden)
namespace frt_sparse {
// what a list's entries are: pixels of the frame (frtx_render_pixels) or first rays (frtx_radiance_rays)
constexpr int kSrcPixels = 0, kSrcRays = 1;
// the lambertian path kernels and the AO kernels (env: the context has an image)
template <int SRC> int pick_base(const frt_ctx *c, int integrator, int flags, bool f64, bool env, Launcher &L);   // piece 0
// the path kernels of the material sets with every material, one function a part
template <int SRC> int pick_all(const frt_ctx *c, int flags, bool f64, int features, Launcher &L);       // piece 1
template <int SRC> int pick_all_env(const frt_ctx *c, int flags, bool f64, int features, Launcher &L);   // piece 2
template <int SRC> int pick_nee(const frt_ctx *c, int flags, bool f64, int features, Launcher &L);       // piece 3
#define FRT_SPARSE_DECLARE(SRC)                                                                   \
    template <> int pick_base<SRC>(const frt_ctx *, int, int, bool, bool, Launcher &);      \
    template <> int pick_all<SRC>(const frt_ctx *, int, bool, int, Launcher &);             \
    template <> int pick_all_env<SRC>(const frt_ctx *, int, bool, int, Launcher &);         \
    template <> int pick_nee<SRC>(const frt_ctx *, int, bool, int, Launcher &);
FRT_SPARSE_DECLARE(kSrcPixels)
FRT_SPARSE_DECLARE(kSrcRays)
#undef FRT_SPARSE_DECLARE
}  // namespace frt_sparse
#pragma GCC visibility pop
using frt_sparse::kSrcPixels;
using frt_sparse::kSrcRays;

namespace {

constexpr int kSparseCounterWord = 48;   // the context's queue words (kCounterBytes): 0 render, 32 ray queries, 48 this unit

// the work of one call: items are (64-entry block of the list, chunk), block-major, so a refill
// hands adjacent list entries to the lanes of a wave and a pixel's chunks run close in time
struct SparseWork {
    int nx, ny, spp, max_depth;
    uint32_t seed, s_off;
    int spi, n_chunks;
    uint32_t npix, npad, n_items;        // list entries, ... padded to 64, npad * n_chunks
    int trav_min, min_desc;
    union {                              // the list, by the kernel's SRC
        const int32_t *pixels;           // [npix] linear pixel y * nx + x
        const float4 *rays;              // [npix][2] frt_trace_device's record: (origin, t_max), (direction, stream id)
    };
    float *partial;                      // [n_chunks][npad][3]; padding entries are never written
    unsigned *counter;
    unsigned long long *wave_rays;       // [n_waves][4]: camera, extension, shadow, samples
    uint32_t grab;
};

// The unit's two kernels stand in a namespace named after the film_reduce family.  The plan
// table's test (tests/test_plans_host.py) sorts every kernel of the library by the first name of
// its qualified name into the families that frtx_selftest_plan's dispatch chooses from
// (path_megakernel, trace_kernel, the PSS-MLT pair: each must be a row of tests/golden/plans.json)
// and a fixed list of families that no such plan chooses, film_reduce among them.  These kernels
// have a dispatch of their own (sparse_plan below) and are no rows of that table, so they are
// declared under the second kind; their own names stay sparse_kernel and sparse_reduce, which
// is what a profile shows.
namespace film_reduce {
// path_megakernel's loop (frt_kernels.hpp) over a pixel list: the per-sample plan (a sample's
// radiance is summed in P.L and rounded into the item's fp32 sum when the sample ends), the
// scene from HBM, the item state and the stack columns in LDS
// SRC = kSrcRays: the list holds first rays.  A sample starts with ray_begin on its entry's record
// (read again at every start: 32 bytes that stay in L2, against a path's traversal), the stream
// id of the record keys its RNG, and the item state keeps no pixel (kIsPix, kIsPx, kIsPy unused).
// A copy of path_megakernel's loop, not a shared one: a change there goes here too (DESIGN.md "One device loop")
template <int STACK, int WORLD, int MATS, int KIND, typename R, int SRC = kSrcPixels>
__global__ __launch_bounds__(kBlock) void sparse_kernel(const DevScene S0, const SparseWork W)
{
    extern __shared__ __attribute__((aligned(16))) int lds_mem[];
    int *stk = lds_mem + threadIdx.x;
    constexpr int kStackInts = WORLD != FRT_WORLD_LIST ? STACK * kBlock : 0;
    DevScene S = S0;
    scene_strides_hbm(S);
    const int lane = threadIdx.x & 63;
    bool have_item = false, exhausted = false, active = false;
    uint32_t q_cur = 0, q_end = 0;
    const ItemState I{lds_mem + kStackInts + (int)threadIdx.x};
    PathState<R> P;
    Trav<R> T;
    bool tracing = false, pending = false;
    int ovf[kOverflow<WORLD>];
    unsigned long long n_cam = 0, n_ext = 0, n_sh = 0, n_smp = 0;
    for (;;) {
        for (;;) {
            bool shadow_done = false;
            if (tracing && trav_step_world<WORLD, kBlock, STACK, kPathStep<KIND>>(T, S, P.ro, P.rd, P.shadow, stk, ovf,
                                                                                  W.min_desc)) {
                if (KIND == FRT_INTEGRATOR_PATH && P.shadow) {
                    if (path_after_shadow<MATS>(P, T.h.prim < 0)) {
                        shadow_done = true;
                        tracing = trav_begin_world<WORLD>(T, S, P.ro, P.rd, P.rtmax);
                        pending = !tracing;
                    } else {
                        tracing = false;
                        pending = true;
                    }
                } else {
                    tracing = false;
                    pending = true;
                }
            }
            n_ext += __popcll(__ballot(shadow_done));
            if (__popcll(__ballot(tracing)) <= W.trav_min) break;
        }
        uint32_t ne = 0, ns = 0;
        bool next_ray = false;
        if (pending) {
            pending = false;
            const bool done = shade_kind<KIND, MATS>(P, S, T.h, W.max_depth, ne, ns);
            if (done) {
                I.set(kIsAcc + 0, f2i(i2f(I.get(kIsAcc + 0)) + (float)P.L.x));
                I.set(kIsAcc + 1, f2i(i2f(I.get(kIsAcc + 1)) + (float)P.L.y));
                I.set(kIsAcc + 2, f2i(i2f(I.get(kIsAcc + 2)) + (float)P.L.z));
            }
            active = !done;
            next_ray = !done;
        }
        n_ext += __popcll(__ballot(ne != 0));
        n_sh += __popcll(__ballot(ns != 0));
        // a finished item: its chunk sum goes to its own (chunk, entry) element
        if (!active && have_item && I.get(kIsCur) >= I.get(kIsEnd)) {
            float *dst = W.partial + 3ull * ((size_t)(uint32_t)I.get(kIsChunk) * W.npad + (uint32_t)I.get(kIsSlot));
            dst[0] = i2f(I.get(kIsAcc + 0)); dst[1] = i2f(I.get(kIsAcc + 1)); dst[2] = i2f(I.get(kIsAcc + 2));
            have_item = false;
        }
        // wave-aggregated refill (path_megakernel): the wave's own range first, then one atomic
        const bool need = !active && !have_item && !exhausted;
        const uint64_t m = __ballot(need);
        if (m) {
            const uint32_t nm = (uint32_t)__popcll(m), r = lane_rank(m);
            const uint32_t left = q_end - q_cur;
            uint32_t w;
            if (nm <= left) {
                w = q_cur + r;
                q_cur += nm;
            } else {
                const uint32_t take = max(W.grab, nm - left);
                const int leader = __ffsll((unsigned long long)m) - 1;
                uint32_t base = 0;
                if (lane == leader) base = atomicAdd(W.counter, take);
                base = __shfl(base, leader);
                w = r < left ? q_cur + r : base + (r - left);
                q_cur = base + (nm - left);
                q_end = base + take;
            }
            if (need) {
                if (w >= W.n_items) {
                    exhausted = true;
                } else {
                    const uint32_t q = w >> 6;
                    const uint32_t chunk = q % (uint32_t)W.n_chunks;
                    const uint32_t entry = (q / (uint32_t)W.n_chunks) * 64u + (w & 63u);
                    if (entry < W.npix) {   // padding entries of the last block carry no work
                        have_item = true;
                        int pix = 0;
                        if constexpr (SRC == kSrcPixels) pix = W.pixels[entry];
                        const int s_cur = (int)chunk * W.spi;
                        I.set(kIsCur, s_cur);
                        I.set(kIsSlot, (int)entry);
                        I.set(kIsChunk, (int)chunk);
                        if constexpr (SRC == kSrcPixels) I.set(kIsPix, pix);
                        I.set(kIsEnd, min(W.spp, s_cur + W.spi));
                        if constexpr (SRC == kSrcPixels) {
                            I.set(kIsPx, pix % W.nx);
                            I.set(kIsPy, pix / W.nx);
                        }
                        I.set(kIsAcc + 0, 0); I.set(kIsAcc + 1, 0); I.set(kIsAcc + 2, 0);
                    }
                }
            }
        }
        const bool start = !active && have_item && I.get(kIsCur) < I.get(kIsEnd);
        if (start) {
            const int s_cur = I.get(kIsCur);
            if constexpr (SRC == kSrcPixels) {
                path_begin<MATS>(P, S, I.get(kIsPx), I.get(kIsPy), W.nx, W.ny, W.seed, (uint32_t)I.get(kIsPix),
                                 (uint32_t)s_cur + W.s_off);
            } else {
                const float4 *q = W.rays + 2 * (size_t)(uint32_t)I.get(kIsSlot);
                ray_begin<MATS>(P, q[0], q[1], W.seed, (uint32_t)s_cur + W.s_off);
            }
            I.set(kIsCur, s_cur + 1);
            active = true;
            next_ray = true;
        }
        const unsigned long long started = __popcll(__ballot(start));
        n_cam += started;
        n_smp += started;
        if (next_ray) {
            // an area-light shadow ray starts at the shadow root (the environment-NEE ray has t_max = tmax)
            const bool occl = KIND == FRT_INTEGRATOR_PATH && P.shadow && ((MATS & kMatsEnvNee) == 0 || P.rtmax < R(1));
            tracing = trav_begin_world<WORLD>(T, S, P.ro, P.rd, P.rtmax, occl);
            pending = !tracing;
        }
        if (__ballot(active || !exhausted) == 0) break;
    }
    const unsigned long long c[4] = {n_cam, n_ext, n_sh, n_smp};
    if (lane == 0) {
        const size_t wv = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
        for (int k = 0; k < 4; ++k) W.wave_rays[4 * wv + k] = c[k];
    }
}

}  // namespace film_reduce

template <int STACK, int WORLD, int MATS, int KIND, typename R, int SRC>
Launcher make_sparse()
{
    Launcher L;   // the scene stays in HBM and there is no register cap: waves 0, lds_scene false, scene_lds 0
    L.fn = reinterpret_cast<const void *>(&film_reduce::sparse_kernel<STACK, WORLD, MATS, KIND, R, SRC>);
    L.lds = lds_block_bytes(STACK, 0, WORLD != FRT_WORLD_LIST);
    L.stack = STACK;
    L.wide = WORLD == kWorldBvh4;
    L.f64 = kIsF64<R>;
    return L;
}

// the rung of the context's scene with the scene in HBM
template <int MATS, int KIND, int SRC>
int sparse_plan(const frt_ctx *c, int flags, bool f64, Launcher &L)
{
    if (f64) {   // plan_f64's rungs
        if constexpr (KIND == FRT_INTEGRATOR_PATH) {
            if (c->world_kind == FRT_WORLD_LIST) L = make_sparse<16, FRT_WORLD_LIST, MATS, KIND, double, SRC>();
            else if (c->stack_needed < 32) L = make_sparse<32, FRT_WORLD_BVH, MATS, KIND, double, SRC>();
            else if (c->stack_needed < 64) L = make_sparse<64, FRT_WORLD_BVH, MATS, KIND, double, SRC>();
            else return FRT_E_UNSUPPORTED;
            return FRT_OK;
        } else {
            return FRT_E_UNSUPPORTED;
        }
    }
    return walk_plan(c, flags | FRT_FLAG_NO_LDS_SCENE, [&](auto r, size_t) -> int {
        using Rg = decltype(r);
        if constexpr (Rg::lds) {
            return FRT_E_UNSUPPORTED;   // not reached: the flag forces HBM residency
        } else {
            L = make_sparse<Rg::stack, Rg::world, MATS, KIND, float, SRC>();
            return FRT_OK;
        }
    });
}
template <int BASE, int SRC>
int sparse_plan_features(const frt_ctx *c, int flags, bool f64, int features, Launcher &L)
{
    switch (features) {
    case 0: return sparse_plan<BASE, FRT_INTEGRATOR_PATH, SRC>(c, flags, f64, L);
    case kMatsRoulette: return sparse_plan<BASE | kMatsRoulette, FRT_INTEGRATOR_PATH, SRC>(c, flags, f64, L);
    case kMatsSobol: return sparse_plan<BASE | kMatsSobol, FRT_INTEGRATOR_PATH, SRC>(c, flags, f64, L);
    default: return sparse_plan<BASE | kMatsSobol | kMatsRoulette, FRT_INTEGRATOR_PATH, SRC>(c, flags, f64, L);
    }
}

}  // namespace

// the pieces of one source: 0 lambertian and AO, 1 .. 3 the material sets with every material
#define FRT_SPARSE_PIECE0(SRC)                                                                                                   \
    template <> int frt_sparse::pick_base<SRC>(const frt_ctx *c, int integrator, int flags, bool f64, bool env, Launcher &L) \
    {                                                                                                                            \
        if (integrator == FRT_INTEGRATOR_AO)                                                                                     \
            return env ? sparse_plan<kMatsAll | kMatsEnv, FRT_INTEGRATOR_AO, SRC>(c, flags, false, L)                            \
                       : sparse_plan<kMatsAll, FRT_INTEGRATOR_AO, SRC>(c, flags, false, L);                                      \
        return sparse_plan<kMatsNone, FRT_INTEGRATOR_PATH, SRC>(c, flags, f64, L);                                               \
    }
#define FRT_SPARSE_PIECE(NAME, BASE, SRC)                                                                        \
    template <> int frt_sparse::NAME<SRC>(const frt_ctx *c, int flags, bool f64, int features, Launcher &L) \
    {                                                                                                            \
        return sparse_plan_features<BASE, SRC>(c, flags, f64, features, L);                                      \
    }
#if FRT_SPARSE_HAS(0, 0)
FRT_SPARSE_PIECE0(kSrcPixels)
#endif
#if FRT_SPARSE_HAS(0, 1)
FRT_SPARSE_PIECE(pick_all, kMatsAll, kSrcPixels)
#endif
#if FRT_SPARSE_HAS(0, 2)
FRT_SPARSE_PIECE(pick_all_env, kMatsAll | kMatsEnv, kSrcPixels)
#endif
#if FRT_SPARSE_HAS(0, 3)
FRT_SPARSE_PIECE(pick_nee, kMatsAll | kMatsEnv | kMatsEnvNee, kSrcPixels)
#endif
#if FRT_SPARSE_HAS(1, 0)
FRT_SPARSE_PIECE0(kSrcRays)
#endif
#if FRT_SPARSE_HAS(1, 1)
FRT_SPARSE_PIECE(pick_all, kMatsAll, kSrcRays)
#endif
#if FRT_SPARSE_HAS(1, 2)
FRT_SPARSE_PIECE(pick_all_env, kMatsAll | kMatsEnv, kSrcRays)
#endif
#if FRT_SPARSE_HAS(1, 3)
FRT_SPARSE_PIECE(pick_nee, kMatsAll | kMatsEnv | kMatsEnvNee, kSrcRays)
#endif

#if FRT_SPARSE_HAS(0, 0)
namespace {

namespace film_reduce {   // see sparse_kernel
// entry i of the list: mean = sum over chunks (fixed order) * (1 / spp), film_reduce's arithmetic,
// and V per channel through frt_error.hpp.  Entries i >= npix (padding) are never read.
// divide (the ray lists): mean = sum / spp, correctly rounded, so that a ray whose every sample
// returns the same exactly-summed value (a light seen directly) returns it exactly at any spp;
// 1 / spp is rounded unless spp is a power of two.  The same value at spp = 1.
__global__ __launch_bounds__(256) void sparse_reduce(const float *__restrict__ partial, float *__restrict__ out_rgb,
                                                     float *__restrict__ out_var, uint32_t npix, uint32_t npad, int n_chunks,
                                                     int spp, int spi, int divide)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    float sum[3] = {0.0f, 0.0f, 0.0f};
    ChunkVar a[3];
    for (int c = 0; c < n_chunks; ++c) {
        const float *q = partial + 3ull * ((size_t)c * npad + i);
        const float x[3] = {q[0], q[1], q[2]};
        sum[0] += x[0]; sum[1] += x[1]; sum[2] += x[2];
        if (out_var) {
            const float n = chunk_samples(c, n_chunks, spp, spi), r = chunk_ratio(c, n_chunks, spp, spi);
            chunk_var_add(a[0], x[0], n, r); chunk_var_add(a[1], x[1], n, r); chunk_var_add(a[2], x[2], n, r);
        }
    }
    const float k = 1.0f / (float)spp;
    for (int ch = 0; ch < 3; ++ch) {
        out_rgb[3ull * i + ch] = divide ? sum[ch] / (float)spp : sum[ch] * k;
        if (out_var) out_var[3ull * i + ch] = chunk_var_result(a[ch], n_chunks, spp);
    }
}

// frtx_camera_rays_device: entry i = the first ray path_begin<MATS, float> makes for pixel pixels[i]
// at one sample, as frt_trace_device's record (t_max = the kernels' Cst<float>::tmax, word 7 = the pixel)
template <int MATS>
__global__ __launch_bounds__(256) void camera_rays(const DevScene S, const int32_t *__restrict__ pixels, uint32_t npix, int nx,
                                                   int ny, uint32_t seed, uint32_t sample, float4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= npix) return;
    const int pix = pixels[i];
    PathState<float> P;
    path_begin<MATS>(P, S, pix % nx, pix / nx, nx, ny, seed, (uint32_t)pix, sample);
    out[2ull * i] = make_float4(P.ro.x, P.ro.y, P.ro.z, P.rtmax);
    out[2ull * i + 1] = make_float4(P.rd.x, P.rd.y, P.rd.z, i2f(pix));
}

}  // namespace film_reduce

// a refusal of the ray entry points: the context's text, or frt_last_error(NULL)'s without one
int ray_err(frt_ctx *c, int code, const std::string &m)
{
    if (!c) frt::null_ctx_err() = m;
    return set_err(c, code, m);
}

template <int SRC>
int pick_sparse(const frt_ctx *c, int integrator, int flags, bool f64, bool env_sampling, Launcher &L)
{
    const bool env = c->env_texels != nullptr;
    if (integrator == FRT_INTEGRATOR_AO) return frt_sparse::pick_base<SRC>(c, integrator, flags, false, env, L);
    const int features = ((flags & FRT_FLAG_ROULETTE) ? kMatsRoulette : 0) | ((flags & FRT_FLAG_SOBOL) ? kMatsSobol : 0);
    if (env_sampling) return frt_sparse::pick_nee<SRC>(c, flags, f64, features, L);
    if (env) return frt_sparse::pick_all_env<SRC>(c, flags, f64, features, L);
    if (c->mats != kMatsNone || features) return frt_sparse::pick_all<SRC>(c, flags, f64, features, L);
    return frt_sparse::pick_base<SRC>(c, integrator, flags, f64, env, L);
}

// the first entry of a pixel list that lies outside the frame: its refusal's text ("": none does)
std::string bad_pixel(const std::string &who, const frt_render_params *p, const int32_t *pixels, int64_t npix)
{
    const int64_t n = (int64_t)p->nx * p->ny;
    for (int64_t i = 0; i < npix; ++i)
        if (pixels[i] < 0 || pixels[i] >= n)
            return who + ": entry " + std::to_string(i) + " is pixel " + std::to_string(pixels[i]) + ", outside [0, nx * ny)";
    return "";
}

// what can be refused without a context or a device: the request and the list (host memory)
// (rays: frtx_radiance_rays asks -- its name in the texts, which a call without a context keeps too)
int check_request(frt_ctx *c, const frt_render_params *p, const int32_t *pixels_host, int64_t npix, int *spi, int *n_chunks,
                  bool want_var, bool rays = false)
{
    const std::string who = rays ? "radiance_rays" : "render_pixels";
    auto set_err = [rays](frt_ctx *ctx, int code, const std::string &m) { return rays ? ray_err(ctx, code, m) : ::set_err(ctx, code, m); };
    if (!p || npix < 0) return set_err(c, FRT_E_INVALID, who + ": bad arguments");
    const int k = p->integrator;
    if (k == FRT_INTEGRATOR_NORMALS || k == FRT_INTEGRATOR_ALBEDO || k == FRT_INTEGRATOR_DEPTH)
        return set_err(c, FRT_E_UNSUPPORTED, who + ": path and ao only (normals, albedo and depth have no sparse kernel)");
    if (k != FRT_INTEGRATOR_PATH && k != FRT_INTEGRATOR_AO)
        return set_err(c, FRT_E_INVALID, who + ": path and ao only (pssmlt is no per-pixel estimator; denoise and error "
                                               "are films of a whole frame)");
    if (p->shard_count != 1)
        return set_err(c, FRT_E_INVALID, who + ": shard_count must be 1 (split the list instead)");
    frt_render_params q = *p;
    q.tile_size = 0;   // ignored here
    if (!params_ok(&q)) return set_err(c, FRT_E_INVALID, "bad render params");
    *spi = p->samples_per_item > 0 ? std::min(p->samples_per_item, p->spp) : std::max(1, p->spp / 16);
    *n_chunks = (p->spp + *spi - 1) / *spi;
    if (want_var && *n_chunks < 2)
        return set_err(c, FRT_E_INVALID, who + ": the variance needs at least 2 chunks a pixel; pass samples_per_item "
                                               "< spp (e.g. spp / 2)");
    const std::string bad = pixels_host ? bad_pixel(who, p, pixels_host, npix) : "";
    return bad.empty() ? FRT_OK : set_err(c, FRT_E_INVALID, bad);
}

// the list, the outputs: device memory; the request is checked
// SRC = kSrcRays: `list` holds npix ray records (checked) instead of pixels
template <int SRC>
int sparse_impl(frt_ctx *c, const frt_render_params *p, const void *list, int64_t npix, int spi, int n_chunks,
                float *out_rgb, float *out_var, hipStream_t st, frt_stats *stats)
{
    Persist P;
    bool env_sampling = false, f64 = false;
    if (const int rc = render_preamble(c, p, &env_sampling, &f64)) return rc;
    Launcher L;
    if (pick_sparse<SRC>(c, p->integrator, p->flags, f64, env_sampling, L) != FRT_OK || !L.fn)
        return set_err(c, FRT_E_UNSUPPORTED, "BVH deeper than 63 levels");
    const uint64_t npad = ((uint64_t)npix + 63) & ~63ull;
    const uint64_t n_items = npad * (uint64_t)n_chunks;
    if (const int rc = persist_plan(c, L.fn, L.lds, (int64_t)((n_items + kBlock - 1) / kBlock), &c->sp_wave_rays, P)) return rc;
    // the queue head runs past n_items by at most one grab per wave
    if (const int rc = queue_headroom(c, P, n_items, kQueueGrab + 64, std::string(SRC == kSrcRays ? "radiance_rays" : "render_pixels") +
                                                                    ": list too long for one call: split it"))
        return rc;
    if (const int rc = c->sp_partial.reserve(c, (size_t)n_items * 3 * sizeof(float))) return rc;
    SparseWork W{};
    W.nx = p->nx; W.ny = p->ny; W.spp = p->spp; W.max_depth = p->max_depth; W.seed = p->seed;
    W.s_off = (uint32_t)p->sample_offset;
    W.spi = spi; W.n_chunks = n_chunks;
    W.npix = (uint32_t)npix; W.npad = (uint32_t)npad; W.n_items = (uint32_t)n_items;
    W.trav_min = trav_min(false, p->integrator == FRT_INTEGRATOR_PATH);
    W.min_desc = min_desc(false);
    if constexpr (SRC == kSrcRays) W.rays = static_cast<const float4 *>(list);
    else W.pixels = static_cast<const int32_t *>(list);
    W.partial = c->sp_partial;
    W.counter = c->counter + kSparseCounterWord;   // a queue word of its own
    W.wave_rays = c->sp_wave_rays;
    W.grab = kQueueGrab;
    DevScene Sarg = c->S;
    void *args[] = {&Sarg, &W};
    if (const int rc = persist_launch(c, P, "sparse_kernel", L.fn, L.lds, args, W.counter, sizeof(unsigned), st)) return rc;
    hipLaunchKernelGGL(film_reduce::sparse_reduce, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, c->sp_partial.get(), out_rgb,
                       out_var, W.npix, W.npad, n_chunks, p->spp, spi, SRC == kSrcRays ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, st));   // kernel_ms: the render with its reduction
    if (const int rc = persist_finish(c, P, c->sp_wave_rays, st, stats)) return rc;
    if (stats) {
        stats->pixels = (uint64_t)npix;
        stats->work_items = (uint64_t)npix * n_chunks;
    }
    fill_plan_stats(stats, c, L);
    return FRT_OK;
}

// frtx_radiance_rays: the request and, when it is in host memory, the list
int check_rays(frt_ctx *c, const frt_render_params *p, const float *rays_host, int64_t n, int *spi, int *n_chunks, bool want_var)
{
    if (!p || n < 0) return ray_err(c, FRT_E_INVALID, "radiance_rays: bad arguments");
    frt_render_params q = *p;
    q.nx = q.ny = 1;   // ignored here, as tile_size is
    if (const int rc = check_request(c, &q, nullptr, n, spi, n_chunks, want_var, true)) return rc;
    if (rays_host) {
        std::string why;
        if (frt::rays_first_bad(rays_host, n, why) >= 0) return ray_err(c, FRT_E_INVALID, "radiance_rays: " + why);
    }
    return FRT_OK;
}

// What differs between the two kinds of list: the name in the texts, a record (kPer values of T),
// the check of the request (with the list where it is in host memory) and the context's device
// copy of a host call's list.  A refusal of the ray calls made without a context keeps its text
// for frt_last_error(NULL).
struct PixelList {
    using T = int32_t;
    static constexpr int kSrc = kSrcPixels, kPer = 1;
    static constexpr const char *kWho = "render_pixels";
    static int check(frt_ctx *c, const frt_render_params *p, const T *host, int64_t n, int *spi, int *n_chunks, bool want_var)
    {
        return check_request(c, p, host, n, spi, n_chunks, want_var);
    }
    static DevBuf<T> &dev(frt_ctx *c) { return c->sp_pixels; }
    static int err(frt_ctx *c, int code, const std::string &m) { return set_err(c, code, m); }
};
struct RayList {
    using T = float;
    static constexpr int kSrc = kSrcRays, kPer = 8;
    static constexpr const char *kWho = "radiance_rays";
    static constexpr auto check = check_rays;
    static DevBuf<T> &dev(frt_ctx *c) { return c->sp_rays; }
    static constexpr auto err = ray_err;
};

// The four list entry points.  device: the list and the outputs are device memory and the call
// runs on the caller's stream; else they are host memory, copied through the context's buffers.
template <typename L>
int list_call(frt_ctx *c, const frt_render_params *p, const typename L::T *list, int64_t n, float *out_rgb, float *out_var,
              bool device, void *hip_stream, frt_stats *st)
{
    const std::string who = L::kWho;
    int spi = 0, n_chunks = 0;
    if (!device && n > 0 && !list) return L::err(c, FRT_E_INVALID, who + ": bad arguments");
    if (const int rc = L::check(c, p, device ? nullptr : list, n, &spi, &n_chunks, out_var != nullptr)) return rc;
    if (!c) return L::kSrc == kSrcRays ? L::err(c, FRT_E_INVALID, who + ": null context") : FRT_E_INVALID;
    if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
    if (st) memset(st, 0, sizeof(*st));
    if (n == 0) return FRT_OK;
    if (!list || !out_rgb) return set_err(c, FRT_E_INVALID, who + ": bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = (size_t)n * 3, list_bytes = (size_t)n * L::kPer * sizeof(typename L::T);
    if (device) {
        hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
        // the list is read back and checked before any kernel runs
        std::vector<typename L::T> host((size_t)n * L::kPer);
        HIPCHK(c, hipMemcpyAsync(host.data(), list, list_bytes, hipMemcpyDeviceToHost, stream));
        HIPCHK(c, hipStreamSynchronize(stream));
        if (const int rc = L::check(c, p, host.data(), n, &spi, &n_chunks, out_var != nullptr)) return rc;
        return sparse_impl<L::kSrc>(c, p, list, n, spi, n_chunks, out_rgb, out_var, stream, st);
    }
    DevBuf<typename L::T> &dev = L::dev(c);
    if (const int rc = dev.reserve(c, list_bytes)) return rc;
    if (const int rc = c->sp_out.reserve(c, 2 * n3 * sizeof(float))) return rc;
    HIPCHK(c, hipMemcpyAsync(dev, list, list_bytes, hipMemcpyHostToDevice, c->stream));
    const int rc = sparse_impl<L::kSrc>(c, p, dev.get(), n, spi, n_chunks, c->sp_out, out_var ? c->sp_out + n3 : nullptr, c->stream, st);
    if (rc != FRT_OK) return rc;
    HIPCHK(c, hipMemcpy(out_rgb, c->sp_out, n3 * sizeof(float), hipMemcpyDeviceToHost));
    if (out_var) HIPCHK(c, hipMemcpy(out_var, c->sp_out + n3, n3 * sizeof(float), hipMemcpyDeviceToHost));
    return FRT_OK;
}

}  // namespace

extern "C" int frtx_render_pixels_device(frt_ctx *c, const frt_render_params *p, const int32_t *pixels, int64_t npix,
                                         float *out_rgb, float *out_var, void *hip_stream, frt_stats *st)
{
    return list_call<PixelList>(c, p, pixels, npix, out_rgb, out_var, true, hip_stream, st);
}
extern "C" int frtx_render_pixels(frt_ctx *c, const frt_render_params *p, const int32_t *pixels, int64_t npix, float *out_rgb,
                                  float *out_var, frt_stats *st)
{
    return list_call<PixelList>(c, p, pixels, npix, out_rgb, out_var, false, nullptr, st);
}
extern "C" int frtx_radiance_rays_device(frt_ctx *c, const frt_render_params *p, const float *rays, int64_t n, float *out_rgb,
                                         float *out_var, void *hip_stream, frt_stats *st)
{
    return list_call<RayList>(c, p, rays, n, out_rgb, out_var, true, hip_stream, st);
}
extern "C" int frtx_radiance_rays(frt_ctx *c, const frt_render_params *p, const float *rays, int64_t n, float *out_rgb,
                                  float *out_var, frt_stats *st)
{
    return list_call<RayList>(c, p, rays, n, out_rgb, out_var, false, nullptr, st);
}

extern "C" int frtx_camera_rays_device(frt_ctx *c, const frt_render_params *p, const int32_t *pixels, int64_t npix,
                                       float *rays_out, void *hip_stream)
{
    if (!c) return ray_err(c, FRT_E_INVALID, "camera_rays: null context");
    if (!p || npix < 0 || npix > (int64_t)0xffffff00LL || p->nx <= 0 || p->ny <= 0 ||
        (int64_t)p->nx * p->ny > (int64_t)INT32_MAX || p->sample_offset < 0)
        return set_err(c, FRT_E_INVALID, "camera_rays: bad arguments");
    if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
    if (npix == 0) return FRT_OK;
    if (!pixels || !rays_out) return set_err(c, FRT_E_INVALID, "camera_rays: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t stream = hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<int32_t> host((size_t)npix);
    HIPCHK(c, hipMemcpyAsync(host.data(), pixels, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIPCHK(c, hipStreamSynchronize(stream));
    const std::string bad = bad_pixel("camera_rays", p, host.data(), npix);
    if (!bad.empty()) return set_err(c, FRT_E_INVALID, bad);
    const dim3 grid((unsigned)((npix + 255) / 256)), block(256);
    float4 *out = reinterpret_cast<float4 *>(rays_out);
    if (p->flags & FRT_FLAG_SOBOL)
        hipLaunchKernelGGL(film_reduce::camera_rays<kMatsSobol>, grid, block, 0, stream, c->S, pixels, (uint32_t)npix, p->nx, p->ny,
                           p->seed, (uint32_t)p->sample_offset, out);
    else
        hipLaunchKernelGGL(film_reduce::camera_rays<kMatsNone>, grid, block, 0, stream, c->S, pixels, (uint32_t)npix, p->nx, p->ny,
                           p->seed, (uint32_t)p->sample_offset, out);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(stream));
    return FRT_OK;
}
#endif  // part 0
