// frt_prt.hip -- precomputed radiance transfer on the device (frt.h frtx_prt_transfer,
// frtx_prt_rays): the transfer kernels, their reduction, and the shade kernel.
//
// Transfer.  (triangle corners) x (sphere directions) visibility rays, never written to memory:
// a persistent kernel whose work item is (block of 64 corners, chunk of kPrtChunk directions).
// A wave takes an item; its lane owns one corner for the whole item and walks the chunk's
// directions in order with the resumable traversal, starting its next direction as soon as its
// ray ends.  Neighbouring corners are neighbouring origins, so a wave's rays stay coherent, and a
// corner skips the directions under its horizon -- the waves of a flat wall skip together.  The
// chunk's directions and Y rows stand in the wave's LDS table (lanes read different rows: the row
// stride is odd).  A lane's accumulators never leave its registers, so there is no cross-lane
// reduction and the order of a corner's sum is fixed (frt_prt.hpp): the result does not depend on
// the schedule or on how the host batches the corners.
//
// Kernels.  Rungs: walk_plan with HBM residency forced, as frt_render_sparse.hip -- the list
// world, the binary tree at stacks 16 / 32 / 64, the 4-wide tree; fp32 only; two ray kinds
// (any-hit for bounce 0, closest hit with the gather of the previous bounce): ten kernels, no
// register cap.  The 4-wide traversal's overflow stack (frt_path.hpp bvh4_step) stands in LDS
// here, sized by the host from the tree's depth, so that no kernel of the unit uses scratch.
// The gather variant keeps all 75 accumulators (25 coefficients x 3 channels) in registers.
//
// The kernels stand in a namespace named after the film_reduce family, as the sparse unit's do:
// they have a dispatch of their own and are no rows of the plan table (tests/test_plans_host.py).
#undef FRT_DIAG
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "frt_kernels.hpp"
#include "frt_plans.hpp"
#include "frt_prt.hpp"
#include "frt_rays.hpp"
#include "host/prt.hpp"

namespace {

constexpr int kPrtCounterWord = 56;   // the context's queue words (kCounterBytes): 0 render, 32 ray queries, 48 lists, 56 this unit
constexpr int kPrtRow = 29;           // floats of a direction's row in the wave's table: d (3), Y (25), one of padding (odd stride)
constexpr size_t kPrtTableBytes = (size_t)(kBlock / 64) * kPrtChunk * kPrtRow * sizeof(float);

// the work of one launch: the corners [c0, c0 + nb) against every chunk
struct PrtWork {
    const float4 *corner;    // [n_corners][2]: (origin, -), (normal, -)
    const float *dirs;       // [n_dirs][3]
    const float *Y;          // [n_dirs][25]
    const float *Tprev;      // the previous bounce [n_corners][25][3] (gather)
    float *partial;          // [n_chunks][nb][25 or 75]
    uint32_t c0, nb, n_items;
    int n_chunks, n_dirs, min_desc, n_ovf, unshadowed;
    unsigned *counter;
    unsigned long long *wave_rays;   // [n_waves][4]: -, gathers, visibility rays, -
};

struct PrtLi { float v[kPrtT]; };

namespace film_reduce {

template <int STACK, int WORLD, bool GATHER>
__global__ __launch_bounds__(kBlock) void prt_transfer_kernel(const DevScene S0, const PrtWork W)
{
    extern __shared__ __attribute__((aligned(16))) int lds_mem[];
    constexpr int kStackInts = WORLD != FRT_WORLD_LIST ? STACK * kBlock : 0;
    constexpr int NACC = GATHER ? kPrtT : kPrtCoef;
    int *stk = lds_mem + threadIdx.x;
    // the 4-wide tree's overflow entries: a run of n_ovf (odd) ints a lane, behind the stack columns
    const int ovf_ints = WORLD == kWorldBvh4 ? W.n_ovf * kBlock : 0;
    int *ovf = WORLD == kWorldBvh4 ? lds_mem + kStackInts + (int)threadIdx.x * W.n_ovf : stk;
    float *tab = reinterpret_cast<float *>(lds_mem + kStackInts + ovf_ints) + (threadIdx.x >> 6) * (kPrtChunk * kPrtRow);
    DevScene S = S0;
    scene_strides_hbm(S);
    const int lane = threadIdx.x & 63;
    unsigned long long n_rays = 0;
    Trav<float> T;
    for (;;) {
        uint32_t item = 0;
        if (lane == 0) item = atomicAdd(W.counter, 1u);
        item = (uint32_t)__builtin_amdgcn_readfirstlane((int)item);
        if (item >= W.n_items) break;
        const uint32_t blk = item / (uint32_t)W.n_chunks, chunk = item - blk * (uint32_t)W.n_chunks;
        const uint32_t ci = blk * 64u + (uint32_t)lane;
        const bool valid = ci < W.nb;
        f3 o = mk3(0, 0, 0), n = mk3(0, 0, 0);
        if (valid) {
            o = xyz(W.corner[2 * (size_t)(W.c0 + ci)]);
            n = xyz(W.corner[2 * (size_t)(W.c0 + ci) + 1]);
        }
        const int j0 = (int)chunk * kPrtChunk, jn = min(kPrtChunk, W.n_dirs - j0);
        // the wave's table: every lane has left the previous item (the loop below ends wave-wide)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < jn * (kPrtRow - 1); i += 64) {
            const int r = i / (kPrtRow - 1), k = i - r * (kPrtRow - 1);
            tab[r * kPrtRow + k] = k < 3 ? W.dirs[3 * (size_t)(j0 + r) + k] : W.Y[kPrtCoef * (size_t)(j0 + r) + (k - 3)];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        float acc[NACC];
#pragma unroll
        for (int k = 0; k < NACC; ++k) acc[k] = 0.0f;
        int j = 0;
        bool more = valid, tracing = false;
        float cj = 0.0f;
        f3 d = mk3(0, 0, 1);
        // a finished ray of direction j: bounce 0 adds an unoccluded one, a gather the front of a triangle
        auto finish = [&]() {
            if constexpr (!GATHER) {
                if (T.h.prim < 0) prt_add(acc, cj, tab + j * kPrtRow + 3);
            } else {
                const int p = T.h.prim;
                if (p >= 0 && !(p & FRT_PRIM_SPHERE)) {
                    float u, v;
                    prt_bary(S, p, o, d, u, v);
                    if (prt_front(S, p, o, d, u, v)) prt_gather(acc, cj, u, v, W.Tprev + (size_t)S.tri_view[p] * (3 * kPrtT));
                }
            }
            ++j;
        };
        for (;;) {
            bool started = false;
            if (more && !tracing) {
                for (; j < jn; ++j) {   // the next direction above the corner's horizon
                    const float *row = tab + j * kPrtRow;
                    d = mk3(row[0], row[1], row[2]);
                    cj = prt_cos(n, d);
                    if (cj > 0.0f) break;
                }
                if (j >= jn) {
                    more = false;
                } else if (!GATHER && W.unshadowed) {
                    prt_add(acc, cj, tab + j * kPrtRow + 3);
                    ++j;
                } else {
                    started = true;
                    tracing = trav_begin_world<WORLD>(T, S, o, d, kPrtTmax);
                    if (!tracing) finish();   // the ray misses the scene's box
                }
            }
            n_rays += __popcll(__ballot(started));
            if (__ballot(tracing || more) == 0) break;
            if (tracing && trav_step_world<WORLD, kBlock, STACK>(T, S, o, d, !GATHER, stk, ovf, W.min_desc)) {
                tracing = false;
                finish();
            }
        }
        if (valid) {
            float *dst = W.partial + ((size_t)chunk * W.nb + ci) * NACC;
#pragma unroll
            for (int k = 0; k < NACC; ++k) dst[k] = acc[k];
        }
    }
    if (lane == 0) {
        const size_t wv = ((size_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
        W.wave_rays[4 * wv] = 0;
        W.wave_rays[4 * wv + 1] = GATHER ? n_rays : 0;
        W.wave_rays[4 * wv + 2] = GATHER ? 0 : n_rays;
        W.wave_rays[4 * wv + 3] = 0;
    }
}

// (corner ci of the batch, coefficient k): the chunk partials added in ascending chunk order, then
// the albedo and the scale (prt_final).  Tcur (NULL: no later bounce reads it) gets this bounce,
// Tout the sum over the bounces so far.
__global__ __launch_bounds__(256) void prt_reduce(const float *__restrict__ partial, const float *__restrict__ albedo,
                                                  float *__restrict__ Tcur, float *__restrict__ Tout, uint32_t c0, uint32_t nb,
                                                  int n_chunks, float scale, int gather)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)nb * kPrtCoef) return;
    const uint32_t ci = (uint32_t)(i / kPrtCoef), k = (uint32_t)(i - (uint64_t)ci * kPrtCoef);
    const size_t corner = (size_t)c0 + ci;
    for (int ch = 0; ch < 3; ++ch) {
        const size_t at = corner * kPrtT + 3 * k + ch;
        const float *p = gather ? partial + (size_t)ci * kPrtT + 3 * k + ch : partial + (size_t)ci * kPrtCoef + k;
        const float v = prt_final(albedo[3 * corner + ch], scale, prt_chunk_sum(p, n_chunks, (size_t)nb * (gather ? kPrtT : kPrtCoef)));
        if (Tcur) Tcur[at] = v;
        Tout[at] = gather ? Tout[at] + v : v;
    }
}

// the device triangle of every scene-view triangle (DevScene::tri_view inverted)
__global__ __launch_bounds__(256) void prt_invert(const int *__restrict__ tri_view, int n_tris, int32_t *__restrict__ inv)
{
    const int d = (int)(blockIdx.x * 256u + threadIdx.x);
    if (d < n_tris) inv[tri_view[d]] = d;
}

// ray i: prt_shade of its closest-hit record
__global__ __launch_bounds__(256) void prt_shade_kernel(const DevScene S0, const int32_t *__restrict__ inv,
                                                        const float *__restrict__ T, const PrtLi li,
                                                        const float4 *__restrict__ rays, const float4 *__restrict__ hits,
                                                        uint32_t n, float *__restrict__ rgb)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    DevScene S = S0;
    scene_strides_hbm(S);
    const f3 c = prt_shade(S, inv, T, li.v, xyz(rays[2 * (size_t)i]), xyz(rays[2 * (size_t)i + 1]), hits[i]);
    rgb[3 * (size_t)i] = c.x; rgb[3 * (size_t)i + 1] = c.y; rgb[3 * (size_t)i + 2] = c.z;
}

}  // namespace film_reduce

// LDS entries a lane needs behind the 4-wide traversal's kBvh4LdsStack: 3 pending siblings a
// level (bvh4_stack_fits), rounded up to an odd run so that the lanes' runs start on distinct banks
int prt_ovf(const frt_ctx *c) { return std::max(0, 3 * c->depth4 - kBvh4LdsStack) | 1; }

template <int STACK, int WORLD, bool GATHER>
Launcher make_prt(const frt_ctx *c)
{
    Launcher L;   // the scene stays in HBM and there is no register cap
    L.fn = reinterpret_cast<const void *>(&film_reduce::prt_transfer_kernel<STACK, WORLD, GATHER>);
    L.stack = WORLD != FRT_WORLD_LIST ? STACK : 0;   // a list world has none
    L.wide = WORLD == kWorldBvh4;
    L.lds = (WORLD != FRT_WORLD_LIST ? (size_t)STACK * kBlock * sizeof(int) : 0) +
            (WORLD == kWorldBvh4 ? (size_t)prt_ovf(c) * kBlock * sizeof(int) : 0) + kPrtTableBytes;
    return L;
}
template <bool GATHER>
int prt_plan(const frt_ctx *c, int flags, Launcher &L)
{
    return walk_plan(c, flags | FRT_FLAG_NO_LDS_SCENE, [&](auto r, size_t) -> int {
        using Rg = decltype(r);
        if constexpr (Rg::lds) {
            return FRT_E_UNSUPPORTED;   // not reached: the flag forces HBM residency
        } else {
            L = make_prt<Rg::stack, Rg::world, GATHER>(c);
            return FRT_OK;
        }
    });
}

int prt_err(frt_ctx *c, int code, const std::string &m)
{
    if (!c) frt::null_ctx_err() = m;
    return set_err(c, code, m);
}

// T: device memory [n_tris][3][25][3]; the request is checked and the scene view's corners are in `on`, `rho`
int transfer_impl(frt_ctx *c, const float *dirs, int n_dirs, int bounces, int flags, float *T, hipStream_t st, frt_stats *stats)
{
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    const size_t nc = (size_t)c->n_tris * 3;
    Launcher L0, L1;
    if (prt_plan<false>(c, flags, L0) != FRT_OK || prt_plan<true>(c, flags, L1) != FRT_OK)
        return set_err(c, FRT_E_UNSUPPORTED, "BVH deeper than 63 levels");
    const int n_chunks = (n_dirs + kPrtChunk - 1) / kPrtChunk;
    // the Y table: fp64 on the host, rounded once
    std::vector<float> Y((size_t)n_dirs * kPrtCoef);
    frt_prt::y_table(dirs, n_dirs, Y.data());
    if (const int rc = c->prt_dirs.reserve(c, (size_t)n_dirs * 3 * sizeof(float))) return rc;
    if (const int rc = c->prt_y.reserve(c, Y.size() * sizeof(float))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->prt_dirs, dirs, (size_t)n_dirs * 3 * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->prt_y, Y.data(), Y.size() * sizeof(float), hipMemcpyHostToDevice, st));
    if (bounces > 0) {
        if (const int rc = c->prt_bounce_a.reserve(c, nc * kPrtT * sizeof(float))) return rc;
        if (const int rc = c->prt_bounce_b.reserve(c, nc * kPrtT * sizeof(float))) return rc;
    }
    const float scale = 4.0f / (float)n_dirs;
    frt_stats total{};
    float *cur = bounces > 0 ? c->prt_bounce_a.get() : nullptr, *prev = c->prt_bounce_b.get();
    for (int b = 0; b <= bounces; ++b) {
        const bool gather = b > 0;
        const Launcher &L = gather ? L1 : L0;
        const size_t nacc = gather ? kPrtT : kPrtCoef;
        // corners of a batch: what the budget holds, in whole blocks of 64, one block at the least
        const size_t per = (size_t)n_chunks * nacc * sizeof(float);
        const size_t nb_max = prt_batch_corners(frt_prt::batch_budget(), n_chunks, (int)nacc, nc);
        if (const int rc = c->prt_partial.reserve(c, nb_max * per)) return rc;
        for (size_t c0 = 0; c0 < nc; c0 += nb_max) {
            const size_t nb = std::min(nb_max, nc - c0);
            const uint64_t n_items = (uint64_t)((nb + 63) / 64) * (uint64_t)n_chunks;
            Persist P;
            if (const int rc = persist_plan(c, L.fn, L.lds, (int64_t)((n_items + kBlock / 64 - 1) / (kBlock / 64)), &c->prt_wave_rays, P))
                return rc;
            if (const int rc = queue_headroom(c, P, n_items, 1, "prt_transfer: too many work items for one launch")) return rc;
            PrtWork W{};
            W.corner = c->prt_corner; W.dirs = c->prt_dirs; W.Y = c->prt_y; W.Tprev = prev;
            W.partial = c->prt_partial;
            W.c0 = (uint32_t)c0; W.nb = (uint32_t)nb; W.n_items = (uint32_t)n_items;
            W.n_chunks = n_chunks; W.n_dirs = n_dirs; W.min_desc = min_desc(false); W.n_ovf = prt_ovf(c);
            W.unshadowed = (flags & FRTX_PRT_UNSHADOWED) ? 1 : 0;
            W.counter = c->counter + kPrtCounterWord;
            W.wave_rays = c->prt_wave_rays;
            DevScene Sarg = c->S;
            void *args[] = {&Sarg, &W};
            if (const int rc = persist_launch(c, P, "prt_transfer_kernel", L.fn, L.lds, args, W.counter, sizeof(unsigned), st)) return rc;
            hipLaunchKernelGGL(film_reduce::prt_reduce, dim3((unsigned)((nb * kPrtCoef + 255) / 256)), dim3(256), 0, st,
                               c->prt_partial.get(), c->prt_albedo.get(), cur, T, W.c0, W.nb, n_chunks, scale, gather ? 1 : 0);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipEventRecord(c->ev1, st));   // kernel_ms: the transfer kernel with its reduction
            frt_stats one{};
            if (const int rc = persist_finish(c, P, c->prt_wave_rays, st, &one)) return rc;
            total.extension_rays += one.extension_rays;
            total.shadow_rays += one.shadow_rays;
            total.kernel_ms += one.kernel_ms;
            total.work_items += n_items;
        }
        std::swap(cur, prev);   // the next bounce gathers what this one wrote
        if (!cur) cur = c->prt_bounce_a.get();
    }
    if (stats) {
        *stats = total;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
        fill_plan_stats(stats, c, L0);
    }
    return FRT_OK;
}

int upload_corners(frt_ctx *c, const frt_scene_view *sv, hipStream_t st);

// the two transfer entry points: the request checked once (frt_prt::transfer_request_bad, the replay's
// validator too), the corner records of the view, then the bounces
int transfer_call(frt_ctx *c, const frt_scene_view *sv, const float *dirs, int64_t n_dirs, int bounces, int flags, float *T,
                  bool device, void *hip_stream, frt_stats *stats)
{
    if (!c) return prt_err(c, FRT_E_INVALID, "prt_transfer: null context");
    const std::string bad = frt_prt::transfer_request_bad(dirs, n_dirs, bounces, flags);
    if (!bad.empty()) return set_err(c, FRT_E_INVALID, bad);
    if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (c->n_tris == 0) return FRT_OK;
    if (!T) return set_err(c, FRT_E_INVALID, "prt_transfer: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = device && hip_stream ? (hipStream_t)hip_stream : c->stream;
    if (const int rc = upload_corners(c, sv, st)) return rc;
    const size_t nt = (size_t)c->n_tris * 3 * kPrtT;
    float *Tdev = T;
    if (!device) {
        if (const int rc = c->prt_t.reserve(c, nt * sizeof(float))) return rc;
        Tdev = c->prt_t;
    }
    const int rc = transfer_impl(c, dirs, (int)n_dirs, bounces, flags, Tdev, st, stats);
    if (rc != FRT_OK) return rc;
    if (!device) HIPCHK(c, hipMemcpy(T, Tdev, nt * sizeof(float), hipMemcpyDeviceToHost));
    return FRT_OK;
}

// the rays of frtx_prt_rays, checked: host memory
int check_rays(frt_ctx *c, const float *T, const float *li, const float *rays, int64_t n, const float *rgb)
{
    if (!c) return prt_err(c, FRT_E_INVALID, "prt_rays: null context");
    if (n < 0 || n > (int64_t)0xffffff00LL || !li) return prt_err(c, FRT_E_INVALID, "prt_rays: bad arguments");
    for (int k = 0; k < kPrtT; ++k)
        if (!std::isfinite(li[k])) return prt_err(c, FRT_E_INVALID, "prt_rays: li[" + std::to_string(k) + "] is not finite");
    return FRT_OK;
}

// T, rgb: device memory; rays_host: the checked records (host memory), uploaded with word 7 cleared
int rays_impl(frt_ctx *c, const float *T, const float *li, std::vector<float> &rays_host, int64_t n, float *rgb, hipStream_t st,
              frt_stats *stats)
{
    const std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();
    // word 7 is frt_trace_device's flags here: 0 = the closest hit (a caller's stream id is not read)
    for (int64_t i = 0; i < n; ++i) rays_host[8 * (size_t)i + 7] = 0.0f;
    if (const int rc = c->prt_rays.reserve(c, (size_t)n * 8 * sizeof(float))) return rc;
    if (const int rc = c->prt_hits.reserve(c, (size_t)n * 4 * sizeof(float))) return rc;
    if (const int rc = c->prt_inv.reserve(c, (size_t)std::max(c->n_tris, 1) * sizeof(int32_t))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->prt_rays, rays_host.data(), (size_t)n * 8 * sizeof(float), hipMemcpyHostToDevice, st));
    frt_stats ts{};
    if (const int rc = frt_trace_device(c, reinterpret_cast<const float *>(c->prt_rays.get()), n,
                                        reinterpret_cast<float *>(c->prt_hits.get()), 0, st, &ts))
        return rc;
    PrtLi L;
    memcpy(L.v, li, sizeof(L.v));
    HIPCHK(c, hipEventRecord(c->ev0, st));
    if (c->n_tris > 0)
        hipLaunchKernelGGL(film_reduce::prt_invert, dim3((unsigned)((c->n_tris + 255) / 256)), dim3(256), 0, st, c->S.tri_view,
                           c->n_tris, c->prt_inv.get());
    hipLaunchKernelGGL(film_reduce::prt_shade_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c->S, c->prt_inv.get(), T, L,
                       c->prt_rays.get(), c->prt_hits.get(), (uint32_t)n, rgb);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, st));
    HIPCHK(c, hipStreamSynchronize(st));
    float ms = 0.0f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (stats) {
        *stats = ts;   // the closest-hit query's plan and camera_rays = n
        stats->kernel_ms = ts.kernel_ms + ms;
        stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return FRT_OK;
}

int rays_call(frt_ctx *c, const float *T, const float *li, const float *rays, int64_t n, float *rgb, bool device, void *hip_stream,
              frt_stats *stats)
{
    if (const int rc = check_rays(c, T, li, rays, n, rgb)) return rc;
    if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) return FRT_OK;
    if (!rays || !rgb || (c->n_tris > 0 && !T)) return set_err(c, FRT_E_INVALID, "prt_rays: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = device && hip_stream ? (hipStream_t)hip_stream : c->stream;
    std::vector<float> host((size_t)n * 8);
    if (device) {   // the list is read back and checked before any kernel runs
        HIPCHK(c, hipMemcpyAsync(host.data(), rays, host.size() * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
    } else {
        memcpy(host.data(), rays, host.size() * sizeof(float));
    }
    std::string why;
    if (frt::rays_first_bad(host.data(), n, why) >= 0) return set_err(c, FRT_E_INVALID, "prt_rays: " + why);
    if (device) return rays_impl(c, T, li, host, n, rgb, st, stats);
    const size_t nt = (size_t)c->n_tris * 3 * kPrtT;
    if (const int rc = c->prt_t.reserve(c, nt * sizeof(float))) return rc;
    if (const int rc = c->prt_rgb.reserve(c, (size_t)n * 3 * sizeof(float))) return rc;
    if (nt) HIPCHK(c, hipMemcpyAsync(c->prt_t, T, nt * sizeof(float), hipMemcpyHostToDevice, st));
    if (const int rc = rays_impl(c, c->prt_t, li, host, n, c->prt_rgb, st, stats)) return rc;
    HIPCHK(c, hipMemcpy(rgb, c->prt_rgb, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return FRT_OK;
}

// the context's copy of the uploaded scene's corner records: frtx_prt_transfer takes the scene view
// again, since an upload keeps none of the view's fp64 arrays
int upload_corners(frt_ctx *c, const frt_scene_view *sv, hipStream_t st)
{
    if (!sv || sv->n_tris != c->n_tris)
        return set_err(c, FRT_E_INVALID, "prt_transfer: the scene view is not the uploaded one (its triangle count differs)");
    const size_t nc = (size_t)c->n_tris * 3;
    std::vector<float> on(nc * 8), rho(nc * 3);
    const std::string bad = frt_prt::corners(sv, on.data(), rho.data());
    if (!bad.empty()) return set_err(c, FRT_E_INVALID, bad);
    if (const int rc = c->prt_corner.reserve(c, on.size() * sizeof(float))) return rc;
    if (const int rc = c->prt_albedo.reserve(c, rho.size() * sizeof(float))) return rc;
    HIPCHK(c, hipMemcpyAsync(c->prt_corner, on.data(), on.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->prt_albedo, rho.data(), rho.size() * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));   // the vectors end with this function
    return FRT_OK;
}

}  // namespace

extern "C" int frtx_prt_transfer(frt_ctx *c, const frt_scene_view *sv, const float *dirs, int64_t n_dirs, int bounces, int flags,
                                 float *T, frt_stats *st)
{
    return transfer_call(c, sv, dirs, n_dirs, bounces, flags, T, false, nullptr, st);
}
extern "C" int frtx_prt_transfer_device(frt_ctx *c, const frt_scene_view *sv, const float *dirs, int64_t n_dirs, int bounces,
                                        int flags, float *T, void *hip_stream, frt_stats *st)
{
    return transfer_call(c, sv, dirs, n_dirs, bounces, flags, T, true, hip_stream, st);
}
extern "C" int frtx_prt_rays(frt_ctx *c, const float *T, const float *li, const float *rays, int64_t n, float *rgb, frt_stats *st)
{
    return rays_call(c, T, li, rays, n, rgb, false, nullptr, st);
}
extern "C" int frtx_prt_rays_device(frt_ctx *c, const float *T, const float *li, const float *rays, int64_t n, float *rgb,
                                    void *hip_stream, frt_stats *st)
{
    return rays_call(c, T, li, rays, n, rgb, true, hip_stream, st);
}

// A PRT frame through the scene's camera: per sample s the first rays a render makes for every pixel
// at sample sample_offset + s (frtx_camera_rays_device into a context buffer), shaded as
// frtx_prt_rays shades them, the samples averaged by frt_film_accumulate's rule
extern "C" int frtx_prt_render(frt_ctx *c, const frt_render_params *p, const float *T, const float *li, float *film, frt_stats *stats)
{
    if (!c) return prt_err(c, FRT_E_INVALID, "prt_render: null context");
    if (!p || !film || p->nx <= 0 || p->ny <= 0 || p->spp <= 0 || p->sample_offset < 0 || (int64_t)p->nx * p->ny > (int64_t)INT32_MAX ||
        (int64_t)p->sample_offset + p->spp > (int64_t)INT32_MAX)
        return set_err(c, FRT_E_INVALID, "prt_render: bad arguments");
    const int64_t n = (int64_t)p->nx * p->ny;
    if (const int rc = check_rays(c, T, li, nullptr, n, film)) return rc;
    if (!c->have_scene) return set_err(c, FRT_E_NO_SCENE, "no scene uploaded");
    if (c->n_tris > 0 && !T) return set_err(c, FRT_E_INVALID, "prt_render: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t nt = (size_t)c->n_tris * 3 * kPrtT;
    if (const int rc = c->prt_t.reserve(c, nt * sizeof(float))) return rc;
    if (const int rc = c->prt_rgb.reserve(c, (size_t)n * 3 * sizeof(float))) return rc;
    if (const int rc = c->sp_pixels.reserve(c, (size_t)n * sizeof(int32_t))) return rc;   // the list calls' buffers: scratch of one call
    if (const int rc = c->sp_rays.reserve(c, (size_t)n * 8 * sizeof(float))) return rc;
    std::vector<int32_t> pix((size_t)n);
    for (int64_t i = 0; i < n; ++i) pix[(size_t)i] = (int32_t)i;
    if (nt) HIPCHK(c, hipMemcpyAsync(c->prt_t, T, nt * sizeof(float), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->sp_pixels, pix.data(), pix.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    std::vector<float> rays((size_t)n * 8), pass((size_t)n * 3);
    frt_stats total{};
    for (int s = 0; s < p->spp; ++s) {
        frt_render_params q = *p;
        q.spp = 1;
        q.sample_offset = p->sample_offset + s;
        if (const int rc = frtx_camera_rays_device(c, &q, c->sp_pixels, n, c->sp_rays, st)) return rc;
        HIPCHK(c, hipMemcpy(rays.data(), c->sp_rays, rays.size() * sizeof(float), hipMemcpyDeviceToHost));
        frt_stats one{};
        if (const int rc = rays_impl(c, c->prt_t, li, rays, n, c->prt_rgb, st, &one)) return rc;
        HIPCHK(c, hipMemcpy(s ? pass.data() : film, c->prt_rgb, pass.size() * sizeof(float), hipMemcpyDeviceToHost));
        if (s && frt_film_accumulate(film, s, pass.data(), 1, (int64_t)pass.size()) != FRT_OK)
            return set_err(c, FRT_E_INVALID, "prt_render: frt_film_accumulate");
        const double ms = total.kernel_ms + one.kernel_ms, all = total.total_ms + one.total_ms;
        const uint64_t cam = total.camera_rays + one.camera_rays;
        total = one;   // the plan fields of the ray query
        total.kernel_ms = ms; total.total_ms = all; total.camera_rays = cam;
    }
    total.samples = (uint64_t)n * (uint64_t)p->spp;
    total.pixels = (uint64_t)n;
    if (stats) *stats = total;
    return FRT_OK;
}
