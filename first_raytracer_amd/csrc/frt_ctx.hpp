// frt_ctx.hpp -- the context behind the C-ABI's frt_ctx handle, the error
// helpers, the residency rule of the launch plans and the few host functions
// that cross the library's units.  Internal to libfrt.so.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "frt.h"
#include "frt_devbuf.hpp"
#include "frt_kernels.hpp"

struct ncclComm;   // rccl's communicator; only frt_multi.hip includes rccl.h

struct frt_ctx {
    int device = -1;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    std::string err;
    // scene
    bool have_scene = false;
    DevScene S{};
    int world_kind = 0, stack_needed = 0;
    bool has_bvh4 = false;        // nodes4 holds the 4-wide BVH4Q
    int depth4 = 0;               // levels of that wide tree
    int n_tris = 0, n_spheres = 0, n_list = 0;
    bool has_spec_mats = false;   // a non-lambertian scattering material or a texture: MATS kernels
    int mats = kMatsNone;         // kMats* mask of the scene's material set (pick_launcher)
    // frt_set_env_image: the environment image's texels in a device buffer of their own, kept
    // across uploads.  A context with one renders with the kernels compiled with the lookup
    // (kMatsEnv, from frt_render_mats.hip); without one every scene keeps its kernels.
    float4 *env_texels = nullptr;
    int env_nx = 0, env_ny = 0;
    uint64_t env_hash = 0;        // of the texels (frt_render_multi: every context must hold the same image)
    // FRT_FLAG_ENV_SAMPLING: the image's sampling tables (csrc/host/envdist.cpp) behind the texels
    // in env_texels, built by the first render that asks for them and kept until the image changes
    enum { kEnvTabNone, kEnvTabBuilt, kEnvTabDark } env_tab = kEnvTabNone;   // Dark: no luminance, not sampled
    bool has_metal = false;       // ao::Li cannot sample metal (constant_pdf::generate throws, pdf.h:195-198)
    size_t scene_lds_bytes = 0;                         // LDS copy with the binary nodes
    size_t scene_lds_bytes_oct = 0;                     // ... with the 8 octant copies of the binary nodes
    int precision = FRT_PRECISION_AUTO;                 // frt_set_precision
    bool has_f64 = false;                               // the scene's fp64 records are in HBM
    double last_mlt_b = 0.0;
    uint64_t mlt_rows = 0;        // chains whose state rows the last PSS-MLT render left in `partial`
    std::vector<void *> scene_bufs;
    // FRT_INTEGRATOR_ERROR: what the last successful path / AO / normals / albedo / depth render
    // left in `partial` -- the parameters an ERROR call must repeat and the granule it ran with.
    // render_impl clears it before anything reuses `partial` and on every failure.
    struct {
        bool valid = false;
        int nx = 0, ny = 0, spp = 0, tile = 0, shard_index = 0, shard_count = 0;
        int spi = 0, n_chunks = 0;
        uint32_t n_slots = 0;
    } last_render;
    // workspace: grow-only device buffers (frt_devbuf.hpp), each on the list that frt_destroy frees
    std::vector<DevBufAny *> bufs;
    DevBuf<float> partial{bufs}, slots_out{bufs};
    unsigned *counter = nullptr;
    DevBuf<unsigned long long> wave_rays{bufs}, splat{bufs};   // splat: the PSS-MLT fixed-point film
    // FRT_INTEGRATOR_DENOISE: the three feature films in slot order, and the pixel-order planes
    // of the filter (the packed guides and the two iterates, frt_denoise.hip)
    DevBuf<float> dn_feat{bufs};
    DevBuf<float4> dn_planes{bufs};
    // frt_render_multi on this context as shard 0: RCCL communicators over the
    // member devices (one per member, cached while the device list is the
    // same), the gather buffer and the device film
    std::vector<int> comm_devs;
    std::vector<ncclComm *> comms;   // ncclComm_t (frt_multi.hip)
    DevBuf<float> gather{bufs}, film_dev{bufs};
    // frtx_render_pixels (frt_render_sparse.hip): buffers of its own -- the chunk sums, the
    // per-wave ray counters, and the host call's device copies of the list and the outputs --
    // so that `partial` and last_render still describe the last full render
    DevBuf<float> sp_partial{bufs}, sp_out{bufs};
    DevBuf<unsigned long long> sp_wave_rays{bufs};
    DevBuf<int32_t> sp_pixels{bufs};
    DevBuf<float> sp_rays{bufs};   // frtx_radiance_rays: the host call's device copy of its list
    // frtx_prt_transfer / frtx_prt_rays (frt_prt.hip): the corner records, the directions with
    // their Y table, the chunk partials of one batch of corners, the previous and the current
    // bounce, the per-wave ray counters, the host calls' device copies of T and of the outputs;
    // for the rays their records and hits and the device triangle of every scene-view triangle
    DevBuf<float4> prt_corner{bufs}, prt_rays{bufs}, prt_hits{bufs};
    DevBuf<float> prt_albedo{bufs}, prt_dirs{bufs}, prt_y{bufs}, prt_partial{bufs}, prt_bounce_a{bufs}, prt_bounce_b{bufs};
    DevBuf<float> prt_t{bufs}, prt_rgb{bufs};
    DevBuf<unsigned long long> prt_wave_rays{bufs};
    DevBuf<int32_t> prt_inv{bufs};
};

#pragma GCC visibility push(hidden)
inline int set_err(frt_ctx *c, int code, const std::string &m)
{
    if (c) c->err = m;
    return code;
}
#define HIPCHK(ctx, x)                                                                             \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess)                                                                      \
            return set_err(ctx, FRT_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));       \
    } while (0)

// 4-wide traversal holds at most 3 pending siblings per level of the path
inline bool bvh4_stack_fits(int depth4, int lds_entries) { return 3 * depth4 <= lds_entries + kBvh4Overflow; }
#ifndef FRT_EXP_BVH4_LSTACK
#define FRT_EXP_BVH4_LSTACK 12
#endif
// LDS entries of the 4-wide stack; deeper ones go to scratch.  12 since round 5
// (was 16): 12 KiB of stack + 10 KiB of item state a block let 7 blocks share a
// CU's 160 KiB, and the lambertian 4-wide kernel runs 7 waves/SIMD (72 VGPRs,
// no spills since the SLP vectorizer is off): cornell_1m 360.3 -> 344.3 ms
// (+4.6 %, same call, profiles/r05/r05i/ab_m.jsonl)
constexpr int kBvh4LdsStack = FRT_EXP_BVH4_LSTACK;

// Where a plan keeps the scene (every integrator's plan and the ray queries
// decide it here): lds = the binary tree with the scene in LDS, oct = ... with
// the per-octant node copies, wide = the 4-wide quantized tree from HBM.  List
// worlds have no tree: all false.  The stack sizes stay with each plan.
struct Residency { bool lds, oct, wide; };
inline Residency residency(const frt_ctx *c, int flags)
{
    Residency r;
    r.lds = c->world_kind == FRT_WORLD_BVH && c->stack_needed < kLdsMaxDepth && lds_planar_fits(c->scene_lds_bytes) &&
            !(flags & FRT_FLAG_NO_LDS_SCENE);
    r.oct = r.lds && !(flags & FRT_FLAG_NO_OCT) && lds_octant_fits(c->scene_lds_bytes_oct);
    r.wide = !r.lds && c->has_bvh4 && !(flags & FRT_FLAG_BVH2) && bvh4_stack_fits(c->depth4, kBvh4LdsStack);
    return r;
}

// frt_render.hip
int eff_tile(const frt_render_params *p);
bool params_ok(const frt_render_params *p);
int render_impl(frt_ctx *c, const frt_render_params *p, float *dev_slots, hipStream_t st, frt_stats *stats);
int trav_min(bool lds_scene, bool path = false);
int min_desc(bool lds_scene);
bool use_f64(const frt_ctx *c, const frt_render_params *p);
int env_tables(frt_ctx *c);
// What a path / AO render (a frame or a list) settles before it picks its plan: the sampling tables
// of FRT_FLAG_ENV_SAMPLING (*env_sampling: the kernels that sample the image), the refusal of AO
// over metal, and *f64 with the refusal of fp64 kernels for a scene uploaded without fp64 records
int render_preamble(frt_ctx *c, const frt_render_params *p, bool *env_sampling, bool *f64);
// One launch of a persistent kernel (path, PSS-MLT, the lists, the ray queries), in this order:
// persist_plan, queue_headroom, persist_launch, the caller's follow-up kernels and its
// hipEventRecord(c->ev1) where its kernel_ms ends, persist_finish, fill_plan_stats.
struct Launcher;   // frt_plans.hpp
struct Persist {
    std::chrono::steady_clock::time_point t_start = std::chrono::steady_clock::now();   // of total_ms
    int grid = 0;
    size_t n_waves = 0;
    bool diag = false;   // FRT_DIAG builds: the launch fills the per-phase counters (frt_diag_read)
};
// grid: the blocks of fn that the device holds at once, max_blocks at the most; counters, where the
// kernel keeps per-wave ray counters: room for [n_waves][4]
int persist_plan(frt_ctx *c, const void *fn, size_t lds, int64_t max_blocks, DevBuf<unsigned long long> *counters, Persist &P);
// the 32-bit queue head runs past n_items by up to per_wave for each wave: refused with `msg`
int queue_headroom(frt_ctx *c, const Persist &P, uint64_t n_items, uint64_t per_wave, const std::string &msg);
// zero the queue (queue_bytes from `queue`), record ev0, launch (run = false: no work, no launch)
int persist_launch(frt_ctx *c, const Persist &P, const char *name, const void *fn, size_t lds, void **args, unsigned *queue,
                   size_t queue_bytes, hipStream_t st, bool run = true);
// copy the counters (NULL: none were written), wait for the stream; *stats (may be NULL) is zeroed
// and gets the counters' sums over the waves, kernel_ms = ev0 .. ev1 and total_ms, then the plan's fields
int persist_finish(frt_ctx *c, const Persist &P, const unsigned long long *counters, hipStream_t st, frt_stats *stats);
void fill_plan_stats(frt_stats *stats, const frt_ctx *c, const Launcher &L);
// frt_multi.hip
void free_comms(frt_ctx *c);
// frt_denoise.hip: the filter of FRT_INTEGRATOR_DENOISE over a whole frame in slot order (shard 0
// of 1) -- colour_slots in place, guided by the three feature films in the same order; *ms gets
// the device time of its kernels
namespace frt_denoise {
int run(frt_ctx *c, const frt_render_params *p, float *colour_slots, const float *normals_slots,
        const float *albedo_slots, const float *depth_slots, uint32_t n_slots, hipStream_t st, float *ms);
}
// frt_error.hip: the variance film of FRT_INTEGRATOR_ERROR in slot order (padding slots 0) from the
// n_chunks x n_slots chunk sums in c->partial (chunks of spi samples, the last what is left of
// p->spp); *ms gets the device time of its kernel
namespace frt_error {
int run(frt_ctx *c, const frt_render_params *p, float *out_slots, uint32_t n_slots, int n_chunks, int spi,
        hipStream_t st, float *ms);
}
#pragma GCC visibility pop
