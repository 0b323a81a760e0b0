// frt_plans.hpp -- the launch plans: which kernel instantiation (frt_kernels.hpp)
// renders a context's scene, and with how much LDS.  Included only by the units
// that instantiate kernels: a plan template emits the kernels it names into
// the unit that calls it.
#pragma once
#include <cstdlib>

#include "frt_ctx.hpp"

// ---- launch plans ----
// Shared by the kernel units of the library: frt_render.hip, and
// frt_render_mats.hip, which holds every kernel compiled with a material set
// (MATS != kMatsNone: the path
// kernels of specular / textured scenes, AO, the fp64 kernels of such scenes,
// PSS-MLT on them).  That unit is compiled with the basic SGPR register
// allocator (Makefile): under the default greedy allocator these kernels
// have given the oracle's ray counts with wrong radiance at some register
// caps, in every failing source state on record, and the basic SGPR (or
// VGPR) allocator removed every such failure at an equal or larger spill
// count (DESIGN.md "Register-cap hazard").  The lambertian kernels (the
// bench configurations) stay on the greedy allocator.
struct Launcher {
    const void *fn = nullptr;
    size_t lds = 0;
    int stack = 0;
    int waves = 0;
    bool lds_scene = false;
    bool wide = false;      // 4-wide quantized BVH
    bool f64 = false;       // the fp64 kernel
    size_t scene_lds = 0;   // scene bytes the plan loads into LDS (octant copies or planar tree), 0 = HBM
};
template <int STACK, int WORLD, bool LDS, int WAVES = 1, int MATS = kMatsNone,
          int KIND = FRT_INTEGRATOR_PATH, typename R = float>
static Launcher make_launcher(size_t scene_bytes)
{
    Launcher L;
    L.fn = reinterpret_cast<const void *>(&path_megakernel<STACK, WORLD, LDS, WAVES, MATS, KIND, R>);
    L.f64 = kIsF64<R>;
    L.lds = (WORLD != FRT_WORLD_LIST ? (size_t)STACK * kBlock * sizeof(int) : 0) +
            (size_t)kItemWords * kBlock * sizeof(int) + (LDS ? scene_bytes : 0);
    L.scene_lds = LDS ? scene_bytes : 0;
    L.stack = STACK;
    L.waves = WAVES > 1 ? WAVES : 0;
    L.lds_scene = LDS;
    L.wide = WORLD == kWorldBvh4;
    return L;
}
#ifndef FRT_EXP_W6
#define FRT_EXP_W6 6   // experiment builds: the register cap behind the "6 waves" plans
#endif
#ifndef FRT_EXP_W7
#define FRT_EXP_W7 7   // experiment builds: the register cap behind the 4-wide "7 waves" plan
#endif
template <int STACK, bool LDS, int WORLD = FRT_WORLD_BVH, int MATS = kMatsNone>
static Launcher bvh_launcher(int waves, size_t sb)
{
    // Every material set has a 6-wave build again (round 3).  Under the greedy
    // register allocator the material kernels have compiled, at some caps, to
    // kernels with the oracle's ray counts and wrong radiance; they now come
    // from frt_render_mats.hip, built with the basic SGPR allocator, which
    // removed every such failure on record (DESIGN.md "Register-cap hazard";
    // test_register_caps_agree checks every cap and plan).  The defaults stay
    // 4 / 5 waves for the specular sets (faster than 6:
    // profiles/r02/r02_ab_sphere_hbm_mats.jsonl).
    if constexpr (MATS == kMatsNone && WORLD == kWorldBvh4)   // the lambertian 4-wide HBM plan (round 5)
        if (waves == 7) return make_launcher<STACK, WORLD, LDS, FRT_EXP_W7, MATS>(sb);
    if (waves == 6) return make_launcher<STACK, WORLD, LDS, FRT_EXP_W6, MATS>(sb);
    if (waves == 5) return make_launcher<STACK, WORLD, LDS, 5, MATS>(sb);
    if constexpr (MATS != kMatsNone) {
        if (waves == 4) return make_launcher<STACK, WORLD, LDS, 4, MATS>(sb);
        if (waves == 3) return make_launcher<STACK, WORLD, LDS, 3, MATS>(sb);
    }
    return make_launcher<STACK, WORLD, LDS, 1, MATS>(sb);
}
// Two more units for the lambertian kernels of the octant LDS plan, each under
// the machine scheduling strategy that measured fastest for it (same call, two
// alternations): frt_render_lds.hip holds the path kernels (C2) under
// max-memory-clause (Makefile LDSFLAGS; Cornell 229.4 / 229.7 -> 227.5 / 227.5
// ms, profiles/r06/r06f), frt_render_chain.hip the PSS-MLT chain kernels (C5)
// under iterative-maxocc (CHAINFLAGS; 576.8 / 576.1 -> 570.6 / 571.6 ms against
// max-memory-clause, profiles/r06/r06h).  The 4-wide HBM kernel (cornell_1m)
// loses under every other strategy (max-memory-clause 1.6 %, iterative ones
// 9-26 %), so it stays in the main unit on the default one.  Diagnostic builds
// (FRT_DIAG: their counters are a device global of the main unit) keep these
// kernels in the main unit; the two units then compile their entry points to
// FRT_E_UNSUPPORTED and hold no kernel.
#if defined(FRT_DIAG) || defined(FRT_EXP_NO_LDS_SPLIT)
constexpr bool kSplitLds = false;
#else
constexpr bool kSplitLds = true;
#endif
namespace frt_lds {
int path_oct(int stack, int waves, size_t scene_bytes, Launcher &L);
int path_oct_roulette(int stack, size_t scene_bytes, Launcher &L);   // FRT_FLAG_ROULETTE: the 5-wave kernels
int path_oct_sobol(int stack, bool roulette, size_t scene_bytes, Launcher &L);   // FRT_FLAG_SOBOL [| _ROULETTE]: the same
int mlt_oct(int stack, const void **boot, const void **chains);
}  // namespace frt_lds

// MATS: the material set the kernel is compiled for (kMats* mask, frt_path.hpp)
template <int MATS>
static int pick_launcher_t(const frt_ctx *c, int flags, Launcher &L)
{
    if (c->world_kind == FRT_WORLD_LIST) { L = make_launcher<16, FRT_WORLD_LIST, false, 1, MATS>(0); return FRT_OK; }
    const int d = c->stack_needed;
    const size_t sb = c->scene_lds_bytes;
    const auto [lds, oct, wide] = residency(c, flags);
    // register cap: waves/SIMD the compiler must fit (its spills land in the
    // shading code, not the traversal loops).  Measured (profiles/r01_ab_perf3.jsonl):
    // 5 waves best for LDS-resident scenes, 6 for HBM-resident ones.  The
    // material kernels (MATS) in LDS run 15-21 % faster on the compiler's own
    // allocation than under the 5-wave cap (profiles/r01d_perf_mats.jsonl).
    // Material kernels: textures alone cost about the lambertian kernel's
    // registers (117 vs 111 VGPRs uncapped; the compiler's 4 waves are best),
    // the specular branch 152, the rough conductor lobes 170 -- capped at 4
    // waves/SIMD (128 VGPRs; a few spills in the specular shading) they run
    // +40 % over the compiler's 2-wave allocation (same-call A/B,
    // profiles/r02/r02_mats*.jsonl).
    // (The lambertian LDS kernel fits 111 VGPRs without spills since its work-
    // item state moved to LDS; the compiler's 4 waves win 2 % at 64 spp but lose
    // 10 % at the bench's 512 spp -- 337 vs 307 ms, same call --, so the cap stays:
    // profiles/r02/r02_ab_cornell_knobs.jsonl, r02_ab_cornell_512spp.jsonl.)
    int waves = (MATS & kMatsSpecAny) ? (lds ? 4 : 5) : (MATS & ~kMatsEnv) == kMatsTex && lds ? 0 : lds ? 5 : 6;
    // the lambertian 4-wide HBM plan: 7 waves (round 5; the binary HBM fallback keeps 6)
    if (MATS == kMatsNone && wide) waves = 7;
    if constexpr (MATS != kMatsNone) {   // FRT_MATS_WAVES: register cap of the material kernels (tuning knob, not part of the C-ABI)
        const char *e = std::getenv("FRT_MATS_WAVES");
        if (e) waves = std::atoi(e);
    }
    if (flags & FRT_FLAG_WAVES4) waves = 0;   // the compiler's own allocation (~120 VGPRs, 4 waves)
    if (flags & FRT_FLAG_WAVES5) waves = 5;
    if (flags & FRT_FLAG_WAVES6) waves = 6;
    // (Measured and removed A/B plans, DESIGN.md section 5: lockstep brute force over tiny
    // scenes, 4-wide nodes from LDS, speculative traversal, an 8-wide HBM tree.)
    // HBM-resident scenes: the 4-wide quantized BVH (half the bytes per box test)
    if (wide) {
        L = bvh_launcher<kBvh4LdsStack, false, kWorldBvh4, MATS>(waves, 0);
        return FRT_OK;
    }
    // LDS-resident binary tree: the per-octant node copies when they fit
    if (oct) {
        if constexpr (MATS == kMatsNone && kSplitLds) {   // the third unit's kernels (frt_lds)
            return frt_lds::path_oct(d < 8 ? 8 : 16, waves, c->scene_lds_bytes_oct, L);
        } else {
            L = d < 8 ? bvh_launcher<8, true, kWorldBvh2Oct, MATS>(waves, c->scene_lds_bytes_oct)
                      : bvh_launcher<16, true, kWorldBvh2Oct, MATS>(waves, c->scene_lds_bytes_oct);
            return FRT_OK;
        }
    }
    if (d < 8) L = lds ? bvh_launcher<8, true, FRT_WORLD_BVH, MATS>(waves, sb)
                       : bvh_launcher<8, false, FRT_WORLD_BVH, MATS>(waves, 0);
    else if (d < 16) L = lds ? bvh_launcher<16, true, FRT_WORLD_BVH, MATS>(waves, sb)
                             : bvh_launcher<16, false, FRT_WORLD_BVH, MATS>(waves, 0);
    else if (d < 24) L = bvh_launcher<24, false, FRT_WORLD_BVH, MATS>(waves, 0);
    else if (d < 32) L = bvh_launcher<32, false, FRT_WORLD_BVH, MATS>(waves, 0);
    else if (d < 64) L = make_launcher<64, FRT_WORLD_BVH, false, 1, MATS>(0);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
}
// AO / normals: the default plans only (LDS-resident binary BVH, HBM 4-wide or
// binary), register caps as for path; ao keeps the specular generate() code
// (M = kMatsAll), normals has none (kMatsNone); a context with an environment
// image runs both with kMatsEnv (the lookup on a miss).
template <int KIND, int M>
static int pick_launcher_kind(const frt_ctx *c, int flags, Launcher &L)
{
    if (c->world_kind == FRT_WORLD_LIST) { L = make_launcher<16, FRT_WORLD_LIST, false, 1, M, KIND>(0); return FRT_OK; }
    const int d = c->stack_needed;
    const size_t sb = c->scene_lds_bytes;
    const auto [lds, oct, wide] = residency(c, flags);
    if (oct) {
        L = d < 8 ? make_launcher<8, kWorldBvh2Oct, true, 5, M, KIND>(c->scene_lds_bytes_oct)
                  : make_launcher<16, kWorldBvh2Oct, true, 5, M, KIND>(c->scene_lds_bytes_oct);
    } else if (lds) {
        L = d < 8 ? make_launcher<8, FRT_WORLD_BVH, true, 5, M, KIND>(sb)
                  : make_launcher<16, FRT_WORLD_BVH, true, 5, M, KIND>(sb);
    } else if (wide) {
        L = make_launcher<kBvh4LdsStack, kWorldBvh4, false, 6, M, KIND>(0);
    } else if (d < 16) {
        L = make_launcher<16, FRT_WORLD_BVH, false, 6, M, KIND>(0);
    } else if (d < 32) {
        L = make_launcher<32, FRT_WORLD_BVH, false, 6, M, KIND>(0);
    } else if (d < 64) {
        L = make_launcher<64, FRT_WORLD_BVH, false, 1, M, KIND>(0);
    } else {
        return FRT_E_UNSUPPORTED;
    }
    return FRT_OK;
}
// fp64 kernels (path only; DESIGN.md "Precision"): the list world with the
// scene's material set, or the binary tree from HBM with every material
// compiled in (the debugging build; no register cap, stack 32 or 64)
#ifndef FRT_EXP_F64_LIST_WAVES
#define FRT_EXP_F64_LIST_WAVES 1   // experiment builds: register cap of the fp64 list kernels (1 = the compiler's own)
#endif
template <int MATS>
static int pick_launcher_f64_t(const frt_ctx *c, Launcher &L)
{
    if (c->world_kind == FRT_WORLD_LIST) {
        // (a 2-wave register cap changed nothing: profiles/r03/r03c_ab_veach_listbox_f64waves.jsonl)
        L = make_launcher<16, FRT_WORLD_LIST, false, FRT_EXP_F64_LIST_WAVES, MATS, FRT_INTEGRATOR_PATH, double>(0);
        return FRT_OK;
    }
    const int d = c->stack_needed;
    constexpr int kAll = kMatsAll | (MATS & kMatsEnv);
    if (d < 32) L = make_launcher<32, FRT_WORLD_BVH, false, 1, kAll, FRT_INTEGRATOR_PATH, double>(0);
    else if (d < 64) L = make_launcher<64, FRT_WORLD_BVH, false, 1, kAll, FRT_INTEGRATOR_PATH, double>(0);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
}
// Path renders with FRT_FLAG_ROULETTE (the kMatsRoulette kernels): as the
// kernels of FRT_FLAG_ENV_SAMPLING, one register cap per residency -- W_LDS,
// W_HBM, W_WIDE, the defaults of the sibling kernels without roulette -- so the
// FRT_FLAG_WAVES* A/B flags and FRT_MATS_WAVES do not apply.  Every residency a
// context can have is covered: the flag never falls back to a kernel without
// roulette.  The octant plan's lambertian kernels come from frt_lds
// (path_oct_roulette), under that unit's scheduler flag.
// The kMatsSobol kernels (FRT_FLAG_SOBOL, with or without roulette) take the
// same plans with the same caps: MATS then carries kMatsSobol, and the octant
// plan's lambertian kernels are frt_lds::path_oct_sobol's.
template <int MATS, int W_LDS, int W_HBM, int W_WIDE>
static int pick_launcher_roulette_t(const frt_ctx *c, int flags, Launcher &L)
{
    static_assert((MATS & kMatsFeatures) != 0, "the roulette and Sobol' kernels' plans");
    if (c->world_kind == FRT_WORLD_LIST) { L = make_launcher<16, FRT_WORLD_LIST, false, 1, MATS>(0); return FRT_OK; }
    const int d = c->stack_needed;
    const size_t sb = c->scene_lds_bytes;
    const auto [lds, oct, wide] = residency(c, flags);
    if (oct) {
        if constexpr (MATS == kMatsRoulette && kSplitLds) {
            return frt_lds::path_oct_roulette(d < 8 ? 8 : 16, c->scene_lds_bytes_oct, L);
        } else if constexpr ((MATS & ~kMatsRoulette) == kMatsSobol && kSplitLds) {
            return frt_lds::path_oct_sobol(d < 8 ? 8 : 16, (MATS & kMatsRoulette) != 0, c->scene_lds_bytes_oct, L);
        } else {
            L = d < 8 ? make_launcher<8, kWorldBvh2Oct, true, W_LDS, MATS>(c->scene_lds_bytes_oct)
                      : make_launcher<16, kWorldBvh2Oct, true, W_LDS, MATS>(c->scene_lds_bytes_oct);
        }
    } else if (lds) {
        L = d < 8 ? make_launcher<8, FRT_WORLD_BVH, true, W_LDS, MATS>(sb)
                  : make_launcher<16, FRT_WORLD_BVH, true, W_LDS, MATS>(sb);
    } else if (wide) {
        L = make_launcher<kBvh4LdsStack, kWorldBvh4, false, W_WIDE, MATS>(0);
    } else if (d < 16) {
        L = make_launcher<16, FRT_WORLD_BVH, false, W_HBM, MATS>(0);
    } else if (d < 32) {
        L = make_launcher<32, FRT_WORLD_BVH, false, W_HBM, MATS>(0);
    } else if (d < 64) {
        L = make_launcher<64, FRT_WORLD_BVH, false, 1, MATS>(0);
    } else {
        return FRT_E_UNSUPPORTED;
    }
    return FRT_OK;
}
// ... and their fp64 kernels: the list world, or the binary tree from HBM
// (stack 32 or 64), no register cap
template <int MATS>
static int pick_launcher_roulette_f64_t(const frt_ctx *c, Launcher &L)
{
    static_assert((MATS & kMatsFeatures) != 0, "the roulette and Sobol' kernels' plans");
    if (c->world_kind == FRT_WORLD_LIST)
        L = make_launcher<16, FRT_WORLD_LIST, false, FRT_EXP_F64_LIST_WAVES, MATS, FRT_INTEGRATOR_PATH, double>(0);
    else if (c->stack_needed < 32) L = make_launcher<32, FRT_WORLD_BVH, false, 1, MATS, FRT_INTEGRATOR_PATH, double>(0);
    else if (c->stack_needed < 64) L = make_launcher<64, FRT_WORLD_BVH, false, 1, MATS, FRT_INTEGRATOR_PATH, double>(0);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
}
template <int STACK, int WORLD, bool LDS, bool MATS, bool ENV = false>
static void mlt_kernels_t(const void **boot, const void **chains)
{
    *boot = reinterpret_cast<const void *>(&mlt_bootstrap<STACK, WORLD, MATS, ENV>);
    *chains = reinterpret_cast<const void *>(&mlt_megakernel<STACK, WORLD, LDS, MATS, ENV>);
}

// the material unit's entry points (frt_render_mats.hip)
namespace frt_mats {
// path (KIND = FRT_INTEGRATOR_PATH, fp32), fp64 path (f64) or AO: the plan for
// the scene's material set c->mats (!= kMatsNone); and every integrator of a
// context with an environment image (the kMatsEnv kernels)
int pick(const frt_ctx *c, int integrator, int flags, bool f64, Launcher &L);
// the path kernels that also sample the environment image (FRT_FLAG_ENV_SAMPLING)
int pick_env_sampling(const frt_ctx *c, int flags, bool f64, Launcher &L);
// the path kernels with Russian roulette (FRT_FLAG_ROULETTE) of every scene but
// the lambertian ones without an image (those: the main unit and frt_lds);
// env_sampling: the kernels that also sample the image
int pick_roulette(const frt_ctx *c, int flags, bool f64, bool env_sampling, Launcher &L);
// the path kernels of FRT_FLAG_SOBOL (roulette: with FRT_FLAG_ROULETTE as well) of the
// same scenes, on the same plans and caps
int pick_sobol(const frt_ctx *c, int flags, bool f64, bool env_sampling, bool roulette, Launcher &L);
// PSS-MLT with the material branch or (env) the environment image, for the
// (stack, world, lds) plans of render_mlt
int mlt(int stack, int world, bool lds, bool env, const void **boot, const void **chains);
}  // namespace frt_mats

// the feature unit's entry point (frt_render_feat.hip): the kernels of
// FRT_INTEGRATOR_ALBEDO and FRT_INTEGRATOR_DEPTH, on the plans of normals
// (pick_launcher_kind).  One kernel set for every scene and context: albedo
// always carries the texture lookup, and neither reads the environment, so a
// context with an image runs them too (no kMatsEnv variant).
namespace frt_feat {
int pick(const frt_ctx *c, int integrator, int flags, Launcher &L);
}  // namespace frt_feat
