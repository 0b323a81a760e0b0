// frt_plans.hpp -- the launch plans: which kernel instantiation (frt_kernels.hpp)
// renders a context's scene, and with how much LDS.  Included only by the units
// that instantiate kernels: a plan template emits the kernels it names into
// the unit that calls it.
//
// The plans come in two shapes, and the kernel set is exactly what the two emit:
//  * the fixed shape (walk_plan): one rung per residency and stack class -- the
//    list world (stack 16); the octant copies or the planar tree in LDS (8 / 16);
//    the 4-wide tree (kBvh4LdsStack); the binary tree from HBM (16 / 32, then 64
//    without a register cap); deeper: FRT_E_UNSUPPORTED.  Every integrator but
//    the default path render walks it, as do the path kernels of the estimator
//    flags, PSS-MLT and the ray queries: plan_fixed (path_megakernel with one
//    register cap per residency), pick_mlt and pick_trace (frt_render.hip) hand
//    it a callable that names the kernel of a rung.  A flag's kernels cover every
//    rung, so a flag never falls back to a kernel without it.
//  * the tunable shape (pick_launcher_t): the default path render, the one the
//    benchmarks time.  It has two rungs the fixed shape lacks, a stack-8 kernel
//    from HBM and a stack-24 one, and its register cap is a run-time choice
//    (bvh_launcher: the A/B flags FRT_FLAG_WAVES*, FRT_MATS_WAVES) with one
//    kernel per cap.  Folding it into the walk would add or drop kernels.
// fp64 renders have a rule of their own, plan_f64.
#pragma once
#include <cstdlib>
#include <type_traits>

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
    L.lds = lds_block_bytes(STACK, LDS ? scene_bytes : 0, WORLD != FRT_WORLD_LIST);
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
// each answers FRT_E_UNSUPPORTED unless the context's rung is an octant one
int path_oct(const frt_ctx *c, int flags, int waves, Launcher &L);   // the tunable shape's rung
// FRT_FLAG_ROULETTE, FRT_FLAG_SOBOL: the 5-wave kernels of the sets features = kMatsRoulette, kMatsSobol or both
int path_oct_features(const frt_ctx *c, int flags, int features, Launcher &L);
int mlt_oct(const frt_ctx *c, int flags, const void **boot, const void **chains);
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
            return frt_lds::path_oct(c, flags, waves, L);
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

// ---- the fixed shape ----
// A rung as compile-time constants, and the register cap a plan gives it out of
// its three: the scene in LDS, the binary tree from HBM, the 4-wide tree.  The
// list world and the 64-entry stack take the compiler's own allocation.
template <int STACK, int WORLD, bool LDS>
struct Rung {
    static constexpr int stack = STACK, world = WORLD;
    static constexpr bool lds = LDS;
    template <int W_LDS, int W_HBM, int W_WIDE>
    static constexpr int cap()
    {
        return LDS ? W_LDS : WORLD == kWorldBvh4 ? W_WIDE : (WORLD == FRT_WORLD_LIST || STACK == 64) ? 1 : W_HBM;
    }
};
// f(rung, scene bytes the rung loads into LDS) for the rung of the context's scene; its return code
template <typename F>
static int walk_plan(const frt_ctx *c, int flags, F &&f)
{
    if (c->world_kind == FRT_WORLD_LIST) return f(Rung<16, FRT_WORLD_LIST, false>{}, size_t(0));
    const int d = c->stack_needed;
    const auto [lds, oct, wide] = residency(c, flags);
    if (oct) return d < 8 ? f(Rung<8, kWorldBvh2Oct, true>{}, c->scene_lds_bytes_oct)
                          : f(Rung<16, kWorldBvh2Oct, true>{}, c->scene_lds_bytes_oct);
    if (lds) return d < 8 ? f(Rung<8, FRT_WORLD_BVH, true>{}, c->scene_lds_bytes)
                          : f(Rung<16, FRT_WORLD_BVH, true>{}, c->scene_lds_bytes);
    if (wide) return f(Rung<kBvh4LdsStack, kWorldBvh4, false>{}, size_t(0));
    if (d < 16) return f(Rung<16, FRT_WORLD_BVH, false>{}, size_t(0));
    if (d < 32) return f(Rung<32, FRT_WORLD_BVH, false>{}, size_t(0));
    if (d < 64) return f(Rung<64, FRT_WORLD_BVH, false>{}, size_t(0));
    return FRT_E_UNSUPPORTED;
}
// The fixed shape with path_megakernel<MATS, KIND>: one register cap per residency, so the
// FRT_FLAG_WAVES* A/B flags and FRT_MATS_WAVES do not apply.  Its users:
//  * AO, normals, albedo, depth: caps 5, 6, 6.  AO keeps the specular generate() code (kMatsAll),
//    normals has none (kMatsNone); a context with an environment image runs both with kMatsEnv;
//  * the path kernels of FRT_FLAG_ENV_SAMPLING (kMatsEnvNee), FRT_FLAG_ROULETTE (kMatsRoulette)
//    and FRT_FLAG_SOBOL (kMatsSobol): the caps of the sibling kernels without the flag -- 4, 5, 5
//    with every material (the material unit), 5, 6, 7 (FRT_EXP_W6, FRT_EXP_W7) for a lambertian
//    scene without an image (the main unit).  The latter's octant rung comes from frt_lds, under
//    that unit's scheduler flag.
template <int MATS, int KIND, int W_LDS, int W_HBM, int W_WIDE>
static int plan_fixed(const frt_ctx *c, int flags, Launcher &L)
{
    return walk_plan(c, flags, [&](auto r, size_t scene_bytes) -> int {
        using R = decltype(r);
        if constexpr (R::world == kWorldBvh2Oct && kSplitLds && KIND == FRT_INTEGRATOR_PATH &&
                      (MATS & kMatsFeatures) != 0 && (MATS & ~kMatsFeatures) == 0) {
            static_assert(W_LDS == 5, "frt_lds::path_oct_features holds the 5-wave kernels");
            return frt_lds::path_oct_features(c, flags, MATS, L);
        } else {
            L = make_launcher<R::stack, R::world, R::lds, R::template cap<W_LDS, W_HBM, W_WIDE>(), MATS, KIND>(scene_bytes);
            return FRT_OK;
        }
    });
}
// f(std::integral_constant<int, features>) for a non-empty set of kMatsFeatures bits
template <typename F>
static int with_features(int features, F &&f)
{
    switch (features) {
    case kMatsRoulette: return f(std::integral_constant<int, kMatsRoulette>{});
    case kMatsSobol: return f(std::integral_constant<int, kMatsSobol>{});
    case kMatsSobol | kMatsRoulette: return f(std::integral_constant<int, kMatsSobol | kMatsRoulette>{});
    default: return FRT_E_INVALID;
    }
}

// fp64 kernels (path only; DESIGN.md "Precision"): the list world, or the binary tree from HBM
// (stack 32 or 64), no register cap.  BVH = false: the list rung alone -- the main unit's
// lambertian sets and the material unit's smaller sets have no kernel for a tree (a BVH world's
// fp64 render of those scenes takes the every-material kernels, the debugging build).
#ifndef FRT_EXP_F64_LIST_WAVES
#define FRT_EXP_F64_LIST_WAVES 1   // experiment builds: register cap of the fp64 list kernels (1 = the compiler's own)
#endif
template <int MATS, bool BVH = true>
static int plan_f64(const frt_ctx *c, Launcher &L)
{
    // (a 2-wave register cap changed nothing: profiles/r03/r03c_ab_veach_listbox_f64waves.jsonl; the
    // knob covers the sets with a material or a feature bit, the plain lambertian kernel has none)
    constexpr int kListCap = MATS == kMatsNone ? 1 : FRT_EXP_F64_LIST_WAVES;
    if (c->world_kind == FRT_WORLD_LIST) {
        L = make_launcher<16, FRT_WORLD_LIST, false, kListCap, MATS, FRT_INTEGRATOR_PATH, double>(0);
        return FRT_OK;
    }
    if constexpr (BVH) {
        if (c->stack_needed < 32) L = make_launcher<32, FRT_WORLD_BVH, false, 1, MATS, FRT_INTEGRATOR_PATH, double>(0);
        else if (c->stack_needed < 64) L = make_launcher<64, FRT_WORLD_BVH, false, 1, MATS, FRT_INTEGRATOR_PATH, double>(0);
        else return FRT_E_UNSUPPORTED;
        return FRT_OK;
    }
    return FRT_E_UNSUPPORTED;
}
template <int STACK, int WORLD, bool LDS, bool MATS, bool ENV = false>
static void mlt_kernels_t(const void **boot, const void **chains)
{
    *boot = reinterpret_cast<const void *>(&mlt_bootstrap<STACK, WORLD, MATS, ENV>);
    *chains = reinterpret_cast<const void *>(&mlt_megakernel<STACK, WORLD, LDS, MATS, ENV>);
}

// the material unit's entry points (frt_render_mats.hip)
namespace frt_mats {
// Every kernel with a material set: path (fp32 or f64) and AO of a scene with materials
// (c->mats != kMatsNone), every integrator of a context with an environment image (kMatsEnv),
// the path kernels that sample it (env_sampling: kMatsEnvNee), and the path kernels of
// FRT_FLAG_ROULETTE / _SOBOL (features: their kMatsFeatures bits, 0 = none) of every scene but
// the lambertian ones without an image (those: the main unit and frt_lds).
int pick(const frt_ctx *c, int integrator, int flags, bool f64, bool env_sampling, int features, Launcher &L);
// PSS-MLT with the material branch or (env) the environment image
int mlt(const frt_ctx *c, int flags, bool env, const void **boot, const void **chains);
}  // namespace frt_mats

// the feature unit's entry point (frt_render_feat.hip): the kernels of
// FRT_INTEGRATOR_ALBEDO and FRT_INTEGRATOR_DEPTH, on the plans of normals
// (plan_fixed).  One kernel set for every scene and context: albedo
// always carries the texture lookup, and neither reads the environment, so a
// context with an image runs them too (no kMatsEnv variant).
namespace frt_feat {
int pick(const frt_ctx *c, int integrator, int flags, Launcher &L);
}  // namespace frt_feat
