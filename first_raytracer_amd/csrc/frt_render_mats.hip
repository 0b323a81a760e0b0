// The library's second translation unit: every kernel compiled with a
// material set (MATS != kMatsNone), reached through frt_mats::pick /
// frt_mats::mlt (frt_plans.hpp).  Built with the basic SGPR register
// allocator (Makefile, MATSFLAGS); see DESIGN.md "Register-cap hazard".
#undef FRT_DIAG
#include "frt_kernels.hpp"
#include "frt_plans.hpp"

// a context with an environment image: two material sets carry the lookup --
// textures alone (lambertian and textured scenes) and every material
static int pick_env(const frt_ctx *c, int integrator, int flags, bool f64, Launcher &L)
{
    if (integrator == FRT_INTEGRATOR_AO) return pick_launcher_kind<FRT_INTEGRATOR_AO, kMatsAll | kMatsEnv>(c, flags, L);
    if (integrator == FRT_INTEGRATOR_NORMALS) return pick_launcher_kind<FRT_INTEGRATOR_NORMALS, kMatsEnv>(c, flags, L);
    if (f64) return pick_launcher_f64_t<kMatsAll | kMatsEnv>(c, L);
    if ((c->mats & ~kMatsTex) == 0) return pick_launcher_t<kMatsTex | kMatsEnv>(c, flags, L);
    return pick_launcher_t<kMatsAll | kMatsEnv>(c, flags, L);
}
int frt_mats::pick(const frt_ctx *c, int integrator, int flags, bool f64, Launcher &L)
{
    if (c->env_texels) return pick_env(c, integrator, flags, f64, L);
    if (integrator == FRT_INTEGRATOR_AO) return pick_launcher_kind<FRT_INTEGRATOR_AO, kMatsAll>(c, flags, L);
    if (f64) {
        switch (c->mats) {   // (a lambertian scene comes here with a BVH world only: the kMatsAll kernels)
        case kMatsTex: return pick_launcher_f64_t<kMatsTex>(c, L);
        case kMatsSpec: return pick_launcher_f64_t<kMatsSpec>(c, L);   // veach_mis (C3): phong plates
        case kMatsSpec | kMatsTex: return pick_launcher_f64_t<kMatsSpec | kMatsTex>(c, L);
        default: return pick_launcher_f64_t<kMatsAll>(c, L);
        }
    }
    switch (c->mats) {   // the smallest kernel covering the scene's materials
    case kMatsTex: return pick_launcher_t<kMatsTex>(c, flags, L);
    case kMatsSpec:
    case kMatsSpec | kMatsTex: return pick_launcher_t<kMatsSpec | kMatsTex>(c, flags, L);
    default: return pick_launcher_t<kMatsAll>(c, flags, L);
    }
}
// Path renders with FRT_FLAG_ENV_SAMPLING on a context with an environment image
// (the kMatsEnvNee kernels): one material set, every material, and one register
// cap per residency -- the specular sets' defaults, 4 waves from LDS and 5 from
// HBM -- so the FRT_FLAG_WAVES* A/B flags and FRT_MATS_WAVES do not apply here.
// Every residency a context can have is covered: the flag never falls back to a
// kernel without the sampling.
constexpr int kMatsNee = kMatsAll | kMatsEnv | kMatsEnvNee;
static int pick_launcher_nee(const frt_ctx *c, int flags, Launcher &L)
{
    if (c->world_kind == FRT_WORLD_LIST) { L = make_launcher<16, FRT_WORLD_LIST, false, 1, kMatsNee>(0); return FRT_OK; }
    const int d = c->stack_needed;
    const size_t sb = c->scene_lds_bytes;
    const auto [lds, oct, wide] = residency(c, flags);
    if (oct) {
        L = d < 8 ? make_launcher<8, kWorldBvh2Oct, true, 4, kMatsNee>(c->scene_lds_bytes_oct)
                  : make_launcher<16, kWorldBvh2Oct, true, 4, kMatsNee>(c->scene_lds_bytes_oct);
    } else if (lds) {
        L = d < 8 ? make_launcher<8, FRT_WORLD_BVH, true, 4, kMatsNee>(sb)
                  : make_launcher<16, FRT_WORLD_BVH, true, 4, kMatsNee>(sb);
    } else if (wide) {
        L = make_launcher<kBvh4LdsStack, kWorldBvh4, false, 5, kMatsNee>(0);
    } else if (d < 16) {
        L = make_launcher<16, FRT_WORLD_BVH, false, 5, kMatsNee>(0);
    } else if (d < 32) {
        L = make_launcher<32, FRT_WORLD_BVH, false, 5, kMatsNee>(0);
    } else if (d < 64) {
        L = make_launcher<64, FRT_WORLD_BVH, false, 1, kMatsNee>(0);
    } else {
        return FRT_E_UNSUPPORTED;
    }
    return FRT_OK;
}
static int pick_launcher_nee_f64(const frt_ctx *c, Launcher &L)
{
    if (c->world_kind == FRT_WORLD_LIST)
        L = make_launcher<16, FRT_WORLD_LIST, false, FRT_EXP_F64_LIST_WAVES, kMatsNee, FRT_INTEGRATOR_PATH, double>(0);
    else if (c->stack_needed < 32) L = make_launcher<32, FRT_WORLD_BVH, false, 1, kMatsNee, FRT_INTEGRATOR_PATH, double>(0);
    else if (c->stack_needed < 64) L = make_launcher<64, FRT_WORLD_BVH, false, 1, kMatsNee, FRT_INTEGRATOR_PATH, double>(0);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
}
int frt_mats::pick_env_sampling(const frt_ctx *c, int flags, bool f64, Launcher &L)
{
    return f64 ? pick_launcher_nee_f64(c, L) : pick_launcher_nee(c, flags, L);
}
// Path renders with FRT_FLAG_ROULETTE (the kMatsRoulette kernels): every material,
// without an image, with one (kMatsEnv) or sampling it (kMatsEnvNee); the register
// caps of the every-material siblings, 4 waves from LDS and 5 from HBM.
// Lambertian and textured scenes take these supersets too (a lambertian scene
// without an image: kMatsNone | kMatsRoulette, main unit).
template <int MATS>
static int pick_roulette_t(const frt_ctx *c, int flags, bool f64, Launcher &L)
{
    return f64 ? pick_launcher_roulette_f64_t<MATS>(c, L) : pick_launcher_roulette_t<MATS, 4, 5, 5>(c, flags, L);
}
int frt_mats::pick_roulette(const frt_ctx *c, int flags, bool f64, bool env_sampling, Launcher &L)
{
    if (env_sampling) return pick_roulette_t<kMatsNee | kMatsRoulette>(c, flags, f64, L);
    if (c->env_texels) return pick_roulette_t<kMatsAll | kMatsEnv | kMatsRoulette>(c, flags, f64, L);
    return pick_roulette_t<kMatsAll | kMatsRoulette>(c, flags, f64, L);
}
// ... and with FRT_FLAG_SOBOL (the kMatsSobol kernels), alone or with roulette: the same
// material sets, plans and caps
template <int EXTRA>
static int pick_sobol_t(const frt_ctx *c, int flags, bool f64, bool env_sampling, Launcher &L)
{
    if (env_sampling) return pick_roulette_t<kMatsNee | EXTRA>(c, flags, f64, L);
    if (c->env_texels) return pick_roulette_t<kMatsAll | kMatsEnv | EXTRA>(c, flags, f64, L);
    return pick_roulette_t<kMatsAll | EXTRA>(c, flags, f64, L);
}
int frt_mats::pick_sobol(const frt_ctx *c, int flags, bool f64, bool env_sampling, bool roulette, Launcher &L)
{
    return roulette ? pick_sobol_t<kMatsSobol | kMatsRoulette>(c, flags, f64, env_sampling, L)
                    : pick_sobol_t<kMatsSobol>(c, flags, f64, env_sampling, L);
}
template <bool MATS, bool ENV>
static int mlt_pick(int stack, int world, bool lds, const void **boot, const void **chains)
{
    if (world == FRT_WORLD_LIST) mlt_kernels_t<16, FRT_WORLD_LIST, false, MATS, ENV>(boot, chains);
    else if (world == kWorldBvh4) mlt_kernels_t<kBvh4LdsStack, kWorldBvh4, false, MATS, ENV>(boot, chains);
    else if (world == kWorldBvh2Oct && stack == 8) mlt_kernels_t<8, kWorldBvh2Oct, true, MATS, ENV>(boot, chains);
    else if (world == kWorldBvh2Oct && stack == 16) mlt_kernels_t<16, kWorldBvh2Oct, true, MATS, ENV>(boot, chains);
    else if (lds && stack == 8) mlt_kernels_t<8, FRT_WORLD_BVH, true, MATS, ENV>(boot, chains);
    else if (lds && stack == 16) mlt_kernels_t<16, FRT_WORLD_BVH, true, MATS, ENV>(boot, chains);
    else if (!lds && stack == 16) mlt_kernels_t<16, FRT_WORLD_BVH, false, MATS, ENV>(boot, chains);
    else if (!lds && stack == 32) mlt_kernels_t<32, FRT_WORLD_BVH, false, MATS, ENV>(boot, chains);
    else if (!lds && stack == 64) mlt_kernels_t<64, FRT_WORLD_BVH, false, MATS, ENV>(boot, chains);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
}
// (an environment image always takes the material branch: one chain kernel per plan carries the lookup)
int frt_mats::mlt(int stack, int world, bool lds, bool env, const void **boot, const void **chains)
{
    return env ? mlt_pick<true, true>(stack, world, lds, boot, chains) : mlt_pick<true, false>(stack, world, lds, boot, chains);
}
