// The library's second translation unit: every kernel compiled with a
// material set (MATS != kMatsNone), reached through frt_mats::pick /
// frt_mats::mlt (frt_plans.hpp).  Built with the basic SGPR register
// allocator (Makefile, MATSFLAGS); see DESIGN.md "Register-cap hazard".
#undef FRT_DIAG
#include "frt_kernels.hpp"
#include "frt_plans.hpp"

// The path kernels of an estimator flag: one material set -- every material, with the image's
// lookup and sampling as the context and the call have them -- on the fixed shape, with the
// register caps of the specular sets' defaults (4 waves from LDS, 5 from HBM).  Lambertian and
// textured scenes take these supersets too.
template <int MATS>
static int plan_estimator(const frt_ctx *c, int flags, bool f64, Launcher &L)
{
    return f64 ? plan_f64<MATS>(c, L) : plan_fixed<MATS, FRT_INTEGRATOR_PATH, 4, 5, 5>(c, flags, L);
}
constexpr int kMatsNee = kMatsAll | kMatsEnv | kMatsEnvNee;
template <int FEATURES>
static int plan_features(const frt_ctx *c, int flags, bool f64, bool env_sampling, Launcher &L)
{
    if (env_sampling) return plan_estimator<kMatsNee | FEATURES>(c, flags, f64, L);
    if (c->env_texels) return plan_estimator<kMatsAll | kMatsEnv | FEATURES>(c, flags, f64, L);
    return plan_estimator<kMatsAll | FEATURES>(c, flags, f64, L);
}
int frt_mats::pick(const frt_ctx *c, int integrator, int flags, bool f64, bool env_sampling, int features, Launcher &L)
{
    const bool env = c->env_texels != nullptr;
    if (integrator == FRT_INTEGRATOR_AO)
        return env ? plan_fixed<kMatsAll | kMatsEnv, FRT_INTEGRATOR_AO, 5, 6, 6>(c, flags, L)
                   : plan_fixed<kMatsAll, FRT_INTEGRATOR_AO, 5, 6, 6>(c, flags, L);
    if (integrator == FRT_INTEGRATOR_NORMALS)   // (here with an image only)
        return plan_fixed<kMatsEnv, FRT_INTEGRATOR_NORMALS, 5, 6, 6>(c, flags, L);
    if (features)   // FRT_FLAG_ROULETTE, FRT_FLAG_SOBOL
        return with_features(features, [&](auto x) -> int {
            return plan_features<decltype(x)::value>(c, flags, f64, env_sampling, L);
        });
    if (env_sampling) return plan_estimator<kMatsNee>(c, flags, f64, L);   // FRT_FLAG_ENV_SAMPLING
    // the default path render (the tunable shape): the smallest kernel covering the scene's
    // materials; with an image two sets carry the lookup -- textures alone (lambertian and
    // textured scenes) and every material.  fp64: a BVH world runs every material.
    if (f64 && (env || c->world_kind != FRT_WORLD_LIST))
        return env ? plan_f64<kMatsAll | kMatsEnv>(c, L) : plan_f64<kMatsAll>(c, L);
    if (env)
        return (c->mats & ~kMatsTex) == 0 ? pick_launcher_t<kMatsTex | kMatsEnv>(c, flags, L)
                                          : pick_launcher_t<kMatsAll | kMatsEnv>(c, flags, L);
    if (f64) {   // a list world: the scene's own set
        switch (c->mats) {
        case kMatsTex: return plan_f64<kMatsTex, false>(c, L);
        case kMatsSpec: return plan_f64<kMatsSpec, false>(c, L);   // veach_mis (C3): phong plates
        case kMatsSpec | kMatsTex: return plan_f64<kMatsSpec | kMatsTex, false>(c, L);
        default: return plan_f64<kMatsAll>(c, L);
        }
    }
    switch (c->mats) {
    case kMatsTex: return pick_launcher_t<kMatsTex>(c, flags, L);
    case kMatsSpec:
    case kMatsSpec | kMatsTex: return pick_launcher_t<kMatsSpec | kMatsTex>(c, flags, L);
    default: return pick_launcher_t<kMatsAll>(c, flags, L);
    }
}
// (an environment image always takes the material branch: one chain kernel per plan carries the lookup)
int frt_mats::mlt(const frt_ctx *c, int flags, bool env, const void **boot, const void **chains)
{
    return walk_plan(c, flags, [&](auto r, size_t) -> int {
        using R = decltype(r);
        if (env) mlt_kernels_t<R::stack, R::world, R::lds, true, true>(boot, chains);
        else mlt_kernels_t<R::stack, R::world, R::lds, true, false>(boot, chains);
        return FRT_OK;
    });
}
