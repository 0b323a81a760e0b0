// The library's third translation unit: the lambertian path kernels of the
// octant LDS plan (C2), reached through frt_lds::path_oct (frt_plans.hpp).
// Built with the machine scheduler's max-memory-clause strategy (Makefile,
// LDSFLAGS); see the comment at kSplitLds.
// Diagnostic and no-split builds (recorded before FRT_DIAG is dropped) keep these
// kernels in the main unit: this one then holds none.
#if defined(FRT_DIAG) || defined(FRT_EXP_NO_LDS_SPLIT)
#define FRT_OCT_IN_MAIN 1
#endif
#undef FRT_DIAG
#include "frt_kernels.hpp"
#include "frt_plans.hpp"

// L = f(rung, scene bytes) on the octant rungs of the walk
template <typename F>
static int oct_rung(const frt_ctx *c, int flags, Launcher &L, F &&f)
{
#if defined(FRT_OCT_IN_MAIN)
    return FRT_E_UNSUPPORTED;
#else
    return walk_plan(c, flags, [&](auto r, size_t scene_bytes) -> int {
        if constexpr (decltype(r)::world == kWorldBvh2Oct) {
            L = f(r, scene_bytes);
            return FRT_OK;
        } else {
            return FRT_E_UNSUPPORTED;
        }
    });
#endif
}
int frt_lds::path_oct(const frt_ctx *c, int flags, int waves, Launcher &L)
{
    return oct_rung(c, flags, L, [&](auto r, size_t scene_bytes) {
        return bvh_launcher<decltype(r)::stack, true, kWorldBvh2Oct, kMatsNone>(waves, scene_bytes);
    });
}
// ... with Russian roulette (FRT_FLAG_ROULETTE), the Sobol' sampler (FRT_FLAG_SOBOL) or both: one
// register cap, the default plan's 5 waves
int frt_lds::path_oct_features(const frt_ctx *c, int flags, int features, Launcher &L)
{
    return with_features(features, [&](auto x) -> int {
        return oct_rung(c, flags, L, [&](auto r, size_t scene_bytes) {
            return make_launcher<decltype(r)::stack, kWorldBvh2Oct, true, 5, decltype(x)::value>(scene_bytes);
        });
    });
}
