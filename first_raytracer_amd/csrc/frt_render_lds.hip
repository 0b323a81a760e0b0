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

int frt_lds::path_oct(int stack, int waves, size_t scene_bytes, Launcher &L)
{
#if defined(FRT_OCT_IN_MAIN)
    return FRT_E_UNSUPPORTED;
#else
    if (stack == 8) L = bvh_launcher<8, true, kWorldBvh2Oct, kMatsNone>(waves, scene_bytes);
    else if (stack == 16) L = bvh_launcher<16, true, kWorldBvh2Oct, kMatsNone>(waves, scene_bytes);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
#endif
}
// ... and with Russian roulette (FRT_FLAG_ROULETTE): one register cap, the default plan's 5 waves
int frt_lds::path_oct_roulette(int stack, size_t scene_bytes, Launcher &L)
{
#if defined(FRT_OCT_IN_MAIN)
    return FRT_E_UNSUPPORTED;
#else
    if (stack == 8) L = make_launcher<8, kWorldBvh2Oct, true, 5, kMatsRoulette>(scene_bytes);
    else if (stack == 16) L = make_launcher<16, kWorldBvh2Oct, true, 5, kMatsRoulette>(scene_bytes);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
#endif
}
// ... and with the Sobol' sampler (FRT_FLAG_SOBOL), with or without roulette: the same cap
template <int MATS> static int path_oct_sobol_t(int stack, size_t scene_bytes, Launcher &L)
{
    if (stack == 8) L = make_launcher<8, kWorldBvh2Oct, true, 5, MATS>(scene_bytes);
    else if (stack == 16) L = make_launcher<16, kWorldBvh2Oct, true, 5, MATS>(scene_bytes);
    else return FRT_E_UNSUPPORTED;
    return FRT_OK;
}
int frt_lds::path_oct_sobol(int stack, bool roulette, size_t scene_bytes, Launcher &L)
{
#if defined(FRT_OCT_IN_MAIN)
    return FRT_E_UNSUPPORTED;
#else
    return roulette ? path_oct_sobol_t<kMatsSobol | kMatsRoulette>(stack, scene_bytes, L)
                    : path_oct_sobol_t<kMatsSobol>(stack, scene_bytes, L);
#endif
}
