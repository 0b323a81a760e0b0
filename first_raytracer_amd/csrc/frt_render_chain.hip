// The library's fourth translation unit: the lambertian PSS-MLT chain kernels
// of the octant LDS plan (C5), reached through frt_lds::mlt_oct (frt_plans.hpp).
// Built with the machine scheduler's iterative-maxocc strategy (Makefile,
// CHAINFLAGS); see the comment at kSplitLds.
// Diagnostic and no-split builds (recorded before FRT_DIAG is dropped) keep these
// kernels in the main unit: this one then holds none.
#if defined(FRT_DIAG) || defined(FRT_EXP_NO_LDS_SPLIT)
#define FRT_OCT_IN_MAIN 1
#endif
#undef FRT_DIAG
#include "frt_kernels.hpp"
#include "frt_plans.hpp"

int frt_lds::mlt_oct(const frt_ctx *c, int flags, const void **boot, const void **chains)
{
#if defined(FRT_OCT_IN_MAIN)
    return FRT_E_UNSUPPORTED;
#else
    return walk_plan(c, flags, [&](auto r, size_t) -> int {
        using R = decltype(r);
        if constexpr (R::world == kWorldBvh2Oct) {
            mlt_kernels_t<R::stack, kWorldBvh2Oct, true, false>(boot, chains);
            return FRT_OK;
        } else {
            return FRT_E_UNSUPPORTED;
        }
    });
#endif
}
