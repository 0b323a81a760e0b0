// The library's feature unit: the first-hit kernels of FRT_INTEGRATOR_ALBEDO
// and FRT_INTEGRATOR_DEPTH (albedo_shade / depth_shade, frt_path.hpp), reached
// through frt_feat::pick (frt_plans.hpp).  Nine plans each, those of normals;
// a unit of its own so that the other units' kernels compile as before.
#undef FRT_DIAG
#include "frt_kernels.hpp"
#include "frt_plans.hpp"

int frt_feat::pick(const frt_ctx *c, int integrator, int flags, Launcher &L)
{
    if (integrator == FRT_INTEGRATOR_ALBEDO) return plan_fixed<kMatsNone, FRT_INTEGRATOR_ALBEDO, 5, 6, 6>(c, flags, L);
    if (integrator == FRT_INTEGRATOR_DEPTH) return plan_fixed<kMatsNone, FRT_INTEGRATOR_DEPTH, 5, 6, 6>(c, flags, L);
    return FRT_E_INVALID;
}
