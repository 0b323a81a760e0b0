// frt_rays.hpp -- what frtx_radiance_rays / frtx_camera_rays_device (frt_render_sparse.hip) and
// their host replays (frt_selftest.hip) share: the input domain of a ray list, checked on the
// host before anything runs, and the text of a refusal that has no context to stand in.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "frt.h"

#pragma GCC visibility push(hidden)
namespace frt {

// The text of the last refusal of a frtx_*_rays entry point or hook that was called without a
// context (the self-test hooks have none): frt_last_error(NULL) returns it.  Per thread.
std::string &null_ctx_err();

// frt_trace_device's domain for the first segment: finite origin and direction, a direction that
// is not zero, a finite t_max > 0, |origin| < 1e8.  Word 7 (the stream id) is bits, never a float.
// Returns the index of the first bad entry and says why, or -1.
inline int64_t rays_first_bad(const float *rays, int64_t n, std::string &why)
{
    for (int64_t i = 0; i < n; ++i) {
        float q[7];
        memcpy(q, rays + 8 * i, sizeof(q));
        bool finite = true;
        for (int k = 0; k < 7; ++k)
            if (k != 3 && !std::isfinite(q[k])) finite = false;
        const char *bad = nullptr;
        if (!finite) bad = "has an origin or a direction that is not finite";
        else if (q[4] == 0.0f && q[5] == 0.0f && q[6] == 0.0f) bad = "has a zero direction";
        else if (!(std::isfinite(q[3]) && q[3] > 0.0f)) bad = "has a t_max that is not finite and > 0";
        else if (!(std::sqrt((double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2]) < 1e8))
            bad = "has an origin with |origin| >= 1e8";
        if (bad) {
            why = "entry " + std::to_string(i) + " " + bad;
            return i;
        }
    }
    return -1;
}

}  // namespace frt
#pragma GCC visibility pop
