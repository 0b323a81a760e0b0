// prt.hpp -- the host side of precomputed radiance transfer: the real SH basis
// (5 bands, 25 coefficients, index l (l + 1) + m), the Y table of a direction list, the corner
// records of a scene view, the projection of an environment and the stratified direction
// generator.  Plain C++, fp64 throughout; what the kernels read is rounded to fp32 once, here.
// One convention, frt_set_env_image's (frt.h): for a unit direction d, theta = acos(d.y),
// phi = atan2(d.x, -d.z) (+ 2 pi when negative).  Internal to libfrt.so.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "frt.h"

#pragma GCC visibility push(hidden)
namespace frt_prt {

constexpr int kBands = 5, kCoef = kBands * kBands;
constexpr double kCornerEps = 1e-4;   // EPSILON (util.h): a corner's origin is v + EPSILON n

// Y_lm(theta, phi): K P with the Condon-Shortley phase; m > 0 takes cos(m phi), m < 0 sin(-m phi)
double sh_eval(int l, int m, double theta, double phi);
// the 25 values at (theta, phi), index l (l + 1) + m
void sh_all(double theta, double phi, double Y[kCoef]);
// (theta, phi) of a direction in the convention above (d.y clamped to [-1, 1])
void dir_angles(const float d[3], double &theta, double &phi);
// Y[n][25] of a direction list, fp64 rounded to fp32: the table the kernel and the replay read
void y_table(const float *dirs, int64_t n, float *Y);
// the first direction that is not finite or whose length is off 1 by more than 1e-3: its index
// and the refusal's text, or -1
int64_t dirs_first_bad(const float *dirs, int64_t n, std::string &why);
// what frtx_prt_transfer and its host replay refuse before they look at a scene: "" or the text
std::string transfer_request_bad(const float *dirs, int64_t n_dirs, int bounces, int flags);
// bytes of chunk sums one batch of corners may take: 256 MiB, or what frtx_selftest_prt_budget set
size_t batch_budget();
// corner records of a scene view (frt.h frtx_prt_corners); "" or the refusal's text
std::string corners(const frt_scene_view *sv, float *origin_normal, float *albedo);
// Li[k][ch] of an environment image (NULL: the constant colour); "" or the refusal's text
std::string project(const frt_image *img, const double env[3], double li[3 * kCoef]);
// sqrt_n^2 jittered strata, uniform on the sphere, jitter keyed by (seed, stratum)
void sample_dirs(int sqrt_n, uint32_t seed, float *dirs);

}  // namespace frt_prt
#pragma GCC visibility pop
