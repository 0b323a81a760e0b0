// frt_denoise.hpp -- the arithmetic of FRT_INTEGRATOR_DENOISE (frt.h): an
// edge-avoiding a-trous wavelet filter (Dammertz, Sewtz, Hanika, Lensch 2010)
// over albedo-demodulated colour, guided by the first-hit normals, albedo and
// depth films.  One function gives one pixel of one iteration; the kernels
// (frt_denoise.hip) and the host probe (tests/denoise_probe.hip) compile the
// same code.  DESIGN.md "Denoiser" states the weights; tests/denoise_specs.py
// restates them in fp64 and reads the constants below by parsing this file.
#pragma once
#include "frt_device.hpp"

namespace frt {

// The filter's constants.  The structure (frt.h) is fixed; these five
// numbers were tuned on the CPU with tests/test_denoise_host.py's harness: host
// path films of Cornell 64 x 64 at 4 spp, seeds 300..303, 16-spp host feature
// films, per-pixel RMSE against golden/cornell_64x64_16384spp.pfm, mean over the
// seeds (tools/denoise_tune.py; the whole table: profiles/denoise/tuning_cpu.txt).
// Unfiltered 0.15487; the values below 0.10480 (every seed lower than unfiltered,
// the worst by a factor 0.857); the starting values (5, 1e-3, 64, 0.1, 4) 0.56805.
// One constant varied at a time around the values below:
//   I        2: 0.10925   3: 0.10480   4: 0.10871   5: 0.10880
//   sigma_z  0.003: 0.11014   0.005: 0.10480   0.007: 0.11269   0.02: 0.21838   0.1: 0.51507
//   sigma_l0 1: 0.12446   2: 0.10776   4: 0.10480   8: 0.10882   16: 0.11286
//   sigma_n  16 .. 128 and eps_a 1e-4 .. 1e-2: 0.10480 .. 0.10481 (Cornell's walls are flat
//            and no albedo is near 0)
// What decides sigma_z: Cornell's light is seen directly (radiance 17 against 0.3 around
// it) in the ceiling's plane with the ceiling's normal, and its albedo film is 1, so only
// its 1 cm step in depth and w_l keep it out of the ceiling; a wider sigma_z smears it
// (the RMSE of 0.1 and above).  The price is less smoothing along surfaces seen at a
// grazing angle.  sigma_n stays a power of two (denoise_pow_sigma_n).
constexpr int kDenoiseIterations = 3;        // I: steps 1, 2, 4
constexpr float kDenoiseEpsAlbedo = 1e-3f;   // eps_a: floor of the albedo the colour is divided by
constexpr float kDenoiseSigmaN = 64.0f;      // sigma_n: exponent of the normals' cosine
constexpr float kDenoiseSigmaZ = 0.005f;     // sigma_z: relative depth difference
constexpr float kDenoiseSigmaL0 = 4.0f;      // sigma_l0: relative luminance difference, halved every iteration

// the 5 x 5 B3-spline taps, per axis, offsets -2 .. 2
FRT_HD float denoise_tap(int d)
{
    const int a = d < 0 ? -d : d;
    return a == 0 ? 0.375f : a == 1 ? 0.25f : 0.0625f;
}

// A pixel as the filter reads it: two 16-byte records.
//   g = (unit normal, z): z = D.x / k the mean hit distance (0 when k = 0); the
//       normal is (0, 0, 0) where it cannot guide -- k < 1 (the normals film of a
//       partly covered pixel holds environment radiance) or |N| = 0
//   c = (colour / max(A, eps_a), k): the current iterate and the coverage k = D.z
struct DenoisePixel { float4 g, c; };

FRT_HD float denoise_floor(float a) { return a > kDenoiseEpsAlbedo ? a : kDenoiseEpsAlbedo; }

// step 1: demodulate and pack the guides (N, A, D: the pixel's feature films)
FRT_HD DenoisePixel denoise_pack(f3 colour, f3 N, f3 A, f3 D)
{
    const float k = D.z;
    const float z = k > 0.0f ? D.x / k : 0.0f;
    const float n2 = N.x * N.x + N.y * N.y + N.z * N.z;
    f3 n = f3{0.0f, 0.0f, 0.0f};
    if (k >= 1.0f && n2 > 0.0f) {
        const float inv = 1.0f / sqrtf(n2);
        n = f3{N.x * inv, N.y * inv, N.z * inv};
    }
    DenoisePixel P;
    P.g = make_float4(n.x, n.y, n.z, z);
    P.c = make_float4(colour.x / denoise_floor(A.x), colour.y / denoise_floor(A.y), colour.z / denoise_floor(A.z), k);
    return P;
}

// step 4: multiply the albedo back
FRT_HD f3 denoise_unpack(float4 c, f3 A)
{
    return f3{c.x * denoise_floor(A.x), c.y * denoise_floor(A.y), c.z * denoise_floor(A.z)};
}

FRT_HD float denoise_luminance(float4 c) { return 0.2126f * c.x + 0.7152f * c.y + 0.0722f * c.z; }   // Rec. 709

// sigma_l of iteration i: sigma_l0 2^-i (the Dammertz schedule, relative form)
FRT_HD float denoise_sigma_l(int i) { return kDenoiseSigmaL0 / (float)(1 << i); }

// |a - b| / (sigma max(a, b) + 1e-20): the exponent of the relative-difference weights w_z and w_l
FRT_HD float denoise_rel_diff(float a, float b, float sigma)
{
    return fabsf(a - b) / (sigma * fmaxf(a, b) + 1e-20f);
}

// c^sigma_n for c in [0, 1].  sigma_n is kept a power of two, so this is log2(sigma_n)
// squarings -- the same bits on the host and the device, and no powf in the tap loop.
FRT_HD float denoise_pow_sigma_n(float c)
{
    constexpr int kN = (int)kDenoiseSigmaN;
    static_assert((float)kN == kDenoiseSigmaN && kN >= 1 && (kN & (kN - 1)) == 0, "sigma_n: a power of two");
    for (int m = kN; m > 1; m >>= 1) c *= c;
    return c;
}

// steps 2 and 3: the new iterate of pixel (x, y) from the iterate `fetch` reads,
// at tap spacing `step` with luminance sigma `sigma_l`.  fetch(qx, qy) returns
// the DenoisePixel of an in-frame pixel; taps outside the frame are skipped.
// Sums in fp32, dy outer and dx inner; the centre tap has weight 9/64 > 0.
template <typename Fetch>
FRT_HD float4 denoise_iterate(int x, int y, int nx, int ny, int step, float sigma_l, Fetch fetch)
{
    const DenoisePixel p = fetch(x, y);
    const float zp = p.g.w, kp = p.c.w, lp = denoise_luminance(p.c);
    const bool guide_p = p.g.x != 0.0f || p.g.y != 0.0f || p.g.z != 0.0f;
    float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + dy * step;
        if (qy < 0 || qy >= ny) continue;
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * step;
            if (qx < 0 || qx >= nx) continue;
            const DenoisePixel q = fetch(qx, qy);
            const bool guide_q = q.g.x != 0.0f || q.g.y != 0.0f || q.g.z != 0.0f;
            float w_n = 1.0f;
            if (guide_p && guide_q)
                w_n = denoise_pow_sigma_n(fmaxf(0.0f, p.g.x * q.g.x + p.g.y * q.g.y + p.g.z * q.g.z));
            const float w_k = 1.0f - fabsf(kp - q.c.w);
            // w_z w_l: one exponential of the two exponents' sum
            const float w_zl = expf(-(denoise_rel_diff(zp, q.g.w, kDenoiseSigmaZ) +
                                      denoise_rel_diff(lp, denoise_luminance(q.c), sigma_l)));
            const float w = denoise_tap(dx) * denoise_tap(dy) * w_n * w_k * w_zl;
            sw += w;
            sr += w * q.c.x; sg += w * q.c.y; sb += w * q.c.z;
        }
    }
    return make_float4(sr / sw, sg / sw, sb / sw, kp);
}

}  // namespace frt
