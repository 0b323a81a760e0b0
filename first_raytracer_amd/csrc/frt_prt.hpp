// frt_prt.hpp -- the arithmetic of precomputed radiance transfer, __host__
// __device__ so that the transfer and shade kernels (frt_prt.hip) and their host replays
// (frt_selftest.hip) run the same code: a term's cosine, the accumulate step, the gather of the
// previous bounce at a hit, the final scale and the shade dot product.  Every fused multiply-add
// is written out, so no result depends on what a compiler contracts.
//
// The sum of a corner (part of the contract, frt.h): directions are cut into chunks of kPrtChunk;
// within a chunk the terms are added in ascending j into fp32 accumulators, the chunk partials in
// ascending chunk order, and the albedo and 4 / n_dirs are applied last (prt_final).
#pragma once
#include "frt_path.hpp"

namespace frt {

constexpr int kPrtCoef = 25;           // 5 bands, index l (l + 1) + m
constexpr int kPrtChunk = 64;          // directions of one chunk
constexpr int kPrtT = 3 * kPrtCoef;    // floats of one corner's transfer: [k][channel]
constexpr float kPrtTmax = 3.402823466e+38f;   // FLT_MAX: a visibility ray has no far end

// cos of direction d at a corner with normal n
FRT_HD float prt_cos(f3 n, f3 d) { return vfma(n.z, d.z, vfma(n.y, d.y, n.x * d.x)); }

// bounce 0: an unoccluded direction adds cos Y_k
FRT_HD void prt_add(float acc[kPrtCoef], float c, const float *Y)
{
#pragma unroll
    for (int k = 0; k < kPrtCoef; ++k) acc[k] = vfma(c, Y[k], acc[k]);
}

// the barycentric mix of three corner values at (u, v): (1 - u - v) a + u b + v c
FRT_HD float prt_mix(float u, float v, float a, float b, float c) { return vfma(v, c, vfma(u, b, ((1.0f - u) - v) * a)); }

// bounce b >= 1: a ray that hit the front of triangle q at (u, v) adds cos times the previous
// bounce's transfer there; Tq = that triangle's three corners, kPrtT floats each
FRT_HD void prt_gather(float acc[kPrtT], float c, float u, float v, const float *Tq)
{
#pragma unroll
    for (int i = 0; i < kPrtT; ++i) acc[i] = vfma(c, prt_mix(u, v, Tq[i], Tq[kPrtT + i], Tq[2 * kPrtT + i]), acc[i]);
}

// The barycentrics (u, v) of the point where the ray (o, d) meets the plane of device triangle `tri`,
// in exactly rounded steps (written-out fused multiply-adds, IEEE division).  The traversal's own
// (u, v) go through the device's approximate reciprocal, an ulp away from the host's; a gather and
// the shade take these instead, so that a transfer and an image are the same bits on both.
FRT_HD f3 prt_cross(f3 a, f3 b)
{
    return mk3(vfma(a.y, b.z, -(a.z * b.y)), vfma(a.z, b.x, -(a.x * b.z)), vfma(a.x, b.y, -(a.y * b.x)));
}
FRT_HD void prt_bary(const DevScene &S, int tri, f3 o, f3 d, float &u, float &v)
{
    const f3 v0 = tri_vec<float>(S, tri, 0), e1 = tri_vec<float>(S, tri, 1), e2 = tri_vec<float>(S, tri, 2);
    const f3 h = prt_cross(d, e2), s = mk3(o.x - v0.x, o.y - v0.y, o.z - v0.z);
    const float a = prt_cos(e1, h);
    u = prt_cos(s, h) / a;
    v = prt_cos(d, prt_cross(s, e1)) / a;
}

// the side test of a gather: the hit triangle's shading normal faces the ray's origin
FRT_HD bool prt_front(const DevScene &S, int prim, f3 o, f3 d, float u, float v)
{
    f3 n;
    int mat;
    prim_shade(S, prim, o, o, u, v, n, mat);
    return prt_cos(n, -d) > 0.0f;
}

// what a finished sum becomes: albedo and scale = 4 / n_dirs (fp32, taken on the host) last
FRT_HD float prt_final(float rho, float scale, float sum) { return (rho * scale) * sum; }

// the chunk partials of one accumulator, `stride` floats apart, added in ascending chunk order
FRT_HD float prt_chunk_sum(const float *p, int n_chunks, size_t stride)
{
    float s = 0.0f;
    for (int c = 0; c < n_chunks; ++c) s += p[(size_t)c * stride];
    return s;
}

// corners of one batch: what `budget` bytes of chunk partials hold (nacc accumulators a corner and
// chunk), in whole blocks of 64, one block at the least.  The result never depends on it.
inline size_t prt_batch_corners(size_t budget, int n_chunks, int nacc, size_t n_corners)
{
    const size_t per = (size_t)n_chunks * (size_t)nacc * sizeof(float);
    const size_t blocks = budget / per / 64;
    const size_t nb = (blocks > 0 ? blocks : 1) * 64, all = (n_corners + 63) / 64 * 64;
    return nb < all ? nb : all;
}

// Shading a ray (frt.h frtx_prt_rays): (ro, rd) the ray, hit its closest-hit record (t, u, v, the
// scene view's prim as int bits), inv the device triangle of a scene-view triangle, T the
// transfer [n_tris][3][25][3], li [25][3].
FRT_HD f3 prt_shade(const DevScene &S, const int *inv, const float *T, const float *li, f3 ro, f3 rd, float4 hit)
{
    const int ref = f2i(hit.w);
    if (ref < 0) return S.env_nx > 0 ? env_eval<float>(S, rd) : S.env;   // the environment, as every integrator looks it up
    if (ref & FRT_PRIM_SPHERE) return mk3(0.0f, 0.0f, 0.0f);
    const int tri = inv[ref];
    const int mat = f2i(shade_part(S, tri, 1).x);
    const float4 m0 = S.mats[kMatStride * mat];
    const int type = f2i(m0.w);
    if (type == FRT_MAT_DIFFUSE_LIGHT) return xyz(S.mats[kMatStride * mat + 1]);   // shown, but no PRT light
    if (type != FRT_MAT_LAMBERTIAN) return mk3(0.0f, 0.0f, 0.0f);
    const float *Tq = T + (size_t)ref * (3 * kPrtT);
    float u, v;
    prt_bary(S, tri, ro, rd, u, v);
    float rgb[3] = {0.0f, 0.0f, 0.0f};
    for (int k = 0; k < kPrtCoef; ++k)
        for (int ch = 0; ch < 3; ++ch) {
            const int i = 3 * k + ch;
            rgb[ch] = vfma(li[i], prt_mix(u, v, Tq[i], Tq[kPrtT + i], Tq[2 * kPrtT + i]), rgb[ch]);
        }
    return mk3(rgb[0], rgb[1], rgb[2]);
}

}  // namespace frt
