// frt_denoise.hip -- the kernels of FRT_INTEGRATOR_DENOISE (frt.h): de-slot the
// colour and the three feature films into pixel-order planes, the a-trous
// iterations between two planes, re-slot.  The arithmetic is frt_denoise.hpp's;
// render_denoise (frt_render.hip) calls frt_denoise::run.
//
// Planes (the context's dn_planes, reused): guides, iterate A, iterate B, one
// float4 a pixel each, rows contiguous -- a tap is two 16-byte loads, and the
// taps of a wave's 32 x 2 pixels stay coalesced at every spacing.  An
// iteration must read 32 B and write 16 B a pixel.  At spacing 1 and 2 a block
// stages its 32 x 8 pixels plus the halo in LDS (25 taps a pixel from 1.7 /
// 2.5 staged pixels); from 4 on the halo would outgrow the tile, and L2 and
// the Infinity Cache serve the reuse.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "frt_ctx.hpp"
#include "frt_denoise.hpp"

using namespace frt;

namespace {

constexpr int kDnBx = 32, kDnBy = 8;                       // a block's pixels
constexpr int kDnLdsStep = 2;                              // largest tap spacing staged in LDS
constexpr int kDnLdsPixels = (kDnBx + 4 * kDnLdsStep) * (kDnBy + 4 * kDnLdsStep);   // 40 x 16

// slot s of the whole frame (shard 0 of 1) -> pixel index, -1 = padding
__device__ __forceinline__ int64_t slot_pixel(uint32_t s, int tile, int ntx, int nx, int ny)
{
    const int T2 = tile * tile;
    const int tile_id = (int)(s / (uint32_t)T2), sl = (int)(s % (uint32_t)T2);
    int lx, ly;
    slot_to_local(sl, tile, lx, ly);
    const int px = (tile_id % ntx) * tile + lx, py = (tile_id / ntx) * tile + ly;
    return px < nx && py < ny ? (int64_t)py * nx + px : -1;
}
__device__ __forceinline__ f3 load3(const float *p, size_t i) { return f3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

__global__ __launch_bounds__(256) void denoise_deslot(const float *__restrict__ colour, const float *__restrict__ normals,
                                                      const float *__restrict__ albedo, const float *__restrict__ depth,
                                                      uint32_t n_slots, int tile, int ntx, int nx, int ny,
                                                      float4 *__restrict__ guides, float4 *__restrict__ iterate)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const int64_t pix = slot_pixel(s, tile, ntx, nx, ny);
    if (pix < 0) return;
    const DenoisePixel P = denoise_pack(load3(colour, s), load3(normals, s), load3(albedo, s), load3(depth, s));
    guides[pix] = P.g;
    iterate[pix] = P.c;
}

__global__ __launch_bounds__(256) void denoise_reslot(const float4 *__restrict__ iterate, const float *__restrict__ albedo,
                                                      uint32_t n_slots, int tile, int ntx, int nx, int ny,
                                                      float *__restrict__ colour)
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_slots) return;
    const int64_t pix = slot_pixel(s, tile, ntx, nx, ny);
    if (pix < 0) return;                                   // padding slots stay as they are
    const f3 c = denoise_unpack(iterate[pix], load3(albedo, s));
    colour[3 * (size_t)s] = c.x; colour[3 * (size_t)s + 1] = c.y; colour[3 * (size_t)s + 2] = c.z;
}

// one iteration: block b of a 1-D grid filters pixels [32 bx, +32) x [8 by, +8).
// Every load and the store are of in-frame pixels only.
template <bool LDS>
__global__ __launch_bounds__(kDnBx * kDnBy) void denoise_filter(const float4 *__restrict__ guides,
                                                                const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                                int nx, int ny, int nbx, int step, float sigma_l)
{
    const int bx0 = (int)(blockIdx.x % (uint32_t)nbx) * kDnBx, by0 = (int)(blockIdx.x / (uint32_t)nbx) * kDnBy;
    const int x = bx0 + (int)(threadIdx.x % kDnBx), y = by0 + (int)(threadIdx.x / kDnBx);
    const bool inside = x < nx && y < ny;
    float4 out;
    if constexpr (LDS) {
        __shared__ float4 lg[kDnLdsPixels], lc[kDnLdsPixels];
        const int halo = 2 * step, w = kDnBx + 2 * halo, h = kDnBy + 2 * halo;   // step <= kDnLdsStep
        const int x0 = bx0 - halo, y0 = by0 - halo;
        for (int i = threadIdx.x; i < w * h; i += kDnBx * kDnBy) {
            const int gx = x0 + i % w, gy = y0 + i / w;
            if (gx >= 0 && gx < nx && gy >= 0 && gy < ny) {
                const size_t q = (size_t)gy * nx + gx;
                lg[i] = guides[q];
                lc[i] = src[q];
            }
        }
        __syncthreads();
        if (!inside) return;
        out = denoise_iterate(x, y, nx, ny, step, sigma_l, [&](int qx, int qy) {
            const int i = (qy - y0) * w + (qx - x0);
            return DenoisePixel{lg[i], lc[i]};
        });
    } else {
        if (!inside) return;
        out = denoise_iterate(x, y, nx, ny, step, sigma_l, [&](int qx, int qy) {
            const size_t q = (size_t)qy * nx + qx;
            return DenoisePixel{guides[q], src[q]};
        });
    }
    dst[(size_t)y * nx + x] = out;
}

}  // namespace

int frt_denoise::run(frt_ctx *c, const frt_render_params *p, float *colour_slots, const float *normals_slots,
                     const float *albedo_slots, const float *depth_slots, uint32_t n_slots, hipStream_t st, float *ms)
{
    const int T = eff_tile(p), ntx = (p->nx + T - 1) / T;
    const size_t npix = (size_t)p->nx * p->ny;
    if (const int rc = c->dn_planes.reserve(c, 3 * npix * sizeof(float4))) return rc;
    float4 *guides = c->dn_planes, *a = guides + npix, *b = a + npix;
    const int nbx = (p->nx + kDnBx - 1) / kDnBx, nby = (p->ny + kDnBy - 1) / kDnBy;
    const uint64_t blocks = (uint64_t)nbx * nby;
    if (blocks > 0x7fffffffULL) return set_err(c, FRT_E_UNSUPPORTED, "denoise: frame too large for one call");
    const dim3 slot_grid((n_slots + 255) / 256), slot_block(256);
    HIPCHK(c, hipEventRecord(c->ev0, st));
    hipLaunchKernelGGL(denoise_deslot, slot_grid, slot_block, 0, st, colour_slots, normals_slots, albedo_slots, depth_slots,
                       n_slots, T, ntx, p->nx, p->ny, guides, a);
    HIPCHK(c, hipGetLastError());
    for (int i = 0; i < kDenoiseIterations; ++i) {
        const int step = 1 << i;
        hipLaunchKernelGGL(step <= kDnLdsStep ? denoise_filter<true> : denoise_filter<false>, dim3((unsigned)blocks),
                           dim3(kDnBx * kDnBy), 0, st, guides, a, b, p->nx, p->ny, nbx, step, denoise_sigma_l(i));
        HIPCHK(c, hipGetLastError());
        std::swap(a, b);
    }
    hipLaunchKernelGGL(denoise_reslot, slot_grid, slot_block, 0, st, a, albedo_slots, n_slots, T, ntx, p->nx, p->ny,
                       colour_slots);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return FRT_OK;
}
