// frt_error.hip -- the kernel of FRT_INTEGRATOR_ERROR (frt.h) and its host hook.
// The arithmetic is frt_error.hpp's; render_impl (frt_render.hip) calls
// frt_error::run on the chunk sums the context's last render left in `partial`.
//
// `partial` holds, per chunk, one row of 3 n_slots floats (slot s of chunk c at
// 3 (c n_slots + s)), and the estimate is per channel: every float column of the
// rows is an element of its own.  A lane owns 4 consecutive columns and reads
// them with one 16-byte load a chunk, so a wave reads 1 KiB of a row per
// instruction, every byte of `partial` once; n_slots is a multiple of 64 (tiles
// are multiples of 8 wide), so every row starts 16-byte aligned.  A lane's 4
// columns belong to at most 2 slots.  Padding slots of edge tiles are never
// written by the megakernel: a lane with one of its two slots padding reads
// the valid slot's columns one float at a time, a lane with both padding reads
// nothing, and both write 0 there.
#include <hip/hip_runtime.h>

#include "frt_ctx.hpp"
#include "frt_error.hpp"

using namespace frt;

namespace {

constexpr int kErrBlock = 256;

// film_reduce's mapping: is slot s of this shard a pixel of the frame?
__device__ __forceinline__ bool slot_valid(uint32_t s, int tile, int ntx, int shard_index, int shard_count, int nx, int ny)
{
    const int T2 = tile * tile;
    const int t_ord = (int)(s / (uint32_t)T2), sl = (int)(s % (uint32_t)T2);
    const int tile_id = shard_index + t_ord * shard_count;
    int lx, ly;
    slot_to_local(sl, tile, lx, ly);
    const int px = (tile_id % ntx) * tile + lx, py = (tile_id / ntx) * tile + ly;
    return px < nx && py < ny;
}

__global__ __launch_bounds__(kErrBlock) void film_error(const float *__restrict__ partial, float *__restrict__ out,
                                                        uint32_t n_slots, int n_chunks, int spp, int spi, int tile, int ntx,
                                                        int shard_index, int shard_count, int nx, int ny, int out_vec)
{
    const uint64_t row = 3ull * n_slots;                 // floats a chunk
    const uint64_t j0 = 4ull * ((uint64_t)blockIdx.x * kErrBlock + threadIdx.x);
    if (j0 >= row) return;                               // row is a multiple of 4
    const uint32_t sa = (uint32_t)(j0 / 3), sb = (uint32_t)((j0 + 3) / 3);   // sb <= n_slots - 1
    const bool va = slot_valid(sa, tile, ntx, shard_index, shard_count, nx, ny);
    const bool vb = sb == sa ? va : slot_valid(sb, tile, ntx, shard_index, shard_count, nx, ny);
    float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (va && vb) {
        ChunkVar a[4];
        const float *q = partial + j0;
#pragma unroll 4
        for (int c = 0; c < n_chunks; ++c) {
            const float4 x = *reinterpret_cast<const float4 *>(q + (uint64_t)c * row);
            const float n = chunk_samples(c, n_chunks, spp, spi), r = chunk_ratio(c, n_chunks, spp, spi);
            chunk_var_add(a[0], x.x, n, r); chunk_var_add(a[1], x.y, n, r);
            chunk_var_add(a[2], x.z, n, r); chunk_var_add(a[3], x.w, n, r);
        }
        for (int k = 0; k < 4; ++k) v[k] = chunk_var_result(a[k], n_chunks, spp);
    } else if (va || vb) {
        for (int k = 0; k < 4; ++k) {
            const bool first = (uint32_t)((j0 + k) / 3) == sa;
            if (first ? !va : !vb) continue;
            ChunkVar a;
            for (int c = 0; c < n_chunks; ++c)
                chunk_var_add(a, partial[(uint64_t)c * row + j0 + k], chunk_samples(c, n_chunks, spp, spi),
                              chunk_ratio(c, n_chunks, spp, spi));
            v[k] = chunk_var_result(a, n_chunks, spp);
        }
    }
    if (out_vec) {
        *reinterpret_cast<float4 *>(out + j0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        out[j0] = v[0]; out[j0 + 1] = v[1]; out[j0 + 2] = v[2]; out[j0 + 3] = v[3];
    }
}

}  // namespace

int frt_error::run(frt_ctx *c, const frt_render_params *p, float *out_slots, uint32_t n_slots, int n_chunks, int spi,
                   hipStream_t st, float *ms)
{
    const int T = eff_tile(p), ntx = (p->nx + T - 1) / T;
    *ms = 0.0f;
    if (n_slots == 0) return FRT_OK;
    if ((n_slots & 3u) != 0 || n_chunks < 2 || (size_t)n_chunks * n_slots * 3 * sizeof(float) > c->partial.bytes)
        return set_err(c, FRT_E_INVALID, "error film: the recorded chunk sums do not fit the context's buffer");
    const uint64_t n_vec = 3ull * n_slots / 4;
    const int out_vec = (reinterpret_cast<uintptr_t>(out_slots) & 15u) == 0 ? 1 : 0;
    HIPCHK(c, hipEventRecord(c->ev0, st));
    hipLaunchKernelGGL(film_error, dim3((unsigned)((n_vec + kErrBlock - 1) / kErrBlock)), dim3(kErrBlock), 0, st, c->partial,
                       out_slots, n_slots, n_chunks, p->spp, spi, T, ntx, p->shard_index, p->shard_count, p->nx, p->ny,
                       out_vec);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, st));
    HIPCHK(c, hipStreamSynchronize(st));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return FRT_OK;
}

// Host hook (CPU-only unit tests): frt_error.hpp's arithmetic over chunk sums in host memory,
// in the device layout (chunk c, slot s at 3 (c n_slots + s)), every slot valid; out = 3 n_slots floats.
extern "C" int frtx_selftest_chunk_variance(const float *partial, int n_chunks, int64_t n_slots, int spp, int spi,
                                            float *out)
{
    if (!partial || !out || n_chunks < 2 || n_slots < 0 || spi < 1 || spp < 1) return FRT_E_INVALID;
    if ((int64_t)(n_chunks - 1) * spi >= spp || (int64_t)n_chunks * spi < spp) return FRT_E_INVALID;   // the last chunk: 1 .. spi samples
    const int64_t row = 3 * n_slots;
    for (int64_t j = 0; j < row; ++j) {
        ChunkVar a;
        for (int c = 0; c < n_chunks; ++c)
            chunk_var_add(a, partial[(int64_t)c * row + j], chunk_samples(c, n_chunks, spp, spi), chunk_ratio(c, n_chunks, spp, spi));
        out[j] = chunk_var_result(a, n_chunks, spp);
    }
    return FRT_OK;
}
