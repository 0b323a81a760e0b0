"""Shared pieces of the Sobol' sampler tests (FRT_FLAG_SOBOL: test_sobol_host.py,
test_gpu_sobol.py): the sampler restated in numpy (DESIGN.md section 4,
csrc/frt_device.hpp sobol_key / sobol_word) and the checks that the host replay
and the GPU both have to pass, each written over a `render(params) -> (film,
stats)` callable so that the two files differ only in who renders.

The flag's rule (include/frt.h): dimension d of sample s of pixel p is component
d & 1 of a 2-D Owen-scrambled Sobol' point of pair d >> 1, the point with index
s; shuffle and scrambles are hashed from (frame seed, pixel, pair).  The
estimator and its dimension layout are untouched, so the expectation is the
same and the noise is lower."""
import numpy as np

import first_raytracer_amd as frt
import golden_images as G

ON = frt.FRT_FLAG_SOBOL if hasattr(frt, "FRT_FLAG_SOBOL") else 8192
GOLDEN_SEEDS = range(300, 316)
M32 = np.uint64(0xFFFFFFFF)
# the largest dimension a path of max_depth 33 reads: vertex 33's bsdf direction
MAX_DIM = 4 + 8 * 33 + 7


def _u64(v):
    return np.asarray(v, np.uint64)


def mix32(x):
    x = _u64(x).copy()
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def bitrev(x):
    x = _u64(x)
    x = ((x >> np.uint64(16)) | (x << np.uint64(16))) & M32
    x = ((x & np.uint64(0x00FF00FF)) << np.uint64(8)) | ((x >> np.uint64(8)) & np.uint64(0x00FF00FF))
    x = ((x & np.uint64(0x0F0F0F0F)) << np.uint64(4)) | ((x >> np.uint64(4)) & np.uint64(0x0F0F0F0F))
    x = ((x & np.uint64(0x33333333)) << np.uint64(2)) | ((x >> np.uint64(2)) & np.uint64(0x33333333))
    return ((x & np.uint64(0x55555555)) << np.uint64(1)) | ((x >> np.uint64(1)) & np.uint64(0x55555555))


def lk(x, seed):
    """The Laine-Karras permutation."""
    x = (_u64(x) + _u64(seed)) & M32
    for c in (0x6C50B47C, 0xB82F1E52, 0xC7AFE638, 0x8D22F6E6):
        x = x ^ ((x * np.uint64(c)) & M32)
    return x


def owen(x, seed):
    return bitrev(lk(bitrev(x), seed))


def sobol1_loop(i):
    """The second Sobol' dimension by its generator columns: v0 = 1 << 31, v(b+1) = v(b) ^ (v(b) >> 1)."""
    i = _u64(i)
    x = np.zeros_like(i)
    v = np.uint64(1 << 31)
    for b in range(32):
        x = np.where((i >> np.uint64(b)) & np.uint64(1), x ^ v, x)
        v = v ^ (v >> np.uint64(1))
    return x


def sobol1(i):
    """... without the loop: bitrev, then five butterfly stages."""
    x = bitrev(i)
    for k, m in enumerate((0xAAAAAAAA, 0xCCCCCCCC, 0xF0F0F0F0, 0xFF00FF00, 0xFFFF0000)):
        x = x ^ (((x << np.uint64(1 << k)) & M32) & np.uint64(m))
    return x


def pixel_key(seed, pixel):
    return mix32((mix32(_u64(seed) ^ np.uint64(0x2545F491)) + _u64(pixel) * np.uint64(0x9E3779B9)) & M32)


def pair_seeds(seed, pixel, j):
    """(shuffle, x, y) seeds of pair j."""
    h = mix32(pixel_key(seed, pixel) ^ ((_u64(j) * np.uint64(0x85EBCA77) + np.uint64(0xC2B2AE3D)) & M32))
    return h, mix32(h ^ np.uint64(0x9E3779B9)), mix32(h ^ np.uint64(0x7F4A7C15))


def word(seed, pixel, sample, dim):
    """The sampler's 32-bit word of (frame seed, pixel, global sample index, dimension); broadcasts."""
    dim = _u64(dim)
    sh, sx, sy = pair_seeds(seed, pixel, dim >> np.uint64(1))
    idx = owen(sample, sh)
    return np.where(dim & np.uint64(1), owen(sobol1(idx), sy), bitrev(lk(idx, sx)))


def uniform(seed, pixel, sample, dim):
    return (word(seed, pixel, sample, dim) >> np.uint64(8)).astype(np.float64) * 2.0 ** -24


def pair_points(seed, pixel, j, samples):
    """The 2-D points of pair j as 32-bit integer coordinates, shape (len(samples), 2)."""
    s = _u64(samples)
    return np.stack([word(seed, pixel, s, 2 * j), word(seed, pixel, s, 2 * j + 1)], axis=-1)


def is_net(points, m):
    """2^m points (32-bit integer coordinates) with exactly one in every elementary interval
    2^-a x 2^-(m-a), a = 0..m."""
    assert len(points) == 1 << m
    for a in range(m + 1):
        cx = (points[:, 0] >> np.uint64(32 - a)) if a else np.zeros(len(points), np.uint64)
        cy = (points[:, 1] >> np.uint64(32 - (m - a))) if m - a else np.zeros(len(points), np.uint64)
        cell = (cx << np.uint64(m - a)) | cy
        if not np.array_equal(np.sort(cell), np.arange(1 << m, dtype=np.uint64)):
            return False
    return True


def corr(a, b):
    a = a - a.mean()
    b = b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


# ---- checks over render(params) -> (film, stats) ----
def check_has_effect(render, flags=0):
    """Cornell 48x36x8, seed 11: the film with the flag is finite and differs from the one
    without it; the same samples and camera rays."""
    a, sa = render(frt.RenderParams.make(48, 36, 8, seed=11, flags=flags | ON))
    b, sb = render(frt.RenderParams.make(48, 36, 8, seed=11, flags=flags))
    assert np.isfinite(a).all() and not np.array_equal(a, b)
    assert sa.samples == sb.samples == 48 * 36 * 8 and sa.camera_rays == sb.camera_rays


def check_roulette_prefix(render, flags=0):
    """With max_depth = 2 no vertex plays roulette: SOBOL | ROULETTE is SOBOL, bit for bit."""
    rl = frt.FRT_FLAG_ROULETTE
    a, sa = render(frt.RenderParams.make(48, 36, 8, seed=11, max_depth=2, flags=flags | ON | rl))
    b, sb = render(frt.RenderParams.make(48, 36, 8, seed=11, max_depth=2, flags=flags | ON))
    assert np.array_equal(a, b)
    assert (sa.samples, sa.camera_rays, sa.extension_rays, sa.shadow_rays) == \
           (sb.samples, sb.camera_rays, sb.extension_rays, sb.shadow_rays)
    c, sc = render(frt.RenderParams.make(48, 36, 8, seed=11, max_depth=33, flags=flags | ON | rl))
    d, sd = render(frt.RenderParams.make(48, 36, 8, seed=11, max_depth=33, flags=flags | ON))
    assert np.isfinite(c).all() and not np.array_equal(c, d) and sc.rays < sd.rays


def check_golden(render, spp, flags=0):
    """roulette_specs.check_golden's statistic with this flag (flags: what else the call sets):
    64x64 on 16 frame seeds, which scramble independently; the 8x8 block means of every seed
    give a mean and a standard error per block and channel (192 values)."""
    g = G.cornell64()
    films = [np.asarray(render(frt.RenderParams.make(64, 64, spp, seed=s, flags=flags | ON))[0], np.float64)
             .reshape(64, 64, 3) for s in GOLDEN_SEEDS]
    b = np.array([G.blocks(f, 8) for f in films])                 # (16, 8, 8, 3)
    mean, se = b.mean(axis=0), b.std(axis=0, ddof=1) / np.sqrt(len(films))
    z = np.abs(mean - G.blocks(g, 8)) / se
    rel = np.abs(np.mean(films, axis=(0, 1, 2)) - g.mean((0, 1))) / g.mean((0, 1))
    print("z: max", z.max(), "count > 4:", int((z > 4).sum()), "image-mean relative difference", rel)
    assert z.size == 192
    assert (z > 4).sum() <= 2 and not (z > 6).any()
    assert (rel < 0.005).all()


def seed_variance(render, spp, max_depth, flags):
    """Per-pixel variance over the 16 frame seeds of Cornell 64x64, averaged over pixels and channels."""
    films = np.array([np.asarray(render(frt.RenderParams.make(64, 64, spp, seed=s, max_depth=max_depth, flags=flags))[0],
                                 np.float64).reshape(-1, 3) for s in GOLDEN_SEEDS])
    return float(films.var(axis=0, ddof=1).mean())


def check_less_noise(render, spp, max_depth, flags=0):
    """The variance with the flag is below that of the same call without it; returns on / off."""
    on, off = seed_variance(render, spp, max_depth, flags | ON), seed_variance(render, spp, max_depth, flags)
    print(f"max_depth {max_depth} spp {spp}: variance on {on:.6e} off {off:.6e} ratio on / off {on / off:.4f}")
    assert on < off
    return on / off


def check_progressive(render, spp, flags=0):
    """Two passes of spp / 2 (sample_offset 0 and spp / 2) accumulated equal one call of spp, up to
    fp32 summation order (the tolerance of test_gpu_parity.test_progressive_passes)."""
    h = spp // 2
    full, st = render(frt.RenderParams.make(64, 64, spp, seed=9, flags=flags | ON))
    p1, s1 = render(frt.RenderParams.make(64, 64, h, seed=9, flags=flags | ON))
    p2, s2 = render(frt.RenderParams.make(64, 64, h, seed=9, flags=flags | ON, sample_offset=h))
    acc = frt.film_accumulate(np.asarray(p1, np.float32), h, np.asarray(p2, np.float32), h)
    assert s1.rays + s2.rays == st.rays
    assert np.allclose(acc, full, rtol=1e-5, atol=1e-7)
