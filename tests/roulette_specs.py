"""Shared pieces of the Russian-roulette tests (FRT_FLAG_ROULETTE:
test_roulette_host.py, test_gpu_roulette.py): the checks that the host replay
and the GPU both have to pass, each written over a `render(params) -> (film,
stats)` callable so that the two files differ only in who renders.

The flag's rule (include/frt.h): a scattering vertex at depth >= 3 lets the
path go on with probability q = min(1, largest throughput component) and divides
the throughput by q.  The vertices at depth 0, 1, 2 never play, so a render
with max_depth = 2 (whose deepest scattering vertex is at depth 2) is the
render without the flag, bit for bit."""
import numpy as np

import first_raytracer_amd as frt
import golden_images as G

ON = frt.FRT_FLAG_ROULETTE
GOLDEN_SEEDS = range(300, 316)


def check_prefix(render, flags):
    """1. Untouched prefix: Cornell 48x36x8; max_depth 2 bit-identical, max_depth 33 not."""
    nx, ny, spp = 48, 36, 8
    a, sa = render(frt.RenderParams.make(nx, ny, spp, seed=11, max_depth=2, flags=flags | ON))
    b, sb = render(frt.RenderParams.make(nx, ny, spp, seed=11, max_depth=2, flags=flags))
    assert np.array_equal(a, b)
    assert (sa.samples, sa.camera_rays, sa.extension_rays, sa.shadow_rays) == \
           (sb.samples, sb.camera_rays, sb.extension_rays, sb.shadow_rays)
    c, _ = render(frt.RenderParams.make(nx, ny, spp, seed=11, max_depth=33, flags=flags | ON))
    d, _ = render(frt.RenderParams.make(nx, ny, spp, seed=11, max_depth=33, flags=flags))
    assert np.isfinite(c).all() and not np.array_equal(c, d)


def check_fewer_rays(render):
    """3. Fewer rays, same samples: Cornell 64x64x64, seed 7."""
    on, s_on = render(frt.RenderParams.make(64, 64, 64, seed=7, flags=ON))
    off, s_off = render(frt.RenderParams.make(64, 64, 64, seed=7))
    print("rays / sample: on", s_on.rays / s_on.samples, "off", s_off.rays / s_off.samples, "ratio",
          s_on.rays / s_off.rays, "(fp64 oracle patch: 5.58 / 12.00 = 0.465)")
    assert s_on.samples == s_off.samples == 64 * 64 * 64
    assert s_on.camera_rays == s_off.camera_rays
    assert s_on.extension_rays < s_off.extension_rays
    assert s_on.rays < s_off.rays
    assert s_on.shadow_rays <= s_off.shadow_rays
    assert np.isfinite(on).all()


def check_golden(render, spp, flags=0):
    """4. Same expectation as the oracle's converged image (rendered without
    roulette): 64x64 with the flag on 16 seeds; the 8x8 block means of every seed
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
