"""FRT_INTEGRATOR_ERROR on the CPU: the accepted parameters, the arithmetic of
csrc/frt_error.hpp through the host hook frtx_selftest_chunk_variance against the
formula in float64, the refusal of the host replay, and the combination rules
of render_until as pure functions.  (tests/test_gpu_error.py runs the kernel.)

The estimate (include/frt.h): K chunks, chunk c with n_c samples and sum S_c,
N = sum n_c, m_c = S_c / n_c, m = sum S_c / N,
    V = sum_c n_c (m_c - m)^2 / ((K - 1) N)."""
import numpy as np
import pytest

import first_raytracer_amd as frt
from test_abi_symbols import HERE, exported

ERROR = 8
EPS = 2.0 ** -24


def chunk_sizes(k, spp, spi):
    n = np.full(k, spi, np.float64)
    n[-1] = spp - (k - 1) * spi
    assert 1 <= n[-1] <= spi
    return n


def variance64(partial, spp, spi):
    """(V, m) in float64 from chunk sums (K, ..., 3) as the formula states them."""
    s = np.asarray(partial, np.float64)
    k = s.shape[0]
    n = chunk_sizes(k, spp, spi).reshape((k,) + (1,) * (s.ndim - 1))
    big_n = n.sum()
    m = s.sum(axis=0) / big_n
    v = (n * (s / n - m) ** 2).sum(axis=0) / ((k - 1) * big_n)
    return v, m


def bound(v64, m):
    """|V - V64| <= 1e-5 V64 + 8 eps |m| sqrt(V64) + 64 eps^2 m^2, eps = 2^-24: a relative term for
    the K fp32 updates, the rounding of each chunk mean (eps |m|) seen through the derivative of
    V (about sqrt(V)), and the floor that rounding leaves where the true spread is below it."""
    return 1e-5 * v64 + 8 * EPS * np.abs(m) * np.sqrt(v64) + 64 * EPS ** 2 * m ** 2


# ---- 1. accepted parameters ----
def test_error_takes_the_geometry_of_path():
    a = frt.shard_slots(frt.RenderParams.make(40, 24, 8, integrator=ERROR))
    b = frt.shard_slots(frt.RenderParams.make(40, 24, 8, integrator=frt.FRT_INTEGRATOR_PATH))
    assert frt.FRT_INTEGRATOR_ERROR == ERROR and np.array_equal(a, b) and (a < 0).any()
    a = frt.shard_slots(frt.RenderParams.make(40, 24, 8, integrator=ERROR, shard_index=1, shard_count=2))
    b = frt.shard_slots(frt.RenderParams.make(40, 24, 8, shard_index=1, shard_count=2))
    assert np.array_equal(a, b)
    for bad in (7, 9):
        with pytest.raises(frt.FrtError):
            frt.shard_slots(frt.RenderParams.make(40, 24, 8, integrator=bad))


def test_abi_is_unchanged():
    import os
    assert frt.lib().frt_get_abi_version() == 9 == frt.ABI_VERSION
    with open(os.path.join(HERE, "abi_symbols.txt")) as f:
        want = f.read().split()
    got = exported(os.path.join(os.path.dirname(os.path.abspath(frt.__file__)), "libfrt.so"))
    assert got == want and len(got) == 41
    assert "frtx_selftest_chunk_variance" in frt.EXPORTS_X


# ---- 2. the arithmetic ----
MAGNITUDES = (1e-3, 1.0, 1e3)
SPREADS = (1e-8, 1e-6, 1e-4, 1e-2, 1.0, 10.0)


def synthetic(k, spp, spi, seed, per_case=32):
    """(K, n_slots, 3) float32 chunk sums: one block of slots per (magnitude, relative spread)."""
    rng = np.random.default_rng(seed)
    n = chunk_sizes(k, spp, spi)
    blocks = []
    for mag in MAGNITUDES:
        for spread in SPREADS:
            centre = mag * rng.uniform(0.5, 2.0, (1, per_case, 3))
            means = centre * (1.0 + spread * rng.standard_normal((k, per_case, 3)))
            blocks.append(means * n[:, None, None])
    return np.concatenate(blocks, axis=1).astype(np.float32)


@pytest.mark.parametrize("spi", [1, 3, 4, 8])
@pytest.mark.parametrize("k", [2, 3, 16, 128])
def test_arithmetic_against_float64(k, spi):
    for last in sorted({1, max(1, spi - 1), spi}):           # a shorter last chunk, and a full one
        spp = (k - 1) * spi + last
        partial = synthetic(k, spp, spi, seed=1000 * k + 10 * spi + last)
        v = frt.selftest_chunk_variance(partial, spp, spi).astype(np.float64)
        v64, m = variance64(partial, spp, spi)
        assert np.isfinite(v).all() and (v >= 0).all()
        ratio = np.abs(v - v64) / bound(v64, m)
        print(f"K {k} spi {spi} last {last}: worst |V - V64| / bound = {ratio.max():.3f}")
        assert (ratio <= 1.0).all()


@pytest.mark.parametrize("k,spi,last", [(2, 4, 4), (3, 4, 2), (16, 3, 1), (128, 8, 5), (5, 1, 1)])
def test_equal_chunk_means_give_exactly_zero(k, spi, last):
    """x with 11 mantissa bits: n x is exact for n <= 8, so every chunk mean is x again."""
    rng = np.random.default_rng(k)
    x = (np.floor(rng.uniform(1.0, 2.0, (1, 96, 3)) * 1024) / 1024 * 2.0 ** rng.integers(-10, 10, (1, 96, 3))).astype(np.float32)
    spp = (k - 1) * spi + last
    n = chunk_sizes(k, spp, spi).astype(np.float32)[:, None, None]
    partial = x * n
    assert np.array_equal(partial / n, np.broadcast_to(x, partial.shape))
    v = frt.selftest_chunk_variance(partial, spp, spi)
    assert v.tobytes() == np.zeros_like(v).tobytes()         # +0.0f, every bit


def test_scaling_by_four_scales_by_sixteen():
    for k, spi, last in [(2, 4, 3), (16, 8, 8), (128, 3, 2)]:
        spp = (k - 1) * spi + last
        partial = synthetic(k, spp, spi, seed=7)
        a = frt.selftest_chunk_variance(partial, spp, spi)
        b = frt.selftest_chunk_variance(partial * np.float32(4), spp, spi)
        assert np.array_equal(b, a * np.float32(16)) and a.max() > 0


def test_hook_refuses_what_is_no_cut():
    p = np.zeros((1, 4, 3), np.float32)
    with pytest.raises(frt.FrtError):
        frt.selftest_chunk_variance(p, 4, 4)                  # one chunk
    p = np.zeros((3, 4, 3), np.float32)
    for spp, spi in [(8, 4), (13, 4), (12, 0)]:               # an empty last chunk, too many samples, no granule
        with pytest.raises(frt.FrtError):
            frt.selftest_chunk_variance(p, spp, spi)


# ---- 3. the host replay has no such integrator ----
def test_host_replay_refuses_error(cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 1.0)
    pixels = np.arange(4, dtype=np.int32)
    with pytest.raises(frt.FrtError, match="invalid"):
        frt.selftest_path_host(hs, frt.RenderParams.make(8, 8, 2, integrator=ERROR), pixels)
    with pytest.raises(frt.FrtError, match="invalid"):
        frt.selftest_path_host(hs, frt.RenderParams.make(8, 8, 2, integrator=ERROR), pixels,
                               env_image=np.ones((2, 4, 3), np.float32))
    out, _ = frt.selftest_path_host(hs, frt.RenderParams.make(8, 8, 2), pixels)      # path still replays
    assert np.isfinite(out).all()


# ---- 4. the driver's combination rules ----
def test_combining_independent_passes():
    rng = np.random.default_rng(3)
    v1, v2, v3 = (rng.uniform(0, 1, (6, 5, 3)).astype(np.float32) for _ in range(3))
    v12 = frt.combine_variance(16, v1, 16, v2)
    v = frt.combine_variance(32, v12, 32, v3)
    want = (16.0 ** 2 * v1.astype(np.float64) + 16.0 ** 2 * v2 + 32.0 ** 2 * v3) / 64.0 ** 2
    assert v.dtype == np.float32 and np.allclose(v, want, rtol=3e-7, atol=0)
    # the mean of two equal passes halves the variance
    assert np.array_equal(frt.combine_variance(16, v1, 16, v1), (v1.astype(np.float64) / 2).astype(np.float32))


def test_replicate_variance():
    rng = np.random.default_rng(4)
    films = [rng.uniform(0, 2, (6, 5, 3)).astype(np.float32) for _ in range(4)]
    mean, v = frt.replicate_variance(films)
    want = np.var(np.stack(films).astype(np.float64), axis=0, ddof=1) / 4
    assert v.dtype == np.float32 and np.allclose(v, want, rtol=3e-7, atol=0)
    assert np.allclose(mean, np.mean(np.stack(films).astype(np.float64), axis=0), rtol=3e-7)
    e = frt.frame_error(mean, v)
    assert e == pytest.approx(np.sqrt(want.mean()) / np.mean(np.stack(films).astype(np.float64)), rel=1e-6)


def test_driver_loop_on_a_synthetic_renderer():
    """The loop over callables: an estimator whose V is exactly 1 / spp per pass halves its V
    every pass, so e = sqrt(1 / total); targets, the cap and the refusals."""
    class St:
        kernel_ms, work_items = 1.0, 0
    calls = []

    def render(p):
        calls.append((p.spp, p.sample_offset, p.seed))
        return np.ones((4, 4, 3), np.float32), St()

    def error(p):
        return np.full((4, 4, 3), 1.0 / p.spp, np.float32)
    p = frt.RenderParams.make(4, 4, 1, seed=5)
    film, v, spp, e, ok, passes = frt.render_until(render, error, p, 0.1, 1 << 20)
    assert ok and spp == 128 and e == pytest.approx(np.sqrt(1 / 128)) and e <= 0.1
    assert calls == [(16, 0, 5), (16, 16, 5), (32, 32, 5), (64, 64, 5)]
    assert [s for s, _, _ in passes] == [16, 32, 64, 128]
    _, _, spp, e, ok, _ = frt.render_until(render, error, p, 1e-9, 32)
    assert not ok and spp == 32
    _, _, spp2, _, ok, _ = frt.render_until(render, error, p, 0.2, 1 << 20)
    assert ok and spp2 <= 128
    # a pass that came out as one chunk a pixel is rendered again in two, and the later passes ask for two
    slots = len(frt.shard_slots(p))
    asked = []

    def render_one_chunk(q):
        asked.append((q.spp, q.samples_per_item))
        st = St()
        st.work_items = slots * (1 if q.samples_per_item == 0 else -(-q.spp // q.samples_per_item))
        return np.ones((4, 4, 3), np.float32), st
    _, _, spp, _, ok, _ = frt.render_until(render_one_chunk, error, p, 0.15, 1 << 20)
    assert ok and spp == 64 and asked == [(16, 0), (16, 8), (16, 8), (32, 16)]
    for bad in (0, 1, 3, 24):
        with pytest.raises(frt.FrtError, match="first_spp"):
            frt.render_until(render, error, p, 0.1, 1024, first_spp=bad)
    with pytest.raises(frt.FrtError, match="path and ao"):
        frt.render_until(render, error, frt.RenderParams.pssmlt(4, 4, 4, 16), 0.1, 1024)
    with pytest.raises(frt.FrtError, match="path and ao"):
        frt.render_until(render, error, frt.RenderParams.make(4, 4, 1, integrator=frt.FRT_INTEGRATOR_DENOISE), 0.1, 1024)
