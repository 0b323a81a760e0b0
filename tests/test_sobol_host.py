"""FRT_FLAG_SOBOL on the host: the Owen-scrambled Sobol' sampler of
csrc/frt_device.hpp (sobol_key / sobol_word) against its numpy restatement
(tests/sobol_specs.py), the restatement's net, marginal and correlation
properties, and the path integrator under the flag run by the host replay
(frt_selftest_path_host).  The oracle has no such sampler, so the expected
values are the estimator without the flag in expectation (the oracle's converged
golden image) and the construction's own guarantees."""
import os
import re
import subprocess

import numpy as np
import pytest

import env_sampling_specs as E
import env_specs as ES
import first_raytracer_amd as frt
import sobol_specs as SB

ON = SB.ON
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "frt.h")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def host_render(hs, nx, ny, env=None):
    pixels = np.arange(nx * ny, dtype=np.int32)
    return lambda p: frt.selftest_path_host(hs, p, pixels, env_image=env)


@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, 1.0)


# ---- the sampler: the code against the numpy restatement ----
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """tests/sobol_probe.hip (its own main over csrc/frt_device.hpp) built as host code."""
    exe = str(tmp_path_factory.mktemp("probe") / "sobol_probe")
    subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17",
                    "-I" + os.path.join(ROOT, "first_raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "sobol_probe.hip"), "-o", exe], check=True, timeout=300)

    def run(tuples):
        text = "".join("%d %d %d %d\n" % tuple(t) for t in tuples)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True, timeout=60).stdout
        rows = [tuple(int(v) for v in line.split()) for line in out.splitlines()]
        assert len(rows) == len(tuples)
        return rows
    return run


def check_probe(probe, tuples):
    for (seed, p, s, d), (w, u24) in zip(tuples, probe(tuples)):
        expect = int(SB.word(seed, p, s, d))
        assert w == expect, (seed, p, s, d, w, expect)
        assert u24 == expect >> 8 and u24 * 2.0 ** -24 == float(SB.uniform(seed, p, s, d)) < 1.0


def test_probe_matches_numpy_random(probe):
    rng = np.random.default_rng(5)
    tuples = [tuple(int(v) for v in rng.integers(0, 2 ** 32, 3)) + (int(rng.integers(0, SB.MAX_DIM + 1)),)
              for _ in range(200)]
    check_probe(probe, tuples)


def test_probe_matches_numpy_edges(probe):
    big = 2 ** 32 - 1
    tuples = [(seed, p, s, d) for seed in (0, 7, big) for p in (0, 1919 * 1080, big) for s in (0, 1, big)
              for d in (0, 1, SB.MAX_DIM - 1, SB.MAX_DIM)]
    check_probe(probe, tuples)


def test_net_property_of_the_code(probe):
    """The net property on the words the code itself gives: 4 keys, the pairs, block lengths and
    block positions of test_net_property."""
    rng = np.random.default_rng(3)
    keys = [tuple(int(v) for v in rng.integers(0, 2 ** 32, 2)) for _ in range(4)]
    n = 4 << 8                                          # covers block 3 of length 2^8
    tuples = [(seed, pixel, s, 2 * j + c) for seed, pixel in keys for j in (0, 1, 5, 135) for s in range(n)
              for c in (0, 1)]
    words = np.array([w for w, _ in probe(tuples)], np.uint64).reshape(len(keys), 4, n, 2)
    for k in range(len(keys)):
        for j in range(4):
            for m in (2, 4, 6, 8):
                for b in (0, 1, 3):
                    assert SB.is_net(words[k, j, b << m:(b + 1) << m], m), (keys[k], j, m, b)


# ---- the sampler's properties, on the restatement ----
def test_sobol1_butterfly_is_the_generator_matrix():
    i = np.random.default_rng(2).integers(0, 2 ** 32, 4096, dtype=np.uint64)
    i[:4] = [0, 1, 2 ** 31, 2 ** 32 - 1]
    assert np.array_equal(SB.sobol1(i), SB.sobol1_loop(i))


def test_net_property():
    """Every aligned block of 2^m indices is a (0, m, 2)-net in every pair: exact, no failure allowed."""
    rng = np.random.default_rng(1)
    for _ in range(50):
        seed, pixel = (int(v) for v in rng.integers(0, 2 ** 32, 2))
        for j in (0, 1, 5, 135):
            for m in (2, 4, 6, 8):
                for b in (0, 1, 3):
                    pts = SB.pair_points(seed, pixel, j, np.arange(b << m, (b + 1) << m))
                    assert SB.is_net(pts, m), (seed, pixel, j, m, b)


def test_marginals():
    """Over 4096 pixels at fixed (sample, dimension): mean and variance of a uniform, 4 standard errors."""
    n = 4096
    for s, d in ((0, 0), (0, 1), (5, 2), (17, 270), (2 ** 32 - 1, SB.MAX_DIM), (100, 11)):
        u = SB.uniform(0, np.arange(n), s, d)
        assert abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12 / n)
        assert abs(u.var() - 1 / 12) < 4 * np.sqrt(1 / 180 / n)   # var of (u - 1/2)^2 = 1/80 - 1/144


def test_decorrelation():
    """|corr| < 4 / sqrt(N) over N = 65,536 (pixel, sample) points.  The bound is four standard
    errors of the correlation of N independent points, and the points of one pixel are
    stratified, not independent; so every point comes from its own pixel (a 256 x 256 frame),
    with sample indices that run through 0..63."""
    n = 65536
    p = np.arange(n)
    s = (p * 7) % 64
    lim = 4 / np.sqrt(n)
    for d1, d2 in ((0, 2), (1, 3), (0, 3), (2, 10), (11, 271), (10, 270), (7, 8), (6, 12)):   # different pairs of one sample
        c = SB.corr(SB.uniform(0, p, s, d1), SB.uniform(0, p, s, d2))
        assert abs(c) < lim, (d1, d2, c)
    for d in (0, 1, 10, 11, 270):                       # the same pair of neighbouring pixels
        c = SB.corr(SB.uniform(0, p, s, d), SB.uniform(0, p + 1, s, d))
        assert abs(c) < lim, (d, c)


def test_seed_dependence():
    s = np.arange(64)
    a, b = SB.pair_points(1, 77, 0, s), SB.pair_points(2, 77, 0, s)
    assert not np.array_equal(a, b) and (a != b).mean() > 0.9
    assert not np.array_equal(SB.pair_points(1, 77, 3, s), SB.pair_points(1, 78, 3, s))


# ---- constants and parameter checks ----
def test_flag_value_matches_header():
    m = re.search(r"FRT_FLAG_SOBOL\s*=\s*(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == frt.FRT_FLAG_SOBOL == 8192
    assert frt.lib().frt_get_abi_version() == 9


def test_params_accept_the_flag():
    p = frt.RenderParams.make(40, 24, 2, flags=ON, shard_index=1, shard_count=2)
    q = frt.RenderParams.make(40, 24, 2, shard_index=1, shard_count=2)
    assert np.array_equal(frt.shard_slots(p), frt.shard_slots(q))
    assert len(frt.shard_slots(frt.RenderParams.pssmlt(8, 8, 1, 16, flags=ON))) == 64   # refused at render, not here


# ---- no effect: AO, normals ----
def test_no_effect_on_ao_and_normals():
    nx, ny = 24, 18
    hs = frt.HostScene.from_spec(ES.plain_cornell(), nx / ny)
    render = host_render(hs, nx, ny, env=ES.random_env(16, 8))
    for integrator in (frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS):
        a, sa = render(frt.RenderParams.make(nx, ny, 4, seed=2, flags=ON, integrator=integrator))
        b, sb = render(frt.RenderParams.make(nx, ny, 4, seed=2, integrator=integrator))
        assert np.array_equal(a, b) and sa.rays == sb.rays


# ---- the flag has an effect (fails where the bit is ignored) ----
@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_FP64])
def test_flag_has_an_effect(cornell_obj, flags):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 48 / 36)
    SB.check_has_effect(host_render(hs, 48, 36), flags)


# ---- same expectation, against the fp64 golden image ----
@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_ROULETTE])
def test_golden_expectation(cornell, flags):
    SB.check_golden(host_render(cornell, 64, 64), 16, flags)


def test_roulette_prefix_survives(cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 48 / 36)
    SB.check_roulette_prefix(host_render(hs, 48, 36))


def test_env_sampling_expectation():
    """plain_cornell under an image, 48x36x16 on 8 seeds: SOBOL | ENV_SAMPLING against ENV_SAMPLING."""
    nx, ny, spp, k = 48, 36, 16, 8
    render = host_render(frt.HostScene.from_spec(ES.plain_cornell(), nx / ny), nx, ny, env=ES.random_env(16, 8))
    es = frt.FRT_FLAG_ENV_SAMPLING
    on = [render(frt.RenderParams.make(nx, ny, spp, seed=100 + s, flags=ON | es))[0] for s in range(k)]
    off = [render(frt.RenderParams.make(nx, ny, spp, seed=200 + s, flags=es))[0] for s in range(k)]
    assert np.isfinite(on).all() and not np.array_equal(on[0], off[0])
    assert E.mean_difference_ok(on, off)


def test_progressive_passes(cornell):
    """8 + 8 spp (sample_offset 0 and 8) accumulated equal one 16-spp call."""
    SB.check_progressive(host_render(cornell, 64, 64), 16)


# ---- less noise than the same call without the flag ----
@pytest.mark.parametrize("max_depth", [0, 33])
def test_less_noise(cornell, max_depth):
    """Cornell 64x64x16, seeds 300..315, per-pixel variance over the seeds averaged over pixels
    and channels.  The host replay is deterministic: the ratios on / off are 0.2428 (max_depth 0)
    and 0.2458 (max_depth 33); profiles/LOG.md."""
    SB.check_less_noise(host_render(cornell, 64, 64), 16, max_depth)
