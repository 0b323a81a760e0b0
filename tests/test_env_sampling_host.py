"""FRT_FLAG_ENV_SAMPLING on the host: next-event estimation toward the
environment image in path_shade (csrc/frt_path.hpp: env_sample, env_pdf) and the
tables of csrc/host/envdist.cpp, run by the host replay
(frt_selftest_path_host_env).  The oracle has no environment images, so the
expected values are analytic (the floor scene, tests/env_sampling_specs.py) or
come from the estimator without the flag, which is the one pinned to the
oracle."""
import numpy as np
import pytest

import env_sampling_specs as E
import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS

ALL = np.arange(E.FLOOR_NX * E.FLOOR_NY, dtype=np.int32)


# ---- 1. the analytic floor ----
@pytest.mark.parametrize("world", ["bvh", "list"])
@pytest.mark.parametrize("prec", [0, frt.FRT_FLAG_FP64])
def test_floor_analytic(world, prec):
    hs, img = E.floor_scene(world), E.sun_image()
    on, st_on = frt.selftest_path_host(hs, E.floor_params(E.ON | prec), ALL, env_image=img)
    off, st_off = frt.selftest_path_host(hs, E.floor_params(prec), ALL, env_image=img)
    assert st_on.fp64 == (1 if prec else 0)
    E.check_floor(on, st_on, off, st_off, img)


# ---- 2. area lights and the environment together ----
SCENES = {"plain": ES.plain_cornell, "conductors": SS.cornell_conductors}


@pytest.mark.parametrize("scene", ["plain", "conductors"])
def test_expectation_unchanged_with_area_lights(scene):
    """The ceiling light and the image are both sampled (selection 1/2 each at
    lambertian and rough conductor vertices, the reference's pick after metal):
    occlusion, the selection and the specular exclusions leave the image mean
    where the estimator without the flag has it."""
    nx, ny, spp, k = 24, 18, 16, 8
    hs = frt.HostScene.from_spec(SCENES[scene](world="bvh"), nx / ny)
    img = ES.random_env(16, 8)
    pixels = np.arange(0, nx * ny, 3, dtype=np.int32)
    on, off = [], []
    for seed in range(k):
        a, st = frt.selftest_path_host(hs, frt.RenderParams.make(nx, ny, spp, seed=100 + seed, flags=E.ON), pixels,
                                       env_image=img)
        b, _ = frt.selftest_path_host(hs, frt.RenderParams.make(nx, ny, spp, seed=200 + seed), pixels, env_image=img)
        assert np.isfinite(a).all() and st.shadow_rays > 0
        on.append(a)
        off.append(b)
    assert not np.array_equal(on[0], off[0])
    assert E.mean_difference_ok(on, off)


# ---- 4. the tables ----
def test_one_texel_image():
    """An image with one non-zero texel T (row j, value E) over the floor scene at
    1 spp.  The scene has no lights, so the camera vertex samples the image with
    probability 1, and T with probability 1: pdf_env = 1 / Omega (Omega: T's solid
    angle).  The bsdf ray always leaves the scene.  With pb(d) = cos(theta_d) / pi
    and the power heuristic w_l = pl^2 / (pl^2 + pb^2), w_b = 1 - w_l, a sample is

        L = w_l(d1) * albedo / pi * cos(theta_1) * E * Omega          (d1: the drawn direction, in T)
          + [d2 in T] * w_b(d2) * albedo * E                          (d2: the bsdf direction)

    The two terms do not share a direction, so one sample is not the constant
    albedo / pi * E * integral_T cos: that is their sum's expectation.  What holds
    per pixel: cos(theta) over T lies in [c1, c0] = [cos(theta_{j+1}), cos(theta_j)],
    w_l falls and w_b rises with cos, so the first term lies in
    [w_l(c0) c1, w_l(c1) c0] * albedo / pi * E * Omega and the second is 0 or in
    [w_b(c1), w_b(c0)] * albedo * E.  A sample outside T (value 0), a wrong Omega
    or a wrong table probability leaves these intervals; the mean over pixels is
    checked against the integral with its own standard error."""
    nx, ny, j, col = 128, 64, 12, 37
    val = np.array([40.0, 20.0, 10.0])
    img = E.one_texel_image(nx, ny, j, col, val)
    hs = E.floor_scene()
    p = frt.RenderParams.make(E.FLOOR_NX, E.FLOOR_NY, 1, seed=5, flags=E.ON)
    out, st = frt.selftest_path_host(hs, p, ALL, env_image=img)
    out = out.astype(np.float64)
    assert st.shadow_rays == st.samples == len(ALL) and st.extension_rays == st.samples
    c0, c1 = np.cos(np.pi * j / ny), np.cos(np.pi * (j + 1) / ny)
    omega = (2.0 * np.pi / nx) * (c0 - c1)
    pl = 1.0 / omega
    w_l = lambda c: pl ** 2 / (pl ** 2 + (c / np.pi) ** 2)      # noqa: E731
    k1, k2 = E.ALBEDO / np.pi * omega, E.ALBEDO
    lo1, hi1 = k1 * w_l(c0) * c1, k1 * w_l(c1) * c0
    lo2, hi2 = k2 * (1.0 - w_l(c1)), k2 * (1.0 - w_l(c0))
    r = out / val                                                # per unit of E, every channel
    tol = 1e-5
    first_only = (r >= lo1 * (1 - tol)) & (r <= hi1 * (1 + tol))
    both = (r >= (lo1 + lo2) * (1 - tol)) & (r <= (hi1 + hi2) * (1 + tol))
    print("range", r.min(), r.max(), "bounds", lo1, hi1, "with a bsdf hit", lo1 + lo2, hi1 + hi2, "bsdf hits",
          int((both & ~first_only).all(axis=1).sum()))
    assert (first_only | both).all()
    assert np.allclose(r[:, 0], r[:, 1], rtol=1e-6) and np.allclose(r[:, 0], r[:, 2], rtol=1e-6)
    want = E.ALBEDO / np.pi * E.texel_cos_integral(nx, ny, j)
    m, se = r[:, 0].mean(), r[:, 0].std(ddof=1) / np.sqrt(len(r))
    assert abs(m - want) <= 4.0 * se
    assert np.allclose(E.floor_expectation(img), want * val)


def test_no_effect_cases():
    """An image without luminance, a constant-colour environment, AO and normals:
    films bit-identical to the same call without the flag."""
    hs = E.floor_scene()
    px = ALL[::5]
    dark = np.zeros((8, 16, 3), np.float32)
    for env in (dark, None):
        a, sa = frt.selftest_path_host(hs, E.floor_params(E.ON), px, env_image=env)
        b, sb = frt.selftest_path_host(hs, E.floor_params(0), px, env_image=env)
        assert np.array_equal(a, b) and sa.shadow_rays == sb.shadow_rays == 0
    hc = frt.HostScene.from_spec(ES.plain_cornell(), E.FLOOR_NX / E.FLOOR_NY)
    hc.set_env((0.25, 0.5, 1.0))
    a, sa = frt.selftest_path_host(hc, E.floor_params(E.ON), px)
    b, sb = frt.selftest_path_host(hc, E.floor_params(0), px)
    assert np.array_equal(a, b) and sa.rays == sb.rays
    img = E.sun_image()
    for integrator in (frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS):
        a, _ = frt.selftest_path_host(hc, E.floor_params(E.ON, integrator=integrator), px, env_image=img)
        b, _ = frt.selftest_path_host(hc, E.floor_params(0, integrator=integrator), px, env_image=img)
        assert np.array_equal(a, b)


def test_flag_value():
    assert frt.FRT_FLAG_ENV_SAMPLING == 2048 and frt.lib().frt_get_abi_version() == 9
