"""FRT_FLAG_ENV_SAMPLING on the GPU: the kMatsEnvNee path kernels (next-event
estimation toward the environment image, MIS with the bsdf sample) through
Context.render on every residency and precision, against the analytic floor
(tests/env_sampling_specs.py), the estimator without the flag, and the host
replay of the same call."""
import subprocess

import numpy as np
import pytest

import env_sampling_specs as E
import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx64():
    c = frt.Context(0, precision="fp64")
    yield c
    c.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64).reshape(-1, 3) - np.asarray(b, np.float64).reshape(-1, 3)) ** 2)))


# ---- 1. the analytic floor ----
@pytest.mark.parametrize("world,flags,f64", [
    ("bvh", 0, 0),                               # LDS-resident binary BVH (octant copies)
    ("bvh", frt.FRT_FLAG_NO_OCT, 0),             # ... the planar LDS tree
    ("bvh", frt.FRT_FLAG_NO_LDS_SCENE, 0),       # HBM
    ("list", frt.FRT_FLAG_FP32, 0),              # hitable_list world, fp32
    ("list", 0, 1)])                             # ... its default, the fp64 kernel
def test_floor_analytic(ctx, world, flags, f64):
    img = E.sun_image()
    ctx.upload(E.floor_scene(world))
    ctx.set_env_image(img)
    on, st_on = ctx.render(E.floor_params(E.ON | flags))
    off, st_off = ctx.render(E.floor_params(flags))
    assert st_on.fp64 == st_off.fp64 == f64
    assert st_on.scene_in_lds == st_off.scene_in_lds
    E.check_floor(on, st_on, off, st_off, img)


def test_floor_analytic_fp64_bvh(ctx64):
    img = E.sun_image()
    ctx64.upload(E.floor_scene("bvh"))
    ctx64.set_env_image(img)
    on, st_on = ctx64.render(E.floor_params(E.ON | frt.FRT_FLAG_FP64))
    off, st_off = ctx64.render(E.floor_params(frt.FRT_FLAG_FP64))
    assert st_on.fp64 == st_off.fp64 == 1
    E.check_floor(on, st_on, off, st_off, img)


# ---- 2. area lights and the environment together ----
SCENES = {"plain": ES.plain_cornell, "conductors": SS.cornell_conductors}


@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_NO_LDS_SCENE])
@pytest.mark.parametrize("scene", ["plain", "conductors"])
def test_expectation_unchanged_with_area_lights(ctx, scene, flags):
    nx, ny, spp, k = 48, 36, 16, 8
    ctx.upload(frt.HostScene.from_spec(SCENES[scene](world="bvh"), nx / ny))
    ctx.set_env_image(ES.random_env(16, 8))
    on, off = [], []
    for seed in range(k):
        a, st = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=100 + seed, flags=E.ON | flags))
        b, _ = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=200 + seed, flags=flags))
        assert np.isfinite(a).all() and st.shadow_rays > 0
        on.append(a.reshape(-1, 3))
        off.append(b.reshape(-1, 3))
    assert not np.array_equal(on[0], off[0])
    assert E.mean_difference_ok(on, off)


# ---- 3. the GPU film against the host replay of the same call ----
def check_replay(ctx, hs, img, p, pixels):
    ctx.upload(hs)
    ctx.set_env_image(img)
    film, st = ctx.render(p)
    ref, cnt = frt.selftest_path_host(hs, p, pixels, env_image=img)
    e = rmse(film.reshape(-1, 3)[pixels], ref)
    print("rmse", e, "rays", st.rays, cnt.rays)
    assert st.shadow_rays > 0 and cnt.shadow_rays > 0
    assert e <= 1e-3
    return st, cnt


def test_replay_floor(ctx):
    pixels = np.arange(E.FLOOR_NX * E.FLOOR_NY, dtype=np.int32)
    st, cnt = check_replay(ctx, E.floor_scene(), E.sun_image(), E.floor_params(E.ON | frt.FRT_FLAG_BVH2), pixels)
    assert st.samples == cnt.samples and abs(st.rays - cnt.rays) / cnt.rays < 2e-3


@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_NO_LDS_SCENE])
def test_replay_cornell(ctx, flags):
    nx, ny, spp = 48, 36, 8
    pixels = np.arange(nx * ny, dtype=np.int32)
    hs = frt.HostScene.from_spec(ES.plain_cornell(), nx / ny)
    p = frt.RenderParams.make(nx, ny, spp, seed=17, flags=E.ON | flags)
    st, cnt = check_replay(ctx, hs, ES.random_env(16, 8), p, pixels)
    assert st.samples == cnt.samples and abs(st.rays - cnt.rays) / cnt.rays < 2e-3


# ---- 4b. cases where the flag has no effect ----
def test_no_effect_cases(ctx):
    nx, ny = E.FLOOR_NX, E.FLOOR_NY
    hs = frt.HostScene.from_spec(ES.plain_cornell(), nx / ny)
    hs.set_env((0.25, 0.5, 1.0))
    ctx.upload(hs)
    ctx.set_env_image(None)
    for env in (None, np.zeros((8, 16, 3), np.float32)):        # constant colour; an image without luminance
        ctx.set_env_image(env)
        a, sa = ctx.render(E.floor_params(E.ON))
        b, sb = ctx.render(E.floor_params(0))
        assert np.array_equal(a, b) and sa.rays == sb.rays
        assert (sa.waves_cap, sa.stack_entries) == (sb.waves_cap, sb.stack_entries)   # the same kernel
    ctx.set_env_image(E.sun_image())
    for integrator in (frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS):
        a, _ = ctx.render(E.floor_params(E.ON, integrator=integrator))
        b, _ = ctx.render(E.floor_params(0, integrator=integrator))
        assert np.array_equal(a, b)


# ---- 5. state and errors ----
def test_tables_follow_the_image(ctx):
    """The cached tables belong to one image: after set_env_image the render is a fresh context's."""
    img_a, img_b = E.sun_image(), np.roll(E.sun_image(), (2, 9), axis=(0, 1))
    hs = E.floor_scene()
    p = E.floor_params(E.ON)
    fresh = frt.Context(0)
    try:
        fresh.upload(hs)
        fresh.set_env_image(img_b)
        want_b, _ = fresh.render(p)
        fresh.set_env_image(None)
        want_none, _ = fresh.render(p)
    finally:
        fresh.close()
    ctx.upload(hs)
    ctx.set_env_image(img_a)
    film_a, _ = ctx.render(p)
    again, _ = ctx.render(p)                      # the cached tables
    assert np.array_equal(film_a, again)
    ctx.set_env_image(img_b)
    film_b, _ = ctx.render(p)
    assert np.array_equal(film_b, want_b) and not np.array_equal(film_b, film_a)
    ctx.set_env_image(None)                       # cleared: the flag has nothing to sample
    none, _ = ctx.render(p)
    assert np.array_equal(none, want_none)
    ctx.set_env_image(img_a)
    back, _ = ctx.render(p)
    assert np.array_equal(back, film_a)


def test_pssmlt_refuses_the_flag(ctx):
    ctx.upload(frt.HostScene.from_spec(ES.plain_cornell(), 1.0))
    ctx.set_env_image(E.sun_image())
    film = np.zeros((16, 16, 3), np.float32)
    with pytest.raises(frt.FrtError, match="FRT_FLAG_ENV_SAMPLING"):
        ctx.render(frt.RenderParams.pssmlt(16, 16, 2, 64, seed=1, bootstrap=100, flags=E.ON), film)
    ctx.set_env_image(None)
    with pytest.raises(frt.FrtError, match="FRT_FLAG_ENV_SAMPLING"):
        ctx.render(frt.RenderParams.pssmlt(16, 16, 2, 64, seed=1, bootstrap=100, flags=E.ON), film)


def test_render_multi_and_shards(ctx):
    """Two contexts on one device (each builds its own tables) give the
    single-context film bit for bit, and so do two shards rendered in turn."""
    nx, ny, spp = 48, 36, 8
    hs = frt.HostScene.from_spec(ES.plain_cornell(), nx / ny)
    img = ES.random_env(16, 8)
    p = frt.RenderParams.make(nx, ny, spp, seed=13, tile_size=16, flags=E.ON)
    ctx.upload(hs)
    ctx.set_env_image(img)
    one, st1 = ctx.render(p)
    assert st1.shadow_rays > 0
    film = np.zeros_like(one)
    for k in range(2):
        ctx.render(frt.RenderParams.make(nx, ny, spp, seed=13, tile_size=16, flags=E.ON, shard_index=k, shard_count=2),
                   film)
    assert np.array_equal(film, one)
    other = frt.Context(0)
    try:
        other.upload(hs)
        other.set_env_image(img)
        many, stm = frt.render_multi([ctx, other], p)
        assert np.array_equal(many, one) and stm.rays == st1.rays
    finally:
        other.close()


# ---- the command-line tool ----
def test_cli_env_sampling(cornell_obj, tmp_path):
    """frt_render --env-sampling renders the binding's film for the flag; without --env-map,
    or with another integrator, it refuses to run (before anything is created)."""
    hdr = tmp_path / "env.hdr"
    hdr.write_bytes(ES.hdr_bytes(ES.rgbe_random(32, 16, seed=6), rle=True))
    out = str(tmp_path / "s.pfm")
    base = [CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x48", "--ns", "8", "--seed", "3", "--out", out]
    r = subprocess.run(base + ["--env-sampling"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--env-map" in r.stderr
    r = subprocess.run(base + ["--env-map", str(hdr), "--env-sampling", "--integrator", "pssmlt"], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 2 and "path" in r.stderr
    r = subprocess.run(base + ["--env-map", str(hdr), "--env-sampling"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ctx = frt.Context(0)
    try:
        ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 64 / 48))
        ctx.set_env_image(frt.read_hdr(str(hdr)))
        film, st = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3, flags=E.ON))
        off, _ = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3))
    finally:
        ctx.close()
    assert np.array_equal(read_pfm(out), film) and not np.array_equal(film, off)
