"""FRT_FLAG_ROULETTE on the GPU: the kMatsRoulette path kernels through
Context.render on every residency, precision and kernel set, against the render
without the flag (bit for bit where no vertex can play, in expectation
elsewhere), the oracle's converged golden image and the host replay of the same
call (tests/roulette_specs.py holds the checks shared with the host tests)."""
import subprocess

import numpy as np
import pytest

import env_sampling_specs as E
import env_specs as ES
import first_raytracer_amd as frt
import roulette_specs as RS
import scene_specs as SS
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu

ON = RS.ON
HBM = frt.FRT_FLAG_NO_LDS_SCENE


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


def upload(ctx, hs, img=None):
    ctx.upload(hs)
    ctx.set_env_image(img)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64).reshape(-1, 3) - np.asarray(b, np.float64).reshape(-1, 3)) ** 2)))


# ---- 1. the untouched prefix ----
@pytest.mark.parametrize("flags", [0, HBM])
def test_prefix_untouched(ctx, cornell_obj, flags):
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, 48 / 36))
    RS.check_prefix(ctx.render, flags)


# ---- 2. no effect, and the refusal ----
def test_no_effect_on_ao_and_normals(ctx):
    nx, ny = 48, 36
    upload(ctx, frt.HostScene.from_spec(ES.plain_cornell(), nx / ny))
    for img in (None, ES.random_env(16, 8)):
        ctx.set_env_image(img)
        for integrator in (frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS):
            a, sa = ctx.render(frt.RenderParams.make(nx, ny, 8, seed=2, flags=ON, integrator=integrator))
            b, sb = ctx.render(frt.RenderParams.make(nx, ny, 8, seed=2, integrator=integrator))
            assert np.array_equal(a, b) and sa.rays == sb.rays
            assert (sa.waves_cap, sa.stack_entries) == (sb.waves_cap, sb.stack_entries)   # the same kernel


def test_pssmlt_refuses_the_flag(ctx):
    upload(ctx, frt.HostScene.from_spec(ES.plain_cornell(), 1.0))
    film = np.zeros((16, 16, 3), np.float32)
    with pytest.raises(frt.FrtError, match="FRT_FLAG_ROULETTE"):
        ctx.render(frt.RenderParams.pssmlt(16, 16, 2, 64, seed=1, bootstrap=100, flags=ON), film)
    a, st = ctx.render(frt.RenderParams.make(16, 16, 4, seed=1, flags=ON))     # the context renders on
    b, _ = ctx.render(frt.RenderParams.make(16, 16, 4, seed=1, flags=ON))
    assert st.samples == 16 * 16 * 4 and np.isfinite(a).all() and a.max() > 0 and np.array_equal(a, b)


# ---- 3. fewer rays, same samples ----
def test_fewer_rays_same_samples(ctx, cornell_obj):
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    RS.check_fewer_rays(ctx.render)


# ---- 4. same expectation, against the fp64 golden image ----
@pytest.mark.parametrize("flags", [0, HBM])
def test_golden_expectation(ctx, cornell_obj, flags):
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    RS.check_golden(ctx.render, 64, flags)


# ---- 5. same expectation where no golden image exists: flag on against off ----
def on_off_scene(name, glass_obj):
    if name == "conductors":
        return frt.HostScene.from_spec(SS.cornell_conductors(), 48 / 36), None, 0
    if name == "glass":
        return frt.HostScene("cornell_box_obj", glass_obj, 48 / 36), None, 0
    both = frt.FRT_FLAG_ENV_SAMPLING if name == "image_sampled" else 0
    return frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), ES.random_env(16, 8), both


@pytest.mark.parametrize("name", ["conductors", "glass", "image", "image_sampled"])
def test_expectation_unchanged(ctx, glass_obj, name):
    nx, ny, spp, k = 48, 36, 16, 8
    hs, img, flags = on_off_scene(name, glass_obj)
    upload(ctx, hs, img)
    on, off = [], []
    for seed in range(k):
        a, sa = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=100 + seed, flags=ON | flags))
        b, sb = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=200 + seed, flags=flags))
        assert np.isfinite(a).all() and sa.samples == sb.samples
        on.append(a.reshape(-1, 3))
        off.append(b.reshape(-1, 3))
    print("rays on / off", sa.rays / sb.rays)
    assert sa.rays < sb.rays
    assert E.mean_difference_ok(on, off)


def test_expectation_unchanged_veach(ctx, veach_obj):
    """veach_mis (list world, fp64 by default): its golden image is itself noisy, so on against off."""
    nx, ny, spp, k = 96, 64, 16, 8
    upload(ctx, frt.HostScene("veach_mis", veach_obj, nx / ny))
    on, off = [], []
    for seed in range(k):
        a, sa = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=100 + seed, flags=ON))
        b, sb = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=200 + seed))
        assert np.isfinite(a).all() and sa.fp64 == sb.fp64 == 1
        on.append(a.reshape(-1, 3))
        off.append(b.reshape(-1, 3))
    assert E.mean_difference_ok(on, off)


# ---- 6. the GPU film against the host replay of the same call ----
def check_replay(ctx, hs, img, flags, host_flags=0):
    """Gate of test_gpu_env_sampling.check_replay, and the launch is the no-flag sibling's:
    the same precision, residency and register cap.  host_flags: what the replay needs said
    explicitly (FRT_FLAG_FP64 where the context picks the fp64 kernel by itself)."""
    nx, ny, spp = 48, 36, 8
    pixels = np.arange(nx * ny, dtype=np.int32)
    upload(ctx, hs, img)
    film, st = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=17, flags=ON | flags))
    _, sib = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=17, flags=flags))
    ref, cnt = frt.selftest_path_host(hs, frt.RenderParams.make(nx, ny, spp, seed=17, flags=ON | flags | host_flags),
                                      pixels, env_image=img)
    e = rmse(film.reshape(-1, 3)[pixels], ref)
    print("rmse", e, "rays", st.rays, cnt.rays, "sibling", sib.rays, "waves", st.waves_cap, "lds", st.scene_in_lds)
    assert e <= 1e-3
    assert st.samples == cnt.samples and abs(st.rays - cnt.rays) / cnt.rays < 2e-3
    assert st.fp64 == cnt.fp64
    assert (st.fp64, st.scene_in_lds, st.waves_cap) == (sib.fp64, sib.scene_in_lds, sib.waves_cap)
    assert st.rays < sib.rays
    return st


@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_NO_OCT, HBM, HBM | frt.FRT_FLAG_BVH2])
def test_replay_cornell(ctx, flags):
    st = check_replay(ctx, frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), None, flags)
    assert st.scene_in_lds == (0 if flags & HBM else 1) and st.fp64 == 0


@pytest.mark.parametrize("flags,f64", [(frt.FRT_FLAG_FP32, 0), (0, 1)])
def test_replay_list_world(ctx, flags, f64):
    st = check_replay(ctx, frt.HostScene.from_spec(ES.plain_cornell(world="list"), 48 / 36), None, flags,
                      host_flags=frt.FRT_FLAG_FP64 if f64 else 0)
    assert st.fp64 == f64


def test_replay_conductors(ctx):
    check_replay(ctx, frt.HostScene.from_spec(SS.cornell_conductors(), 48 / 36), None, 0)


def test_replay_env_image(ctx):
    """(a scene with specular materials: its kernel without the flag is the every-material one
    these kernels are the siblings of; a lambertian scene with an image runs the same superset)"""
    check_replay(ctx, frt.HostScene.from_spec(SS.cornell_conductors(), 48 / 36), ES.random_env(16, 8), 0)
    check_replay(ctx, frt.HostScene.from_spec(SS.cornell_conductors(), 48 / 36), ES.random_env(16, 8), HBM)


def test_replay_env_image_lambertian(ctx):
    """A lambertian scene under an image renders with the every-material roulette kernel (4 waves
    where its kernel without the flag, kMatsTex | kMatsEnv, has the compiler's allocation): the
    replay gate alone."""
    nx, ny, spp = 48, 36, 8
    pixels = np.arange(nx * ny, dtype=np.int32)
    hs, img = frt.HostScene.from_spec(ES.plain_cornell(), nx / ny), ES.random_env(16, 8)
    upload(ctx, hs, img)
    p = frt.RenderParams.make(nx, ny, spp, seed=17, flags=ON)
    film, st = ctx.render(p)
    ref, cnt = frt.selftest_path_host(hs, p, pixels, env_image=img)
    assert rmse(film, ref) <= 1e-3
    assert st.samples == cnt.samples and abs(st.rays - cnt.rays) / cnt.rays < 2e-3


@pytest.mark.parametrize("flags", [0, HBM])
def test_replay_env_sampling(ctx, flags):
    check_replay(ctx, frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), ES.random_env(16, 8),
                 frt.FRT_FLAG_ENV_SAMPLING | flags)


def test_replay_fp64_bvh(ctx64):
    st = check_replay(ctx64, frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), None, frt.FRT_FLAG_FP64)
    assert st.fp64 == 1


# ---- 7. determinism ----
def test_runs_and_shards_bit_identical(ctx, cornell_obj):
    nx, ny, spp = 80, 72, 8
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, nx / ny))
    p = frt.RenderParams.make(nx, ny, spp, seed=13, tile_size=16, flags=ON)
    one, st = ctx.render(p)
    two, st2 = ctx.render(p)
    assert np.array_equal(one, two) and st.rays == st2.rays
    film = np.zeros_like(one)
    rays = 0
    for k in range(3):
        _, s = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=13, tile_size=16, flags=ON, shard_index=k,
                                                shard_count=3), film)
        rays += s.rays
    assert np.array_equal(film, one) and rays == st.rays
    many, stm = frt.render_multi([ctx], p)
    assert np.array_equal(many, one) and stm.rays == st.rays
    off, st_off = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=13, tile_size=16))
    assert not np.array_equal(off, one) and st.rays < st_off.rays


def test_progressive_passes(ctx, cornell_obj):
    """Two passes of 32 spp (sample_offset 0 and 32) accumulated equal one 64-spp call up to fp32
    summation order (the tolerance of test_gpu_parity.test_progressive_passes)."""
    nx, ny = 64, 64
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    full, st = ctx.render(frt.RenderParams.make(nx, ny, 64, seed=9, flags=ON))
    p1, s1 = ctx.render(frt.RenderParams.make(nx, ny, 32, seed=9, flags=ON))
    p2, s2 = ctx.render(frt.RenderParams.make(nx, ny, 32, seed=9, flags=ON, sample_offset=32))
    acc = frt.film_accumulate(p1, 32, p2, 32)
    assert s1.rays + s2.rays == st.rays
    assert np.allclose(acc, full, rtol=1e-5, atol=1e-7)


# ---- 8. the command-line tool ----
def test_cli_roulette(cornell_obj, tmp_path):
    """frt_render --roulette renders the binding's film for the flag; with another integrator it
    refuses to run (before anything is created)."""
    out = str(tmp_path / "r.pfm")
    base = [CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x48", "--ns", "8", "--seed", "3", "--out", out]
    r = subprocess.run(base + ["--roulette", "--integrator", "ao"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--roulette" in r.stderr and "path" in r.stderr
    r = subprocess.run(base + ["--roulette"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ctx = frt.Context(0)
    try:
        ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 64 / 48))
        film, _ = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3, flags=ON))
        off, _ = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3))
    finally:
        ctx.close()
    assert np.array_equal(read_pfm(out), film) and not np.array_equal(film, off)
