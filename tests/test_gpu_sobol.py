"""FRT_FLAG_SOBOL on the GPU: the kMatsSobol path kernels through Context.render
on every residency, precision and kernel set, against the host replay of the
same call, the oracle's converged golden image and the render without the flag
(tests/sobol_specs.py holds the checks shared with the host tests)."""
import subprocess

import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS
import sobol_specs as SB
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu

ON = SB.ON
HBM = frt.FRT_FLAG_NO_LDS_SCENE
RL = frt.FRT_FLAG_ROULETTE


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


# ---- 1. the GPU film against the host replay of the same call ----
def check_replay(ctx, hs, img, flags, host_flags=0):
    """Gate of test_gpu_roulette.check_replay, and the launch is the sibling's without
    FRT_FLAG_SOBOL: the same precision, residency and register cap.  host_flags: what the replay
    needs said explicitly (FRT_FLAG_FP64 where the context picks the fp64 kernel by itself)."""
    nx, ny, spp = 48, 36, 8
    pixels = np.arange(nx * ny, dtype=np.int32)
    upload(ctx, hs, img)
    film, st = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=17, flags=ON | flags))
    off, sib = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=17, flags=flags))
    ref, cnt = frt.selftest_path_host(hs, frt.RenderParams.make(nx, ny, spp, seed=17, flags=ON | flags | host_flags),
                                      pixels, env_image=img)
    e = rmse(film.reshape(-1, 3)[pixels], ref)
    print("rmse", e, "rays", st.rays, cnt.rays, "sibling", sib.rays, "waves", st.waves_cap, "lds", st.scene_in_lds)
    assert e <= 1e-3
    assert st.samples == cnt.samples and abs(st.rays - cnt.rays) / cnt.rays < 2e-3
    assert st.fp64 == cnt.fp64
    assert (st.fp64, st.scene_in_lds, st.waves_cap) == (sib.fp64, sib.scene_in_lds, sib.waves_cap)
    assert not np.array_equal(film, off)
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


@pytest.mark.parametrize("flags", [0, HBM])
@pytest.mark.parametrize("image", [False, True])
def test_replay_conductors(ctx, image, flags):
    check_replay(ctx, frt.HostScene.from_spec(SS.cornell_conductors(), 48 / 36), ES.random_env(16, 8) if image else None,
                 flags)


@pytest.mark.parametrize("flags", [0, HBM])
def test_replay_env_sampling(ctx, flags):
    check_replay(ctx, frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), ES.random_env(16, 8),
                 frt.FRT_FLAG_ENV_SAMPLING | flags)


def test_replay_fp64_bvh(ctx64):
    st = check_replay(ctx64, frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), None, frt.FRT_FLAG_FP64)
    assert st.fp64 == 1


@pytest.mark.parametrize("flags", [0, HBM])
def test_replay_with_roulette(ctx, flags):
    check_replay(ctx, frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), None, RL | flags)


@pytest.mark.parametrize("flags", [0, HBM])
def test_replay_with_roulette_and_env_sampling(ctx, flags):
    check_replay(ctx, frt.HostScene.from_spec(ES.plain_cornell(), 48 / 36), ES.random_env(16, 8),
                 RL | frt.FRT_FLAG_ENV_SAMPLING | flags)


# ---- 2. same expectation, against the fp64 golden image ----
@pytest.mark.parametrize("flags", [0, HBM])
def test_golden_expectation(ctx, cornell_obj, flags):
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    SB.check_golden(ctx.render, 64, flags)


# ---- 3. less noise than the same call without the flag ----
@pytest.mark.parametrize("max_depth", [0, 33])
def test_less_noise(ctx, cornell_obj, max_depth):
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    SB.check_less_noise(ctx.render, 64, max_depth)


# ---- 4. determinism ----
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
    off, _ = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=13, tile_size=16))
    assert not np.array_equal(off, one)


def test_progressive_passes(ctx, cornell_obj):
    """32 + 32 spp (sample_offset 0 and 32) accumulated equal one 64-spp call."""
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    SB.check_progressive(ctx.render, 64)


# ---- 5. the refusal, and no effect ----
def test_pssmlt_refuses_the_flag(ctx):
    upload(ctx, frt.HostScene.from_spec(ES.plain_cornell(), 1.0))
    film = np.zeros((16, 16, 3), np.float32)
    with pytest.raises(frt.FrtError, match="FRT_FLAG_SOBOL"):
        ctx.render(frt.RenderParams.pssmlt(16, 16, 2, 64, seed=1, bootstrap=100, flags=ON), film)
    a, st = ctx.render(frt.RenderParams.make(16, 16, 4, seed=1, flags=ON))     # the context renders on
    b, _ = ctx.render(frt.RenderParams.make(16, 16, 4, seed=1, flags=ON))
    assert st.samples == 16 * 16 * 4 and np.isfinite(a).all() and a.max() > 0 and np.array_equal(a, b)


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


# ---- 6. the command-line tool ----
def test_cli_sobol(cornell_obj, tmp_path):
    """frt_render --sobol renders the binding's film for the flag; with another integrator it
    refuses to run (before anything is created)."""
    out = str(tmp_path / "s.pfm")
    base = [CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x48", "--ns", "8", "--seed", "3", "--out", out]
    r = subprocess.run(base + ["--sobol", "--integrator", "ao"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--sobol" in r.stderr and "path" in r.stderr
    r = subprocess.run(base + ["--sobol"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ctx = frt.Context(0)
    try:
        ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 64 / 48))
        film, _ = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3, flags=ON))
        off, _ = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3))
    finally:
        ctx.close()
    assert np.array_equal(read_pfm(out), film) and not np.array_equal(film, off)
