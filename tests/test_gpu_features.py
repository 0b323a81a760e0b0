"""FRT_INTEGRATOR_ALBEDO and FRT_INTEGRATOR_DEPTH on the GPU (the KIND kernels of
csrc/frt_render_feat.hip) against the host replay of the same call, on the plans of
normals; the counters, shards, and a context with an environment image.

Agreement rule (tests/test_gpu_integrators.py): per-pixel max |diff| <= 1e-3 except where
fp32 rounding sends a sample to another primitive (at most 1 % of the pixels); RMSE < 1e-5
over the others.  Host and device run the same fp32 code, so the films are usually equal to
the last bits."""
import os
import subprocess

import numpy as np
import pytest

import denoise_specs as DS
import first_raytracer_amd as frt
import scene_specs as SS

pytestmark = pytest.mark.gpu

ALBEDO, DEPTH = frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH
NX, NY, SPP, SEED = 48, 36, 8, 4
CLI = os.path.join(DS.ROOT, "first_raytracer_amd", "frt_render")


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


def scene(name, request):
    a = NX / NY
    if name == "veach":
        return frt.HostScene("veach_mis", request.getfixturevalue("veach_obj"), a)
    if name == "textured":
        return frt.HostScene.from_spec(SS.cornell_image_textured(), a)
    return frt.HostScene("cornell_box_obj", request.getfixturevalue("cornell_obj"), a)


CASES = [("cornell", 0),                                                  # LDS-resident binary BVH
         ("cornell", frt.FRT_FLAG_NO_LDS_SCENE),                          # HBM, 4-wide quantized BVH
         ("cornell", frt.FRT_FLAG_NO_LDS_SCENE | frt.FRT_FLAG_BVH2),      # HBM, binary BVH
         ("veach", 0),                                                    # list world
         ("textured", 0)]                                                 # image textures on three materials


@pytest.mark.parametrize("kind", [ALBEDO, DEPTH])
@pytest.mark.parametrize("name,flags", CASES)
def test_gpu_matches_host_replay(ctx, name, flags, kind, request):
    hs = scene(name, request)
    ctx.upload(hs)
    p = frt.RenderParams.make(NX, NY, SPP, seed=SEED, integrator=kind, flags=flags)
    film, st = ctx.render(p)
    ref, _ = frt.selftest_path_host(hs, p, np.arange(NX * NY, dtype=np.int32))
    flips = DS.check_depth_close(film, ref, far=name == "veach") if kind == DEPTH else DS.check_close(film, ref)
    print(f"{name} flags {flags} integrator {kind}: {flips} pixels outside 1e-3, "
          f"max |diff| {np.abs(film.reshape(-1, 3) - ref).max():.3e}")
    assert st.camera_rays == st.samples == NX * NY * SPP
    assert st.extension_rays == 0 and st.shadow_rays == 0 and st.pixels == NX * NY and st.fp64 == 0
    if name == "cornell":
        assert st.scene_in_lds == (0 if flags else 1)
    if kind == DEPTH:
        cov = film[..., 2]
        assert (cov >= 0).all() and (cov <= 1).all() and (cov == 1).any()
        if name == "cornell":                              # at 4 : 3 the sides see past the box
            assert (cov == 0).any() and ((cov > 0) & (cov < 1)).any()
    else:                                                  # (the textured scene's HDR image has texels above 1)
        assert (film >= 0).all() and ((film <= 1).all() or name == "textured")


@pytest.mark.parametrize("kind", [ALBEDO, DEPTH])
def test_shards_and_determinism(ctx, cornell_obj, kind):
    """Shards 0 / 2 and 1 / 2 make the whole frame, bit for bit; so does a second run."""
    ctx.upload(frt.HostScene.from_spec(SS.cornell_textured(), 80 / 72))
    whole, _ = ctx.render(frt.RenderParams.make(80, 72, 5, seed=9, integrator=kind))
    again, _ = ctx.render(frt.RenderParams.make(80, 72, 5, seed=9, integrator=kind))
    assert np.array_equal(whole, again)
    parts = np.full_like(whole, -1.0)
    for k in range(2):
        ctx.render(frt.RenderParams.make(80, 72, 5, seed=9, integrator=kind, shard_index=k, shard_count=2), parts)
    assert np.array_equal(whole, parts)


@pytest.mark.parametrize("kind", [ALBEDO, DEPTH])
def test_flags_offsets_and_environment_image(cornell_obj, kind):
    """The estimator flags do nothing; passes with sample_offset accumulate; and a context with
    an environment image runs the same kernels: bit-equal films."""
    hs = frt.HostScene.from_spec(SS.cornell_textured(), NX / NY)
    plain, with_env = frt.Context(0), frt.Context(0)
    try:
        plain.upload(hs)
        with_env.upload(hs)
        with_env.set_env_image(np.random.default_rng(2).uniform(0.5, 4.0, (16, 32, 3)).astype(np.float32))
        base, st = plain.render(frt.RenderParams.make(NX, NY, SPP, seed=SEED, integrator=kind))
        for ctx in (plain, with_env):
            for flags in (0, frt.FRT_FLAG_SOBOL, frt.FRT_FLAG_ROULETTE, frt.FRT_FLAG_ENV_SAMPLING, frt.FRT_FLAG_FP64):
                film, st2 = ctx.render(frt.RenderParams.make(NX, NY, SPP, seed=SEED, integrator=kind, flags=flags))
                assert np.array_equal(film, base), flags
                assert (st2.waves_cap, st2.stack_entries, st2.scene_in_lds) == (st.waves_cap, st.stack_entries,
                                                                              st.scene_in_lds)
        h = SPP // 2
        p1, _ = plain.render(frt.RenderParams.make(NX, NY, h, seed=SEED, integrator=kind))
        p2, _ = plain.render(frt.RenderParams.make(NX, NY, h, seed=SEED, integrator=kind, sample_offset=h))
        assert np.allclose(frt.film_accumulate(p1, h, p2, h), base, rtol=1e-5, atol=1e-7)
    finally:
        plain.close()
        with_env.close()


def test_coverage_is_exact_at_odd_spp(ctx, cornell_obj):
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    for spp in (3, 41, 49):
        film, _ = ctx.render(frt.RenderParams.make(16, 16, spp, seed=2, integrator=DEPTH))
        assert (film[4:12, 4:12, 2] == np.float32(1.0)).all(), spp


def test_multi_equals_single(ctx, cornell_obj):
    """frt_render_multi over two contexts of this GPU: shards gathered to the one-context film."""
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    other = frt.Context(0)
    try:
        ctx.upload(hs)
        other.upload(hs)
        for kind in (ALBEDO, DEPTH):
            p = frt.RenderParams.make(NX, NY, SPP, seed=SEED, integrator=kind)
            one, _ = ctx.render(p)
            two, st = frt.render_multi([ctx, other], p)
            assert np.array_equal(one, two) and st.samples == NX * NY * SPP
    finally:
        other.close()


@pytest.mark.parametrize("integ,kind", [("albedo", ALBEDO), ("depth", DEPTH)])
def test_cli_writes_the_library_film(ctx, cornell_obj, tmp_path, integ, kind):
    from test_gpu_cli import read_pfm
    out = str(tmp_path / f"{integ}.pfm")
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x48", "--ns", "4", "--seed", "5",
                        "--integrator", integ, "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 64 / 48))
    film, _ = ctx.render(frt.RenderParams.make(64, 48, 4, seed=5, integrator=kind))
    assert np.array_equal(read_pfm(out), film)
