"""FRT_INTEGRATOR_DENOISE on the GPU (csrc/frt_denoise.hip) through the real calls: against the
fp64 numpy restatement (denoise_specs.denoise_ref) fed with the GPU's own public normals,
albedo and depth renders of the same parameters, within the probe's tolerance
(denoise_specs.PROBE_TOLERANCE, relative to the film maximum); the exact properties; the
refusals; whether it helps against the golden image; the CLI and frt_render_multi."""
import os
import subprocess

import numpy as np
import pytest

import denoise_specs as DS
import first_raytracer_amd as frt
import golden_images as G
import scene_specs as SS

pytestmark = pytest.mark.gpu

NORMALS, ALBEDO, DEPTH, DENOISE = (frt.FRT_INTEGRATOR_NORMALS, frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH,
                                   frt.FRT_INTEGRATOR_DENOISE)
CLI = os.path.join(DS.ROOT, "first_raytracer_amd", "frt_render")


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


def features(ctx, nx, ny, spp, seed, tile=32, sample_offset=0, flags=0):
    """The public renders the filter's passes must equal: (N, A, D) films and their stats."""
    films, stats = [], []
    for kind in (NORMALS, ALBEDO, DEPTH):
        f, st = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=seed, integrator=kind, tile_size=tile,
                                                 sample_offset=sample_offset, flags=flags))
        films.append(f)
        stats.append(st)
    return films, stats


@pytest.mark.parametrize("nx,ny,tile", [(48, 36, 32), (41, 23, 8), (64, 64, 32), (8, 8, 32), (1, 1, 32)])
def test_matches_restatement(ctx, cornell_obj, nx, ny, tile):
    """8 x 8 is smaller than the last iteration's stencil; 41 x 23 at tile 8 has ragged tiles and
    filter blocks; 48 x 36 and 64 x 64 span several filter blocks; 1 x 1 has the centre tap alone."""
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, nx / ny))
    spp, seed = 4, 7
    (N, A, D), fst = features(ctx, nx, ny, spp, seed, tile)
    colour = DS.random_colour(nx, ny)
    ref = DS.denoise_ref(colour, N, A, D)
    film, st = ctx.denoise(colour.copy(), nx, ny, spp=spp, seed=seed, tile_size=tile)
    d = DS.rel_diff(film, ref)
    print(f"{nx} x {ny} tile {tile}: |gpu - restatement| / max = {d:.3e} (allowed {DS.PROBE_TOLERANCE:.1e}); "
          f"kernel_ms {st.kernel_ms:.3f}")
    assert d <= DS.PROBE_TOLERANCE
    # stats: the sums of the three passes, the plan of the albedo pass
    assert st.samples == st.camera_rays == 3 * nx * ny * spp and st.extension_rays == st.shadow_rays == 0
    assert st.work_items == sum(s.work_items for s in fst) and st.pixels == nx * ny
    assert (st.scene_in_lds, st.waves_cap, st.stack_entries, st.bvh_depth) == \
           (fst[1].scene_in_lds, fst[1].waves_cap, fst[1].stack_entries, fst[1].bvh_depth)
    assert st.kernel_ms > 0


def test_textured_scene_offset_and_flags(ctx):
    """sample_offset = 16 and plan flags reach the feature passes: the film is the restatement's
    for the offset features; the estimator flags and max_depth change nothing."""
    nx, ny, spp, seed = 48, 36, 4, 3
    ctx.upload(frt.HostScene.from_spec(SS.cornell_textured(), nx / ny))
    colour = DS.random_colour(nx, ny, seed=2)
    (N, A, D), _ = features(ctx, nx, ny, spp, seed, sample_offset=16, flags=frt.FRT_FLAG_NO_LDS_SCENE)
    (N0, _, _), _ = features(ctx, nx, ny, spp, seed)
    assert not np.array_equal(N, N0)
    p = frt.RenderParams.make(nx, ny, spp, seed=seed, integrator=DENOISE, sample_offset=16,
                              flags=frt.FRT_FLAG_NO_LDS_SCENE)
    film, _ = ctx.render(p, film=colour.copy())
    assert DS.rel_diff(film, DS.denoise_ref(colour, N, A, D)) <= DS.PROBE_TOLERANCE
    p.flags |= frt.FRT_FLAG_SOBOL | frt.FRT_FLAG_ROULETTE | frt.FRT_FLAG_ENV_SAMPLING | frt.FRT_FLAG_FP64
    p.max_depth = 2
    film2, _ = ctx.render(p, film=colour.copy())
    assert np.array_equal(film, film2)


def test_render_device_filters_slots_in_place(ctx, cornell_obj):
    """Slot order in, slot order out, padding slots untouched: equal to frt_render bit for bit."""
    import torch
    nx, ny, tile = 41, 23, 16
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, nx / ny))
    colour = DS.random_colour(nx, ny, seed=4)
    p = frt.RenderParams.make(nx, ny, 4, seed=7, integrator=DENOISE, tile_size=tile)
    slots = frt.shard_slots(p)
    valid = slots >= 0
    host = np.full((len(slots), 3), -5.0, np.float32)        # the padding's mark
    host[valid] = colour.reshape(-1, 3)[slots[valid]]
    buf = torch.from_numpy(host).cuda()
    ctx.render_device(p, buf.data_ptr(), torch.cuda.current_stream().cuda_stream)
    got = buf.cpu().numpy()
    film, _ = ctx.render(p, film=colour.copy())
    assert np.array_equal(got[valid], film.reshape(-1, 3)[slots[valid]])
    assert (got[~valid] == -5.0).all() and (~valid).any()


def test_exact_properties(ctx, cornell_obj):
    """Point by point as on the probe, through frt_render.  A constant colour returns itself
    within 1e-5 where the albedo film is constant: Cornell with every mesh white lambertian
    (albedo 1, and 1 on a miss).  Over Cornell's own albedo the demodulated output stays inside
    the range of the demodulated input.  Colour := the albedo film returns the albedo film."""
    nx, ny, spp, seed = 48, 36, 4, 7
    const = np.full((ny, nx, 3), (0.7, 0.25, 1.5), np.float32)
    white = {"objects": [{"obj": SS.CORNELL_OBJ, "geo": True, "bsdf": {"type": "lambertian", "albedo": (1.0, 1.0, 1.0)}}],
             "camera": SS.CORNELL_CAM, "world": "bvh"}
    ctx.upload(frt.HostScene.from_spec(white, nx / ny))
    film, _ = ctx.denoise(const.copy(), nx, ny, spp=spp, seed=seed)
    assert np.abs(film / const - 1.0).max() <= 1e-5
    for hs in (frt.HostScene("cornell_box_obj", cornell_obj, nx / ny), frt.HostScene.from_spec(SS.cornell_textured(), nx / ny)):
        ctx.upload(hs)
        A, _ = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=seed, integrator=ALBEDO))
        floor = np.maximum(A.astype(np.float64), DS.constants()["eps_a"])
        film, _ = ctx.denoise(const.copy(), nx, ny, spp=spp, seed=seed)
        r0, r = const / floor, film / floor
        for ch in range(3):
            assert r[..., ch].min() >= r0[..., ch].min() * (1 - 1e-5)
            assert r[..., ch].max() <= r0[..., ch].max() * (1 + 1e-5)
        assert A.min() > DS.constants()["eps_a"]
        film, _ = ctx.denoise(A.copy(), nx, ny, spp=spp, seed=seed)
        assert np.abs(film / A - 1.0).max() <= 1e-5
        zero, _ = ctx.denoise(np.zeros((ny, nx, 3), np.float32), nx, ny, spp=spp, seed=seed)
        assert not zero.any()
        noisy = DS.random_colour(nx, ny, seed=5)
        noisy[10, 7] = (1e4, 0.0, 1e-6)
        out, _ = ctx.denoise(noisy, nx, ny, spp=spp, seed=seed)
        assert np.isfinite(out).all() and (out >= 0).all()


def test_refusals(ctx, cornell_obj):
    """shard_count = 2, and a NaN, a negative or an infinite film value: FRT_E_INVALID with a
    text, and the film is unchanged."""
    nx, ny = 40, 24
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, nx / ny))
    colour = DS.random_colour(nx, ny)
    film = colour.copy()
    with pytest.raises(frt.FrtError, match="invalid .*shard_count"):
        ctx.render(frt.RenderParams.make(nx, ny, 4, integrator=DENOISE, shard_count=2), film=film)
    assert np.array_equal(film, colour)
    for bad in (np.nan, -1e-3, np.inf):
        film = colour.copy()
        film[11, 13, 1] = bad
        before = film.copy()
        with pytest.raises(frt.FrtError, match="invalid .*finite"):
            ctx.denoise(film, nx, ny, spp=4)
        assert np.array_equal(film, before, equal_nan=True)
    out, _ = ctx.denoise(colour.copy(), nx, ny, spp=4)      # and the context still works
    assert np.isfinite(out).all()


def test_filter_helps_on_gpu_renders(ctx, cornell_obj):
    """Point 6 with GPU path renders: per-pixel RMSE against the golden image falls, for every seed."""
    gold = G.cornell64()
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    for seed in (300, 301, 302, 303):
        film, _ = ctx.render(frt.RenderParams.make(64, 64, 4, seed=seed))
        film = np.maximum(film, 0.0)                        # a path sum can end a few 1e-6 below 0
        before = DS.rmse(film, gold)
        out, st = ctx.denoise(film.copy(), 64, 64, spp=16, seed=seed)
        after = DS.rmse(out, gold)
        print(f"seed {seed}: rmse {before:.4f} -> {after:.4f}, ratio {after / before:.3f}")
        assert after < before


def test_cli_denoise_equals_path_then_denoise(ctx, cornell_obj, tmp_path):
    from test_gpu_cli import read_pfm
    out = str(tmp_path / "d.pfm")
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x48", "--ns", "4", "--seed", "5",
                        "--denoise", "--denoise-spp", "8", "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Denoised" in r.stdout
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 64 / 48))
    film, _ = ctx.render(frt.RenderParams.make(64, 48, 4, seed=5))
    want, _ = ctx.denoise(np.maximum(film, 0.0), 64, 48, spp=8, seed=5)   # the CLI clamps the path film at 0
    assert np.array_equal(read_pfm(out), want)
    assert not np.array_equal(want, film)


def test_render_multi_runs_on_the_first_context(ctx, cornell_obj):
    """Two contexts (a second GPU when there is one): the film equals frt_render's on the first."""
    import torch
    nx, ny = 48, 36
    hs = frt.HostScene("cornell_box_obj", cornell_obj, nx / ny)
    other = frt.Context(1 if torch.cuda.device_count() > 1 else 0)
    try:
        ctx.upload(hs)
        other.upload(hs)
        colour = DS.random_colour(nx, ny, seed=8)
        p = frt.RenderParams.make(nx, ny, 4, seed=7, integrator=DENOISE)
        one, _ = ctx.render(p, film=colour.copy())
        two, _ = frt.render_multi([ctx, other], p, film=colour.copy())
        assert np.array_equal(one, two)
    finally:
        other.close()
