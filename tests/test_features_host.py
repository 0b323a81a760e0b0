"""FRT_INTEGRATOR_ALBEDO and FRT_INTEGRATOR_DEPTH on the CPU: the device code
(csrc/frt_path.hpp albedo_shade / depth_shade) through the host self-test hook,
against the Python restatement over the oracle's scene (denoise_specs.features_ref).

Agreement rule (tests/test_gpu_integrators.py): per-pixel max |diff| <= 1e-3 except
where fp32 rounding sends a sample to another primitive (at most 1 % of the pixels;
a depth pixel also moves when a sample changes sides of a silhouette); RMSE < 1e-5
over the others."""
import os
import re

import numpy as np
import pytest

import denoise_specs as DS
import first_raytracer_amd as frt
import oracle
import scene_specs as SS

ALBEDO, DEPTH, DENOISE = frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH, frt.FRT_INTEGRATOR_DENOISE
NX, NY, SPP, SEED = 24, 18, 4, 5


def test_constants_agree_with_the_header():
    text = open(os.path.join(DS.ROOT, "include", "frt.h")).read()
    for name, value in (("ALBEDO", 4), ("DEPTH", 5), ("DENOISE", 6)):
        m = re.search(r"FRT_INTEGRATOR_" + name + r"\s*=\s*(\d+)", text)
        assert m and int(m.group(1)) == value == getattr(frt, "FRT_INTEGRATOR_" + name)


def test_denoise_takes_the_whole_frame():
    """shard_count must be 1 (params_ok); the slots are then the frame rounded up to tiles."""
    with pytest.raises(frt.FrtError):
        frt.shard_slots(frt.RenderParams.make(40, 20, 1, integrator=DENOISE, shard_count=2))
    slots = frt.shard_slots(frt.RenderParams.make(40, 20, 1, integrator=DENOISE, shard_count=1))
    assert len(slots) == 2 * 1 * 32 * 32 and (slots >= 0).sum() == 40 * 20
    for kind in (ALBEDO, DEPTH):
        assert len(frt.shard_slots(frt.RenderParams.make(40, 20, 1, integrator=kind, shard_count=2))) == 32 * 32
    with pytest.raises(frt.FrtError):                     # 7 stays the bad value
        frt.shard_slots(frt.RenderParams.make(8, 8, 1, integrator=7))


def scenes(request):
    """name -> (HostScene, OracleScene, spec or None) builders for NX x NY."""
    a = NX / NY

    def kind(k, fix):
        obj = request.getfixturevalue(fix)
        return lambda: (frt.HostScene(k, obj, a), oracle.OracleScene(k, obj, a), None)

    def spec(s):
        return lambda: (frt.HostScene.from_spec(s, a), oracle.OracleScene.from_spec(s, a), s)
    return {"cornell": kind("cornell_box_obj", "cornell_obj"), "textured": spec(SS.cornell_textured()),
            "image_textured": spec(SS.cornell_image_textured()), "conductors": spec(SS.cornell_conductors()),
            "glass": kind("cornell_box_obj", "glass_obj"), "glossy": kind("cornell_box_obj", "glossy_floor_obj"),
            "veach": kind("veach_mis", "veach_obj")}


def host_films(hs, nx=NX, ny=NY, spp=SPP, seed=SEED, flags=0, sample_offset=0, env_image=None):
    pix = np.arange(nx * ny, dtype=np.int32)
    out = {}
    for kind in (ALBEDO, DEPTH):
        p = frt.RenderParams.make(nx, ny, spp, seed=seed, integrator=kind, flags=flags, sample_offset=sample_offset)
        out[kind] = frt.selftest_path_host(hs, p, pix, env_image=env_image)
    return out


@pytest.mark.parametrize("name", ["cornell", "textured", "image_textured", "conductors", "glass", "glossy", "veach"])
def test_host_replay_matches_restatement(name, request):
    hs, osc, spec = scenes(request)[name]()
    films = host_films(hs)
    alb_ref, dep_ref = DS.features_ref(osc, NX, NY, SPP, SEED, spec)
    alb, st_a = films[ALBEDO]
    dep, st_d = films[DEPTH]
    flips_a = DS.check_close(alb, alb_ref)
    flips_d = DS.check_depth_close(dep, dep_ref, far=name == "veach")
    print(f"{name}: pixels outside 1e-3: albedo {flips_a}, depth {flips_d} of {NX * NY}")
    for st in (st_a, st_d):
        assert st.camera_rays == st.samples == NX * NY * SPP and st.extension_rays == 0 and st.shadow_rays == 0
    # exact properties
    # albedo in [0, 1] where the scene's colours are; image_textured puts an HDR image (texels up
    # to 1.5) on a conductor's specular reflectance, which is then the bound
    top = 1.0 if name != "image_textured" else float(max(1.0, max(i["data"].max() for i in spec["images"][1:])))
    assert (alb >= 0.0).all() and (alb <= np.float32(top)).all()
    d = dep.astype(np.float64)
    assert (d[:, 2] >= 0).all() and (d[:, 2] <= 1).all()
    assert (d[:, 1] >= d[:, 0] ** 2 / np.maximum(d[:, 2], 1e-30) - 1e-6).all()
    if name == "cornell":                                 # the box fills the middle of the frame
        inner = dep.reshape(NY, NX, 3)[NY // 4:-(NY // 4), NX // 4:-(NX // 4), 2]
        assert (inner == np.float32(1.0)).all()
        # ... and at 4 : 3 the frame's sides see past it: misses, and partly covered pixels
        assert (d[:, 2] == 0).any() and ((d[:, 2] > 0) & (d[:, 2] < 1)).any()
    if name == "veach":                                   # a list world; its floor and wall fill the frame
        assert (d[:, 2] == 1).all()
    if name in ("textured", "image_textured"):            # the texture shows: more colours than materials
        assert len(np.unique(alb_ref.round(6), axis=0)) > 12


def test_coverage_is_exact_at_any_spp(cornell_obj):
    """sum / spp, not sum * (1 / spp): 1.0f where every sample hit."""
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 1.0)
    pix = np.array([8 * 16 + 8], np.int32)
    for spp in (3, 7, 41, 49):
        out, _ = frt.selftest_path_host(hs, frt.RenderParams.make(16, 16, spp, seed=2, integrator=DEPTH), pix)
        assert out[0, 2] == np.float32(1.0), spp


@pytest.mark.parametrize("flag", ["FRT_FLAG_SOBOL", "FRT_FLAG_ROULETTE", "FRT_FLAG_ENV_SAMPLING", "FRT_FLAG_FP64"])
def test_estimator_flags_have_no_effect(flag, request):
    hs, _, _ = scenes(request)["textured"]()
    base = host_films(hs)
    with_flag = host_films(hs, flags=getattr(frt, flag))
    env = np.random.default_rng(1).uniform(0.5, 4.0, (8, 16, 3)).astype(np.float32)
    with_env = host_films(hs, flags=getattr(frt, flag), env_image=env)
    for kind in (ALBEDO, DEPTH):
        assert np.array_equal(base[kind][0], with_flag[kind][0])
        assert np.array_equal(base[kind][0], with_env[kind][0])    # neither reads the environment
        assert with_flag[kind][1].fp64 == 0


def test_progressive_passes_accumulate(request):
    """sample_offset: passes of 2 + 2 samples accumulate to the 4-sample film (fp32 summation
    order apart, the tolerance of sobol_specs.check_progressive)."""
    hs, _, _ = scenes(request)["textured"]()
    full = host_films(hs)
    p1 = host_films(hs, spp=2)
    p2 = host_films(hs, spp=2, sample_offset=2)
    for kind in (ALBEDO, DEPTH):
        acc = frt.film_accumulate(p1[kind][0], 2, p2[kind][0], 2)
        assert np.allclose(acc, full[kind][0], rtol=1e-5, atol=1e-7)
    assert not np.array_equal(p1[DEPTH][0], p2[DEPTH][0])


def test_denoise_is_no_per_pixel_hook(cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 1.0)
    with pytest.raises(frt.FrtError):
        frt.selftest_path_host(hs, frt.RenderParams.make(8, 8, 1, integrator=DENOISE), np.arange(4, dtype=np.int32))
