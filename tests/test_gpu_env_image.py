"""Image-based environment maps (frt_set_env_image) on the GPU, in every
integrator, against the fp64 oracle.

1. Composition: a uniform image must render what the oracle renders with the
   constant env of the same colour (the project's gates: RMSE <= 1e-3, PSS-MLT
   2e-3 * max(1, |ref|max), ray counts within 2e-3 / 5e-3).
2. Direction map: distinct random texels; on pixels whose samples all miss and
   whose footprint lies inside one texel (the oracle hooks ora_env_uv +
   ora_image_lookup decide both, tests/env_specs.py) the film is that texel.
3. Poles, 4. context state and errors, 5. sharding."""
import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt
import oracle
import scene_specs as SS

pytestmark = pytest.mark.gpu

C = (0.75, 0.5, 1.25)          # exact in fp32
UNIFORM = np.tile(np.float32(C), (2, 4, 1))   # 4 x 2, F32
SCENES = {"textured": SS.cornell_textured, "plain": ES.plain_cornell}


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.set_env_image(None)
    c.close()


@pytest.fixture(scope="module")
def ctx64():
    c = frt.Context(0, precision="fp64")
    yield c
    c.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64).reshape(-1, 3) - np.asarray(b, np.float64).reshape(-1, 3)) ** 2)))


_refs = {}


def oracle_ref(scene, world, nx, ny, spp, seed, integrator):
    """The oracle's render with set_env(C), computed once per configuration."""
    key = (scene, world, nx, ny, spp, seed, integrator)
    if key not in _refs:
        osc = oracle.OracleScene.from_spec(SCENES[scene](world), nx / ny)
        osc.set_env(C)
        _refs[key] = osc.render(nx, ny, spp, seed=seed, integrator=integrator)
    return _refs[key]


def check_film(film, st, ref, cnt, tol=1e-3, rays=2e-3):
    e = rmse(film, ref)
    print("rmse", e, "rays", st.rays, cnt.rays)
    assert st.samples == cnt.samples and st.camera_rays == cnt.camera_rays
    assert abs(st.rays - cnt.rays) / cnt.rays < rays
    assert np.isfinite(film).all()
    assert e <= tol


# ---- 1. composition against the oracle's constant environment ----
@pytest.mark.parametrize("scene", ["textured", "plain"])
@pytest.mark.parametrize("world,flags", [
    ("bvh", 0),                               # LDS-resident binary BVH
    ("bvh", frt.FRT_FLAG_NO_LDS_SCENE),       # HBM 4-wide BVH
    ("list", 0),                              # hitable_list world (fp64 under the default precision)
    ("list", frt.FRT_FLAG_FP32)])             # ... and its fp32 kernel
def test_uniform_image_path(ctx, scene, world, flags):
    nx, ny, spp = 96, 72, 32
    ctx.upload(frt.HostScene.from_spec(SCENES[scene](world), nx / ny))
    ctx.set_env_image(UNIFORM)
    film, st = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=11, flags=flags))
    assert st.fp64 == (1 if world == "list" and not flags else 0)
    check_film(film, st, *oracle_ref(scene, world, nx, ny, spp, 11, 0))


@pytest.mark.parametrize("scene", ["textured", "plain"])
def test_uniform_image_path_fp64(ctx64, scene):
    nx, ny, spp = 96, 72, 32
    ctx64.upload(frt.HostScene.from_spec(SCENES[scene]("bvh"), nx / ny))
    ctx64.set_env_image(UNIFORM)
    film, st = ctx64.render(frt.RenderParams.make(nx, ny, spp, seed=11, flags=frt.FRT_FLAG_FP64))
    assert st.fp64 == 1
    check_film(film, st, *oracle_ref(scene, "bvh", nx, ny, spp, 11, 0))


@pytest.mark.parametrize("scene", ["textured", "plain"])
@pytest.mark.parametrize("integrator", [frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS])
def test_uniform_image_ao_normals(ctx, scene, integrator):
    nx, ny, spp = 64, 48, 16
    ctx.upload(frt.HostScene.from_spec(SCENES[scene]("bvh"), nx / ny))
    ctx.set_env_image(UNIFORM)
    film, st = ctx.render(frt.RenderParams.make(nx, ny, spp, seed=5, integrator=integrator))
    check_film(film, st, *oracle_ref(scene, "bvh", nx, ny, spp, 5, integrator))


@pytest.mark.parametrize("scene", ["textured", "plain"])
def test_uniform_image_pssmlt(ctx, scene):
    nx, ny, mpp, chains = 48, 48, 4, 2304
    spec = SCENES[scene]("bvh")
    ctx.upload(frt.HostScene.from_spec(spec, 1.0))
    ctx.set_env_image(UNIFORM)
    film = np.zeros((ny, nx, 3), np.float32)
    film, st = ctx.render(frt.RenderParams.pssmlt(nx, ny, mpp, chains, seed=4, bootstrap=2000), film)
    steps = mpp * nx * ny // chains
    osc = oracle.OracleScene.from_spec(spec, 1.0)
    osc.set_env(C)
    ref, b, cnt = osc.mlt_render(nx, ny, chains, steps, seed=4, n_init=2000)
    assert st.samples == chains * steps == cnt.samples
    assert abs(st.rays - cnt.rays) / cnt.rays < 5e-3
    assert np.isfinite(film).all()
    assert rmse(film, ref) <= 2e-3 * max(1.0, float(np.abs(ref).max()))


# ---- 2. direction map against the oracle hooks ----
ENV_NX, ENV_NY = 32, 16


@pytest.fixture(scope="module")
def direction():
    image = ES.random_env(ENV_NX, ENV_NY)
    exp = ES.direction_expectation(image)
    ES.check_direction_conditions(exp)      # conditions on the oracle side alone
    return image, exp


def render_direction(ctx, image, exp, integrator, flags=0, **kw):
    nx, ny = exp["nx"], exp["ny"]
    ctx.upload(frt.HostScene.from_spec(ES.direction_spec(), nx / ny))
    ctx.set_env_image(image)
    film, _ = ctx.render(frt.RenderParams.make(nx, ny, exp["spp"], seed=exp["seed"], integrator=integrator,
                                               flags=flags, **kw))
    return film


@pytest.mark.parametrize("integrator", [frt.FRT_INTEGRATOR_NORMALS, frt.FRT_INTEGRATOR_PATH])
def test_direction_map(ctx, direction, integrator):
    image, exp = direction
    film = render_direction(ctx, image, exp, integrator).reshape(-1, 3)
    print("missed", len(exp["miss"]), "tested", len(exp["tested"]), "of", exp["nx"] * exp["ny"])
    assert np.isfinite(film).all()
    np.testing.assert_allclose(film[exp["tested"]], exp["value"], rtol=1e-6, atol=0)


def test_direction_map_ao_camera_ray(ctx, direction):
    """ao::Li evaluates the environment with the camera ray (ao.cpp:27): hit
    pixels the oracle reports unoccluded hold the texel the camera ray points at."""
    image, exp = direction
    assert len(exp["ao_tested"]) > 0
    film = render_direction(ctx, image, exp, frt.FRT_INTEGRATOR_AO).reshape(-1, 3)
    print("ao tested", len(exp["ao_tested"]))
    np.testing.assert_allclose(film[exp["ao_tested"]], exp["ao_value"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(film[exp["tested"]], exp["value"], rtol=1e-6, atol=0)


def test_direction_map_srgb8(ctx):
    image = ES.random_env(ENV_NX, ENV_NY, srgb=True)
    exp = ES.direction_expectation(image)
    ES.check_direction_conditions(exp)
    film = render_direction(ctx, image, exp, frt.FRT_INTEGRATOR_NORMALS).reshape(-1, 3)
    np.testing.assert_allclose(film[exp["tested"]], exp["value"], rtol=1e-6, atol=0)


# ---- 3. poles ----
@pytest.mark.parametrize("up", [True, False])
def test_poles(ctx, ctx64, up):
    """Looking along +y (row 0 of the map) and -y (its last row) from outside the
    box with vfov 15: theta stays within 10.6 degrees of the pole, inside the
    11.25 degrees of one row of 16.  d.y rounds to +-1 (and an ulp beyond, in
    fp32) around the frame's centre: every pixel is finite and the pole's colour."""
    top, bottom = np.float32([3.0, 0.5, 0.25]), np.float32([0.125, 2.0, 1.5])
    image = ES.random_env(32, 16)
    image[0], image[15] = top, bottom
    cam = {"lookfrom": (0.0, 2.5, 0.0), "lookat": (0.0, 9.0, 0.0), "vup": (0.0, 0.0, -1.0), "vfov": 15.0,
           "aperture": 0.0, "focus": 10.0}
    if not up:
        cam = dict(cam, lookfrom=(0.0, -0.5, 0.0), lookat=(0.0, -9.0, 0.0))
    want = top if up else bottom
    hs = frt.HostScene.from_spec(ES.plain_cornell(cam=cam), 1.0)
    n = 32
    for c, integrator, flags in ((ctx, frt.FRT_INTEGRATOR_NORMALS, 0), (ctx, frt.FRT_INTEGRATOR_AO, 0),
                                 (ctx, frt.FRT_INTEGRATOR_PATH, frt.FRT_FLAG_FP32),
                                 (ctx64, frt.FRT_INTEGRATOR_PATH, frt.FRT_FLAG_FP64)):
        c.upload(hs)
        c.set_env_image(image)
        film, st = c.render(frt.RenderParams.make(n, n, 4, seed=2, integrator=integrator, flags=flags))
        assert st.fp64 == (1 if flags & frt.FRT_FLAG_FP64 else 0)
        assert st.rays == st.camera_rays == n * n * 4          # every sample missed
        assert np.isfinite(film).all()
        np.testing.assert_allclose(film.reshape(-1, 3), np.tile(want, (n * n, 1)), rtol=1e-6, atol=0)


# ---- 4. state and errors ----
def test_state_and_errors(ctx, direction):
    image, exp = direction
    nx, ny = exp["nx"], exp["ny"]
    hs = frt.HostScene.from_spec(ES.direction_spec(), nx / ny)
    hs.set_env((0.25, 0.5, 1.0))
    p = frt.RenderParams.make(nx, ny, 4, seed=3)
    fresh = frt.Context(0)
    try:
        fresh.upload(hs)
        base, st0 = fresh.render(p)
    finally:
        fresh.close()
    ctx.upload(hs)
    ctx.set_env_image(image)
    with_image, _ = ctx.render(p)
    assert not np.array_equal(with_image, base)
    ctx.upload(hs)                                   # the image survives a second upload
    again, _ = ctx.render(p)
    assert np.array_equal(again, with_image)
    for bad in (-0.25, np.nan, np.inf):              # refused with a message; the old image stays
        img = image.copy()
        img[3, 5, 2] = bad
        with pytest.raises(frt.FrtError, match=r"texel \(5, 3\)"):
            ctx.set_env_image(img)
    still, _ = ctx.render(p)
    assert np.array_equal(still, with_image)
    ctx.set_env_image(None)                          # back to env_color: a fresh context's film
    back, st1 = ctx.render(p)
    assert np.array_equal(back, base)
    assert (st1.waves_cap, st1.scene_in_lds, st1.stack_entries) == (st0.waves_cap, st0.scene_in_lds, st0.stack_entries)


def test_host_scene_forwards_env_image(ctx, direction):
    """upload(HostScene) with the spec key sets the image; a scene without one clears what upload set."""
    image, exp = direction
    nx, ny = exp["nx"], exp["ny"]
    p = frt.RenderParams.make(nx, ny, exp["spp"], seed=exp["seed"], integrator=frt.FRT_INTEGRATOR_NORMALS)
    ctx.set_env_image(None)
    ctx.upload(frt.HostScene.from_spec(dict(ES.direction_spec(), images=[{"data": image}], env_image=0), nx / ny))
    film, _ = ctx.render(p)
    np.testing.assert_allclose(film.reshape(-1, 3)[exp["tested"]], exp["value"], rtol=1e-6, atol=0)
    ctx.upload(frt.HostScene.from_spec(ES.direction_spec(), nx / ny))
    film, _ = ctx.render(p)
    assert (film.reshape(-1, 3)[exp["miss"]] == 0).all()        # the scene's constant (black) env again


# ---- 5. sharding ----
@pytest.mark.parametrize("integrator", [frt.FRT_INTEGRATOR_PATH, frt.FRT_INTEGRATOR_NORMALS])
def test_shards_assemble(ctx, direction, integrator):
    image, exp = direction
    whole = render_direction(ctx, image, exp, integrator)
    film = np.zeros_like(whole)
    for k in range(2):
        p = frt.RenderParams.make(exp["nx"], exp["ny"], exp["spp"], seed=exp["seed"], integrator=integrator,
                                  shard_index=k, shard_count=2)
        ctx.render(p, film)
    assert np.array_equal(film, whole)
