"""frtx_radiance_rays on the CPU: the host replay of the ray-list kernels (frtx_selftest_radiance_host,
ray_begin in path_begin's place), the camera's own rays as records (frtx_selftest_camera_rays_host),
the refusals of the entry points that need no device, and the numpy cameras.
(tests/test_gpu_rays.py runs the kernels.)"""
import ctypes

import numpy as np
import pytest

import env_sampling_specs as E
import env_specs as ES
import first_raytracer_amd as frt
from first_raytracer_amd import cameras

NX, NY = 48, 36
ALL = np.arange(NX * NY, dtype=np.int32)
LIGHT = (17.0, 12.0, 4.0)           # CornellBox-Original's light: Ke
ENV = (0.25, 0.5, 0.75)
UP = frt.ray_records([[0, 1, 0]], [[0, 1, 0]])        # from the middle of the box straight at the light
FRONT = frt.ray_records([[0, 1, 0]], [[0, 0, 1]])     # ... out through the open front


@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)


# ---- identity: the camera's rays through radiance_rays are the pixel replay, bit for bit ----
def scenes(cornell_obj, sphere_obj):
    return {"cornell": (lambda: frt.HostScene("cornell_box_obj", cornell_obj, NX / NY), None, 0, (NX, NY)),
            "sphere": (lambda: frt.HostScene("cornell_box_obj", sphere_obj, NX / NY), None, 0, (NX, NY)),
            "list_fp32": (lambda: frt.HostScene.from_spec(ES.plain_cornell(world="list"), NX / NY), None, frt.FRT_FLAG_FP32,
                          (NX, NY)),
            "sun_floor": (E.floor_scene, E.sun_image(), E.ON, (E.FLOOR_NX, E.FLOOR_NY))}


@pytest.mark.parametrize("name", ["cornell", "sphere", "list_fp32", "sun_floor"])
def test_identity_with_the_pixel_replay(name, cornell_obj, sphere_obj):
    make, img, base, (nx, ny) = scenes(cornell_obj, sphere_obj)[name]
    hs = make()
    px = np.arange(nx * ny, dtype=np.int32)
    for flags in (0, frt.FRT_FLAG_ROULETTE, frt.FRT_FLAG_SOBOL):
        for s in (0, 5):
            p = frt.RenderParams.make(nx, ny, 1, seed=17, sample_offset=s, flags=base | flags)
            rays = frt.selftest_camera_rays_host(hs, p, px)
            assert np.array_equal(rays.view(np.uint32)[:, 7], px.astype(np.uint32)) and (rays[:, 3] == np.finfo(np.float32).max).all()
            a, sa = frt.selftest_radiance_host(hs, p, rays, env_image=img)
            b, sb = frt.selftest_path_host(hs, p, px, env_image=img)
            assert a.tobytes() == b.tobytes(), (name, flags, s)
            assert (sa.camera_rays, sa.extension_rays, sa.shadow_rays, sa.samples, sa.pixels) == \
                   (sb.camera_rays, sb.extension_rays, sb.shadow_rays, sb.samples, sb.pixels)
            assert sa.fp64 == sb.fp64 == 0


def test_camera_rays_differ_between_samples_and_samplers(cornell):
    p = frt.RenderParams.make(NX, NY, 1, seed=17)
    a = frt.selftest_camera_rays_host(cornell, p, ALL[:64])
    b = frt.selftest_camera_rays_host(cornell, frt.RenderParams.make(NX, NY, 1, seed=17, sample_offset=5), ALL[:64])
    c = frt.selftest_camera_rays_host(cornell, frt.RenderParams.make(NX, NY, 1, seed=17, flags=frt.FRT_FLAG_SOBOL), ALL[:64])
    assert not np.array_equal(a[:, 4:7], b[:, 4:7]) and not np.array_equal(a[:, 4:7], c[:, 4:7])
    assert np.array_equal(a[:, 0:3], b[:, 0:3])                       # a pinhole: one origin


# ---- known answers ----
@pytest.mark.parametrize("spp", [1, 3, 7, 16])
@pytest.mark.parametrize("seed", [0, 12345])
def test_the_light_from_below_is_exact(cornell_obj, spp, seed):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    rgb, st = frt.selftest_radiance_host(hs, frt.RenderParams.make(1, 1, spp, seed=seed), UP)
    assert tuple(rgb[0]) == LIGHT
    assert st.camera_rays == st.samples == spp and st.pixels == 1 and st.extension_rays == st.shadow_rays == 0


def test_a_miss_and_a_short_first_segment_return_the_environment(cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    hs.set_env(ENV)
    p = frt.RenderParams.make(1, 1, 5, seed=2)
    assert tuple(frt.selftest_radiance_host(hs, p, FRONT)[0][0]) == ENV
    short = frt.ray_records([[0, 1, 0]], [[0, 1, 0]], t_max=0.5)      # the light is 0.98 away: the segment ends before it
    assert tuple(frt.selftest_radiance_host(hs, p, short)[0][0]) == ENV
    assert tuple(frt.selftest_radiance_host(hs, p, UP)[0][0]) == LIGHT


# ---- the lat-long convention: a probe of an environment image is that image ----
def test_latlong_round_trip(tmp_path):
    obj = tmp_path / "tri.obj"
    obj.write_text("v -0.5 -100 -0.5\nv 0.5 -100 -0.5\nv 0 -100 0.5\nf 1 2 3\n")
    spec = {"objects": [{"obj": str(obj), "bsdf": {"type": "lambertian", "albedo": (0.5, 0.5, 0.5)}, "geo": True}],
            "camera": ES.DIR_CAM, "world": "bvh"}
    hs = frt.HostScene.from_spec(spec, 1.0)
    img = np.random.default_rng(11).uniform(0.5, 4.0, (8, 16, 3)).astype(np.float32)
    rays = cameras.latlong((0.0, 0.0, 0.0), 16, 8)
    hits = frt.selftest_trace_host(hs, np.where(np.arange(8) == 7, 0.0, rays).astype(np.float32))   # word 7 = 0: closest hit
    hit = hits.view(np.int32)[:, 3] >= 0
    assert hit.sum() <= 2                                              # a condition of the fixture
    rgb, _ = frt.selftest_radiance_host(hs, frt.RenderParams.make(1, 1, 2, seed=4), rays, env_image=img)
    assert np.array_equal(rgb[~hit], img.reshape(-1, 3)[~hit])
    assert (~hit).sum() >= 126


# ---- the mean of the parts, and V ----
def chunk_sums(hs, rays, spp, spi, seed):
    """The chunk sums of a call, as the kernels cut it: one replay call per chunk."""
    n_chunks = (spp + spi - 1) // spi
    partial = np.zeros((n_chunks, len(rays), 3), np.float32)
    for c in range(n_chunks):
        n = min(spi, spp - c * spi)
        m, _ = frt.selftest_radiance_host(hs, frt.RenderParams.make(1, 1, n, seed=seed, sample_offset=c * spi), rays)
        partial[c] = m * np.float32(n)
    return partial


def test_mean_of_the_parts_and_variance(cornell):
    rng = np.random.default_rng(5)
    o = np.stack([rng.uniform(-0.8, 0.8, 12), rng.uniform(0.2, 1.6, 12), rng.uniform(-0.8, 0.8, 12)], axis=1)
    d = rng.normal(size=(12, 3))
    rays = np.concatenate([UP, frt.ray_records(o, d, streams=np.arange(1, 13))])
    a, st = frt.selftest_radiance_host(cornell, frt.RenderParams.make(1, 1, 7, seed=5, samples_per_item=3), rays)
    parts = [frt.selftest_radiance_host(cornell, frt.RenderParams.make(1, 1, n, seed=5, sample_offset=s), rays)[0]
             for s, n in ((0, 3), (3, 3), (6, 1))]
    mean = (3 * parts[0].astype(np.float64) + 3 * parts[1] + parts[2]) / 7
    assert np.allclose(a, mean, rtol=1e-5, atol=1e-7) and st.samples == 13 * 7
    v = frt.selftest_chunk_variance(chunk_sums(cornell, rays, 7, 3, 5), 7, 3)
    assert np.isfinite(v).all() and (v >= 0).all() and v[1:].max() > 0
    assert (v[0] == 0).all()                                           # the ray that only sees the light


# ---- refusals ----
def refused(match, code="invalid"):
    return pytest.raises(frt.FrtError, match=f"{code}.*{match}")


def test_refusals_of_the_list(cornell):
    p = frt.RenderParams.make(1, 1, 4)
    good = frt.ray_records([[0, 1, 0]] * 3, [[0, 1, 0]] * 3)

    def bad(word, value):
        r = good.copy()
        r[2, word] = value
        return r
    zero = good.copy()
    zero[1, 4:7] = 0
    with refused("entry 1 has a zero direction"):
        frt.selftest_radiance_host(cornell, p, zero)
    with refused("entry 2 has an origin or a direction that is not finite"):
        frt.selftest_radiance_host(cornell, p, bad(0, np.nan))
    with refused("entry 2 has an origin or a direction that is not finite"):
        frt.selftest_radiance_host(cornell, p, bad(5, np.inf))
    for t in (0.0, -1.0, np.inf, np.nan):
        with refused("entry 2 has a t_max that is not finite and > 0"):
            frt.selftest_radiance_host(cornell, p, bad(3, t))
    with refused(r"entry 2 has an origin with \|origin\| >= 1e8"):
        frt.selftest_radiance_host(cornell, p, bad(1, 1e8))
    frt.selftest_radiance_host(cornell, p, bad(1, 9.9e7))              # inside the domain
    nan_stream = good.copy()
    nan_stream.view(np.uint32)[:, 7] = 0x7fc00001                      # NaN bits in word 7: an id like any other
    rgb, _ = frt.selftest_radiance_host(cornell, p, nan_stream)
    assert (rgb == np.array(LIGHT, np.float32)).all()


def test_refusals_of_the_request(cornell):
    with refused("shard_count must be 1"):
        frt.selftest_radiance_host(cornell, frt.RenderParams.make(1, 1, 4, shard_count=2), UP)
    for k in (frt.FRT_INTEGRATOR_NORMALS, frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH):
        with refused("path and ao only", code="unsupported"):
            frt.selftest_radiance_host(cornell, frt.RenderParams.make(1, 1, 4, integrator=k), UP)
    for k in (frt.FRT_INTEGRATOR_DENOISE, frt.FRT_INTEGRATOR_ERROR):
        with refused("path and ao only"):
            frt.selftest_radiance_host(cornell, frt.RenderParams.make(1, 1, 4, integrator=k), UP)
    with refused("path and ao only"):
        frt.selftest_radiance_host(cornell, frt.RenderParams.pssmlt(1, 1, 2, 64), UP)
    frt.selftest_radiance_host(cornell, frt.RenderParams.make(1, 1, 4, integrator=frt.FRT_INTEGRATOR_AO), UP)


def test_entry_points_refuse_without_a_device():
    """What frtx_radiance_rays refuses before it looks at the context (NULL here), code and text."""
    L = frt.lib()
    assert all(n in frt.EXPORTS_X and hasattr(L, n) for n in
               ("frtx_radiance_rays", "frtx_radiance_rays_device", "frtx_camera_rays_device", "frtx_selftest_radiance_host",
                "frtx_selftest_camera_rays_host"))
    assert L.frt_get_abi_version() == 9
    out, var = np.full((2, 3), 7.0, np.float32), np.full((2, 3), 7.0, np.float32)

    def call(p, rays=np.concatenate([UP, FRONT]), v=None):
        rc = L.frtx_radiance_rays(None, ctypes.byref(p), rays.ctypes.data, len(rays), out.ctypes.data,
                                  v.ctypes.data if v is not None else None, None)
        return rc, L.frt_last_error(None).decode()
    ok = frt.RenderParams.make(1, 1, 8)
    assert call(ok) == (-1, "radiance_rays: null context")               # all is well but the context
    rc, text = call(ok, v=var)                                           # 8 spp: chunks of one sample, V is fine
    assert rc == -1 and "null context" in text
    rc, text = call(frt.RenderParams.make(1, 1, 8, samples_per_item=8), v=var)
    assert rc == -1 and "at least 2 chunks" in text and "samples_per_item" in text
    rc, text = call(frt.RenderParams.make(1, 1, 8, shard_count=2))
    assert rc == -1 and "shard_count must be 1" in text
    rc, text = call(frt.RenderParams.make(1, 1, 8, integrator=frt.FRT_INTEGRATOR_NORMALS))
    assert rc == -4 and "path and ao only" in text
    zero = UP.copy()
    zero[0, 4:7] = 0
    rc, text = call(ok, rays=zero)
    assert rc == -1 and "entry 0 has a zero direction" in text
    rc = L.frtx_radiance_rays_device(None, ctypes.byref(frt.RenderParams.make(1, 1, 8, integrator=frt.FRT_INTEGRATOR_DEPTH)), None, 3,
                                     None, None, None, None)
    assert rc == -4
    assert L.frtx_camera_rays_device(None, ctypes.byref(ok), None, 0, None, None) == -1
    assert (out == 7.0).all() and (var == 7.0).all()                     # nothing was written


def test_empty_list_writes_nothing(cornell):
    out = np.full(6, 7.0, np.float32)
    view = cornell.view()
    rc = frt.lib().frtx_selftest_radiance_host(ctypes.byref(view), ctypes.byref(frt.RenderParams.make(1, 1, 4)), None, 0, None,
                                               out.ctypes.data, None)
    assert rc == 0 and (out == 7.0).all()
    rgb, st = frt.selftest_radiance_host(cornell, frt.RenderParams.make(1, 1, 4), np.zeros((0, 8), np.float32))
    assert rgb.shape == (0, 3) and st.samples == 0


# ---- cameras.py ----
def test_cameras_latlong():
    r = cameras.latlong((1.0, 2.0, 3.0), 16, 8)
    assert r.shape == (128, 8) and r.dtype == np.float32
    assert np.array_equal(r.view(np.uint32)[:, 7], np.arange(128, dtype=np.uint32))
    assert (r[:, 0:3] == np.float32([1, 2, 3])).all() and (r[:, 3] == np.finfo(np.float32).max).all()
    d = cameras.latlong_directions(16, 8)
    assert np.allclose(np.linalg.norm(d, axis=-1), 1.0, atol=1e-12)
    assert np.allclose(np.linalg.norm(r[:, 4:7].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (d[0, :, 1] > 0.98).all() and (d[-1, :, 1] < -0.98).all()   # row 0 is the +y pole
    # column 0 starts at phi = 0 = the -z axis and turns towards +x
    assert d[4, 0, 2] < 0 < d[4, 0, 0] and d[4, 4, 0] > 0.9
    for nx, ny in ((16, 8), (64, 32), (7, 5)):
        assert abs(cameras.latlong_solid_angles(nx, ny).sum() - 4 * np.pi) <= 1e-6
    j = cameras.latlong((0, 0, 0), 16, 8, jitter=(0.25, 0.75))
    assert not np.array_equal(j[:, 4:7], r[:, 4:7])
    per = cameras.latlong((0, 0, 0), 16, 8, jitter=np.full((8, 16, 2), 0.5))
    assert np.array_equal(per[:, 4:7], r[:, 4:7])
    with pytest.raises(ValueError):
        cameras.latlong((0, 0, 0), 16, 8, jitter=(1.0, 0.0))


def test_cameras_orthographic():
    r = cameras.orthographic((0.0, 1.0, 5.0), (0, 0, -1), (0, 1, 0), 4.0, 2.0, 8, 4)
    o = r[:, 0:3].reshape(4, 8, 3)
    assert np.allclose(r[:, 4:7], (0, 0, -1))
    assert np.allclose(o[0, 0], (-2 + 0.25, 2 - 0.25, 5)) and np.allclose(o[-1, -1], (2 - 0.25, 0 + 0.25, 5))
    lo = cameras.orthographic((0.0, 1.0, 5.0), (0, 0, -1), (0, 1, 0), 4.0, 2.0, 8, 4, jitter=(0.0, 0.0))[:, 0:3]
    assert np.allclose(lo.min(axis=0), (-2, 0.5, 5)) and np.allclose(lo.max(axis=0), (1.5, 2, 5))
    with pytest.raises(ValueError):
        cameras.orthographic((0, 0, 0), (0, 1, 0), (0, 1, 0), 1, 1, 2, 2)


def test_cameras_fisheye():
    nx, ny = 32, 24
    r, outside = cameras.fisheye((0, 1, 0), (0, 0, -1), (0, 1, 0), 180.0, nx, ny)
    assert r.shape == (nx * ny, 8) and outside.shape == (nx * ny,) and outside.dtype == bool
    d = r[:, 4:7].astype(np.float64)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-6)
    x, y = np.meshgrid(np.arange(nx) + 0.5 - nx / 2, np.arange(ny) + 0.5 - ny / 2)
    rad = np.sqrt(x * x + y * y).reshape(-1) / (min(nx, ny) / 2)
    assert np.array_equal(outside, rad > 1.0) and 0 < outside.sum() < nx * ny
    # inside: the angle from forward is the radius times fov / 2
    ang = np.arccos(np.clip(-d[:, 2], -1, 1))
    assert np.allclose(ang[~outside], rad[~outside] * np.pi / 2, atol=1e-6)
    top = (ny // 2 - 6) * nx + nx // 2                                # above the centre: leans towards up
    assert d[top, 1] > 0 and abs(d[top, 0]) < 0.1
