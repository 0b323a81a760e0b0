"""frtx_radiance_rays / frtx_camera_rays_device on the GPU (csrc/frt_render_sparse.hip, the kernels
of source kSrcRays): the camera's own rays through the ray kernel against render_pixels of the same
pixels, bit for bit; seeded rays against the host replay; the list shapes; streams; the known
answers; the device entry; a lat-long probe, also through frt_render --camera latlong.

Frames are 48 x 36.  The replay gates are check_replay's: RMSE <= 1e-3, equal sample counts, ray
counts within 2e-3."""
import subprocess

import numpy as np
import pytest

import env_sampling_specs as E
import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS
from first_raytracer_amd import cameras
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu

NX, NY = 48, 36
ALL = np.arange(NX * NY, dtype=np.int32)
LIGHT = (17.0, 12.0, 4.0)
ENV = (0.25, 0.5, 0.75)
UP = frt.ray_records([[0, 1, 0]], [[0, 1, 0]])
FRONT = frt.ray_records([[0, 1, 0]], [[0, 0, 1]])


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)


def upload(ctx, hs, img=None):
    ctx.upload(hs)
    ctx.set_env_image(img)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def counters(st):
    return (st.camera_rays, st.extension_rays, st.shadow_rays, st.samples, st.pixels)


# ---- the kernel's main test: the camera's rays give the pixel list's bytes and counters ----
def check_identity(ctx, hs, img=None, flags=0, integrator=frt.FRT_INTEGRATOR_PATH, frame=(NX, NY)):
    upload(ctx, hs, img)
    nx, ny = frame
    px = np.arange(nx * ny, dtype=np.int32)
    for s in (0, 5):
        p = frt.RenderParams.make(nx, ny, 1, seed=17, sample_offset=s, flags=flags, integrator=integrator)
        rays = ctx.camera_rays(p, px)
        assert np.array_equal(rays.view(np.uint32)[:, 7], px.astype(np.uint32))
        a, _, sa = ctx.radiance_rays(p, rays, variance=False)
        b, _, sb = ctx.render_pixels(p, px, variance=False)
        print("sample", s, "rays", sa.rays, sb.rays, "kernel ms", sa.kernel_ms, sb.kernel_ms, "fp64", sa.fp64)
        assert a.tobytes() == b.tobytes()
        assert counters(sa) == counters(sb) and sa.camera_rays == sa.samples == nx * ny and sa.fp64 == sb.fp64 == 0
        assert sa.stack_entries == sb.stack_entries and sa.work_items == sb.work_items and sa.kernel_ms > 0
    return sa


def test_identity_cornell_default_plan(ctx, cornell):
    check_identity(ctx, cornell)


def test_identity_cornell_bvh2(ctx, cornell):
    assert check_identity(ctx, cornell, flags=frt.FRT_FLAG_BVH2).stack_entries in (16, 32, 64)


def test_identity_specular(ctx, sphere_obj):
    check_identity(ctx, frt.HostScene("cornell_box_obj", sphere_obj, NX / NY))


def test_identity_textured(ctx):
    check_identity(ctx, frt.HostScene.from_spec(SS.cornell_textured(), NX / NY))


def test_identity_list_world_fp32(ctx):
    check_identity(ctx, frt.HostScene.from_spec(ES.plain_cornell(world="list"), NX / NY), flags=frt.FRT_FLAG_FP32)


def test_identity_env_sampling_floor(ctx):
    st = check_identity(ctx, E.floor_scene(), img=E.sun_image(), flags=E.ON, frame=(E.FLOOR_NX, E.FLOOR_NY))
    assert st.shadow_rays > 0


@pytest.mark.parametrize("flag", [frt.FRT_FLAG_ROULETTE, frt.FRT_FLAG_SOBOL], ids=["roulette", "sobol"])
def test_identity_estimator_flags(ctx, flag):
    check_identity(ctx, frt.HostScene.from_spec(ES.plain_cornell(), NX / NY), flags=flag)


def test_identity_ao(ctx, cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    hs.set_env((1.0, 0.75, 0.5))
    st = check_identity(ctx, hs, integrator=frt.FRT_INTEGRATOR_AO)
    assert st.extension_rays == 0 and st.shadow_rays > 0


# ---- against the host replay ----
def seeded_rays(n=300, seed=9):
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-0.9, 0.9, n), rng.uniform(0.1, 1.8, n), rng.uniform(-0.9, 0.9, n)], axis=1)
    return frt.ray_records(o, rng.normal(size=(n, 3)))


@pytest.mark.parametrize("world,flags,f64", [("bvh", 0, 0), ("list", 0, 1)], ids=["bvh", "list_fp64"])
def test_against_the_host_replay(ctx, world, flags, f64):
    hs = frt.HostScene.from_spec(ES.plain_cornell(world=world), NX / NY)
    upload(ctx, hs)
    rays = seeded_rays()
    p = frt.RenderParams.make(1, 1, 8, seed=17, flags=flags)
    rgb, v, st = ctx.radiance_rays(p, rays)
    q = frt.RenderParams.from_buffer_copy(p)
    q.flags |= frt.FRT_FLAG_FP64 if f64 else 0
    ref, cnt = frt.selftest_radiance_host(hs, q, rays)
    e = rmse(rgb, ref)
    print("vs host replay: rmse", e, "rays", st.rays, cnt.rays, "kernel ms", st.kernel_ms, "fp64", st.fp64)
    assert st.fp64 == cnt.fp64 == f64
    assert e <= 1e-3
    assert st.samples == cnt.samples == len(rays) * 8 and abs(st.rays - cnt.rays) <= 2e-3 * cnt.rays
    assert st.camera_rays == len(rays) * 8 and st.pixels == len(rays) and st.scene_in_lds == 0
    assert np.isfinite(v).all() and (v >= 0).all() and rgb.max() > 0


# ---- list shapes: every entry is the all-rays call's value, bit for bit ----
@pytest.fixture(scope="module")
def reference(ctx, cornell):
    upload(ctx, cornell)
    p = frt.RenderParams.make(NX, NY, 8, seed=5)
    rays = ctx.camera_rays(p, ALL)
    rgb, v, _ = ctx.radiance_rays(p, rays)
    return p, rays, rgb, v


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_list_lengths(ctx, cornell, reference, n):
    p, rays, rgb, v = reference
    upload(ctx, cornell)
    idx = (np.arange(n) * 37 + 11) % (NX * NY)
    a, va, st = ctx.radiance_rays(p, rays[idx])
    assert a.tobytes() == rgb[idx].tobytes() and va.tobytes() == v[idx].tobytes()
    assert st.samples == st.camera_rays == n * 8 and st.pixels == n


def test_duplicates_and_reverse(ctx, cornell, reference):
    p, rays, rgb, v = reference
    upload(ctx, cornell)
    idx = np.concatenate([ALL[::-1][:200], np.full(70, 123), ALL[:5]])
    a, va, st = ctx.radiance_rays(p, rays[idx])
    assert a.tobytes() == rgb[idx].tobytes() and va.tobytes() == v[idx].tobytes() and st.samples == len(idx) * 8


def test_short_last_chunk(ctx, cornell, reference):
    _, rays, _, _ = reference
    upload(ctx, cornell)
    idx = np.array([0, 5, NX * NY - 1, 700, 701])
    a, va, st = ctx.radiance_rays(frt.RenderParams.make(1, 1, 7, seed=5, samples_per_item=3), rays[idx])
    assert st.work_items == len(idx) * 3 and np.isfinite(va).all() and (va >= 0).all()
    parts = [ctx.radiance_rays(frt.RenderParams.make(1, 1, n, seed=5, sample_offset=o), rays[idx], variance=False)[0]
             for o, n in ((0, 3), (3, 3), (6, 1))]
    mean = (3 * parts[0].astype(np.float64) + 3 * parts[1] + parts[2]) / 7
    assert np.allclose(a, mean, rtol=1e-5, atol=1e-7)


# ---- streams ----
def test_streams(ctx, cornell):
    upload(ctx, cornell)
    down = frt.ray_records([[0.3, 1.0, 0.2]] * 4, [[0.1, -1.0, 0.05]] * 4, streams=[7, 8, 7, 0x7fc00001])   # onto the floor
    rgb, _, _ = ctx.radiance_rays(frt.RenderParams.make(1, 1, 8, seed=3), down, variance=False)
    assert not np.array_equal(rgb[0], rgb[1]) and np.array_equal(rgb[0], rgb[2])
    assert np.isfinite(rgb).all() and not np.array_equal(rgb[3], rgb[0])   # NaN bits in word 7: an id like any other


# ---- known answers ----
@pytest.mark.parametrize("spp", [1, 7, 16])
def test_known_answers(ctx, cornell_obj, spp):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    hs.set_env(ENV)
    upload(ctx, hs)
    short = frt.ray_records([[0, 1, 0]], [[0, 1, 0]], t_max=0.5)
    rays = np.concatenate([UP, FRONT, short])
    rays.view(np.uint32)[:, 7] = (0, 1, 2)
    rgb, v, st = ctx.radiance_rays(frt.RenderParams.make(1, 1, spp, seed=spp, samples_per_item=max(1, spp // 3)), rays, variance=spp > 1)
    assert tuple(rgb[0]) == LIGHT and tuple(rgb[1]) == ENV and tuple(rgb[2]) == ENV
    assert st.extension_rays == st.shadow_rays == 0 and st.camera_rays == 3 * spp
    if spp > 1:
        assert (v == 0).all()


# ---- the device entry ----
def test_device_call(ctx, cornell, reference):
    import torch
    p, rays, rgb, v = reference
    upload(ctx, cornell)
    idx = np.array([9, 8, 7, 1700])
    r = torch.from_numpy(rays[idx].copy()).cuda()
    out = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    var = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    st = frt.Stats()
    stream = torch.cuda.current_stream().cuda_stream
    rc = frt.lib().frtx_radiance_rays_device(ctx.ptr, p, r.data_ptr(), 4, out.data_ptr(), var.data_ptr(), stream, st)
    assert rc == 0 and st.samples == 4 * 8
    assert out.cpu().numpy().tobytes() == rgb[idx].tobytes() and var.cpu().numpy().tobytes() == v[idx].tobytes()
    # the camera's rays straight from device memory: the Python method's records
    px = torch.tensor(idx, dtype=torch.int32, device="cuda")
    cam = torch.zeros((4, 8), dtype=torch.float32, device="cuda")
    assert frt.lib().frtx_camera_rays_device(ctx.ptr, p, px.data_ptr(), 4, cam.data_ptr(), stream) == 0
    assert cam.cpu().numpy().tobytes() == rays[idx].tobytes()
    bad_px = torch.tensor([9, NX * NY], dtype=torch.int32, device="cuda")
    assert frt.lib().frtx_camera_rays_device(ctx.ptr, p, bad_px.data_ptr(), 2, cam.data_ptr(), None) == -1
    # a bad entry in device memory: refused before any kernel runs, nothing written
    bad = rays[idx].copy()
    bad[2, 4:7] = 0
    out.fill_(7.0)
    bad_dev = torch.from_numpy(bad).cuda()
    rc = frt.lib().frtx_radiance_rays_device(ctx.ptr, p, bad_dev.data_ptr(), 4, out.data_ptr(), None, None, st)
    assert rc == -1 and "entry 2 has a zero direction" in frt.lib().frt_last_error(ctx.ptr).decode()
    assert (out.cpu().numpy() == 7.0).all() and st.samples == 0


def test_refusal_texts(ctx, cornell):
    upload(ctx, cornell)
    ok = frt.RenderParams.make(1, 1, 8)
    nan = UP.copy()
    nan[0, 1] = np.nan
    far = UP.copy()
    far[0, 0] = 2e8
    for rays, text in ((nan, "not finite"), (far, r"\|origin\| >= 1e8"),
                       (frt.ray_records([[0, 1, 0]], [[0, 1, 0]], t_max=0.0), "t_max")):
        with pytest.raises(frt.FrtError, match=f"invalid.*entry 0.*{text}"):
            ctx.radiance_rays(ok, rays)
    with pytest.raises(frt.FrtError, match="invalid.*shard_count"):
        ctx.radiance_rays(frt.RenderParams.make(1, 1, 8, shard_count=2), UP)
    with pytest.raises(frt.FrtError, match="invalid.*samples_per_item"):
        ctx.radiance_rays(frt.RenderParams.make(1, 1, 8, samples_per_item=8), UP)
    with pytest.raises(frt.FrtError, match="unsupported.*radiance_rays: path and ao only"):
        ctx.radiance_rays(frt.RenderParams.make(1, 1, 8, integrator=frt.FRT_INTEGRATOR_NORMALS), UP)
    rgb, v, st = ctx.radiance_rays(ok, np.zeros((0, 8), np.float32))
    assert rgb.shape == (0, 3) and st.samples == 0


def test_render_error_still_describes_the_last_render(ctx, cornell):
    upload(ctx, cornell)
    p = frt.RenderParams.make(NX, NY, 16, seed=9, samples_per_item=4)
    ctx.render(p)
    vf, _ = ctx.render_error(p)
    ctx.radiance_rays(frt.RenderParams.make(1, 1, 32, seed=1), seeded_rays(2000))   # more chunk sums than the render left
    assert np.array_equal(ctx.render_error(p)[0], vf)


# ---- a lat-long probe ----
def test_latlong_probe(ctx, cornell):
    upload(ctx, cornell)
    nx, ny = 64, 32
    d0 = cameras.latlong_directions(nx, ny)[0]
    assert (np.arccos(d0[:, 1]) <= np.pi / 32).all()                   # row 0 lies within pi / 32 of +y: inside the light's cone
    rgb, st = ctx.render_camera(frt.RenderParams.make(1, 1, 4, seed=2), lambda j: cameras.latlong((0.0, 1.0, 0.0), nx, ny, j))
    img = rgb.reshape(ny, nx, 3)
    assert (img[0] == np.array(LIGHT, np.float32)).all()
    assert np.isfinite(img).all() and (img >= 0).all() and st.samples == nx * ny * 4
    # two jittered passes: the same expectation, other rays; the light's row stays exact
    two, _ = ctx.render_camera(frt.RenderParams.make(1, 1, 4, seed=2), lambda j: cameras.latlong((0.0, 1.0, 0.0), nx, ny, j), passes=2)
    assert (two.reshape(ny, nx, 3)[0] == np.array(LIGHT, np.float32)).all() and not np.array_equal(two, rgb)
    assert abs(two.mean() - rgb.mean()) <= 0.25 * rgb.mean()


def test_latlong_probe_cli(cornell_obj, tmp_path):
    """The same probe through frt_render --camera latlong (--cam-origin 0,1,0: the Cornell camera itself stands
    outside the box, under a black environment): written upright, so the viewed top row -- the PFM's last --
    is the +y pole, the light."""
    out = str(tmp_path / "probe.pfm")
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--camera", "latlong", "--cam-origin", "0,1,0",
                        "--res", "64x32", "--ns", "4", "--seed", "2", "--out", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    assert "Lat-long probe from (0, 1, 0)" in r.stdout
    img = read_pfm(out)
    assert img.shape == (32, 64, 3) and np.isfinite(img).all() and (img >= 0).all()
    assert (img[-1] == np.array(LIGHT, np.float32)).all()              # the viewed top row
    assert not (img[0] == np.array(LIGHT, np.float32)).any()           # ... and the floor below
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--cam-passes", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "go with --camera" in r.stderr
