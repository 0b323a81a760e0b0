"""frtx_render_pixels on the GPU (csrc/frt_render_sparse.hip): a list of pixels through the
sparse kernel against the full render of the same context and against the host replay of the
per-lane code; the shapes at which the list, the chunking and the reduce kernel can go wrong;
its V against the ERROR film; and the adaptive render_until above it, in Python and through
frt_render --adaptive.

Frames are 48 x 36 at 8 spp (the check_replay shape of the flag tests) unless said otherwise.
The gates are check_replay's: RMSE <= 1e-3 against the reference, equal sample counts, ray
counts within 2e-3."""
import subprocess

import numpy as np
import pytest

import env_sampling_specs as E
import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS
from test_error_host import bound
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu

NX, NY, SPP = 48, 36, 8
ALL = np.arange(NX * NY, dtype=np.int32)


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def upload(ctx, hs, img=None):
    ctx.upload(hs)
    ctx.set_env_image(img)


def check_pixels(ctx, hs, p, img=None, host_flags=0, full=True, pixels=ALL):
    """render_pixels of every pixel against the host replay and (full) the context's own render."""
    upload(ctx, hs, img)
    rgb, _, st = ctx.render_pixels(p, pixels, variance=False)
    q = frt.RenderParams.from_buffer_copy(p)
    q.flags |= host_flags
    ref, cnt = frt.selftest_path_host(hs, q, pixels, env_image=img)
    e = rmse(rgb, ref)
    print("vs host replay: rmse", e, "rays", st.rays, cnt.rays, "kernel ms", st.kernel_ms)
    assert e <= 1e-3
    assert st.samples == cnt.samples == len(pixels) * p.spp and abs(st.rays - cnt.rays) <= 2e-3 * cnt.rays
    assert st.pixels == len(pixels) and st.scene_in_lds == 0 and st.fp64 == cnt.fp64 and st.kernel_ms > 0
    if full:
        film, sf = ctx.render(p)
        e = rmse(rgb, film.reshape(-1, 3)[pixels])
        print("vs ctx.render: rmse", e, "rays", st.rays, sf.rays)
        assert e <= 1e-3 and st.samples == sf.samples
    return rgb, st


# ---- agreement ----
def test_agreement_cornell_default_plan(ctx, cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    _, st = check_pixels(ctx, hs, frt.RenderParams.make(NX, NY, SPP, seed=17))
    assert st.work_items == NX * NY * SPP       # spp / 16 < 1: chunks of one sample


def test_agreement_cornell_bvh2(ctx, cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    a, sa = check_pixels(ctx, hs, frt.RenderParams.make(NX, NY, SPP, seed=17, flags=frt.FRT_FLAG_BVH2))
    assert sa.stack_entries in (16, 32, 64)     # the binary ladder


def test_agreement_specular(ctx, sphere_obj):
    check_pixels(ctx, frt.HostScene("cornell_box_obj", sphere_obj, NX / NY), frt.RenderParams.make(NX, NY, SPP, seed=17))


def test_agreement_textured(ctx):
    check_pixels(ctx, frt.HostScene.from_spec(SS.cornell_textured(), NX / NY), frt.RenderParams.make(NX, NY, SPP, seed=17))


@pytest.mark.parametrize("flags,f64", [(frt.FRT_FLAG_FP32, 0), (0, 1)], ids=["fp32", "fp64"])
def test_list_world(ctx, flags, f64):
    hs = frt.HostScene.from_spec(ES.plain_cornell(world="list"), NX / NY)
    _, st = check_pixels(ctx, hs, frt.RenderParams.make(NX, NY, SPP, seed=17, flags=flags),
                         host_flags=frt.FRT_FLAG_FP64 if f64 else 0)
    assert st.fp64 == f64


@pytest.mark.parametrize("flag", [frt.FRT_FLAG_ROULETTE, frt.FRT_FLAG_SOBOL], ids=["roulette", "sobol"])
def test_estimator_flags(ctx, flag):
    hs = frt.HostScene.from_spec(ES.plain_cornell(), NX / NY)
    on, _ = check_pixels(ctx, hs, frt.RenderParams.make(NX, NY, SPP, seed=17, flags=flag))
    off, _, _ = ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, seed=17), ALL, variance=False)
    assert not np.array_equal(on, off)


def test_env_sampling_floor(ctx):
    pixels = np.arange(E.FLOOR_NX * E.FLOOR_NY, dtype=np.int32)
    _, st = check_pixels(ctx, E.floor_scene(), E.floor_params(E.ON), img=E.sun_image(), pixels=pixels)
    assert st.shadow_rays > 0


def test_ao(ctx, cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    hs.set_env((1.0, 0.75, 0.5))
    rgb, st = check_pixels(ctx, hs, frt.RenderParams.make(NX, NY, SPP, seed=17, integrator=frt.FRT_INTEGRATOR_AO))
    assert st.extension_rays == 0 and rgb.max() > 0


# ---- shapes that can go wrong: every entry is the all-pixels call's value, bit for bit ----
@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)


def reference(ctx, cornell, **kw):
    upload(ctx, cornell)
    p = frt.RenderParams.make(NX, NY, kw.pop("spp", SPP), seed=5, **kw)
    rgb, v, _ = ctx.render_pixels(p, ALL, variance=p.spp > 1)
    return p, rgb, v


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_list_lengths(ctx, cornell, n):
    p, rgb, v = reference(ctx, cornell)
    px = (np.arange(n, dtype=np.int32) * 37 + 11) % (NX * NY)          # scattered, distinct
    a, va, st = ctx.render_pixels(p, px)
    assert a.tobytes() == rgb[px].tobytes() and va.tobytes() == v[px].tobytes()
    assert st.samples == n * SPP and st.pixels == n and st.camera_rays == n * SPP


def test_empty_list(ctx, cornell):
    upload(ctx, cornell)
    rgb, v, st = ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, seed=5), np.zeros(0, np.int32))
    assert rgb.shape == (0, 3) and st.samples == 0 and st.rays == 0
    out = np.full(6, 7.0, np.float32)                                   # npix = 0 writes nothing
    rc = frt.lib().frtx_render_pixels(ctx.ptr, frt.RenderParams.make(NX, NY, SPP), None, 0, out.ctypes.data, None, None)
    assert rc == 0 and (out == 7.0).all()


def test_duplicates_and_reverse(ctx, cornell):
    p, rgb, v = reference(ctx, cornell)
    px = np.concatenate([ALL[::-1][:200], np.full(70, 123, np.int32), ALL[:5]]).astype(np.int32)
    a, va, st = ctx.render_pixels(p, px)
    assert a.tobytes() == rgb[px].tobytes() and va.tobytes() == v[px].tobytes() and st.samples == len(px) * SPP


def test_short_last_chunk(ctx, cornell):
    p, rgb, v = reference(ctx, cornell, spp=7, samples_per_item=3)
    px = np.array([0, 5, NX * NY - 1, 700, 701], np.int32)
    a, va, st = ctx.render_pixels(p, px)
    assert st.work_items == len(px) * 3
    assert a.tobytes() == rgb[px].tobytes() and va.tobytes() == v[px].tobytes()
    # the chunks are samples [0, 3), [3, 6), [6, 7): the mean is that of the three parts
    parts = [ctx.render_pixels(frt.RenderParams.make(NX, NY, n, seed=5, sample_offset=o), px, variance=False)[0]
             for o, n in ((0, 3), (3, 3), (6, 1))]
    mean = (3 * parts[0].astype(np.float64) + 3 * parts[1] + parts[2]) / 7
    assert np.allclose(a, mean, rtol=1e-5, atol=1e-7)


def test_sample_offset(ctx, cornell):
    p, rgb, v = reference(ctx, cornell, sample_offset=8)
    px = np.array([3, 1000, 64, 65], np.int32)
    a, va, _ = ctx.render_pixels(p, px)
    assert a.tobytes() == rgb[px].tobytes() and va.tobytes() == v[px].tobytes()
    film, _ = ctx.render(p)                                            # the full render's samples 8 .. 15
    first, _, _ = ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, seed=5), px, variance=False)
    assert rmse(a, film.reshape(-1, 3)[px]) <= 1e-3 and not np.array_equal(a, first)


# ---- refusals (with a context: the texts) ----
def test_refusals(ctx, cornell):
    upload(ctx, cornell)
    ok = frt.RenderParams.make(NX, NY, SPP, seed=1)
    for bad in ([-1], [NX * NY], [0, 5, NX * NY + 3]):
        with pytest.raises(frt.FrtError, match=r"invalid.*outside \[0, nx \* ny\)"):
            ctx.render_pixels(ok, np.array(bad, np.int32))
    with pytest.raises(frt.FrtError, match="invalid.*shard_count"):
        ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, shard_index=0, shard_count=2), ALL[:4])
    with pytest.raises(frt.FrtError, match="invalid.*samples_per_item"):
        ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, samples_per_item=SPP), ALL[:4])
    ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, samples_per_item=SPP), ALL[:4], variance=False)
    for k in (frt.FRT_INTEGRATOR_NORMALS, frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH):
        with pytest.raises(frt.FrtError, match="unsupported"):
            ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, integrator=k), ALL[:4])
    for k in (frt.FRT_INTEGRATOR_DENOISE, frt.FRT_INTEGRATOR_ERROR):
        with pytest.raises(frt.FrtError, match="invalid"):
            ctx.render_pixels(frt.RenderParams.make(NX, NY, SPP, integrator=k), ALL[:4])
    with pytest.raises(frt.FrtError, match="invalid"):
        ctx.render_pixels(frt.RenderParams.pssmlt(NX, NY, 2, 64), ALL[:4])


def test_device_call(ctx, cornell):
    import torch
    p, rgb, v = reference(ctx, cornell)
    px = torch.tensor([9, 8, 7, 1700], dtype=torch.int32, device="cuda")
    out = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    var = torch.zeros((4, 3), dtype=torch.float32, device="cuda")
    st = frt.Stats()
    rc = frt.lib().frtx_render_pixels_device(ctx.ptr, p, px.data_ptr(), 4, out.data_ptr(), var.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream, st)
    assert rc == 0 and st.samples == 4 * SPP
    idx = px.cpu().numpy()
    assert out.cpu().numpy().tobytes() == rgb[idx].tobytes() and var.cpu().numpy().tobytes() == v[idx].tobytes()
    bad = torch.tensor([9, NX * NY], dtype=torch.int32, device="cuda")
    assert frt.lib().frtx_render_pixels_device(ctx.ptr, p, bad.data_ptr(), 2, out.data_ptr(), None, None, None) == -1


# ---- V ----
def test_variance_against_error_film(ctx, cornell):
    upload(ctx, cornell)
    p = frt.RenderParams.make(NX, NY, 16, seed=9, samples_per_item=4)
    film, sf = ctx.render(p)
    vf, _ = ctx.render_error(p)
    assert sf.work_items == len(frt.shard_slots(p)) * 4                # the full render's spi is the one passed
    px = np.concatenate([ALL[::7], ALL[-3:]]).astype(np.int32)
    rgb, v, _ = ctx.render_pixels(p, px)
    want, m = vf.reshape(-1, 3)[px].astype(np.float64), film.reshape(-1, 3)[px].astype(np.float64)
    ratio = np.abs(v - want) / np.maximum(bound(want, m), 1e-300)
    print("worst |V - V_full| / bound", ratio.max(), "bit-equal", np.array_equal(v, vf.reshape(-1, 3)[px]))
    assert np.isfinite(v).all() and (v >= 0).all() and v.max() > 0
    assert (np.abs(v - want) <= bound(want, m)).all()
    # the sparse call used buffers of its own: the ERROR film still describes the full render
    again, _ = ctx.render_error(p)
    assert np.array_equal(again, vf)
    ctx.render_pixels(frt.RenderParams.make(NX, NY, 32, seed=1), ALL)  # more chunk sums than the render left
    assert np.array_equal(ctx.render_error(p)[0], vf)


# ---- the adaptive driver ----
def test_adaptive_render_until(ctx):
    """The floor under the sun at 64 x 48 with the image sampled.  The target sits 5 % below the e
    that the uniform driver reaches at 32 spp, so that driver pays the doubling to 64 spp for
    every pixel; the adaptive one stops the pixels whose own V is below tau^2 at 32 (their
    estimates scatter around the mean by about sqrt(2 / 15) with 16 chunks) and doubles the rest.
    In expectation both rules spend sum_i sigma_i^2 / tau^2 samples: the gain is the doubling
    granularity, per pixel instead of per frame."""
    nx, ny = 64, 48
    upload(ctx, frt.HostScene.from_spec(E.floor_spec(), nx / ny), E.sun_image())
    p = frt.RenderParams.make(nx, ny, 1, seed=3, flags=E.ON)
    run = lambda q: ctx.render(q)                                      # noqa: E731
    err = lambda q: ctx.render_error(q)[0]                             # noqa: E731
    probe = frt.render_until(run, err, p, 1e-9, 32)[5]
    assert [ps[0] for ps in probe] == [16, 32]
    target, cap = 0.95 * probe[1][1], 1 << 12
    _, _, spp, eu, oku, _ = frt.render_until(run, err, p, target, cap)
    film, v, counts, e, ok, passes = frt.render_until(run, err, p, target, cap, adaptive=True, switch=1.0, first_spp=16,
                                                      render_pixels=lambda q, px: ctx.render_pixels(q, px))
    print("adaptive passes", passes)
    print(f"target {target:.5f}: adaptive {int(counts.sum())} samples e {e:.5f}; uniform {spp} spp = {spp * nx * ny} samples e {eu:.5f}")
    assert oku and spp == 64
    assert ok and e <= target
    tau2 = (target * frt.frame_mean(film)) ** 2
    assert (v.astype(np.float64).reshape(-1, 3).mean(axis=1) <= tau2 * (1 + 1e-12)).all()
    assert any(ps[4] for ps in passes[1:]) and not passes[0][4] and passes[0][3] == nx * ny
    assert int(counts.sum()) < spp * nx * ny and passes[-1][0] == int(counts.sum())
    assert set(np.unique(counts)) <= {16 << k for k in range(9)} and len(np.unique(counts)) > 1
    f2, v2, c2, e2, ok2 = ctx.render_until(p, target, cap, adaptive=True, switch=1.0, first_spp=16)
    assert np.array_equal(f2, film) and np.array_equal(v2, v) and np.array_equal(c2, counts) and e2 == e and ok2
    # switch = 0: every pass is the full render, so the loop is the uniform one
    f3, v3, c3, e3, ok3 = ctx.render_until(p, target, cap, adaptive=True, switch=0.0, first_spp=16)
    assert (c3 == c3.flat[0]).all() and ok3
    with pytest.raises(frt.FrtError, match="SOBOL"):
        ctx.render_until(frt.RenderParams.make(nx, ny, 1, flags=frt.FRT_FLAG_SOBOL), target, cap, adaptive=True)


def test_adaptive_cli(ctx, cornell_obj, tmp_path):
    """frt_render --adaptive: frt::render_until's adaptive loop writes the binding's film, V and
    counts, bit for bit.  Cornell (the tool loads .obj scenes): the light's pixels have V = 0 and
    stop after pass 0; whether the 256-spp cap or the target ends the loop does not matter here."""
    nx, ny = 64, 48
    upload(ctx, frt.HostScene("cornell_box_obj", cornell_obj, nx / ny))
    film, v, counts, e, ok = ctx.render_until(frt.RenderParams.make(nx, ny, 1, seed=12), 0.3, 1 << 8, adaptive=True,
                                              switch=1.0, first_spp=16)
    assert len(np.unique(counts)) > 1 and counts.min() == 16
    out, vout, cout = (str(tmp_path / n) for n in ("f.pfm", "v.pfm", "c.pfm"))
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", f"{nx}x{ny}", "--seed", "12",
                        "--target-error", "0.3", "--max-spp", str(1 << 8), "--adaptive", "--switch", "1.0", "--first-spp", "16", "--out", out,
                        "--error-out", vout, "--counts-out", cout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    assert " sparse " in r.stdout and ("Converged" if ok else "Not converged") in r.stdout
    assert np.array_equal(read_pfm(out), film) and np.array_equal(read_pfm(vout), v)
    assert np.array_equal(read_pfm(cout)[..., 0], counts.astype(np.float32))
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--adaptive"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--adaptive goes with --target-error" in r.stderr
