"""FRT_INTEGRATOR_ERROR on the GPU: the error film of the context's last render
(csrc/frt_error.hip) against the float64 formula on separately rendered chunks,
its layout, the record rules, its calibration against the converged golden
image, and the render-until-converged driver above it (Context.render_until,
frt_render --target-error).  test_error_host.py holds the formula and the bound.

The small frame is Cornell 40 x 24 with tile 32: two tiles, both with padding.  Its sizes are
multiples of 8, so validity changes only every 8 slots and every lane of film_error (four float
columns, at most two slots) is all valid or all padding; the 41 x 23 frame has lanes with one
valid and one padding slot, the kernel's third branch."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import first_raytracer_amd as frt
import golden_images as G
from test_error_host import bound, variance64
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERROR = frt.FRT_INTEGRATOR_ERROR
HBM = frt.FRT_FLAG_NO_LDS_SCENE
NX, NY = 40, 24


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)


@pytest.fixture(scope="module")
def calibration():
    """tools/error_calibration.py's CPU measurement: the windows of tests 9 to 11."""
    with open(os.path.join(ROOT, "profiles", "error", "calibration.json")) as f:
        c = json.load(f)
    for k in ("hash", "sobol"):
        assert c[k]["half_width"] <= 0.25 and c[k]["seeds"] >= 32
    return c


def rendered(ctx, p):
    """(film, V) of one render and the ERROR call after it."""
    film, _ = ctx.render(p)
    v, st = ctx.render_error(p)
    return film, v, st


# ---- 6. exactness against separate calls ----
CASES = [("lds", frt.FRT_INTEGRATOR_PATH, 0, 10, 4), ("hbm", frt.FRT_INTEGRATOR_PATH, HBM, 10, 4),
         ("hbm_bvh2", frt.FRT_INTEGRATOR_PATH, HBM | frt.FRT_FLAG_BVH2, 10, 4), ("ao", frt.FRT_INTEGRATOR_AO, 0, 10, 4),
         ("two_chunks", frt.FRT_INTEGRATOR_PATH, 0, 8, 4)]


def check_against_chunks(ctx, nx, ny, integrator, flags, spp, spi, lds=None, fp64=0):
    p = frt.RenderParams.make(nx, ny, spp, seed=21, flags=flags, integrator=integrator, samples_per_item=spi)
    film, st = ctx.render(p)
    v, se = ctx.render_error(p)
    assert st.work_items == len(frt.shard_slots(p)) * -(-spp // spi) and st.fp64 == fp64
    if lds is not None:
        assert st.scene_in_lds == lds
    chunks = []
    for first in range(0, spp, spi):
        n = min(spi, spp - first)            # 4, 4, 2: powers of two, so sum * (1 / n) is the exact chunk mean
        q = frt.RenderParams.make(nx, ny, n, seed=21, flags=flags, integrator=integrator, samples_per_item=n,
                                  sample_offset=first)
        chunks.append(ctx.render(q)[0])
    n = np.array([min(spi, spp - f) for f in range(0, spp, spi)], np.float64)[:, None, None, None]
    v64, m = variance64(np.array(chunks, np.float64) * n, spp, spi)
    ratio = np.abs(v - v64) / np.maximum(bound(v64, m), 1e-300)
    print(f"V: mean {v.mean():.4e} max {v.max():.4e}; worst |V - V64| / bound {ratio.max():.3f}; kernel {se.kernel_ms:.3f} ms")
    assert np.isfinite(v).all() and (v >= 0).all() and v.max() > 0
    assert (np.abs(v - v64) <= bound(v64, m)).all()
    assert np.allclose(film, m, rtol=1e-5, atol=1e-7)           # the same samples
    assert (se.camera_rays, se.extension_rays, se.shadow_rays, se.samples) == (0, 0, 0, 0)
    assert se.pixels == nx * ny == st.pixels and se.kernel_ms > 0


@pytest.mark.parametrize("name,integrator,flags,spp,spi", CASES, ids=[c[0] for c in CASES])
def test_exact_against_separate_calls(ctx, cornell, cornell_obj, name, integrator, flags, spp, spi):
    if integrator == frt.FRT_INTEGRATOR_AO:                  # under the scene's black environment every AO sample is 0
        cornell = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
        cornell.set_env((1.0, 1.0, 1.0))
    ctx.upload(cornell)
    ctx.set_env_image(None)
    check_against_chunks(ctx, NX, NY, integrator, flags, spp, spi, lds=0 if flags & HBM else 1)


def test_exact_against_separate_calls_fp64(ctx, veach_obj):
    ctx.upload(frt.HostScene("veach_mis", veach_obj, 24 / 16))
    ctx.set_env_image(None)
    check_against_chunks(ctx, 24, 16, frt.FRT_INTEGRATOR_PATH, frt.FRT_FLAG_FP64, 10, 4, fp64=1)


def mixed_lanes(slots):
    """Lanes of film_error (float columns 4 i .. 4 i + 3) whose two slots differ in validity."""
    valid = slots >= 0
    i = np.arange(len(slots) * 3 // 4)
    return int((valid[4 * i // 3] != valid[(4 * i + 3) // 3]).sum())


def test_exact_on_a_frame_with_mixed_lanes(ctx, cornell_obj):
    """41 x 23: validity changes from one slot to the next, so some lanes hold one valid and one
    padding slot and read the valid one float by float."""
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 41 / 23))
    ctx.set_env_image(None)
    assert mixed_lanes(frt.shard_slots(frt.RenderParams.make(41, 23, 10))) > 0
    assert mixed_lanes(frt.shard_slots(frt.RenderParams.make(NX, NY, 10))) == 0
    check_against_chunks(ctx, 41, 23, frt.FRT_INTEGRATOR_PATH, 0, 10, 4, lds=1)
    check_against_chunks(ctx, 41, 23, frt.FRT_INTEGRATOR_PATH, HBM, 8, 4, lds=0)


# ---- 7. layout ----
@pytest.mark.parametrize("nx,ny", [(NX, NY), (41, 23)])
def test_layout_slots_shards_and_multi(ctx, cornell_obj, nx, ny):
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, nx / ny))
    ctx.set_env_image(None)
    p = frt.RenderParams.make(nx, ny, 10, seed=4, samples_per_item=4)
    film, v, _ = rendered(ctx, p)
    slots = frt.shard_slots(p)
    valid = slots >= 0
    assert (~valid).any() and (mixed_lanes(slots) > 0) == (nx == 41)
    q = frt.RenderParams.from_buffer_copy(p)
    q.integrator = ERROR
    stream = torch.cuda.current_stream().cuda_stream
    # the film of the render in a device buffer of the caller's: the ERROR call leaves it alone
    fbuf = torch.full((len(slots) * 3,), float("nan"), dtype=torch.float32, device="cuda")
    ctx.render_device(p, fbuf.data_ptr(), stream)
    before = fbuf.cpu().numpy().copy()
    assert np.array_equal(before.reshape(-1, 3)[valid], film.reshape(-1, 3)[slots[valid]])
    for offset in (0, 1):                                    # a 16-byte aligned buffer, and one that is not
        buf = torch.full((len(slots) * 3 + 4,), float("nan"), dtype=torch.float32, device="cuda")
        view = buf[offset:]
        ctx.render_device(q, view.data_ptr(), stream)
        got = view[:len(slots) * 3].cpu().numpy().reshape(-1, 3)
        assert np.isnan(buf[:offset].cpu().numpy()).all() and np.isnan(buf[offset + len(slots) * 3:].cpu().numpy()).all()
        assert got[~valid].tobytes() == np.zeros_like(got[~valid]).tobytes()     # padding: exactly +0
        assert np.array_equal(got[valid], v.reshape(-1, 3)[slots[valid]])
    assert fbuf.cpu().numpy().tobytes() == before.tobytes()
    tiled = np.full_like(v, -1.0)
    for k in range(2):
        ps = frt.RenderParams.make(nx, ny, 10, seed=4, samples_per_item=4, shard_index=k, shard_count=2)
        ctx.render(ps)
        ps.integrator = ERROR
        ctx.render(ps, tiled)
    assert np.array_equal(tiled, v)
    fm, _ = frt.render_multi([ctx], p)
    vm, st = frt.render_multi([ctx], q)
    assert np.array_equal(fm, film) and np.array_equal(vm, v) and st.pixels == nx * ny and st.rays == 0


# ---- 8. the record ----
def test_record_rules(ctx, cornell, cornell_obj):
    fresh = frt.Context(0)
    try:
        fresh.upload(cornell)
        with pytest.raises(frt.FrtError, match="invalid.*no chunk sums"):
            fresh.render_error(frt.RenderParams.make(NX, NY, 8))
    finally:
        fresh.close()
    ctx.upload(cornell)
    ctx.set_env_image(None)
    p = frt.RenderParams.make(NX, NY, 8, seed=2, samples_per_item=4)
    film, _ = ctx.render(p)
    v, _ = ctx.render_error(p)
    for change in (dict(spp=16), dict(tile_size=16), dict(shard_index=1, shard_count=2), dict(nx=NX + 8)):
        q = frt.RenderParams.from_buffer_copy(p)
        for k, val in change.items():
            setattr(q, k, val)
        with pytest.raises(frt.FrtError, match="invalid.*must be those of the context's last render"):
            ctx.render_error(q)
    q = frt.RenderParams.make(NX, NY, 8, seed=99, max_depth=2, flags=HBM, samples_per_item=1)   # every other field is ignored
    v2, _ = ctx.render_error(q)                               # a refused call leaves the record; so does a call
    assert np.array_equal(v2, v)
    # a scene upload and a ray query do not touch the sums
    ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
    rays = torch.tensor([[0.0, 1.0, 3.0, 100.0, 0.0, 0.0, -1.0, 0.0]] * 64, dtype=torch.float32, device="cuda")
    hits = torch.zeros((64, 4), dtype=torch.float32, device="cuda")
    ctx.trace_device(rays.data_ptr(), 64, hits.data_ptr())
    assert np.array_equal(ctx.render_error(p)[0], v)
    # one chunk
    ctx.upload(cornell)
    one = frt.RenderParams.make(NX, NY, 8, seed=2, samples_per_item=8)
    ctx.render(one)
    with pytest.raises(frt.FrtError, match="invalid.*samples_per_item"):
        ctx.render_error(one)
    # a pssmlt render reuses the buffer
    ctx.render(p)
    ctx.render(frt.RenderParams.pssmlt(NX, NY, 2, 64, seed=1, bootstrap=100))
    with pytest.raises(frt.FrtError, match="invalid.*no chunk sums"):
        ctx.render_error(p)
    # a denoise call fills it with its feature passes
    ctx.render(p)
    ctx.denoise(np.maximum(film, 0), NX, NY, spp=8, seed=2)
    with pytest.raises(frt.FrtError, match="invalid.*no chunk sums"):
        ctx.render_error(p)
    # a failed render
    ctx.render(p)
    with pytest.raises(frt.FrtError):
        ctx.render(frt.RenderParams.make(NX, NY, 8, integrator=7))
    with pytest.raises(frt.FrtError, match="invalid.*no chunk sums"):
        ctx.render_error(p)
    # ... also one refused before it reaches the context's render step
    ctx.render(p)
    with pytest.raises(frt.FrtError, match="whole frame"):
        frt.render_multi([ctx], frt.RenderParams.make(NX, NY, 8, seed=2, shard_index=1, shard_count=2))
    with pytest.raises(frt.FrtError, match="invalid.*no chunk sums"):
        ctx.render_error(p)
    # ... and the context renders on
    ctx.render(p)
    assert np.array_equal(ctx.render_error(p)[0], v)


def test_other_integrators_leave_sums(ctx, cornell):
    ctx.upload(cornell)
    ctx.set_env_image(None)
    for integrator in (frt.FRT_INTEGRATOR_NORMALS, frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH):
        p = frt.RenderParams.make(NX, NY, 8, seed=3, integrator=integrator, samples_per_item=2)
        _, v, _ = rendered(ctx, p)
        assert np.isfinite(v).all() and (v >= 0).all() and v.max() > 0


# ---- 9., 10. calibration against the converged image ----
@pytest.fixture(scope="module")
def cornell64(ctx, cornell_obj):
    def upload():
        ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 1.0))
        ctx.set_env_image(None)
    return upload


def test_calibration_hash_stream(ctx, cornell64, calibration):
    """sum of mean V over sum of the mean squared error against the golden image, 16 spp in 16
    chunks of one sample (what the library picks for this frame by itself), seeds 2000 ...; the
    window 1 +- 4 sd / sqrt(S) is the CPU tool's (profiles/error/calibration.json)."""
    cornell64()
    c = calibration["hash"]
    g = G.cornell64()
    sv = se = 0.0
    for seed in range(2000, 2000 + c["test_seeds"]):
        film, v, _ = rendered(ctx, frt.RenderParams.make(64, 64, 16, seed=seed, samples_per_item=1))
        sv += v.astype(np.float64).mean()
        se += ((film - g) ** 2).mean()
    print(f"sum mean V / sum MSE = {sv / se:.4f}, window 1 +- {c['half_width']:.4f} (S = {c['test_seeds']})")
    assert abs(sv / se - 1.0) <= c["half_width"]


def test_calibration_sobol(ctx, cornell64, calibration):
    """FRT_FLAG_SOBOL, 64 spp: the ERROR film is an upper estimate of the error of the
    stratified render; the replicate V of render_until (4 x 16 spp) is calibrated."""
    cornell64()
    g = G.cornell64()
    SB = frt.FRT_FLAG_SOBOL
    sv = se = 0.0
    for seed in range(2000, 2008):
        film, v, _ = rendered(ctx, frt.RenderParams.make(64, 64, 64, seed=seed, flags=SB, samples_per_item=1))
        sv += v.astype(np.float64).mean()
        se += ((film - g) ** 2).mean()
    print(f"ERROR film under Sobol': sum mean V / sum MSE = {sv / se:.4f} (CPU: "
          f"{calibration['sobol_error_film']['ratio_of_sums']:.4f})")
    assert sv > se
    c = calibration["sobol"]
    sv = se = 0.0
    for k in range(c["test_seeds"]):
        film, v, spp, e, ok = ctx.render_until(frt.RenderParams.make(64, 64, 1, seed=2000 + 4 * k, flags=SB), 1e-9, 64)
        assert spp == 64 and not ok
        sv += v.astype(np.float64).mean()
        se += ((film - g) ** 2).mean()
    print(f"replicates: sum mean V / sum MSE = {sv / se:.4f}, window 1 +- {c['half_width']:.4f} (S = {c['test_seeds']})")
    assert abs(sv / se - 1.0) <= c["half_width"]


# ---- 11. the driver ----
TARGET = 0.25      # a third of the 16-spp figure of this frame (e about 0.75): nine times the samples, so 256 spp


def test_render_until(ctx, cornell64, calibration, cornell_obj, tmp_path):
    cornell64()
    g = G.cornell64()
    p = frt.RenderParams.make(64, 64, 1, seed=31)
    film, v, spp, e, ok = ctx.render_until(p, TARGET, 1 << 14)
    print(f"target {TARGET}: {spp} spp, e {e:.4f}")
    assert ok and e <= TARGET and spp >= 16 and spp & (spp - 1) == 0
    assert e == frt.frame_error(film, v)
    rmse = float(np.sqrt(((film - g) ** 2).mean()))
    print(f"rmse {rmse:.5f}, predicted {e * film.mean():.5f}, allowed {TARGET * film.mean() * (1 + calibration['hash']['half_width']):.5f}")
    assert rmse <= TARGET * float(film.astype(np.float64).mean()) * (1 + calibration["hash"]["half_width"])
    _, _, spp2, e2, ok2 = ctx.render_until(p, 2 * TARGET, 1 << 14)
    assert ok2 and e2 <= 2 * TARGET and spp2 <= spp
    _, _, spp3, e3, ok3 = ctx.render_until(p, 1e-9, 32)
    assert not ok3 and spp3 == 32 and e3 > 1e-9
    # the doubling passes by hand
    acc, vacc, total = None, None, 0
    while total < spp:
        n = 16 if total == 0 else total
        q = frt.RenderParams.make(64, 64, n, seed=31, sample_offset=total)
        f, _ = ctx.render(q)
        vp, _ = ctx.render_error(q)
        acc = f if total == 0 else frt.film_accumulate(acc, total, f, n)
        vacc = vp if total == 0 else frt.combine_variance(total, vacc, n, vp)
        total += n
    assert total == spp and np.array_equal(acc, film) and np.array_equal(vacc, v)
    # the command-line tool: the same two films
    out, vout = str(tmp_path / "f.pfm"), str(tmp_path / "v.pfm")
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x64", "--seed", "31",
                        "--target-error", str(TARGET), "--max-spp", str(1 << 14), "--out", out, "--error-out", vout],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    print(r.stdout)
    assert r.stdout.count("pass: ") == len(bin(spp // 16)) - 2 and f"Converged after {spp} spp" in r.stdout
    assert np.array_equal(read_pfm(out), film) and np.array_equal(read_pfm(vout), v)


def test_cli_sobol_replicates(ctx, cornell64, cornell_obj, tmp_path):
    """frt_render --sobol --target-error: the four-replicate loop of frt::render_until gives the
    binding's mean film and replicate V, bit for bit."""
    cornell64()
    film, v, spp, e, ok = ctx.render_until(frt.RenderParams.make(64, 64, 1, seed=8, flags=frt.FRT_FLAG_SOBOL), 1e-9, 128)
    assert spp == 128 and not ok
    out, vout = str(tmp_path / "f.pfm"), str(tmp_path / "v.pfm")
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x64", "--seed", "8", "--sobol",
                        "--target-error", "1e-9", "--max-spp", "128", "--out", out, "--error-out", vout],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.count("pass: ") == 2 and "Not converged after 128 spp" in r.stdout
    assert np.array_equal(read_pfm(out), film) and np.array_equal(read_pfm(vout), v)


def test_cli_error_out(cornell_obj, tmp_path):
    """frt_render --error-out: the V film of the render it has just done (path_gpu::error)."""
    out, vout = str(tmp_path / "f.pfm"), str(tmp_path / "v.pfm")
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "40x24", "--ns", "16", "--seed", "3",
                        "--out", out, "--error-out", vout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "e = sqrt(mean V) / mean film" in r.stdout
    c = frt.Context(0)
    try:
        c.upload(frt.HostScene("cornell_box_obj", cornell_obj, 40 / 24))
        film, v, _ = rendered(c, frt.RenderParams.make(40, 24, 16, seed=3))
    finally:
        c.close()
    assert np.array_equal(read_pfm(out), film) and np.array_equal(read_pfm(vout), v)
    base = [CLI, "--scene", "cornell", "--obj", cornell_obj]
    for extra, word in ((["--integrator", "normals", "--error-out", vout], "--error-out"),
                        (["--target-error", "0", "--max-spp", "64"], "--target-error must be > 0"),
                        (["--target-error", "0.1"], "needs --max-spp"),
                        (["--max-spp", "64"], "go with --target-error"),
                        (["--first-spp", "8"], "go with --target-error")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and word in r.stderr, (extra, r.stderr)
