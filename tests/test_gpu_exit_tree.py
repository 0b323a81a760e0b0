"""The exit-tree pass (FRT_EXIT_TREE) on the GPU: a scene uploaded with the pass off and on in one process
gives the same films, ray counters and launch plan on every plan that reads the binary tree -- extension
rays start at another root and find the same closest hit (tests/test_exit_tree_host.py checks the drop
sets and the trees)."""
import os

import numpy as np
import pytest
import torch

import first_raytracer_amd as frt
import scene_specs as SS

pytestmark = pytest.mark.gpu
SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")


@pytest.fixture(scope="module")
def cornell():
    hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                  "world": "list"}, 1.0)
    hs.build_bvh_sah()
    info, roots = frt.selftest_exit_tree(hs, 1)[:2]
    assert info["why_name"] == "ran" and roots.any()         # the pass does change what is uploaded
    return hs


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


def both(ctx, scene, monkeypatch, run):
    """run(ctx) after an upload with the pass off, then on"""
    out = []
    for knob in ("0", "1"):
        monkeypatch.setenv("FRT_EXIT_TREE", knob)
        ctx.upload(scene)
        out.append(run(ctx))
    return out


def same_render(a, b):
    (fa, sa), (fb, sb) = a, b
    assert fa.max() > 0 and np.array_equal(fa, fb)
    assert (sa.rays, sa.camera_rays, sa.extension_rays, sa.shadow_rays, sa.samples) == \
        (sb.rays, sb.camera_rays, sb.extension_rays, sb.shadow_rays, sb.samples)
    assert (sa.scene_in_lds, sa.waves_cap, sa.stack_entries, sa.bvh_depth, sa.fp64) == \
        (sb.scene_in_lds, sb.waves_cap, sb.stack_entries, sb.bvh_depth, sb.fp64)    # the same kernel and launch plan
    return sa, sb


SIZES = [(64, 64, 16), (41, 23, 8)]          # the second: partial waves and edge tiles


@pytest.mark.parametrize("nx,ny,spp", SIZES)
@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_NO_OCT, frt.FRT_FLAG_BVH2, frt.FRT_FLAG_ROULETTE | frt.FRT_FLAG_SOBOL])
def test_cornell_films_and_rays_equal(ctx, cornell, monkeypatch, flags, nx, ny, spp):
    p = frt.RenderParams.make(nx, ny, spp, seed=3, flags=flags)
    sa, sb = same_render(*both(ctx, cornell, monkeypatch, lambda c: c.render(p)))
    assert sa.extension_rays > 0
    if flags == 0:
        assert sa.scene_in_lds and sb.scene_bytes > sa.scene_bytes      # the LDS plan ran, with the appended nodes


@pytest.mark.parametrize("nx,ny,spp", SIZES)
def test_cornell_fp64_films_equal(ctx64, cornell, monkeypatch, nx, ny, spp):
    p = frt.RenderParams.make(nx, ny, spp, seed=3, flags=frt.FRT_FLAG_FP64)
    a, b = both(ctx64, cornell, monkeypatch, lambda c: c.render(p))
    assert a[1].fp64 and b[1].fp64
    same_render(a, b)


@pytest.mark.parametrize("nx,ny,spp", SIZES)
def test_cornell_sphere_pass_off(ctx, monkeypatch, nx, ny, spp):
    hs = frt.HostScene("cornell_box_obj", os.path.join(SCENES, "CornellBox-Sphere.obj"), 1.0)
    assert frt.selftest_exit_tree(hs, 1)[0]["why"] != 0
    p = frt.RenderParams.make(nx, ny, spp, seed=3)
    sa, sb = same_render(*both(ctx, hs, monkeypatch, lambda c: c.render(p)))
    assert sa.scene_bytes == sb.scene_bytes


def test_render_pixels_equals_render(ctx, cornell, monkeypatch):
    """64 listed pixels through frtx_render_pixels (its kernel keeps the main root) against frt_render with the pass on"""
    monkeypatch.setenv("FRT_EXIT_TREE", "1")
    ctx.upload(cornell)
    p = frt.RenderParams.make(64, 64, 16, seed=3)
    pixels = np.random.default_rng(5).choice(64 * 64, 64, replace=False).astype(np.int32)
    rgb, _, st = ctx.render_pixels(p, pixels, variance=False)
    film, sf = ctx.render(p)
    # the pixel-list kernel sums a pixel's samples in one fp32 chain, the frame kernel per chunk: fp32 rounding apart
    assert np.abs(rgb - film.reshape(-1, 3)[pixels]).max() <= 1e-5 * max(1.0, float(film.max()))
    monkeypatch.setenv("FRT_EXIT_TREE", "0")
    ctx.upload(cornell)
    off, _, so = ctx.render_pixels(p, pixels, variance=False)
    assert np.array_equal(rgb, off) and st.rays == so.rays


def test_trace_device_hits_equal(ctx, cornell, monkeypatch):
    n = 4096
    rng = np.random.default_rng(11)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rng.uniform(-0.9, 0.9, (n, 3)) + np.array([0.0, 1.0, 0.0])
    rays[:, 4:7] = rng.normal(size=(n, 3))
    rays[:, 3] = 1e30
    d_rays = torch.from_numpy(rays).cuda()

    def run(c):
        hits = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        c.trace_device(d_rays.data_ptr(), n, hits.data_ptr())
        torch.cuda.synchronize()
        return hits.cpu().numpy()
    a, b = both(ctx, cornell, monkeypatch, run)
    assert (a[:, 3].copy().view(np.int32) >= 0).sum() > n // 2
    assert a.tobytes() == b.tobytes()                                    # closest hits, bit for bit


def test_pssmlt_chains_equal(ctx, cornell, monkeypatch):
    """PSS-MLT's extension rays keep the main root; the appended nodes and the root words must not reach it"""
    def run(c):
        film = np.zeros((64, 64, 3), np.float32)
        film, st = c.render(frt.RenderParams.pssmlt(64, 64, 16, 1024, seed=4, bootstrap=1000), film)
        u, fp = c.mlt_chain_state(0, int(st.work_items))
        return film, st, u, fp
    (fa, sa, ua, pa), (fb, sb, ub, pb) = both(ctx, cornell, monkeypatch, run)
    assert len(pa) == 1024 and pa[:, 0].sum() > 0
    assert np.array_equal(pa, pb) and np.array_equal(ua, ub) and np.array_equal(fa, fb)
