"""The tree refinement pass (FRT_TREE_REFINE) on the GPU: a scene uploaded with
the pass off and on in one process gives the same films, ray counts, chain
states and hits on every plan that reads the LDS-resident binary tree -- the
pass moves interior nodes only (tests/test_tree_refine_host.py checks the tree)."""
import numpy as np
import pytest
import torch

import first_raytracer_amd as frt
import scene_specs as SS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene():
    hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                  "world": "list"}, 1.0)
    hs.build_bvh_sah()
    (_, off), (_, on) = frt.selftest_tree_refine(hs)
    assert off.tobytes() != on.tobytes()          # the pass does change this tree
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
        monkeypatch.setenv("FRT_TREE_REFINE", knob)
        ctx.upload(scene)
        out.append(run(ctx))
    return out


def same_render(a, b, lds=True):
    (fa, sa), (fb, sb) = a, b
    assert fa.max() > 0 and np.array_equal(fa, fb)
    assert sa.rays == sb.rays and sa.samples == sb.samples
    assert (sa.scene_in_lds, sa.waves_cap, sa.stack_entries, sa.bvh_depth) == \
        (sb.scene_in_lds, sb.waves_cap, sb.stack_entries, sb.bvh_depth)          # the same kernel and launch plan
    assert bool(sa.scene_in_lds) == lds


@pytest.mark.parametrize("integrator", [frt.FRT_INTEGRATOR_PATH, frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS])
@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_NO_OCT])
def test_films_and_rays_equal(ctx, scene, monkeypatch, integrator, flags):
    if integrator == frt.FRT_INTEGRATOR_AO:
        scene.set_env((1.0, 1.0, 1.0))
    p = frt.RenderParams.make(64, 64, 8, seed=3, flags=flags, integrator=integrator)
    try:
        same_render(*both(ctx, scene, monkeypatch, lambda c: c.render(p)))
    finally:
        scene.set_env((0.0, 0.0, 0.0))


def test_fp64_films_equal(ctx64, scene, monkeypatch):
    p = frt.RenderParams.make(64, 64, 8, seed=3, flags=frt.FRT_FLAG_FP64)
    a, b = both(ctx64, scene, monkeypatch, lambda c: c.render(p))
    assert a[1].fp64 and b[1].fp64
    same_render(a, b, lds=False)      # the fp64 kernel reads the same binary nodes from HBM


def test_pssmlt_chains_equal(ctx, scene, monkeypatch):
    def run(c):
        film = np.zeros((32, 32, 3), np.float32)
        film, st = c.render(frt.RenderParams.pssmlt(32, 32, 16, 256, seed=4, bootstrap=500), film)
        u, fp = c.mlt_chain_state(0, int(st.work_items))
        return film, st, u, fp
    (fa, sa, ua, pa), (fb, sb, ub, pb) = both(ctx, scene, monkeypatch, run)
    assert len(pa) == 256 and pa[:, 0].sum() > 0
    assert np.array_equal(pa, pb) and np.array_equal(ua, ub)
    same_render((fa, sa), (fb, sb))


def test_trace_device_hits_equal(ctx, scene, monkeypatch):
    n = 4096
    rng = np.random.default_rng(11)
    rays = np.zeros((n, 8), np.float32)
    rays[:, :3] = rng.uniform(-0.9, 0.9, (n, 3)) + np.array([0.0, 1.0, 0.0])
    rays[:, 4:7] = rng.normal(size=(n, 3))
    rays[:, 3] = 1e30
    rays[n // 2:, 3] = rng.uniform(0.2, 2.0, n - n // 2)
    rays[n // 2:, 7] = np.array([1], np.int32).view(np.float32)[0]     # any-hit queries
    d_rays = torch.from_numpy(rays).cuda()

    def run(c):
        hits = torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        c.trace_device(d_rays.data_ptr(), n, hits.data_ptr())
        torch.cuda.synchronize()
        return hits.cpu().numpy()
    a, b = both(ctx, scene, monkeypatch, run)
    prim = lambda h: h[:, 3].copy().view(np.int32)   # noqa: E731
    assert (prim(a)[: n // 2] >= 0).sum() > n // 4
    assert a[: n // 2].tobytes() == b[: n // 2].tobytes()                        # closest hits, bit for bit
    assert np.array_equal(prim(a)[n // 2:] >= 0, prim(b)[n // 2:] >= 0)          # occlusion
    assert 100 < (prim(a)[n // 2:] >= 0).sum() < n // 2 - 100
