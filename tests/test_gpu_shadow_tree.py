"""The shadow-tree pass (FRT_SHADOW_TREE) on the GPU: a scene uploaded with the pass off and on in one
process gives the same films, ray counts and chain states on every plan that reads the binary tree --
area-light shadow rays start at another root, and ask only whether a hit exists
(tests/test_shadow_tree_host.py checks what is dropped and the tree)."""
import os

import numpy as np
import pytest

import first_raytracer_amd as frt
import env_specs as ES
import scene_specs as SS
import shadow_tree_scenes as STS

pytestmark = pytest.mark.gpu
SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")


@pytest.fixture(scope="module")
def cornell():
    hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                  "world": "list"}, 1.0)
    hs.build_bvh_sah()
    info = frt.selftest_shadow_tree(hs)[0]
    assert info["why"] == 0 and info["nodes_added"] > 0      # the pass does change what is uploaded
    return hs


@pytest.fixture(scope="module")
def rooms(tmp_path_factory):
    return STS.scenes(str(tmp_path_factory.mktemp("rooms")))


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
        monkeypatch.setenv("FRT_SHADOW_TREE", knob)
        ctx.upload(scene)
        out.append(run(ctx))
    return out


def same_render(a, b):
    (fa, sa), (fb, sb) = a, b
    assert fa.max() > 0 and np.array_equal(fa, fb)
    assert sa.rays == sb.rays and sa.shadow_rays == sb.shadow_rays and sa.samples == sb.samples
    assert (sa.scene_in_lds, sa.waves_cap, sa.stack_entries, sa.bvh_depth) == \
        (sb.scene_in_lds, sb.waves_cap, sb.stack_entries, sb.bvh_depth)          # the same kernel and launch plan
    return sa


@pytest.mark.parametrize("flags,lds", [(0, True), (frt.FRT_FLAG_NO_OCT, True), (frt.FRT_FLAG_BVH2, None)])
def test_cornell_films_and_rays_equal(ctx, cornell, monkeypatch, flags, lds):
    p = frt.RenderParams.make(64, 64, 16, seed=3, flags=flags)
    st = same_render(*both(ctx, cornell, monkeypatch, lambda c: c.render(p)))
    assert st.shadow_rays > 0 and (lds is None or bool(st.scene_in_lds) == lds)
    if flags == 0:      # the octant plan did run: its LDS scene holds the eight node copies, the planar one one
        _, planar = ctx.render(frt.RenderParams.make(64, 64, 1, seed=3, flags=frt.FRT_FLAG_NO_OCT))
        assert planar.scene_in_lds and st.scene_bytes > planar.scene_bytes


@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_NO_OCT, frt.FRT_FLAG_BVH2])
def test_cornell_env_sampling_equal(ctx, cornell, monkeypatch, flags):
    """FRT_FLAG_ENV_SAMPLING under an image: a vertex traces an area-light shadow ray or an environment
    one, and only the first starts at the shadow root (Cornell's front is open: the other would leak)"""
    ctx.set_env_image(ES.random_env(16, 8))
    try:
        p = frt.RenderParams.make(64, 64, 16, seed=3, flags=flags | frt.FRT_FLAG_ENV_SAMPLING)
        st = same_render(*both(ctx, cornell, monkeypatch, lambda c: c.render(p)))
        assert st.shadow_rays > 0
    finally:
        ctx.set_env_image(None)


def test_cornell_fp64_films_equal(ctx64, cornell, monkeypatch):
    p = frt.RenderParams.make(64, 64, 16, seed=3, flags=frt.FRT_FLAG_FP64)
    a, b = both(ctx64, cornell, monkeypatch, lambda c: c.render(p))
    assert a[1].fp64 and b[1].fp64
    same_render(a, b)


@pytest.mark.parametrize("name", ["empty_room", "outside_camera"])
def test_rooms_equal(ctx, rooms, monkeypatch, name):
    p = frt.RenderParams.make(32, 32, 8, seed=5)
    st = same_render(*both(ctx, rooms[name][0].hs, monkeypatch, lambda c: c.render(p)))
    assert st.shadow_rays > 0


def test_pssmlt_chains_equal(ctx, cornell, monkeypatch):
    def run(c):
        film = np.zeros((64, 64, 3), np.float32)
        film, st = c.render(frt.RenderParams.pssmlt(64, 64, 16, 4096, seed=4, bootstrap=2000), film)
        u, fp = c.mlt_chain_state(0, int(st.work_items))
        return film, st, u, fp
    (fa, sa, ua, pa), (fb, sb, ub, pb) = both(ctx, cornell, monkeypatch, run)
    assert len(pa) == 4096 and pa[:, 0].sum() > 0
    assert np.array_equal(pa, pb) and np.array_equal(ua, ub)                     # chain fingerprints and states
    same_render((fa, sa), (fb, sb))


def test_cornell_sphere_pass_off(ctx, monkeypatch):
    hs = frt.HostScene("cornell_box_obj", os.path.join(SCENES, "CornellBox-Sphere.obj"), 1.0)
    assert frt.selftest_shadow_tree(hs)[0]["why"] != 0
    p = frt.RenderParams.make(64, 64, 8, seed=3)
    same_render(*both(ctx, hs, monkeypatch, lambda c: c.render(p)))
