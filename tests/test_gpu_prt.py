"""Precomputed radiance transfer on the GPU (csrc/frt_prt.hip): frtx_prt_transfer against its host
replay, bit for bit, on every rung of its dispatch -- the list world, the binary tree at stacks 16,
32 and 64, the 4-wide tree --, at direction counts below one chunk and with a chunk tail, over a full
and a partial wave of corners, one triangle, and forced-small batches; the device entry; frtx_prt_rays
against its replay for a frame of camera rays with misses into an environment image and a directly
seen emitter; relighting one transfer under two images, through render_prt.  The replay itself is
held to independent fp64 sums in test_prt_host.py; the CLI against render_prt.

Gather and shade take the hit's (u, v) from csrc/frt_prt.hpp prt_bary, exactly rounded on both sides: the
traversal's own pass through the device's approximate reciprocal and are an ulp off the host's."""
import os
import subprocess

import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu

NX, NY = 48, 36
ALL = np.arange(NX * NY, dtype=np.int32)
DIRS = {n: frt.prt_sample_dirs(n, seed=11) for n in (7, 13)}          # 49: below a chunk; 169: two chunks and a tail
LIST, BVH16, BVH32, BVH64, WIDE = "list", "bvh16", "bvh32", "bvh64", "wide"


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)


def rung_of(st):
    """The rung a call's stats name (csrc/frt_prt.hip prt_plan)."""
    assert st.scene_in_lds == 0 and st.waves_cap == 0 and st.fp64 == 0
    r = {0: LIST, 12: WIDE, 16: BVH16, 32: BVH32, 64: BVH64}[st.stack_entries]
    assert r in (LIST, WIDE) or st.bvh_depth < st.stack_entries
    return r


def check_transfer(ctx, scene, rung, flags=0, sqrt_ns=(7, 13), bounces=(0, 2), budget=None):
    ctx.upload(scene if isinstance(scene, frt.HostScene) else scene.view())
    n_corners = 3 * int(frt._view(scene).n_tris)
    for sq in sqrt_ns:
        for b in bounces:
            T, st = ctx.prt_transfer(scene, DIRS[sq], b, flags, budget=budget)
            want = frt.selftest_prt_transfer_host(scene, DIRS[sq], b, flags)
            print(rung, "dirs", sq * sq, "bounces", b, "shadow rays", st.shadow_rays, "gathers", st.extension_rays, "kernel ms",
                  round(st.kernel_ms, 3), "stack", st.stack_entries, "depth", st.bvh_depth)
            assert rung_of(st) == rung or rung is None                     # None: whatever rung the mesh's trees give
            assert T.tobytes() == want.tobytes(), np.argwhere(T != want)[:5]
            assert np.isfinite(T).all() and T.any()
            unshadowed = bool(flags & frt.FRTX_PRT_UNSHADOWED)
            assert (st.shadow_rays == 0) == unshadowed and st.shadow_rays <= n_corners * sq * sq
            assert (st.extension_rays > 0) == (b > 0)
            assert st.kernel_ms > 0


class TreeView:
    """A scene's view with a tree of this test's making over its triangles: `chain` levels that split one
    triangle off, then halves -- as deep as a rung needs.  Boxes are the triangles' bounds."""

    def __init__(self, scene, chain):
        self.scene = scene
        v = scene.arrays()["tri_v"].reshape(-1, 3, 3)
        lo, hi = v.min(axis=1) - 1e-6, v.max(axis=1) + 1e-6
        boxes, children = [], []

        def build(prims, chain):
            if len(prims) == 1:
                return ~int(prims[0])
            me = len(boxes)
            boxes.append(np.concatenate([lo[prims].min(axis=0), hi[prims].max(axis=0)]))
            children.append(None)
            cut = 1 if chain > 0 else len(prims) // 2
            children[me] = (build(prims[:cut], 0), build(prims[cut:], chain - 1))
            return me
        self.root = build(np.arange(len(v)), chain)
        self.box = np.ascontiguousarray(boxes, np.float64)
        self.child = np.ascontiguousarray(children, np.int32)

    def view(self):
        w = self.scene.view()
        w.world_kind, w.n_nodes, w.root = frt.FRT_WORLD_BVH, len(self.box), self.root
        w.node_box, w.node_child = self.box.ctypes.data, self.child.ctypes.data
        return w


# ---- the transfer on every rung ----
def plain(cornell_obj, sphere_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)


def deep(chain):
    return lambda cornell_obj, sphere_obj: TreeView(frt.HostScene("cornell_box_obj", cornell_obj, NX / NY), chain)


# (scene, flags, the rung it must run on, direction sets, bounces)
RUNG_CASES = {
    "cornell_default": (plain, 0, WIDE, (7, 13), (0, 2)),                    # 108 corners: a full and a partial wave
    "cornell_no_lds_flag": (plain, frt.FRT_FLAG_NO_LDS_SCENE, WIDE, (13,), (1,)),   # no other rung: HBM anyway
    "cornell_bvh2": (plain, frt.FRT_FLAG_BVH2, BVH16, (7, 13), (0, 2)),
    "chain18_bvh2": (deep(18), frt.FRT_FLAG_BVH2, BVH32, (13,), (0, 2)),
    "chain35_bvh2": (deep(35), frt.FRT_FLAG_BVH2, BVH64, (13,), (0, 2)),
    "list_world": (lambda c, s: frt.HostScene.from_spec(ES.plain_cornell(world="list"), NX / NY), 0, LIST, (7, 13), (0, 2)),
    "spheres_checker": (lambda c, s: frt.HostScene.from_spec(SS.cornell_textured(), NX / NY), 0, WIDE, (7, 13), (0, 2)),
    "spheres_checker_bvh2": (lambda c, s: frt.HostScene.from_spec(SS.cornell_textured(), NX / NY), frt.FRT_FLAG_BVH2, BVH16, (13,), (0, 2)),
    # vertex normals: the gather's side test interpolates and normalises them
    "smooth_mesh": (lambda c, s: frt.HostScene("obj_smooth", s, NX / NY), 0, None, (7,), (1,)),
    "smooth_mesh_bvh2": (lambda c, s: frt.HostScene("obj_smooth", s, NX / NY), frt.FRT_FLAG_BVH2, None, (7,), (1,)),
}


@pytest.mark.parametrize("case", list(RUNG_CASES))
def test_transfer_on_its_rung(ctx, cornell_obj, sphere_obj, case):
    make, flags, rung, sqrt_ns, bounces = RUNG_CASES[case]
    check_transfer(ctx, make(cornell_obj, sphere_obj), rung, flags=flags, sqrt_ns=sqrt_ns, bounces=bounces)


def test_the_cases_name_every_rung():
    assert {c[2] for c in RUNG_CASES.values()} - {None} == {LIST, BVH16, BVH32, BVH64, WIDE}


def test_transfer_tessellated_cornell(ctx, cornell_obj, tmp_path):
    obj = str(tmp_path / "k6.obj")
    frt.write_tessellated_obj(cornell_obj, 6, obj)                           # 1,226 triangles
    scene = frt.HostScene("cornell_box_obj", obj, NX / NY)
    check_transfer(ctx, scene, WIDE, sqrt_ns=(13,))
    check_transfer(ctx, scene, WIDE, sqrt_ns=(7,), bounces=(1,), budget=1)   # 58 batches of 64 corners


def test_transfer_one_triangle(ctx, tmp_path):
    obj = tmp_path / "one.obj"
    obj.write_text("v -1 0 1\nv 1 0 1\nv 0 0 -1\nf 1 2 3\n")
    spec = {"objects": [{"obj": str(obj), "bsdf": {"type": "lambertian", "albedo": (0.5, 0.25, 1.0)}, "geo": True}],
            "camera": SS.CORNELL_CAM, "world": "bvh"}
    scene = frt.HostScene.from_spec(spec, NX / NY)
    ctx.upload(scene)
    for b in (0, 2):
        T, st = ctx.prt_transfer(scene, DIRS[13], b)
        assert T.shape == (1, 3, 25, 3) and T.tobytes() == frt.selftest_prt_transfer_host(scene, DIRS[13], b).tobytes()
        assert st.shadow_rays == 3 * int((DIRS[13][:, 1] > 0).sum())        # nothing to hit, every upward ray is traced
    assert abs(T[0, 0, 0, 0] - 0.5 * 0.28209479) < 0.02                     # rho / pi A_0 Y_00, A_0 = pi


def test_transfer_unshadowed_and_small_batches(ctx, cornell):
    check_transfer(ctx, cornell, WIDE, flags=frt.FRTX_PRT_UNSHADOWED, sqrt_ns=(13,), bounces=(0, 1))
    check_transfer(ctx, cornell, WIDE, sqrt_ns=(13,), budget=1)              # two batches: 64 and 44 corners


def test_transfer_device_entry(ctx, cornell):
    ctx.upload(cornell)
    T, st = ctx.prt_transfer(cornell, DIRS[13], 2)
    Td, sd = ctx.prt_transfer_device(cornell, DIRS[13], 2)
    assert Td.cpu().numpy().tobytes() == T.tobytes()
    assert (sd.shadow_rays, sd.extension_rays, sd.stack_entries) == (st.shadow_rays, st.extension_rays, st.stack_entries)


def test_refusals(ctx, cornell):
    fresh = frt.Context(0)
    try:
        with pytest.raises(frt.FrtError, match="no scene"):
            fresh.prt_transfer(cornell, DIRS[7])
        with pytest.raises(frt.FrtError, match="no scene"):
            fresh.prt_rays(np.zeros((36, 3, 25, 3), np.float32), np.zeros((25, 3)), frt.ray_records([[0, 1, 0]], [[0, 0, -1]]))
    finally:
        fresh.close()
    ctx.upload(cornell)
    bad = DIRS[7].copy()
    bad[4] = 0.0
    for kw, text in ((dict(dirs=np.zeros((0, 3))), "n_dirs"), (dict(dirs=DIRS[7], bounces=17), "bounces"),
                     (dict(dirs=DIRS[7], flags=frt.FRT_FLAG_SOBOL), "unknown flags"), (dict(dirs=bad), "direction 4")):
        with pytest.raises(frt.FrtError, match=text):
            ctx.prt_transfer(cornell, **kw)
    with pytest.raises(frt.FrtError, match="triangle count"):
        ctx.prt_transfer(frt.HostScene.from_spec(SS.cornell_textured(), NX / NY), DIRS[7])
    with pytest.raises(frt.FrtError, match="entry 1"):
        ctx.prt_rays(np.zeros((36, 3, 25, 3), np.float32), np.zeros((25, 3)), frt.ray_records([[0, 1, 0]] * 2, [[0, 0, -1], [0, 0, 0]]))
    rgb, st = ctx.prt_rays(np.zeros((36, 3, 25, 3), np.float32), np.zeros((25, 3)), np.zeros((0, 8), np.float32))
    assert rgb.shape == (0, 3) and st.camera_rays == 0


# ---- shading rays ----
def camera_frame(ctx, scene, sample=0):
    p = frt.RenderParams.make(NX, NY, 1, seed=5, sample_offset=sample)
    rays = ctx.camera_rays(p, ALL)
    assert rays.view(np.uint32)[:, 7].any()                                  # stream ids: prt_rays must not read them as flags
    return rays


def test_rays_equal_the_replay_with_misses_and_an_emitter(ctx, cornell):
    """The Cornell box from its own camera: a third of the 48 x 36 frame passes beside the box, six pixels see the light."""
    scene = cornell
    image = ES.random_env(16, 8, seed=6)
    ctx.upload(scene)
    T, _ = ctx.prt_transfer(scene, DIRS[13], 1)
    li = frt.sh_project_image(image)
    rays = camera_frame(ctx, scene)
    for img in (image, None):
        ctx.set_env_image(img)
        rgb, st = ctx.prt_rays(T, li, rays)
        want = frt.selftest_prt_rays_host(scene, T, li, rays, env_image=img)
        assert rgb.tobytes() == want.tobytes(), np.argwhere(rgb != want)[:5]
        assert st.camera_rays == len(rays) and st.kernel_ms > 0
    ctx.set_env_image(image)
    rgb, _ = ctx.prt_rays(T, li, rays)
    hits = frt.selftest_trace_host(scene, np.concatenate([rays[:, :7], np.zeros((len(rays), 1), np.float32)], axis=1))
    prim = hits.view(np.int32)[:, 3]
    miss = prim < 0
    assert 0.2 < miss.mean() < 0.9
    texels = {tuple(t) for t in image.reshape(-1, 3)}
    assert all(tuple(c) in texels for c in rgb[miss])                        # the image's own bytes on every miss
    mats = frt.prt_corners(scene)[2]
    light = np.isin(prim, [t for t in range(36) if not mats[t].any()])
    assert light.sum() >= 4 and np.all(rgb[light] == np.float32([17, 12, 4]))
    lit = ~miss & ~light
    assert rgb[lit].max() > 0.05
    ctx.set_env_image(None)


def test_relighting_one_transfer_under_two_images(ctx, cornell):
    ctx.upload(cornell)
    T, _ = ctx.prt_transfer(cornell, frt.prt_sample_dirs(16, seed=3), 1)
    rays = camera_frame(ctx, cornell)
    films = []
    for seed in (1, 2):
        image = ES.random_env(8, 4, seed=seed)
        li = frt.sh_project_image(image)
        ctx.set_env_image(image)
        p = frt.RenderParams.make(NX, NY, 1, seed=5)
        film, _ = ctx.render_prt(p, T, li)
        want = frt.selftest_prt_rays_host(cornell, T, li, rays, env_image=image)
        assert film.shape == (NY, NX, 3) and film.reshape(-1, 3).tobytes() == want.tobytes()
        films.append(film)
    ctx.set_env_image(None)
    assert np.abs(films[0] - films[1]).max() > 0.05                          # another light, the same bake
    # two samples: the mean of the two sample frames, and a camera of cameras.py in the scene camera's place
    p2 = frt.RenderParams.make(NX, NY, 2, seed=5)
    li = frt.sh_project_image(None, env_color=(1.0, 1.0, 1.0))
    both, _ = ctx.render_prt(p2, T, li)
    one = [ctx.prt_rays(T, li, camera_frame(ctx, cornell, s))[0] for s in (0, 1)]
    assert np.array_equal(both.reshape(-1, 3), frt.film_accumulate(one[0].copy(), 1, one[1], 1))
    from first_raytracer_amd import cameras
    probe, _ = ctx.render_prt(frt.RenderParams.make(16, 8, 1), T, li, make_rays=lambda j: cameras.latlong((0.0, 1.0, 0.0), 16, 8, j))
    assert probe.shape == (128, 3) and probe.max() > 0.05


# ---- the CLI: precompute, projection and render in one run ----
def test_cli_prt_equals_render_prt(cornell_obj, tmp_path):
    hdr, out = str(tmp_path / "env.hdr"), str(tmp_path / "prt.pfm")
    with open(hdr, "wb") as f:
        f.write(ES.hdr_bytes(ES.rgbe_random(16, 8, seed=3)))
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", f"{NX}x{NY}", "--ns", "2", "--seed", "5",
                        "--integrator", "prt", "--env-map", hdr, "--prt-dirs", "13", "--prt-bounces", "1", "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    line = [l for l in r.stdout.splitlines() if l.startswith("PRT precompute:")]
    assert len(line) == 1 and "169 directions, 1 bounces" in line[0] and " ms on the GPU" in line[0], r.stdout
    image = frt.read_hdr(hdr)
    scene = frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)
    c = frt.Context(0)
    try:
        c.upload(scene)
        c.set_env_image(image)
        T, st = c.prt_transfer(scene, frt.prt_sample_dirs(13, seed=5), 1)
        assert f"{st.shadow_rays + st.extension_rays} rays" in line[0]
        film, _ = c.render_prt(frt.RenderParams.make(NX, NY, 2, seed=5), T, frt.sh_project_image(image))
    finally:
        c.close()
    assert np.array_equal(read_pfm(out), film)
    bad = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--prt-bounces", "1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode == 2 and "--integrator prt" in bad.stderr
