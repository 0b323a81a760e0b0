"""The tree refinement pass (FRT_TREE_REFINE; csrc/frt_tree_passes.hip refine_tree,
csrc/host/tree_refine.cpp) on the host: the interior nodes of an LDS-resident
binary tree are rearranged, so the tree's structure, every hit, every film and
the counted traversal cost are compared with the pass on and off."""
import os

import numpy as np
import pytest

import first_raytracer_amd as frt
import scene_specs as SS

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")
SPHERE_BIT = frt.FRT_PRIM_SPHERE
GREY = {"type": "lambertian", "albedo": (0.6, 0.6, 0.6)}


def cornell_ref():     # the reference's create_bvh topology
    return frt.HostScene("cornell_box_obj", SS.CORNELL_OBJ, 4 / 3)


def cornell_sah():     # binned SAH, the rule the default GPU builder follows
    hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                  "world": "list"}, 4 / 3)
    hs.build_bvh_sah()
    return hs


def cornell_spheres():  # analytic spheres among the triangles: sphere leaves
    objs = [{"obj": SS.CORNELL_OBJ, "geo": True},
            {"sphere": (-0.4, 0.9, 0.3), "radius": 0.25, "material": GREY},
            {"sphere": (0.5, 1.3, -0.2), "radius": 0.2, "material": {"type": "metal", "albedo": (0.8, 0.8, 0.8)}}]
    return frt.HostScene.from_spec({"objects": objs, "camera": SS.CORNELL_CAM, "world": "bvh"}, 4 / 3)


def cornell_sphere_obj():   # CornellBox-Sphere: 2k triangles, not LDS-resident -- the pass does not run
    return frt.HostScene("cornell_box_obj", os.path.join(SCENES, "CornellBox-Sphere.obj"), 4 / 3)


def make_tiny(tmp):     # two quads, no light: two 2-triangle leaves under one node
    path = os.path.join(tmp, "tiny.obj")
    with open(path, "w") as f:
        f.write("v -1 0 -1\nv 1 0 -1\nv 1 0 1\nv -1 0 1\nv -1 2 -1\nv 1 2 -1\nv 1 2 1\nv -1 2 1\n"
                "f 1 2 3\nf 1 3 4\nf 5 7 6\nf 5 8 7\n")
    return frt.HostScene.from_spec({"objects": [{"obj": path, "bsdf": GREY, "geo": True}], "camera": SS.CORNELL_CAM,
                                    "world": "bvh", "env": (1.0, 1.0, 1.0)}, 4 / 3)


BUILDERS = {"cornell_ref": cornell_ref, "cornell_sah": cornell_sah, "cornell_spheres": cornell_spheres,
            "cornell_sphere_obj": cornell_sphere_obj}
NAMES = list(BUILDERS) + ["tiny"]
APPLIES = {"cornell_ref": True, "cornell_sah": True, "cornell_spheres": True, "cornell_sphere_obj": False, "tiny": True}


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    """name -> (scene, the hook's result), made once"""
    out = {}
    for name in NAMES:
        hs = make_tiny(str(tmp_path_factory.mktemp("tiny"))) if name == "tiny" else BUILDERS[name]()
        out[name] = (hs, frt.selftest_tree_refine(hs))
    return out


def refs(nodes):
    return nodes[:, 12:14].copy().view(np.int32)


def leaf_refs(nodes):
    r = refs(nodes).ravel()
    return np.sort(r[r < 0])


def depth_of(nodes):
    r, best, st = refs(nodes), 0, [(0, 1)]
    while st:
        i, lvl = st.pop()
        best = max(best, lvl)
        st += [(int(c), lvl + 1) for c in r[i] if c >= 0]
    return best if len(nodes) else 0


def child_box(nodes, i, side):
    return nodes[i, 6 * side:6 * side + 6]


# ---- structure ----
@pytest.mark.parametrize("name", NAMES)
def test_structure(scenes, name):
    hs, ((c0, off), (c1, on)) = scenes[name]
    assert c0["applies"] == c1["applies"] == int(APPLIES[name])
    assert len(on) == len(off) == c0["n_nodes"] == c1["n_nodes"]              # leaves - 1 nodes, as before
    assert np.array_equal(leaf_refs(on), leaf_refs(off))                       # the same leaves
    assert len(np.unique(refs(on)[refs(on) >= 0])) == len(on) - 1              # every node but the root has one parent
    assert depth_of(on) <= depth_of(off)
    if APPLIES[name]:
        assert c1["depth"] == depth_of(on) and c0["depth"] == depth_of(off)
    # a leaf keeps its box; an interior child's box is the union of that child's two boxes
    box_of = {int(r): child_box(off, i, s).copy() for i in range(len(off)) for s in (0, 1) if (r := refs(off)[i, s]) < 0}
    for i in range(len(on)):
        for s in (0, 1):
            c, b = int(refs(on)[i, s]), child_box(on, i, s)
            if c < 0:
                assert np.array_equal(b, box_of[c])
            else:
                b0, b1 = child_box(on, c, 0), child_box(on, c, 1)
                assert np.array_equal(b[:3], np.minimum(b0[:3], b1[:3])) and np.array_equal(b[3:], np.maximum(b0[3:], b1[3:]))
    if name in ("tiny", "cornell_sphere_obj"):                                  # nothing to move / not resident
        assert on.tobytes() == off.tobytes()
    if name == "cornell_spheres":                                               # sphere leaves stay one-sphere leaves
        r = ~leaf_refs(on)
        assert sorted(r[(r & SPHERE_BIT) != 0] & ~SPHERE_BIT) == [0, 1]


@pytest.mark.parametrize("name", ["cornell_ref", "cornell_sah", "cornell_spheres"])
def test_two_flattens_are_byte_identical(scenes, name):
    hs, ((c0, off), (c1, on)) = scenes[name]
    (d0, off2), (d1, on2) = frt.selftest_tree_refine(hs)
    assert on2.tobytes() == on.tobytes() and off2.tobytes() == off.tobytes() and (d0, d1) == (c0, c1)
    assert on.tobytes() != off.tobytes()                                        # the pass did move something


# ---- cost ----
@pytest.mark.parametrize("name", NAMES)
def test_validation_cost(scenes, name):
    _, ((c0, _), (c1, _)) = scenes[name]
    print(name, "off", c0, "on", c1)
    assert c1["j"] <= c0["j"] and c0["n_rays"] == c1["n_rays"]
    if name in ("cornell_ref", "cornell_sah"):
        assert c1["j"] < c0["j"] and c0["n_rays"] > 5000
        assert abs(c0["j"] - (c0["v"] + c0["w"] * c0["t"])) < 1e-12


def test_unrefined_visits_match_the_diagnostic_build(scenes):
    """The host counter models the kernel: the diagnostic build counted 7.31 node visits and
    1.96 primitive tests per ray on Cornell at 1080p (profiles/r05/r05c/diag_cornell.json);
    a 40 x 40 frame's 11k rays give that to a few percent."""
    _, ((c0, _), _) = scenes["cornell_sah"]
    assert abs(c0["v"] / 7.31 - 1) < 0.05 and abs(c0["t"] / 1.96 - 1) < 0.08


# ---- hits ----
def ray_set(hs, seed=5):
    """closest-hit and any-hit rays: random ones from inside the scene, rays from the camera
    and from a point inside through every vertex and edge midpoint (exact ties between the
    triangles that share them), and axis-parallel rays (infinite 1/d on two axes)."""
    rng = np.random.default_rng(seed)
    v = hs.arrays()["tri_v"].reshape(-1, 3, 3)
    lo, hi = v.reshape(-1, 3).min(0), v.reshape(-1, 3).max(0)
    n = 3000
    o = lo + (hi - lo) * rng.random((n, 3))
    d = rng.normal(size=(n, 3))
    targets = np.concatenate([v.reshape(-1, 3), 0.5 * (v + np.roll(v, 1, axis=1)).reshape(-1, 3)])
    for eye in (np.array([0.0, 1.0, 3.0]), 0.5 * (lo + hi) + 0.013 * (hi - lo)):
        o = np.concatenate([o, np.broadcast_to(eye, targets.shape)])
        d = np.concatenate([d, targets - eye])
    m = 300
    ao = lo + (hi - lo) * rng.random((m, 3))
    ao[:100] = v.reshape(-1, 3)[rng.integers(0, len(v) * 3, 100)] + np.array([0.0, 0.5, 0.0])   # along edges / through vertices
    ad = np.zeros((m, 3))
    ad[np.arange(m), rng.integers(0, 3, m)] = rng.choice([-1.0, 1.0], m)
    o, d = np.concatenate([o, ao]), np.concatenate([d, ad])
    rays = np.zeros((len(o), 8), np.float32)
    rays[:, :3], rays[:, 4:7] = o, d
    rays[:, 3] = 1e30
    shadow = rays.copy()
    shadow[:, 3] = rng.uniform(0.2, 3.0, len(o)).astype(np.float32)
    shadow[:, 7] = np.array([1], np.int32).view(np.float32)[0]
    return np.concatenate([rays, shadow])


@pytest.mark.parametrize("name", NAMES)
def test_hits_equal(scenes, name, monkeypatch):
    hs = scenes[name][0]
    rays = ray_set(hs)
    monkeypatch.setenv("FRT_TREE_REFINE", "0")
    off = frt.selftest_trace_host(hs, rays)
    monkeypatch.setenv("FRT_TREE_REFINE", "1")
    on = frt.selftest_trace_host(hs, rays)
    monkeypatch.delenv("FRT_TREE_REFINE")
    default = frt.selftest_trace_host(hs, rays)
    anyhit = rays[:, 7].view(np.int32) == 1
    prim = lambda h: h[:, 3].copy().view(np.int32)   # noqa: E731
    # the rays do test something: hits and misses of both kinds (the tiny scene is open: fewer hits)
    assert (prim(off)[~anyhit] >= 0).sum() > (500 if name == "tiny" else 2000)
    assert 100 < (prim(off)[anyhit] >= 0).sum() < anyhit.sum() - 100
    assert off[~anyhit].tobytes() == on[~anyhit].tobytes()                      # t, u, v and prim, bit for bit
    assert np.array_equal(prim(off)[anyhit] >= 0, prim(on)[anyhit] >= 0)        # occlusion
    assert default.tobytes() == on.tobytes()                                    # the pass is on by default


# ---- film ----
@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_FP64])
@pytest.mark.parametrize("name", ["cornell_sah", "cornell_spheres"])
def test_film_bit_identical(scenes, name, flags, monkeypatch):
    hs = scenes[name][0]
    nx, ny = 48, 36
    pixels = np.arange(nx * ny, dtype=np.int32)
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("FRT_TREE_REFINE", knob)
        out[knob] = frt.selftest_path_host(hs, frt.RenderParams.make(nx, ny, 4, seed=9, flags=flags), pixels)
    (a, sa), (b, sb) = out["0"], out["1"]
    assert a.max() > 0 and a.tobytes() == b.tobytes() and sa.rays == sb.rays
    assert sa.stack_entries == sb.stack_entries and sb.bvh_depth <= sa.bvh_depth   # (BVH4Q of the new tree may be shallower)
