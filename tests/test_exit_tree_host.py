"""The exit-tree pass (FRT_EXIT_TREE; csrc/frt_tree_passes.hip exit_tree, csrc/host/exit_tree.cpp) on the host:
which subtree each triangle's extension rays skip, the trees it appends, what the counter says it saves,
and that films and ray counts do not depend on it.  CPU only."""
import os

import numpy as np
import pytest

import first_raytracer_amd as frt
import exit_tree_scenes as ETS
import scene_specs as SS
import shadow_tree_scenes as STS

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")


def cornell_ref():
    return frt.HostScene("cornell_box_obj", SS.CORNELL_OBJ, 1.0)          # the reference's topology


def cornell_sah():
    hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                  "world": "list"}, 1.0)
    hs.build_bvh_sah()
    return hs


CORNELLS = {"ref": cornell_ref, "sah": cornell_sah}


@pytest.fixture(scope="module")
def cornells():
    """name -> (scene, the hook's answer), made once"""
    return {k: (hs, frt.selftest_exit_tree(hs, 1)) for k, hs in ((k, f()) for k, f in CORNELLS.items())}


@pytest.fixture(scope="module")
def rooms(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("rooms"))
    out = dict(ETS.scenes(tmp))
    out.update({"sts_" + k: v[0] for k, v in STS.scenes(tmp).items()})
    return {k: (b, frt.selftest_exit_tree(b.hs, 1)) for k, b in out.items()}


ROOMS = ["outward_wall", "straddle_less", "straddle_more", "box_on_floor", "folded_leaf", "slanted_wall", "specular",
         "scaled", "full_lds"] + ["sts_" + k for k in ("room", "outside_camera", "outward_normal", "ramp", "two_lights",
                                                        "spheres", "empty_room", "dielectric", "scaled")]


# ---- the trees ----
def refs_of(nodes):
    return nodes[:, 12:14].copy().view(np.int32)


def leaves_under(refs, root):
    out, st = [], [int(root)]
    while st:
        r = st.pop()
        if r < 0:
            out.append(r)
        else:
            st += [int(refs[r, 0]), int(refs[r, 1])]
    return out


def leaf_tris(leaf, view_of):
    """scene-view triangles of a leaf ref (a sphere leaf: none)"""
    l = ~leaf
    if l & frt.FRT_PRIM_SPHERE:
        return []
    first, count = l & ((1 << 27) - 1), ((l >> 27) & 7) + 1
    return [int(view_of[first + k]) for k in range(count)]


def depth(refs, root):
    return 0 if root < 0 else 1 + max(depth(refs, int(refs[root, 0])), depth(refs, int(refs[root, 1])))


def check_trees(hs, ans):
    """What every exit tree must be, from the scene's own vertices: a tree over main-tree leaves, no deeper
    than the main tree, boxes that bound their children, and nothing missing from it but triangles that lie
    wholly on or under the origin triangle's plane (1e-5: far above the proof's tolerance, a tenth of eps)."""
    info, roots, taken, n_off, n_on = ans
    tv = hs.arrays()["tri_v"].reshape(-1, 3, 3)
    lights = {int(x) for x in hs.arrays()["lights"] if not (x & frt.FRT_PRIM_SPHERE)}
    assert n_on[:len(n_off)].tobytes() == n_off.tobytes()              # the nodes before it are untouched
    assert len(n_on) == len(n_off) + info["nodes_added"] and info["depth_on"] == info["depth_off"]
    assert info["lds_bytes"] <= info["lds_cap"] or info["lds_bytes_oct"] > 0
    assert info["lds_bytes_oct"] <= info["lds_cap_oct"]
    if info["lds_bytes_oct"]:       # ... and leave as many blocks of the octant plan on a CU as before (1280 B granules of 160 KiB)
        slots = lambda n: 24 * n + (n + 1) // 2                                   # noqa: E731
        before = info["lds_bytes_oct"] - 16 * (slots(len(n_on)) - slots(len(n_off)))
        per_cu = lambda scene: (160 * 1024) // (-(-((8 if info["depth_on"] < 8 else 16) * 1024 + 10 * 1024 + scene) // 1280) * 1280)  # noqa: E731
        assert per_cu(info["lds_bytes_oct"]) == per_cu(before)
    if info["why"] != 0:
        assert not roots.any() and len(n_on) == len(n_off) and info["taken"] == 0
        return {}
    refs = refs_of(n_on)
    assert (refs[len(n_off):] < len(n_on)).all() and info["taken"] == len(taken) > 0
    assert info["nodes_added"] == int(taken[:, 4].sum())
    main = leaves_under(refs, 0)
    all_tris = {t for l in main for t in leaf_tris(l, info["view_of"])}
    hidden = {}
    for k in np.flatnonzero(roots):
        r = int(roots[k])
        assert 0 < r < len(n_on) and r < 1024 and k not in lights
        got = leaves_under(refs, r)
        assert set(got) < set(main) and len(got) == len(set(got))
        assert depth(refs, r) <= depth(refs, 0) <= info["depth_on"] + 1
        kept = {t for l in got for t in leaf_tris(l, info["view_of"])}
        hidden[int(k)] = all_tris - kept
        assert int(k) in hidden[int(k)]                               # its own leaf is gone
        n = np.cross(tv[k, 1] - tv[k, 0], tv[k, 2] - tv[k, 0])
        n /= np.linalg.norm(n)
        for j in hidden[int(k)]:
            assert ((tv[j] - tv[k, 0]) @ n).max() <= 1e-5, (int(k), j)
        # every sphere leaf stays
        assert {l for l in main if ~l & frt.FRT_PRIM_SPHERE} <= set(got)
    for i in range(len(n_off), len(n_on)):                            # a box bounds its children's boxes
        for s in (0, 1):
            c, bx = int(refs[i, s]), n_on[i, 6 * s:6 * s + 6]
            if c >= 0:
                lo, hi = np.minimum(n_on[c, 0:3], n_on[c, 6:9]), np.maximum(n_on[c, 3:6], n_on[c, 9:12])
                assert (bx[:3] <= lo).all() and (bx[3:] >= hi).all()
    return hidden


def cornell_parts(hs):
    """(lights, walls, boxes) of CornellBox-Original by scene-view triangle: a wall has the whole scene on one
    side of its plane; what is left, the lights apart, falls into the two boxes by shared vertices"""
    tv = hs.arrays()["tri_v"].reshape(-1, 3, 3)
    lights = {int(x) for x in hs.arrays()["lights"]}
    walls = set()
    for k in range(len(tv)):
        n = np.cross(tv[k, 1] - tv[k, 0], tv[k, 2] - tv[k, 0])
        s = (tv.reshape(-1, 3) - tv[k, 0]) @ (n / np.linalg.norm(n))
        if k not in lights and (s.min() > -1e-6 or s.max() < 1e-6):
            walls.add(k)
    rest = [k for k in range(len(tv)) if k not in lights and k not in walls]
    comp = {k: {tuple(np.round(v, 6)) for v in tv[k]} for k in rest}
    boxes = []
    for k in rest:
        hit = [b for b in boxes if any(comp[k] & comp[j] for j in b)]
        for b in hit:
            boxes.remove(b)
        boxes.append(set().union({k}, *hit))
    return lights, walls, boxes


@pytest.mark.parametrize("name", list(CORNELLS))
def test_cornell_drop_sets(cornells, name):
    hs, ans = cornells[name]
    info, roots, taken, n_off, n_on = ans
    print(name, {k: v for k, v in info.items() if k != "view_of"}, roots.tolist(), taken.tolist())
    assert info["why_name"] == "ran" and info["taken"] > 0
    hidden = check_trees(hs, ans)
    lights, walls, boxes = cornell_parts(hs)
    assert len(lights) == 2 and len(boxes) == 2 and len(walls) >= 10
    assert not roots[list(lights)].any()
    leaf_of = {}
    for l in leaves_under(refs_of(n_on), 0):
        for t in leaf_tris(l, info["view_of"]):
            leaf_of[t] = set(leaf_tris(l, info["view_of"]))
    for k in walls:                                  # a room wall with an exit root drops exactly its own leaf
        if roots[k]:
            assert hidden[k] == leaf_of[k]
    # a face of a box with an exit root drops its leaf and whatever else of the subtree around it lies behind
    # the face: other faces of the box, and where the tree groups them with it, the floor or the other box
    # (check_trees has put every one of them under the face's plane)
    for box in boxes:
        for k in box:
            if roots[k]:
                assert leaf_of[k] <= hidden[k] and len(hidden[k] & box) >= 2
    assert any(len(hidden[k]) > 2 for box in boxes for k in box if roots[k])
    assert np.flatnonzero(roots).size >= 10


@pytest.mark.parametrize("name", list(CORNELLS))
def test_cornell_counter_gate(cornells, name):
    """V and T of the validation replay's extension rays, and J over all its rays, fall"""
    info = cornells[name][1][0]
    assert info["n_ext"] > 1000 and info["n_rays"] > info["n_ext"]
    assert info["v_ext"][1] < info["v_ext"][0] and info["t_ext"][1] < info["t_ext"][0]
    assert info["j_all"][1] < info["j_all"][0]


@pytest.mark.parametrize("name", list(CORNELLS))
def test_deterministic_and_off_is_parent(cornells, name, monkeypatch):
    hs, (info, roots, taken, n_off, n_on) = cornells[name]
    again = frt.selftest_exit_tree(hs, 1)
    assert again[4].tobytes() == n_on.tobytes() and again[1].tobytes() == roots.tobytes()
    monkeypatch.setenv("FRT_EXIT_TREE", "0")
    off = frt.selftest_exit_tree(hs, -1)
    assert off[0]["why_name"] == "off" and off[4].tobytes() == n_off.tobytes() and not off[1].any()
    monkeypatch.setenv("FRT_EXIT_TREE", "1")
    on = frt.selftest_exit_tree(hs, -1)
    assert on[4].tobytes() == n_on.tobytes()
    # the other hooks keep showing their own pass alone
    assert len(frt.selftest_shadow_tree(hs)[2]) == len(n_off)


def test_vertex_normals_get_no_root():
    hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": False}], "camera": SS.CORNELL_CAM,
                                  "world": "bvh"}, 1.0)
    info, roots, _, n_off, n_on = frt.selftest_exit_tree(hs, 1)
    assert not roots.any() and len(n_on) == len(n_off)


@pytest.mark.parametrize("name", ROOMS)
def test_room_trees(rooms, name):
    b, ans = rooms[name]
    info, roots = ans[0], ans[1]
    print(name, {k: v for k, v in info.items() if k != "view_of"}, roots.tolist(), ans[2].tolist())
    hidden = check_trees(b.hs, ans)
    key = name[4:] if name.startswith("sts_") else name
    want = {"specular": "material", "dielectric": "material", "scaled": "too_large"}.get(key)
    if want:
        assert info["why_name"] == want
    if name == "outward_wall":                       # everything lies behind the flipped wall: no tree would be left
        assert not roots[list(b.tris["back"])].any()
    if name == "straddle_more":                      # the quad stands 1e-3 above the floor: the floor's rays can hit it
        for k in b.tris["floor"]:
            assert not (set(b.tris["poke"]) & hidden.get(k, set()))
    if name == "box_on_floor":                       # the sides stand on the floor: its rays can hit them
        assert any(roots[k] for k in b.tris["floor"])
        for k in b.tris["floor"]:
            assert not ({t for f in ("west", "east", "south", "north", "top") for t in b.tris["box_" + f]} & hidden.get(k, set()))
    if name == "folded_leaf":                        # the fold's two triangles see each other: no drop set holds its leaf
        for k in b.tris["fold"]:
            assert not roots[k]
    if name == "full_lds":                           # no room for a node: refused, or only trees that append none
        assert info["nodes_added"] == 0 and info["lds_cap_oct"] - info["lds_bytes_oct"] < 392
        assert info["why_name"] == "budget" or info["budget_refused"] == 1 or info["classes"] == info["taken"]


# ---- films and ray counters do not depend on it ----
def film(hs, knob, monkeypatch, n=24, spp=8, flags=0):
    monkeypatch.setenv("FRT_EXIT_TREE", knob)
    p = frt.RenderParams.make(n, n, spp, seed=11, flags=flags)
    return frt.selftest_path_host(hs, p, np.arange(n * n, dtype=np.int32))


def same_film(hs, monkeypatch, **kw):
    """off against on: on the tree the replay takes by default (BVH4Q where the scene has one: no exit roots),
    on the binary tree and in fp64 (the binary tree too), where extension rays start at their exit roots"""
    for fl in (0, frt.FRT_FLAG_BVH2, frt.FRT_FLAG_FP64):
        (a, sa), (b, sb) = film(hs, "0", monkeypatch, flags=fl, **kw), film(hs, "1", monkeypatch, flags=fl, **kw)
        assert a.max() > 0 and a.tobytes() == b.tobytes()
        assert (sa.rays, sa.camera_rays, sa.extension_rays, sa.shadow_rays) == \
            (sb.rays, sb.camera_rays, sb.extension_rays, sb.shadow_rays)
    return sa


@pytest.mark.parametrize("name", list(CORNELLS))
def test_cornell_films_bit_equal(cornells, name, monkeypatch):
    st = same_film(cornells[name][0], monkeypatch, n=32)
    assert st.extension_rays > 0


@pytest.mark.parametrize("flags", [frt.FRT_FLAG_ROULETTE | frt.FRT_FLAG_SOBOL | frt.FRT_FLAG_BVH2])
def test_cornell_roulette_sobol_bit_equal(cornells, monkeypatch, flags):
    hs = cornells["sah"][0]
    (a, sa), (b, sb) = film(hs, "0", monkeypatch, flags=flags), film(hs, "1", monkeypatch, flags=flags)
    assert a.tobytes() == b.tobytes() and sa.rays == sb.rays


@pytest.mark.parametrize("name", ROOMS)
def test_room_films_bit_equal(rooms, name, monkeypatch):
    same_film(rooms[name][0].hs, monkeypatch, n=16, spp=8)


def test_cornell_sphere_pass_off(monkeypatch):
    hs = frt.HostScene("cornell_box_obj", os.path.join(SCENES, "CornellBox-Sphere.obj"), 1.0)
    assert frt.selftest_exit_tree(hs, 1)[0]["why_name"] in ("material", "not_resident")
    same_film(hs, monkeypatch, n=16, spp=2)
