"""The shadow-tree pass (FRT_SHADOW_TREE; csrc/frt_tree_passes.hip shadow_tree, csrc/host/shadow_tree.cpp)
on the host: which triangles it proves no area-light shadow segment can hit, the tree it appends, what
the counter says it saves, and that films and ray counts do not depend on it.  CPU only."""
import os

import numpy as np
import pytest

import first_raytracer_amd as frt
import env_sampling_specs as ESS
import env_specs as ES
import scene_specs as SS
import shadow_tree_scenes as STS

SCENES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scenes")


@pytest.fixture(scope="module")
def rooms(tmp_path_factory):
    """name -> (Built, dropped names, kept names, why, the hook's answer with 1e5 segments), made once"""
    out = {}
    for name, (b, drop, keep, why) in STS.scenes(str(tmp_path_factory.mktemp("rooms"))).items():
        out[name] = (b, drop, keep, why, frt.selftest_shadow_tree(b.hs, segments=100000, seed=7))
    return out


ROOMS = ["room", "outside_camera", "outward_normal", "ramp", "two_lights", "spheres", "empty_room", "dielectric", "scaled"]


def film(hs, knob, monkeypatch, n=24, spp=8, flags=0, integrator=frt.FRT_INTEGRATOR_PATH):
    monkeypatch.setenv("FRT_SHADOW_TREE", knob)
    p = frt.RenderParams.make(n, n, spp, seed=11, flags=flags, integrator=integrator)
    return frt.selftest_path_host(hs, p, np.arange(n * n, dtype=np.int32))


def same_film(hs, monkeypatch, flags=0, **kw):
    """off against on, on the tree the host replay takes by default (BVH4Q where the scene has one, which
    has no shadow root) and on the binary tree, where the shadow root is used"""
    for fl in (flags, flags | frt.FRT_FLAG_BVH2):
        (a, sa), (b, sb) = film(hs, "0", monkeypatch, flags=fl, **kw), film(hs, "1", monkeypatch, flags=fl, **kw)
        assert a.tobytes() == b.tobytes() and sa.rays == sb.rays and sa.shadow_rays == sb.shadow_rays
    return a, sa


# ---- what is dropped ----
@pytest.mark.parametrize("name", ROOMS)
def test_dropped_primitives(rooms, name):
    b, drop, keep, why, (info, dropped, nodes) = rooms[name]
    print(name, info)
    assert info["why"] == why
    assert b.dropped_names(dropped) == drop and b.kept_names(dropped) >= keep
    assert info["dropped_prims"] == int(dropped.sum()) == 2 * len(drop)
    if why == 0:
        assert info["rule_a"] + info["rule_b"] == info["dropped_prims"]
        assert info["rule_b"] == (2 if "lamp" in drop else 0)
        assert info["kept_prims"] + info["dropped_prims"] == len(dropped) + int(b.hs.view().n_spheres)


@pytest.mark.parametrize("name", ROOMS)
def test_the_tree(rooms, name):
    b, drop, keep, why, (info, dropped, nodes) = rooms[name]
    (_, _), (_, main) = frt.selftest_tree_refine(b.hs)          # the main tree alone
    nm = info["nodes_main"]
    assert nm == len(main) and nodes[:nm].tobytes() == main.tobytes()   # the main nodes are untouched
    if why != 0:
        assert len(nodes) == nm and info["nodes_added"] == 0           # pass off: byte-equal to the tree without it
        return
    assert len(nodes) == nm + info["nodes_added"]
    refs = nodes[:, 12:14].copy().view(np.int32)
    assert (refs[nm:] < len(nodes)).all()
    if info["empty"]:
        assert name == "empty_room" and info["nodes_added"] == 0
        return
    # the leaves under the shadow root are exactly the main tree's leaves that keep a primitive
    def leaves(root):
        out, st = [], [root]
        while st:
            r = st.pop()
            if r < 0:
                out.append(r)
            else:
                st += [int(refs[r, 0]), int(refs[r, 1])]
        return sorted(out)

    def depth(root):
        return 0 if root < 0 else 1 + max(depth(int(refs[root, 0])), depth(int(refs[root, 1])))
    # (a leaf names device triangle ids, the hook's `dropped` scene-view triangles: compare counts)
    got, all_main = leaves(info["root"]), leaves(0)
    assert set(got) <= set(all_main) and len(got) == len(set(got))
    assert depth(info["root"]) <= depth(0)
    n_tri_kept = sum(((~r >> 27) & 7) + 1 for r in got if not (~r & frt.FRT_PRIM_SPHERE))
    n_tri_gone = sum(((~r >> 27) & 7) + 1 for r in all_main if r not in got)
    assert n_tri_gone <= info["dropped_prims"] <= n_tri_gone + n_tri_kept     # a leaf with a kept triangle stays whole
    assert n_tri_gone > 0
    # a box of the shadow tree bounds its children's boxes
    for i in range(nm, len(nodes)):
        for s in (0, 1):
            c, box = int(refs[i, s]), nodes[i, 6 * s:6 * s + 6]
            if c >= 0:
                lo = np.minimum(nodes[c, 0:3], nodes[c, 6:9])
                hi = np.maximum(nodes[c, 3:6], nodes[c, 9:12])
                assert (box[:3] <= lo).all() and (box[3:] >= hi).all()


@pytest.mark.parametrize("name", ROOMS)
def test_no_segment_hits_a_dropped_triangle(rooms, name):
    """1e5 segments from the replay's own shadow-ray origins to seeded points on the lights, through the
    fp32 tri_intersect of every dropped triangle over (t_min, 1 - shadow_eps]"""
    _, _, _, why, (info, _, _) = rooms[name]
    if why == 0:
        assert info["segments"] == 100000 and info["n_rays"] > 100
    assert info["segment_hits"] == 0


@pytest.mark.parametrize("name", ROOMS)
def test_room_films_bit_equal(rooms, name, monkeypatch):
    b, _, _, _, (info, _, _) = rooms[name]
    a, st = same_film(b.hs, monkeypatch)
    assert a.max() > 0 and st.shadow_rays > 0
    if name == "empty_room":
        assert info["empty"] == 1 and info["root_stops_shadow"] == info["n_rays"] and info["v_shadow"] == 0.0


# ---- the counter: the gate of the pass ----
def test_cornell_visits_gate():
    """at least a quarter fewer node visits for the area-light shadow rays on CornellBox-Original"""
    hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                  "world": "list"}, 1.0)
    hs.build_bvh_sah()
    info, dropped, nodes = frt.selftest_shadow_tree(hs)
    print(info)
    assert info["why"] == 0 and info["n_rays"] > 3000
    assert info["v_shadow"] <= 0.75 * info["v_main"] and info["t_shadow"] <= info["t_main"]
    assert info["nodes_shared"] > 0 and info["nodes_added"] <= 11


# ---- films of the project's scenes ----
def cornell():
    return frt.HostScene("cornell_box_obj", SS.CORNELL_OBJ, 1.0)


def cornell_sphere():
    return frt.HostScene("cornell_box_obj", os.path.join(SCENES, "CornellBox-Sphere.obj"), 1.0)


def veach():
    return frt.HostScene("veach_mis", os.path.join(SCENES, "veach_mi.obj"), 1.0)


SPECS = {"textured": SS.cornell_textured, "conductors": SS.cornell_conductors, "image_textured": SS.cornell_image_textured}


@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_FP64, frt.FRT_FLAG_BVH2])
def test_cornell_films_bit_equal(monkeypatch, flags):
    a, st = same_film(cornell(), monkeypatch, flags=flags)
    assert a.max() > 0 and st.shadow_rays > 0


@pytest.mark.parametrize("integrator", [frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS])
def test_other_integrators_bit_equal(monkeypatch, integrator):
    hs = cornell()
    hs.set_env((1.0, 1.0, 1.0))
    same_film(hs, monkeypatch, integrator=integrator)


@pytest.mark.parametrize("make,why", [(cornell_sphere, (4, 5)), (veach, None)])   # a specular material, not resident
def test_pass_off_scenes(monkeypatch, make, why):
    hs = make()
    same_film(hs, monkeypatch, n=16, spp=2)
    if why is not None:
        assert frt.selftest_shadow_tree(hs)[0]["why"] in why


@pytest.mark.parametrize("name", list(SPECS))
def test_spec_scene_films_bit_equal(monkeypatch, name):
    hs = frt.HostScene.from_spec(SPECS[name](), 1.0)
    same_film(hs, monkeypatch, n=16, spp=4)
    assert frt.selftest_shadow_tree(hs)[0]["why"] in (4, 0)


# ---- the other spec modules' scenes and the remaining golden scenes ----
def cube_spec():
    """tests/golden/scenes/cube.obj under a sphere light, constant environment"""
    objs = [{"obj": SS.CUBE_OBJ, "bsdf": STS.WHITE, "geo": True},
            {"sphere": (0.5, 3.0, 1.0), "radius": 0.4, "material": STS.LIGHT, "where": "both"}]
    cam = dict(SS.CORNELL_CAM, lookfrom=(2.0, 2.5, 5.0), lookat=(0.0, 0.0, 0.0))
    return {"objects": objs, "camera": cam, "world": "bvh", "env": (0.2, 0.2, 0.2)}


MORE = {
    "env_plain_cornell": lambda: frt.HostScene.from_spec(ES.plain_cornell(), 1.0),
    "env_direction": lambda: frt.HostScene.from_spec(ES.direction_spec(), ES.DIR_NX / ES.DIR_NY),
    "env_sampling_floor": lambda: ESS.floor_scene(),                      # quad_uv.obj, no lights
    "mirror": lambda: frt.HostScene("cornell_box_obj", os.path.join(SCENES, "CornellBox-Mirror.obj"), 1.0),
    "glossy_floor": lambda: frt.HostScene("cornell_box_obj", os.path.join(SCENES, "CornellBox-Glossy-Floor.obj"), 1.0),
    "cube": lambda: frt.HostScene.from_spec(cube_spec(), 1.0),
}
# the pass's answer: it runs on the two plain Cornells; no lights (2: the floor, and this glossy box's MTL
# has no emitter), a specular material (4)
MORE_WHY = {"env_plain_cornell": (0,), "env_direction": (0,), "env_sampling_floor": (2,), "mirror": (4,),
            "glossy_floor": (2,), "cube": (0, 6)}


@pytest.mark.parametrize("name", list(MORE))
def test_more_scene_films_bit_equal(monkeypatch, name):
    hs = MORE[name]()
    if name in ("env_sampling_floor", "glossy_floor"):    # no lights: lit by a constant environment
        hs.set_env((1.0, 1.0, 1.0))
    a, st = same_film(hs, monkeypatch, n=16, spp=4)
    assert a.max() > 0
    assert frt.selftest_shadow_tree(hs)[0]["why"] in MORE_WHY[name]


def film_env(hs, knob, monkeypatch, image, flags, n=24, spp=8):
    monkeypatch.setenv("FRT_SHADOW_TREE", knob)
    p = frt.RenderParams.make(n, n, spp, seed=13, flags=flags)
    return frt.selftest_path_host(hs, p, np.arange(n * n, dtype=np.int32), env_image=image)


@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_ENV_SAMPLING, frt.FRT_FLAG_ENV_SAMPLING | frt.FRT_FLAG_BVH2,
                                   frt.FRT_FLAG_ENV_SAMPLING | frt.FRT_FLAG_FP64])   # BVH2, FP64: the binary tree
@pytest.mark.parametrize("name", ["env_plain_cornell", "env_direction", "env_sampling_floor"])
def test_env_image_films_bit_equal(monkeypatch, name, flags):
    """Under an environment image with FRT_FLAG_ENV_SAMPLING a vertex traces either an area-light shadow
    ray or an environment one: only the first may start at the shadow root -- Cornell's front is open, and
    an environment ray that skipped the walls would leak light.  (With light_shadow_ray reduced to
    P.shadow, the binary-tree cases of both Cornells fail here.)"""
    hs = MORE[name]()
    image = ESS.sun_image() if name == "env_sampling_floor" else ES.random_env(16, 8)
    (a, sa), (b, sb) = (film_env(hs, k, monkeypatch, image, flags) for k in ("0", "1"))
    assert a.max() > 0 and a.tobytes() == b.tobytes()
    assert sa.rays == sb.rays and sa.shadow_rays == sb.shadow_rays
    assert sa.shadow_rays > 0 or (name == "env_sampling_floor" and flags == 0)   # no lights, no sampling: no NEE


@pytest.mark.parametrize("integrator", [frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH])
def test_feature_films_bit_equal(monkeypatch, integrator):
    """the feature films of tests/denoise_specs.py (host_features on Cornell)"""
    same_film(cornell(), monkeypatch, n=32, spp=4, integrator=integrator)


def test_mlt_paths_equal(monkeypatch):
    hs = cornell()
    out = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("FRT_SHADOW_TREE", knob)
        out[knob] = frt.selftest_mlt_paths_host(hs, 32, 32, 5, 2000)
    assert out["0"].tobytes() == out["1"].tobytes() and out["0"][:, 5].max() > 0
