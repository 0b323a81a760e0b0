"""Small rooms for the shadow-tree tests (tests/test_shadow_tree_host.py, tests/test_gpu_shadow_tree.py):
quads written as OBJ files, one file per material, each quad named so that a test can say which
ones the pass must drop and which it must keep."""
import os

import numpy as np

import first_raytracer_amd as frt
import scene_specs as SS

WHITE = {"type": "lambertian", "albedo": (0.7, 0.7, 0.7)}
LIGHT = {"type": "diffuse_light", "emit": (15.0, 15.0, 15.0)}
GLASS = {"type": "dielectric", "ior": 1.5, "specular": (1.0, 1.0, 1.0)}
CAM_BEHIND = dict(SS.CORNELL_CAM, lookfrom=(0.0, 1.0, -3.9))   # outside, looking at the back wall's back


def facing(p, toward):
    """the quad's corners ordered so that its geometric normal points along `toward`"""
    p = [np.asarray(x, np.float64) for x in p]
    n = np.cross(p[1] - p[0], p[2] - p[0])
    return p if np.dot(n, toward) > 0 else p[::-1]


def room(s=1.0):
    """name -> quad of a room open to +z: x in [-1, 1], y in [0, 2], z in [-1, 1], normals inward"""
    q = {
        "floor": facing([(-1, 0, -1), (1, 0, -1), (1, 0, 1), (-1, 0, 1)], (0, 1, 0)),
        "ceiling": facing([(-1, 2, -1), (1, 2, -1), (1, 2, 1), (-1, 2, 1)], (0, -1, 0)),
        "back": facing([(-1, 0, -1), (1, 0, -1), (1, 2, -1), (-1, 2, -1)], (0, 0, 1)),
        "left": facing([(-1, 0, -1), (-1, 0, 1), (-1, 2, 1), (-1, 2, -1)], (1, 0, 0)),
        "right": facing([(1, 0, -1), (1, 0, 1), (1, 2, 1), (1, 2, -1)], (-1, 0, 0)),
    }
    return {k: [s * x for x in v] for k, v in q.items()}


def lamp(s=1.0, y=1.98):
    return [s * x for x in facing([(-0.25, y, -0.25), (0.25, y, -0.25), (0.25, y, 0.25), (-0.25, y, 0.25)], (0, -1, 0))]


def block():
    """an occluder in the room: a small quad under the lamp, facing up"""
    return facing([(-0.3, 0.8, -0.3), (0.3, 0.8, -0.3), (0.3, 0.8, 0.3), (-0.3, 0.8, 0.3)], (0, 1, 0))


class Built:
    """a scene and the scene-view triangle ids of each named quad"""
    def __init__(self, hs, tris):
        self.hs, self.tris = hs, tris

    def dropped_names(self, dropped):
        return {k for k, ids in self.tris.items() if all(dropped[i] for i in ids)}

    def kept_names(self, dropped):
        return {k for k, ids in self.tris.items() if not any(dropped[i] for i in ids)}


def build(tmp, groups, spheres=(), camera=None, env=None):
    """groups: [(material, {name: quad})]; triangles are numbered in file order"""
    objs, tris, t = [], {}, 0
    for g, (mat, quads) in enumerate(groups):
        path = os.path.join(tmp, f"g{g}.obj")
        with open(path, "w") as f:
            v = 0
            for name, q in quads.items():
                for p in q:
                    f.write("v %r %r %r\n" % tuple(float(x) for x in p))
                f.write(f"f {v + 1} {v + 2} {v + 3}\nf {v + 1} {v + 3} {v + 4}\n")
                v += 4
                tris[name] = (t, t + 1)
                t += 2
        objs.append({"obj": path, "bsdf": mat, "geo": True})
    objs += list(spheres)
    spec = {"objects": objs, "camera": camera or SS.CORNELL_CAM, "world": "bvh"}
    if env is not None:
        spec["env"] = env
    return Built(frt.HostScene.from_spec(spec, 1.0), tris)


def scenes(tmp):
    """name -> (Built, must be dropped, must be kept, the pass's `why`)"""
    out = {}
    sub = lambda n: (os.makedirs(os.path.join(tmp, n), exist_ok=True), os.path.join(tmp, n))[1]   # noqa: E731
    r = room()
    walls = {"floor", "back", "left", "right"}
    # the plain room: four walls and the lamp go; the ceiling is 0.02 from the lamp, too close to prove
    out["room"] = (build(sub("room"), [(WHITE, dict(r, block=block())), (LIGHT, {"lamp": lamp()})]),
                   walls | {"lamp"}, {"ceiling", "block"}, 0)
    out["outside_camera"] = (build(sub("oc"), [(WHITE, dict(r, block=block())), (LIGHT, {"lamp": lamp()})], camera=CAM_BEHIND),
                             {"floor", "left", "right", "lamp"}, {"back", "ceiling", "block"}, 0)
    flipped = dict(r, back=r["back"][::-1], block=block())
    out["outward_normal"] = (build(sub("on"), [(WHITE, flipped), (LIGHT, {"lamp": lamp()})]),
                             {"floor", "left", "right", "lamp"}, {"back", "ceiling", "block"}, 0)
    # a ramp whose lower edge lies in the floor's plane and whose normal points down: its origins go under the floor
    ramp = facing([(-0.5, 0.0, -0.5), (0.5, 0.0, -0.5), (0.5, 0.6, 0.1), (-0.5, 0.6, 0.1)], (0, -1, 0))
    out["ramp"] = (build(sub("ramp"), [(WHITE, dict(r, ramp=ramp)), (LIGHT, {"lamp": lamp()})]),
                   {"back", "left", "right", "lamp"}, {"floor", "ceiling", "ramp"}, 0)
    side = facing([(0.98, 0.8, -0.2), (0.98, 0.8, 0.2), (0.98, 1.2, 0.2), (0.98, 1.2, -0.2)], (-1, 0, 0))
    out["two_lights"] = (build(sub("two"), [(WHITE, dict(r, block=block())), (LIGHT, {"lamp": lamp(), "side": side})]),
                         {"floor", "back", "left"}, {"lamp", "side", "right", "ceiling", "block"}, 0)
    balls = [{"sphere": (0.4, 0.0, 0.3), "radius": 0.3, "material": WHITE},
             {"sphere": (0.0, 1.0, -1.0), "radius": 0.2, "material": LIGHT, "where": "both"}]
    out["spheres"] = (build(sub("sph"), [(WHITE, r), (LIGHT, {"lamp": lamp()})], spheres=balls),
                      {"left", "right"}, {"floor", "back", "ceiling", "lamp"}, 0)
    empty = {k: v for k, v in r.items() if k != "ceiling"}
    out["empty_room"] = (build(sub("empty"), [(WHITE, empty), (LIGHT, {"lamp": lamp()})]),
                         walls | {"lamp"}, set(), 0)
    shard = facing([(-0.2, 0.5, 0.0), (0.2, 0.5, 0.0), (0.2, 0.9, 0.0), (-0.2, 0.9, 0.0)], (0, 0, 1))
    out["dielectric"] = (build(sub("glass"), [(WHITE, r), (LIGHT, {"lamp": lamp()}), (GLASS, {"shard": shard})]),
                         set(), walls | {"ceiling", "lamp", "shard"}, 4)
    big = {k: v for k, v in room(1000.0).items()}
    cam = dict(SS.CORNELL_CAM, lookfrom=(0.0, 1000.0, 3900.0), lookat=(0.0, 1000.0, 0.0))
    out["scaled"] = (build(sub("big"), [(WHITE, big), (LIGHT, {"lamp": lamp(1000.0)})], camera=cam),
                     set(), walls | {"ceiling", "lamp"}, 3)
    return out
