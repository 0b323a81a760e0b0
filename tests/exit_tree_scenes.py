"""Rooms for the exit-tree tests (tests/test_exit_tree_host.py, tests/test_gpu_exit_tree.py), beside those
of tests/shadow_tree_scenes.py: each is a case the pass's proof must refuse or handle.  name -> Built."""
import os

import numpy as np

import scene_specs as SS
import shadow_tree_scenes as STS


def box(x0, x1, y0, y1, z0, z1):
    """six quads with outward normals"""
    c = ((x0 + x1) / 2, (y0 + y1) / 2, (z0 + z1) / 2)
    out = {}
    for name, q in {
        "bottom": [(x0, y0, z0), (x1, y0, z0), (x1, y0, z1), (x0, y0, z1)],
        "top": [(x0, y1, z0), (x1, y1, z0), (x1, y1, z1), (x0, y1, z1)],
        "west": [(x0, y0, z0), (x0, y0, z1), (x0, y1, z1), (x0, y1, z0)],
        "east": [(x1, y0, z0), (x1, y0, z1), (x1, y1, z1), (x1, y1, z0)],
        "south": [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0)],
        "north": [(x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)],
    }.items():
        mid = np.mean(np.asarray(q, np.float64), axis=0)
        out["box_" + name] = STS.facing(q, mid - np.asarray(c))
    return out


def poke(a):
    """a vertical quad under the floor whose upper edge stands a above the floor's plane"""
    return STS.facing([(-0.3, -0.5, 0.1), (0.3, -0.5, 0.1), (0.3, a, 0.1), (-0.3, a, 0.1)], (0, 0, 1))


def scenes(tmp):
    out = {}
    sub = lambda n: (os.makedirs(os.path.join(tmp, n), exist_ok=True), os.path.join(tmp, n))[1]   # noqa: E731
    r = STS.room()
    lamp = (STS.LIGHT, {"lamp": STS.lamp()})
    # a wall whose stored normal faces out of the room: its rays leave outward, everything is behind them
    out["outward_wall"] = STS.build(sub("ow"), [(STS.WHITE, dict(r, back=r["back"][::-1], block=STS.block())), lamp])
    # a quad that straddles the floor's plane by less than the proof's tolerance (tau = 8 * 2^-24 * 3.9), and by more
    out["straddle_less"] = STS.build(sub("sl"), [(STS.WHITE, dict(r, poke=poke(5e-7), block=STS.block())), lamp])
    out["straddle_more"] = STS.build(sub("sm"), [(STS.WHITE, dict(r, poke=poke(1e-3), block=STS.block())), lamp])
    # a box whose bottom is coplanar with the floor
    out["box_on_floor"] = STS.build(sub("bf"), [(STS.WHITE, dict(r, **box(-0.5, 0.1, 0.0, 0.7, -0.4, 0.2))), lamp])
    # a folded quad, normals up: the two triangles of its leaf are not coplanar and each stands above the other's plane
    fold = [np.asarray(p, np.float64) for p in [(-0.4, 0.3, -0.4), (-0.4, 0.9, 0.4), (0.4, 0.3, 0.4), (0.4, 0.3, -0.4)]]
    out["folded_leaf"] = STS.build(sub("fl"), [(STS.WHITE, dict(r, fold=fold)), lamp])
    # a slanted wall in place of the back wall
    slant = STS.facing([(-1, 0, -0.2), (1, 0, -0.2), (1, 2, -1), (-1, 2, -1)], (0, 0.4, 1))
    out["slanted_wall"] = STS.build(sub("sw"), [(STS.WHITE, dict(r, slant=slant, block=STS.block())), lamp])
    # one specular material: the pass is off
    shard = STS.facing([(-0.2, 0.5, 0.0), (0.2, 0.5, 0.0), (0.2, 0.9, 0.0), (-0.2, 0.9, 0.0)], (0, 0, 1))
    out["specular"] = STS.build(sub("sp"), [(STS.WHITE, r), lamp, (STS.GLASS, {"shard": shard})])
    # a thousand times the size: the offset no longer dominates the rounding
    cam = dict(SS.CORNELL_CAM, lookfrom=(0.0, 1000.0, 3900.0), lookat=(0.0, 1000.0, 0.0))
    out["scaled"] = STS.build(sub("big"), [(STS.WHITE, STS.room(1000.0)), (STS.LIGHT, {"lamp": STS.lamp(1000.0)})], camera=cam)
    # 26 leaves: 25 nodes, 52 triangles and two materials are 14120 of the octant plan's 14336 bytes,
    # so no node can be appended
    tiles = {}
    for i in range(20):
        x, z, y = -0.8 + 0.4 * (i % 5), -0.7 + 0.4 * (i // 5), 0.2 + 0.07 * i
        tiles[f"tile{i}"] = STS.facing([(x, y, z), (x + 0.25, y, z), (x + 0.25, y, z + 0.25), (x, y, z + 0.25)], (0, 1, 0))
    out["full_lds"] = STS.build(sub("full"), [(STS.WHITE, dict(r, **tiles)), lamp])
    return out


WHY = {"specular": "material", "scaled": "too_large"}
