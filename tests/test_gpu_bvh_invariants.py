"""The boxes of the built trees, not only their topology.

The GPU builders' node boxes (k_refit's acquire / release handshake between sibling threads,
k_ploc_merge, k_sah_level: csrc/frt_lbvh.hip) go into the scene unchanged, and films judge
them only at RMSE 1e-4 to 1e-3: a box a few ulps short loses a handful of rays and passes.
Here every node's box must EQUAL the union of the outward-rounded fp32 boxes of the primitives
beneath it (f_down / f_up of frt_scene_build_bvh_gpu_algo, csrc/host/scene.cpp, over the fp64 boxes
of csrc/host/bvh_build.cpp prim_boxes; min and max are exact, so equality is the test), a second build must give the same tree, and the tree must answer rays as the list of
its primitives does (trace_rays.gate_exact).  Inputs: Cornell, its tessellations, veach_mis
(spheres) and the degenerate sets a builder meets first -- 2 and 3 primitives, 64 copies of
one triangle (every Morton code equal, every SAH bin but one empty), 300 triangles in one
plane (no extent on an axis), 257 triangles (one over a block).

CPU: the host builders' trees (csrc/host/bvh_build.cpp: build_bvh_sah, the reference topology) keep fp64 boxes, which
must contain those unions' fp64 sources."""
import numpy as np
import pytest
import torch

import first_raytracer_amd as frt
import trace_rays as TR
from test_gpu_lbvh import check_tree

BUILDERS = ("ploc", "lbvh", "gsah")
GREY = {"type": "lambertian", "albedo": (0.5, 0.5, 0.5)}
INPUTS = ("cornell", "k6", "k24", "veach_mis", "two", "three", "copies64", "flat300", "block257")


def write_obj(path, tris):
    lines, k = [], 1
    for t in tris:
        lines += ["v %r %r %r" % tuple(float(x) for x in v) for v in t]
        lines.append(f"f {k} {k + 1} {k + 2}")
        k += 3
    path.write_text("\n".join(lines) + "\n")
    return str(path)


def small_set(name):
    """(n, 3, 3) triangles of a degenerate input."""
    rng = np.random.default_rng(11)
    if name in ("two", "three"):
        n = 2 if name == "two" else 3
        return rng.uniform(-1.0, 1.0, (n, 3, 3)) + np.arange(n)[:, None, None] * (0.5, 0.0, 0.0)
    if name == "copies64":
        return np.repeat(rng.uniform(-1.0, 1.0, (1, 3, 3)), 64, axis=0)
    if name == "flat300":                       # a 15 x 10 grid of quads in the plane y = 0.25, two triangles each
        out = []
        for i in range(15):
            for j in range(10):
                x, z = 0.1 * i, 0.1 * j
                a, b, c, d = (x, 0.25, z), (x + 0.1, 0.25, z), (x + 0.1, 0.25, z + 0.1), (x, 0.25, z + 0.1)
                out += [(a, b, c), (a, c, d)]
        return np.array(out)
    if name == "block257":
        c = rng.uniform(-1.0, 1.0, (257, 1, 3))
        return c + rng.uniform(-0.05, 0.05, (257, 3, 3))
    raise KeyError(name)


@pytest.fixture(scope="module")
def make(cornell_obj, veach_obj, tmp_path_factory):
    """name -> a fresh list-world scene of that input."""
    tmp = tmp_path_factory.mktemp("bvh_invariants")
    objs = {}

    def get(name):
        if name in TR.MESHES:
            return TR.scene_pair(name, cornell_obj, veach_obj, tmp)[0]
        if name not in objs:
            objs[name] = write_obj(tmp / (name + ".obj"), small_set(name))
        return frt.HostScene.from_spec(TR.obj_spec(objs[name], "list", GREY), 1.0)
    return get


def f_down(x):
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) > x, np.nextafter(f, np.float32(-np.inf)), f)


def f_up(x):
    f = np.asarray(x, np.float64).astype(np.float32)
    return np.where(f.astype(np.float64) < x, np.nextafter(f, np.float32(np.inf)), f)


def prim_boxes(a, rounded):
    """ref -> (lo, hi) as fp64 values for the triangles and spheres of arrays(): the fp64 boxes, or
    (rounded) the fp32 boxes rounded outward that frt_scene_build_bvh_gpu_algo hands the builders."""
    tv = a["tri_v"].reshape(-1, 3, 3)
    sp = a["sphere"].reshape(-1, 4)
    boxes = [tv.min(axis=1), tv.max(axis=1), sp[:, :3] - sp[:, 3:], sp[:, :3] + sp[:, 3:]]
    if rounded:
        boxes = [(f_up if k & 1 else f_down)(b).astype(np.float64) for k, b in enumerate(boxes)]
    tl, th, sl, sh = boxes
    return lambda ref: ((sl[ref & ~frt.FRT_PRIM_SPHERE], sh[ref & ~frt.FRT_PRIM_SPHERE]) if ref & frt.FRT_PRIM_SPHERE
                        else (tl[ref], th[ref]))


def check_topology(a, members):
    """check_tree without its root == 0: every primitive of the world in exactly one leaf, every
    node but the root with one parent."""
    child = a["node_child"].reshape(-1)
    assert len(a["node_child"]) == len(members) - 1
    assert sorted(int(~c) for c in child if c < 0) == [int(m) for m in members]
    assert sorted(int(c) for c in child if c >= 0) == sorted(set(range(len(members) - 1)) - {a["root"]})


def node_unions(a, rounded):
    """Per node the union of the boxes of the primitives beneath it (post-order over node_child);
    rounded: of their outward-rounded fp32 boxes, else of the fp64 boxes."""
    child, box_of = a["node_child"], prim_boxes(a, rounded)
    n = len(child)
    lo, hi = np.zeros((n, 3)), np.zeros((n, 3))
    done = np.zeros(n, bool)
    stack = [a["root"]]
    while stack:
        x = stack[-1]
        kids = [c for c in child[x] if c >= 0]
        if all(done[c] for c in kids):
            stack.pop()
            parts = []
            for c in child[x]:
                if c >= 0:
                    parts.append((lo[c], hi[c]))
                else:
                    parts.append(box_of(int(~c)))
            lo[x] = np.minimum(parts[0][0], parts[1][0])
            hi[x] = np.maximum(parts[0][1], parts[1][1])
            done[x] = True
        else:
            stack += [c for c in kids if not done[c]]
    assert done.all()
    return lo, hi


def canonical(a):
    """The tree with its nodes renumbered in left-first DFS order: [(box bytes | leaf ref), ...]."""
    out, stack = [], [a["root"]]
    while stack:
        x = stack.pop()
        if x < 0:
            out.append(int(~x))
        else:
            out.append(a["node_box"][x].tobytes())
            stack += [a["node_child"][x][1], a["node_child"][x][0]]
    return out


def trace(ctx, rays):
    dev = torch.device("cuda", 0)
    tr = torch.tensor(rays, device=dev)
    th = torch.empty((len(rays), 4), dtype=torch.float32, device=dev)
    ctx.trace_device(tr.data_ptr(), len(rays), th.data_ptr(), 0)
    return th.cpu().numpy()


@pytest.fixture(scope="module")
def ctx():
    c = frt.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def list_answers(make, ctx):
    """name -> (Geometry, rays, the list world's answers): 2,048 inside_random + 2,048 to_vertex."""
    made = {}

    def get(name):
        if name not in made:
            hs = make(name)
            g = TR.Geometry(hs)
            rays = np.concatenate([TR.family("inside_random", g, 2048, 9), TR.family("to_vertex", g, 2048, 9)])
            ctx.upload(hs)
            made[name] = (g, rays, trace(ctx, rays))
        return made[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("how", BUILDERS)
@pytest.mark.parametrize("name", INPUTS)
def test_gpu_built_tree_boxes_and_answers(make, ctx, list_answers, name, how):
    g, rays, hl = list_answers(name)
    hs = make(name)
    n = hs.info.n_list
    assert n == len(g.tri_v) + len(g.sphere)
    hs.build_bvh_gpu(ctx, how)                     # a builder that gives up raises FrtError ("no merge progress", "no progress")
    check_tree(hs, n)
    a = hs.arrays()
    lo, hi = node_unions(a, rounded=True)
    assert np.array_equal(a["node_box"][:, 0:3], lo) and np.array_equal(a["node_box"][:, 3:6], hi)
    again = make(name)
    again.build_bvh_gpu(ctx, how)
    b = again.arrays()
    assert canonical(a) == canonical(b)
    if how != "gsah":                              # gsah hands out node ids with an atomic counter
        assert np.array_equal(a["node_child"], b["node_child"]) and np.array_equal(a["node_box"], b["node_box"])
    ctx.upload(hs)
    c = TR.gate_exact(g, rays, hl, trace(ctx, rays), None, f"{name} {how}")
    assert c["hits"] > 0.02 * len(rays)


@pytest.mark.parametrize("name", INPUTS)
def test_host_built_tree_boxes_contain(make, cornell_obj, veach_obj, tmp_path, name):
    """build_bvh_sah() on every input, and the reference-topology tree where from_spec builds one."""
    trees = [("sah", make(name))]
    members = np.sort(trees[0][1].arrays()["list"])
    trees[0][1].build_bvh_sah()
    if name in ("cornell", "k6", "k24"):
        trees.append(("reference", TR.scene_pair(name, cornell_obj, veach_obj, tmp_path)[1]))
    for label, hs in trees:
        a = hs.arrays()
        check_topology(a, members)
        lo, hi = node_unions(a, rounded=False)
        assert (a["node_box"][:, 0:3] <= lo).all() and (a["node_box"][:, 3:6] >= hi).all(), (name, label)
        # ... and no looser than one fp32 rounding of the union
        assert (a["node_box"][:, 0:3] >= f_down(lo).astype(np.float64)).all(), (name, label)
        assert (a["node_box"][:, 3:6] <= f_up(hi).astype(np.float64)).all(), (name, label)
