"""GPU: every BVH plan of frt_trace_device answers as the list of the same primitives does,
bit for bit, and the ray queue writes exactly the rows it was given.

The list world of a mesh is uploaded and traced once per family: the same fp32 tri_intersect /
sphere_intersect as the trees run, and no tree.  The same rays then go through the octant tree
in LDS (flags 0 where the scene fits), the 4-wide quantized BVH4Q from HBM
(FRT_FLAG_NO_LDS_SCENE), the binary tree from HBM (| FRT_FLAG_BVH2) and, on k24, the trees of
the three GPU builders, under trace_rays.gate_exact (test_trace_exact_host.py has the rule).
The list answer itself is held to the fp64 brute-force answer, so two equal wrong answers
cannot pass.  far(R), R = 10 and 100: every plan against brute force with the 99.8 % cap
(DESIGN.md section 3 has the measured losses beyond).

The queue: trace_kernel hands out 256-ray chunks per 64-lane wave in 256-thread blocks; batch
sizes on and around those boundaries must write rows [0, n) and nothing else, whatever lane a
ray lands in."""
import numpy as np
import pytest
import torch

import first_raytracer_amd as frt
import trace_rays as TR

pytestmark = pytest.mark.gpu

N = 4096
NO_LDS, BVH2 = frt.FRT_FLAG_NO_LDS_SCENE, frt.FRT_FLAG_NO_LDS_SCENE | frt.FRT_FLAG_BVH2
PLANS = (("default", 0), ("bvh4q", NO_LDS), ("bvh2", BVH2))
BUILDERS = ("ploc", "lbvh", "gsah")
SENTINEL = 0x7fc0dead                     # a NaN no kernel writes


def trace(ctx, rays, flags=0, n=None, guard=0):
    """hits (n, 4) float32 and the stats; guard: rows behind the n-th, returned too."""
    dev = torch.device("cuda", 0)
    n = len(rays) if n is None else n
    tr = torch.tensor(rays, device=dev)
    th = torch.full((max(len(rays), n) + guard, 4), SENTINEL, dtype=torch.int32, device=dev)
    st = ctx.trace_device(tr.data_ptr(), n, th.data_ptr(), flags)
    h = th.cpu().numpy()
    return (h.view(np.float32)[:n] if guard == 0 else h), st


def check_plan(st, plan, lds=None):
    """The plan that ran is the one the flags ask for (walk_plan, csrc/frt_plans.hpp)."""
    if plan == "bvh4q":
        assert (st.scene_in_lds, st.stack_entries) == (0, 12), (st.scene_in_lds, st.stack_entries)
    elif plan == "bvh2":
        assert st.scene_in_lds == 0 and st.stack_entries in (16, 32, 64) and st.bvh_depth < st.stack_entries
    elif lds:
        assert st.scene_in_lds == 1 and st.stack_entries in (8, 16) and st.bvh_depth < st.stack_entries
    else:
        assert (st.scene_in_lds, st.stack_entries) == (0, 12), (st.scene_in_lds, st.stack_entries)


class World:
    """One mesh: the list upload, the tree upload, on k24 the three builders' trees; the
    answers of the list world and of brute force per family, computed once."""

    def __init__(self, name, make_pair):
        self.name, self.make_pair = name, make_pair
        self.ls, self.bs = make_pair()
        self.g = TR.Geometry(self.ls)
        self.ctx = {"list": frt.Context(0), "tree": frt.Context(0)}
        self.ctx["list"].upload(self.ls)
        self.ctx["tree"].upload(self.bs)
        self.cache = {}

    def builder(self, how):
        if how not in self.ctx:
            c = frt.Context(0)
            hs = self.make_pair()[0]                      # a second list copy, which the builder turns into a tree
            hs.build_bvh_gpu(c, how)
            assert hs.info.world_kind == frt.FRT_WORLD_BVH and hs.info.n_nodes == len(self.g.tri_v) + len(self.g.sphere) - 1
            c.upload(hs)
            self.ctx[how] = c
        return self.ctx[how]

    def family(self, fam):
        """(rays, list hits, list closest hits for an any-hit family)."""
        if fam not in self.cache:
            rays = TR.rays_of(self.g, fam, N)
            hl, st = trace(self.ctx["list"], rays)
            assert st.stack_entries == 0 and st.scene_in_lds == 0           # the list kernel: no tree, no stack
            hc = trace(self.ctx["list"], TR.closest(rays))[0] if TR.is_anyhit(rays).any() else None
            self.cache[fam] = (rays, hl, hc)
        return self.cache[fam]

    def close(self):
        for c in self.ctx.values():
            c.close()


@pytest.fixture(scope="module")
def world(cornell_obj, veach_obj, tmp_path_factory):
    made, tmp = {}, tmp_path_factory.mktemp("gpu_trace_exact")

    def get(name):
        if name not in made:
            made[name] = World(name, lambda: TR.scene_pair(name, cornell_obj, veach_obj, tmp))
        return made[name]
    yield get
    for w in made.values():
        w.close()


LDS_FITS = {"cornell": True, "k6": None, "k24": False, "veach_mis": True}    # None: either, the stats say which


@pytest.mark.parametrize("fam", TR.FAMILIES)
@pytest.mark.parametrize("mesh", TR.MESHES)
def test_list_answer_meets_fp64(world, mesh, fam):
    w = world(mesh)
    rays, hl, _ = w.family(fam)
    (TR.gate_fp64_edge if fam in TR.EDGE_FAMILIES else TR.gate_fp64)(w.g, rays, hl, None, f"{mesh} {fam} gpu list")


@pytest.mark.parametrize("fam", TR.FAMILIES)
@pytest.mark.parametrize("mesh", TR.MESHES)
def test_every_plan_equals_list(world, mesh, fam):
    w = world(mesh)
    rays, hl, hc = w.family(fam)
    for plan, flags in PLANS:
        hb, st = trace(w.ctx["tree"], rays, flags)
        lds = LDS_FITS[mesh] if LDS_FITS[mesh] is not None else bool(st.scene_in_lds)
        check_plan(st, plan, lds)
        TR.gate_exact(w.g, rays, hl, hb, hc, f"{mesh} {fam} {plan}")


@pytest.mark.parametrize("fam", TR.FAMILIES)
@pytest.mark.parametrize("how", BUILDERS)
def test_gpu_built_trees_equal_list(world, how, fam):
    w = world("k24")
    rays, hl, hc = w.family(fam)
    for plan, flags in (("default", 0), ("bvh2", BVH2)):
        hb, st = trace(w.builder(how), rays, flags)
        check_plan(st, plan, False)
        TR.gate_exact(w.g, rays, hl, hb, hc, f"k24 {how} {fam} {plan}")


@pytest.mark.parametrize("R", [10, 100])
@pytest.mark.parametrize("mesh", TR.MESHES)
def test_far_origins_meet_fp64(world, mesh, R):
    """Every plan against brute force, the list first.  (The host replay loses no ray here.)"""
    w = world(mesh)
    rays, hl, _ = w.family(f"far{R}")
    ref = TR.brute_force(w.g, rays)
    TR.gate_fp64(w.g, rays, hl, ref, f"{mesh} far{R} gpu list")
    trees = [("tree", p, f) for p, f in PLANS]
    if mesh == "k24":
        trees += [(how, p, f) for how in BUILDERS for p, f in (("default", 0), ("bvh2", BVH2))]
    for which, plan, flags in trees:
        hb, st = trace(w.builder(which) if which in BUILDERS else w.ctx["tree"], rays, flags)
        TR.gate_fp64(w.g, rays, hb, ref, f"{mesh} far{R} {which} {plan}")


# ---- the ray queue's edges ----

QUEUE_N = (1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)
GUARD = 64


@pytest.fixture(scope="module")
def queue_batch(world):
    """4,097 fixed rays of every kind on Cornell, and the answers of one 4,097-ray call per plan."""
    w = world("cornell")
    per = 4097 // len(TR.FAMILIES) + 1
    rays = np.concatenate([TR.family(f, w.g, per, 5) for f in TR.FAMILIES])
    rays = rays[np.random.default_rng(5).permutation(len(rays))[:4097]]
    full = {}
    for plan, flags in PLANS[:2]:
        full[plan], st = trace(w.ctx["tree"], rays, flags)
        check_plan(st, plan, True)
    return w, rays, full


@pytest.mark.parametrize("plan,flags", PLANS[:2])
@pytest.mark.parametrize("n", QUEUE_N)
def test_queue_writes_its_rows_and_no_other(queue_batch, n, plan, flags):
    w, rays, full = queue_batch
    raw, st = trace(w.ctx["tree"], rays, flags, n=n, guard=GUARD)
    assert st.camera_rays == n
    assert raw.shape == (4097 + GUARD, 4)
    assert (raw[:n, 0] != SENTINEL).all() and (raw[:n, 3] != SENTINEL).all()        # every row below n is written
    assert (raw[n:] == SENTINEL).all()                                               # and no row behind it
    assert np.array_equal(raw[:n], full[plan][:n].view(np.int32))                    # row i is the big call's row i


@pytest.mark.parametrize("plan,flags", PLANS[:2])
def test_queue_order_and_repeat(queue_batch, plan, flags):
    w, rays, full = queue_batch
    perm = np.random.default_rng(6).permutation(len(rays))
    hp, _ = trace(w.ctx["tree"], rays[perm], flags)
    assert np.array_equal(hp.view(np.int32), full[plan][perm].view(np.int32))        # a permuted batch: permuted answers
    a, _ = trace(w.ctx["tree"], rays, flags)
    b, _ = trace(w.ctx["tree"], rays, flags)                                         # the queue head is reset per call
    assert np.array_equal(a.view(np.int32), full[plan].view(np.int32)) and np.array_equal(a.view(np.int32), b.view(np.int32))
    short, _ = trace(w.ctx["tree"], rays, flags, n=65)                               # a short call after a long one
    assert np.array_equal(short.view(np.int32), full[plan][:65].view(np.int32))
