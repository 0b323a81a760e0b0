"""CPU: a BVH world answers ray queries as the list of its primitives does, bit for bit.

frt.selftest_trace_host runs trace_bvh (the binary tree over the padded fp32 boxes of
flatten_scene) and trace_list on the host: the same fp32 tri_intersect / sphere_intersect on
both sides, so the only thing that can part the answers is a box that culls a hit.  The rays
are trace_rays' families -- zero direction components, exact vertices, shared edges, origins
on a surface, shadow segments -- 4,096 per family on Cornell, its tessellations k6 and k24 and
veach_mis.  trace_rays.gate_exact is the gate: t bit-equal; u, v bit-equal with the same
primitive; another primitive only at a tie proven in fp64; a ray is exempt only where the
BVH's scaled t_min and the list's EPSILON part (at most 0.1 % of a family).

Measured (host replay, seed 1): no ray of any family on any mesh differs outside the t_min
rule; at most 3 of 4,096 are exempt (veach_mis, whose origins reach |o| = 10); up to 980 ties
per family.  40,000 rays per family on k24 give the same picture: 2 exempt rays in to_vertex,
both by the t_min rule, and no lost hit.  With the boxes shrunk by 2e-7 of the scene instead
of padded, to_vertex, to_edge and from_camera fail on every mesh.

Far origins: the no-lost-hit property is a property of origins in or
near the scene.  far(R) at R = 10 and 100 is held to the fp64 brute-force answer with the
project's 99.8 % cap: first the list world alone, then the tree."""
import numpy as np
import pytest

import first_raytracer_amd as frt
import oracle
import trace_rays as TR

N = 4096


@pytest.fixture(scope="module")
def world(cornell_obj, veach_obj, tmp_path_factory):
    """name -> (list scene, tree scene, Geometry), built on first use."""
    made, tmp = {}, tmp_path_factory.mktemp("trace_exact")

    def get(name):
        if name not in made:
            ls, bs = TR.scene_pair(name, cornell_obj, veach_obj, tmp)
            assert ls.info.world_kind == frt.FRT_WORLD_LIST and bs.info.world_kind == frt.FRT_WORLD_BVH
            made[name] = (ls, bs, TR.Geometry(ls))
        return made[name]
    return get


@pytest.mark.parametrize("fam", TR.FAMILIES)
@pytest.mark.parametrize("mesh", TR.MESHES)
def test_tree_replay_equals_list(world, mesh, fam):
    ls, bs, g = world(mesh)
    rays = TR.family(fam, g, N, 1)
    assert rays.shape == (N, 8) and rays.dtype == np.float32 and np.isfinite(rays).all()
    hl, hb = frt.selftest_trace_host(ls, rays), frt.selftest_trace_host(bs, rays)
    hc = frt.selftest_trace_host(ls, TR.closest(rays)) if fam == "shadow_segments" else None
    c = TR.gate_exact(g, rays, hl, hb, hc, f"{mesh} {fam}")
    assert c["hits"] > 0.1 * N


@pytest.mark.parametrize("fam", TR.FAMILIES)
@pytest.mark.parametrize("mesh", ["cornell", "k6", "veach_mis"])
def test_list_replay_meets_fp64(world, mesh, fam):
    """The reference side of the gate is itself right: the list replay against brute force."""
    ls, _, g = world(mesh)
    rays = TR.family(fam, g, N, 1)
    hl = frt.selftest_trace_host(ls, rays)
    (TR.gate_fp64_edge if fam in TR.EDGE_FAMILIES else TR.gate_fp64)(g, rays, hl, None, f"{mesh} {fam} list")


@pytest.mark.parametrize("R", [10, 100])
@pytest.mark.parametrize("mesh", TR.MESHES)
def test_far_origins_meet_fp64(world, mesh, R):
    ls, bs, g = world(mesh)
    rays = TR.far(g, N, 1, R)
    ref = TR.brute_force(g, rays)
    assert (ref[1] >= 0).all()                       # aimed at interior points: every ray has a hit
    TR.gate_fp64(g, rays, frt.selftest_trace_host(ls, rays), ref, f"{mesh} far{R} list")
    TR.gate_fp64(g, rays, frt.selftest_trace_host(bs, rays), ref, f"{mesh} far{R} tree")


def test_families_are_deterministic_and_what_they_say(world):
    _, _, g = world("cornell")
    for fam in TR.FAMILIES:
        a, b = TR.family(fam, g, 257, 3), TR.family(fam, g, 257, 3)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), fam
        assert not np.array_equal(a, TR.family(fam, g, 257, 4)), fam
    d = TR.family("zero_component", g, 512, 1)[:, 4:7]
    assert ((d == 0.0).sum(axis=1) == 1).all() and np.signbit(d[d == 0.0]).any() and not np.signbit(d[d == 0.0]).all()
    d = TR.family("axis_parallel", g, 512, 1)[:, 4:7]
    assert ((d == 0.0).sum(axis=1) == 2).all() and (np.abs(d).sum(axis=1) == 1.0).all()
    r = TR.family("shadow_segments", g, 64, 1)
    assert TR.is_anyhit(r).all() and (r[:, 3] == np.float32(1.0 - 1e-3)).all()
    r = TR.family("to_vertex", g, 512, 1)                # o + d is a vertex, to the rounding of the fp32 subtraction
    tip = r[:, 0:3].astype(np.float64) + r[:, 4:7]
    vert = g.tri_v.reshape(-1, 3)
    assert (np.abs(tip[:, None, :] - vert[None]).max(axis=2).min(axis=1) <= 4e-7).all()
    r = TR.far(g, 512, 1, 100)
    centre = 0.5 * (g.lo + g.hi)
    assert np.allclose(np.linalg.norm(r[:, 0:3] - centre, axis=1), 100.0, rtol=1e-6)
    assert np.allclose(np.linalg.norm(r[:, 4:7].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert (TR.family("from_camera", g, 64, 1)[:, 0:3] == g.lookfrom.astype(np.float32)).all()


def test_gate_catches_what_it_is_for(world):
    """One lost hit, a t one ulp off, a wrong primitive or barycentric among 4,096 rays: each fails the gate."""
    ls, bs, g = world("cornell")
    rays = TR.family("inside_random", g, N, 1)
    hl, hb = frt.selftest_trace_host(ls, rays), frt.selftest_trace_host(bs, rays)
    TR.gate_exact(g, rays, hl, hb)
    i = int(np.flatnonzero(TR.prim_of(hl) >= 0)[7])

    def tampered(col, bits):
        h = hb.copy()
        h.view(np.uint32)[i, col] = bits
        return h
    one_ulp = hb.view(np.uint32)[i, 0] + 1
    wrong_prim = (int(TR.prim_of(hl)[i]) + 5) % len(g.tri_v)        # no triangle of Cornell coincides with the fifth after it
    lost = hb.copy()
    lost[i] = (rays[i, 3], 0.0, 0.0, np.array([-1], np.int32).view(np.float32)[0])
    for bad in (lost, tampered(0, one_ulp), tampered(3, wrong_prim), tampered(1, hb.view(np.uint32)[i, 1] ^ 1)):
        with pytest.raises(AssertionError):
            TR.gate_exact(g, rays, hl, bad)
    with pytest.raises(AssertionError):                             # ... and the fp64 gate a t 2e-5 off
        off = hl.copy()
        off[i, 0] *= np.float32(1.0 + 2e-5) if off[i, 0] >= 1.0 else np.float32(1.0)
        off[i, 0] += np.float32(2e-5) if hl[i, 0] < 1.0 else np.float32(0.0)
        TR.gate_fp64(g, rays, off, None)


def test_brute_force_is_the_oracles_answer(cornell_obj, veach_obj):
    """The numpy reference against the C oracle's world_hit on rays in general position."""
    for kind, obj in (("cornell_box_obj", cornell_obj), ("veach_mis", veach_obj)):
        hs = frt.HostScene(kind, obj, 1.0)
        g = TR.Geometry(hs)
        rays = TR.family("inside_random", g, 256, 2)
        bvh = hs.info.world_kind == frt.FRT_WORLD_BVH
        tmin = TR.bvh_tmin(rays).astype(np.float64) if bvh else None
        t64, p64 = TR.brute_force(g, rays, tmin)
        osc = oracle.OracleScene(kind, obj, 1.0)
        hits = 0
        for i, r in enumerate(rays.astype(np.float64)):
            ok, t, p, _ = osc.world_hit(r[0:3], r[4:7], 1e-4, float(r[3]))
            assert ok == (p64[i] >= 0), (kind, i)
            if ok:
                hits += 1
                assert abs(t - t64[i]) <= 1e-12 * max(1.0, t), (kind, i, t, t64[i])
                # coincident triangles tie: the oracle's tree names the first in its DFS order
                assert p == p64[i] or abs(TR.prim_hit64(g, rays[i:i + 1], [p])[0][0] - t) <= 1e-12 * max(1.0, t)
        assert hits > 64
