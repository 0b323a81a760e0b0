"""Ray families for the ray-query tests, the fp64 brute-force answer to them and
the gate that pins a BVH plan's answers to the list world's.

A ray is 8 float32 as frt_trace_device reads it: origin, t_max, direction, flags
(bit 0 = any hit).  Every family is deterministic in (scene, seed).  The families
sit where a slab test or a leaf tie goes wrong: zero direction components (the
+-1e-30 nudge of slab_ray), rays through exact vertices and along shared edges
(several triangles answer at one t), origins on a surface (t near t_min), and
origins far from the scene (the slab distances lose their low bits).

brute_force is Moller-Trumbore over every triangle plus the sphere test in fp64
numpy, with the acceptance rules of tri_intersect / sphere_intersect
(csrc/frt_device.hpp): a != 0, 0 <= u <= 1, v >= 0, u + v <= 1, t in (t_min,
t_max] for a triangle and [t_min, t_max] for a sphere.  The triple products are
regrouped so that the per-pair work is six (n, 3) x (3, n_tris) products:
  a = e1 . (d x e2)        = -d . N                      N = e1 x e2
  t a = e2 . (s x e1)      = (o - v0) . N
  u a = s . (d x e2)       = e2 . (o x d) - d . (e2 x v0)
  v a = d . (s x e1)       = e1 . (d x o) - d . (v0 x e1)
"""
import numpy as np

FRT_PRIM_SPHERE = 1 << 30
EPS = np.float32(1e-4)                 # util.h EPSILON as the fp32 kernels hold it
T_INF = np.float32(3.4e38)
SHADOW_TMAX = np.float32(1.0 - 1e-3)   # 1 - SHADOW_EPSILON
ANYHIT = np.array([1], np.int32).view(np.float32)[0]

# An aimed ray keeps this |cosine| to the normal of every triangle that holds the point it is
# aimed at (the target's own, those that share the vertex or edge, a face it lies on).  Both gates
# compare an fp32 t with an fp64 one to 1e-5 max(1, t) (test_gpu_trace.py's tolerance), and fp32
# Moller-Trumbore cannot meet that at grazing incidence whatever the traversal does: the rounding
# error of t = e2 . (s x e1) / a is of the order 2^-24 |s| |e1| |e2| |d| / |a|, which grows as
# 1 / cos.  On Cornell (|s|, |e1|, |e2| ~ 2) that is 1e-6 / cos; the host replay of the list
# world, no tree involved, is off the fp64 t by 1.2e-5 at cos 2.6e-3 and 3.7e-5 at cos 7e-4, and
# by at most 5e-6 from cos 5e-3 up.  0.02 leaves a factor 4 to the tolerance.  Rays that graze
# some other triangle on their way stay in.
MIN_COS = 0.02

FAMILIES = ("inside_random", "zero_component", "axis_parallel", "to_vertex", "to_edge", "to_interior", "on_surface",
            "from_camera", "shadow_segments")


class Geometry:
    """What the families and the reference need of a scene: fp64 triangles and
    spheres (HostScene.arrays()), the root box of all primitives, the camera."""

    def __init__(self, hs):
        a = hs.arrays()
        self.tri_v = a["tri_v"].reshape(-1, 3, 3)
        self.sphere_all = a["sphere"].reshape(-1, 4)
        # the world's primitives: a list world's list, a tree's leaves (veach_mis keeps a second
        # copy of its emitting spheres for the light list alone)
        refs = a["list"] if len(a["list"]) else np.array([~c for c in a["node_child"].reshape(-1) if c < 0] or
                                                         [~a["root"]], np.int64)
        self.members = np.sort(np.asarray(refs, np.int64))
        assert np.array_equal(self.members[self.members < FRT_PRIM_SPHERE], np.arange(len(self.tri_v)))
        self.sphere_ids = self.members[self.members >= FRT_PRIM_SPHERE] & ~FRT_PRIM_SPHERE
        self.sphere = self.sphere_all[self.sphere_ids]
        lo = [self.tri_v.reshape(-1, 3).min(0)] if len(self.tri_v) else []
        hi = [self.tri_v.reshape(-1, 3).max(0)] if len(self.tri_v) else []
        if len(self.sphere):
            lo.append((self.sphere[:, :3] - self.sphere[:, 3:]).min(0))
            hi.append((self.sphere[:, :3] + self.sphere[:, 3:]).max(0))
        self.lo, self.hi = np.min(lo, 0), np.max(hi, 0)
        # the region the 'inside' origins come from: the root box, an axis on which the scene is
        # (nearly) flat opened to half the largest extent on either side, or every ray would lie
        # in the scene's plane
        ext = self.hi - self.lo
        pad = np.where(ext < 1e-3 * ext.max(), 0.5 * ext.max(), 0.0)
        self.lo, self.hi = self.lo - pad, self.hi + pad
        self.lookfrom = np.array(hs.view().cam_origin[:], np.float64)
        # precomputed per-triangle terms of the regrouped triple products
        v0, e1, e2 = self.tri_v[:, 0], self.tri_v[:, 1] - self.tri_v[:, 0], self.tri_v[:, 2] - self.tri_v[:, 0]
        self.v0, self.e1, self.e2 = v0, e1, e2
        self.N = np.cross(e1, e2)
        self.v0N = np.einsum("ij,ij->i", v0, self.N)
        self.e2xv0 = np.cross(e2, v0)
        self.v0xe1 = np.cross(v0, e1)
        # ... and of a point's plane distance and barycentrics (_min_cos), of the rounding bound
        self.Nlen = np.linalg.norm(self.N, axis=1)
        self.A, self.B = np.cross(e2, self.N), np.cross(self.N, e1)      # (w x e2) . N = w . A, (e1 x w) . N = w . B
        self.v0A, self.v0B = np.einsum("ij,ij->i", v0, self.A), np.einsum("ij,ij->i", v0, self.B)
        self.v0sq = np.einsum("ij,ij->i", v0, v0)
        self.le1, self.le2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)


MESHES = ("cornell", "k6", "k24", "veach_mis")
CAMERA = {"lookfrom": (0.0, 1.0, float(np.float32(3.9))), "lookat": (0.0, 1.0, 0.0), "vup": (0.0, 1.0, 0.0),
          "vfov": 40.0, "aperture": 0.0, "focus": 10.0}            # cornell_box_obj's


def obj_spec(obj, world, bsdf=None):
    o = {"obj": str(obj), "geo": True}
    if bsdf is not None:
        o["bsdf"] = bsdf
    return {"objects": [o], "camera": CAMERA, "world": world}


def scene_pair(name, cornell_obj, veach_obj, tmpdir):
    """(list-world scene, BVH-world scene) of one of MESHES, the same primitives in both: Cornell,
    its tessellations k6 (1,226 triangles) and k24 (19,586), each built twice from one spec; and
    veach_mis (spheres; a list world), whose BVH side is build_bvh_sah() on a second copy."""
    import first_raytracer_amd as frt
    if name == "veach_mis":
        tree = frt.HostScene("veach_mis", veach_obj, 1.0)
        tree.build_bvh_sah()
        return frt.HostScene("veach_mis", veach_obj, 1.0), tree
    obj = cornell_obj
    if name != "cornell":
        obj = str(tmpdir / (name + ".obj"))
        frt.write_tessellated_obj(cornell_obj, int(name[1:]), obj)
    return frt.HostScene.from_spec(obj_spec(obj, "list"), 1.0), frt.HostScene.from_spec(obj_spec(obj, "bvh"), 1.0)


def rays_of(g, fam, n, seed=1):
    """family() by name, 'far10' / 'far100' / ... included."""
    return far(g, n, seed, int(fam[3:])) if fam.startswith("far") else family(fam, g, n, seed)


def pack(o, d, tmax=T_INF, anyhit=False):
    n = len(o)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = o
    r[:, 3] = tmax
    r[:, 4:7] = d
    if anyhit:
        r[:, 7] = ANYHIT
    return r


def _inside(g, rng, n):
    return rng.uniform(g.lo, g.hi, (n, 3)).astype(np.float32)


def _bary(rng, n, floor):
    """Barycentrics with every weight >= floor."""
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    return floor + (1.0 - 3.0 * floor) * w


def _targets(g, rng, n, what):
    """Points of the triangles as float32 -- exact vertices, points on edges, interior points --
    and the triangle each lies on."""
    k = rng.integers(0, len(g.tri_v), n)
    tri = g.tri_v[k]
    if what == "vertex":
        p = tri[np.arange(n), rng.integers(0, 3, n)]
    elif what == "edge":
        c = rng.integers(0, 3, n)
        a, b = tri[np.arange(n), c], tri[np.arange(n), (c + 1) % 3]
        s = rng.uniform(0.02, 0.98, (n, 1))
        p = a + s * (b - a)
    else:
        p = np.einsum("nk,nkj->nj", _bary(rng, n, 0.05), tri)
    return p.astype(np.float32), k


def _min_cos(g, o, p, block=None):
    """Per ray o -> p: the smallest |cosine| between the ray and the normal of a triangle that
    contains p (to 1e-4 in plane distance and in barycentrics: the triangles that meet in a
    vertex or an edge, coincident copies, a face the point merely lies on)."""
    n, tol = len(o), 1e-4
    out = np.ones(n)
    block = block or max(8, min(256, 300000 // len(g.tri_v)))
    p = p.astype(np.float64)
    d = p - o
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(0, n, block):
            P, D = p[s:s + block], d[s:s + block]
            u = (P @ g.A.T - g.v0A) / (g.Nlen * g.Nlen)
            v = (P @ g.B.T - g.v0B) / (g.Nlen * g.Nlen)
            on = (np.abs(P @ g.N.T - g.v0N) <= tol * g.Nlen) & (u >= -tol) & (v >= -tol) & (u + v <= 1.0 + tol)
            out[s:s + block] = np.where(on, np.abs(D @ g.N.T) / g.Nlen, 1.0).min(axis=1)
    return out


def _aimed(g, rng, n, what, origins, unit=False):
    """Rays from origins(n) to _targets(what), the direction formed in fp32 as a caller would
    (target - origin; unit: normalised).  A ray within MIN_COS of the plane of a triangle that
    holds its target is drawn again: see MIN_COS."""
    o, (p, k) = origins(n), _targets(g, rng, n, what)
    bad = np.ones(n, bool)
    for _ in range(64):
        bad[bad] = ~(_min_cos(g, o[bad], p[bad]) >= MIN_COS)
        if not bad.any():
            break
        m = int(bad.sum())
        o[bad] = origins(m)
        p[bad], k[bad] = _targets(g, rng, m, what)
    assert not bad.any()
    d = p.astype(np.float64) - o
    nd = np.linalg.norm(d, axis=1)
    if unit:
        d = d / nd[:, None]
    return o, d.astype(np.float32)


def _signed_zero(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)


def family(name, g, n, seed):
    """(n, 8) float32 rays of one family."""
    rng = np.random.default_rng([seed, FAMILIES.index(name)])
    if name == "inside_random":
        return pack(_inside(g, rng, n), rng.normal(size=(n, 3)))
    if name == "zero_component":
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d[np.arange(n), rng.integers(0, 3, n)] = _signed_zero(rng, n)
        return pack(_inside(g, rng, n), d)
    if name == "axis_parallel":
        d = np.stack([_signed_zero(rng, n) for _ in range(3)], 1)
        d[np.arange(n), rng.integers(0, 3, n)] = np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0)
        return pack(_inside(g, rng, n), d)
    if name in ("to_vertex", "to_edge", "to_interior"):
        return pack(*_aimed(g, rng, n, name[3:], lambda m: _inside(g, rng, m)))
    if name == "on_surface":
        return pack(_targets(g, rng, n, "interior")[0], rng.normal(size=(n, 3)))
    if name == "from_camera":
        cam = lambda m: np.broadcast_to(g.lookfrom.astype(np.float32), (m, 3)).copy()   # noqa: E731
        k = n // 3
        parts = [_aimed(g, rng, m, what, cam) for m, what in ((k, "vertex"), (k, "edge"), (n - 2 * k, "interior"))]
        return pack(np.concatenate([q[0] for q in parts]), np.concatenate([q[1] for q in parts]))
    if name == "shadow_segments":
        o, p = _inside(g, rng, n), _inside(g, rng, n)
        return pack(o, p - o, SHADOW_TMAX, anyhit=True)
    raise KeyError(name)


def far(g, n, seed, R, what="interior"):
    """Origins at centre + R * (unit vector), unit directions, aimed at interior points (what:
    "vertex" / "edge" for the measurements of DESIGN.md section 3)."""
    rng = np.random.default_rng([seed, 100, int(R)])

    def origins(m):
        w = rng.normal(size=(m, 3))
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        return (0.5 * (g.lo + g.hi) + R * w).astype(np.float32)
    return pack(*_aimed(g, rng, n, what, origins, unit=True))


def closest(rays):
    """The same rays as closest-hit queries (the any-hit bit cleared, t_max kept)."""
    r = rays.copy()
    r[:, 7] = 0.0
    return r


def prim_of(hits):
    return np.ascontiguousarray(hits[:, 3]).view(np.int32)


def bvh_tmin(rays):
    """bvh_tmin of csrc/frt_path.hpp in fp32: EPSILON * max(1, |o|_inf)."""
    return EPS * np.maximum(np.float32(1.0), np.abs(rays[:, 0:3]).max(axis=1))


# ---- the fp64 reference ----

def uv_bound(s_len, d_len, le1, le2, a):
    """How far fp32 barycentrics of a triangle may lie from the fp64 ones.  With e = 2^-24, a
    cross product's components carry <= 2 e |x| |y| and a 3-term dot product adds 3 e, so
    s . (d x e2) and a = e1 . (d x e2) are off by <= 5 e |s| |d| |e2| and 5 e |e1| |d| |e2|;
    u = num / a with |u| <= 1 is then off by <= 5 e (|s| + |e1|) |d| |e2| / |a| + 3 e
    (reciprocal, product).  The fp32 vertices and edges are themselves rounded (another e on
    each factor) and the device reciprocal is 1 ulp: 16 e (|s| + |e1| + |e2|) |d| max(|e1|,
    |e2|) / |a| + 8 e covers u and v alike."""
    return 2.0 ** -24 * (16.0 * (s_len + le1 + le2) * d_len * np.maximum(le1, le2) / np.abs(a) + 8.0)


def _tri_block(g, o, d, tmin, tmax, robust=False):
    """(t, prim) of the closest accepted triangle per ray of one block; t = inf on a miss.
    robust: only hits whose barycentrics are inside the triangle by more than uv_bound, the hits
    that no fp32 rounding can turn into a miss."""
    oxd = np.cross(o, d)
    a = -(d @ g.N.T)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 1.0 / a
        t = (o @ g.N.T - g.v0N) * f
        u = (oxd @ g.e2.T - d @ g.e2xv0.T) * f
        v = (-(oxd @ g.e1.T) - d @ g.v0xe1.T) * f
        if robust:
            s_len = np.sqrt(np.maximum(np.einsum("ij,ij->i", o, o)[:, None] - 2.0 * (o @ g.v0.T) + g.v0sq, 0.0))
            b = uv_bound(s_len, np.linalg.norm(d, axis=1)[:, None], g.le1, g.le2, a)
            ok = (a != 0.0) & (u >= b) & (v >= b) & (u + v <= 1.0 - 2.0 * b) & (t > tmin[:, None]) & (t <= tmax[:, None])
        else:
            ok = ((a != 0.0) & (u >= 0.0) & (u <= 1.0) & (v >= 0.0) & (u + v <= 1.0) & (t > tmin[:, None])
                  & (t <= tmax[:, None]))
    t = np.where(ok, t, np.inf)
    k = t.argmin(axis=1)
    return t[np.arange(len(o)), k], k


def _sphere_t(o, d, c, r, tmin, tmax):
    """sphere_intersect in fp64 for broadcastable (rays, spheres); inf on a miss."""
    oc = o - c
    a = np.einsum("...j,...j->...", d, d)
    b = np.einsum("...j,...j->...", oc, d)
    l = oc - (b / a)[..., None] * d
    disc = a * (r * r - np.einsum("...j,...j->...", l, l))
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(np.where(disc >= 0.0, disc, np.nan))
        t = (-b - sq) / a
        t = np.where(t < tmin, (-b + sq) / a, t)
        ok = (disc >= 0.0) & (t >= tmin) & (t <= tmax)
    return np.where(ok, t, np.inf)


def brute_force(g, rays, tmin=None, block=None, robust=False):
    """Closest hit of every ray over every primitive in fp64: (t, prim), t = inf and prim = -1 on a
    miss; prim is the view's triangle index or FRT_PRIM_SPHERE | k.  tmin: per ray (default EPSILON,
    the list world's).  robust: triangles count only where no fp32 rounding can lose them
    (_tri_block); spheres as ever."""
    from concurrent.futures import ThreadPoolExecutor
    r = rays.astype(np.float64)
    n = len(r)
    o, d, tmax = r[:, 0:3], r[:, 4:7], r[:, 3]
    tmin = np.full(n, float(EPS)) if tmin is None else np.asarray(tmin, np.float64)
    t, prim = np.full(n, np.inf), np.full(n, -1, np.int64)
    if len(g.tri_v):
        if block is None:        # (rays x triangles) temporaries of ~2.5 MB stay in cache: 2 to 4 times faster
            block = max(8, min(256, 300000 // len(g.tri_v)))
        cuts = [(s, min(s + block, n)) for s in range(0, n, block)]
        with ThreadPoolExecutor(8) as pool:          # numpy releases the GIL in the products and the element passes
            parts = list(pool.map(lambda se: _tri_block(g, o[se[0]:se[1]], d[se[0]:se[1]], tmin[se[0]:se[1]],
                                                        tmax[se[0]:se[1]], robust), cuts))
        t = np.concatenate([p[0] for p in parts])
        prim = np.where(np.isfinite(t), np.concatenate([p[1] for p in parts]), -1)
    if len(g.sphere):
        ts = _sphere_t(o[:, None, :], d[:, None, :], g.sphere[None, :, :3], g.sphere[None, :, 3], tmin[:, None],
                       tmax[:, None])
        k = ts.argmin(axis=1)
        tk = ts[np.arange(n), k]
        better = tk < t
        t = np.where(better, tk, t)
        prim = np.where(better, FRT_PRIM_SPHERE | g.sphere_ids[k], prim)
    return t, prim


def prim_hit64(g, rays, prim, tmin=None):
    """Ray i against primitive prim[i] alone in fp64: (t, u, v, uv_bound), t = inf on a miss
    (u = v = 0 for a sphere).  This is the tie proof, asked about a primitive that the fp32 code
    accepted: where the ray goes through a vertex or along an edge the fp64 barycentrics sit
    within rounding of 0 or 1 on either side, so a triangle counts as hit when they are inside
    it to within uv_bound(), and the caller compares t itself."""
    r = rays.astype(np.float64)
    n = len(r)
    o, d, tmax = r[:, 0:3], r[:, 4:7], r[:, 3]
    tmin = np.full(n, float(EPS)) if tmin is None else np.asarray(tmin, np.float64)
    prim = np.asarray(prim, np.int64)
    t_out, u_out, v_out, bound = np.full(n, np.inf), np.zeros(n), np.zeros(n), np.zeros(n)
    sph = (prim >= 0) & ((prim & FRT_PRIM_SPHERE) != 0)
    tri = (prim >= 0) & ~sph
    if tri.any():
        k = prim[tri]
        v0, e1, e2 = g.v0[k], g.e1[k], g.e2[k]
        h = np.cross(d[tri], e2)
        a = np.einsum("ij,ij->i", e1, h)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = 1.0 / a
            s = o[tri] - v0
            u = f * np.einsum("ij,ij->i", s, h)
            q = np.cross(s, e1)
            v = f * np.einsum("ij,ij->i", d[tri], q)
            t = f * np.einsum("ij,ij->i", e2, q)
            ln = lambda x: np.linalg.norm(x, axis=1)   # noqa: E731
            b = uv_bound(ln(s), ln(d[tri]), ln(e1), ln(e2), a)
            ok = (a != 0.0) & (u >= -b) & (v >= -b) & (u + v <= 1.0 + 2.0 * b)
        t_out[tri], u_out[tri], v_out[tri], bound[tri] = np.where(ok, t, np.inf), u, v, b
    if sph.any():
        q = g.sphere_all[prim[sph] & ~FRT_PRIM_SPHERE]
        t_out[sph] = _sphere_t(o[sph], d[sph], q[:, :3], q[:, 3], tmin[sph], tmax[sph])
    return t_out, u_out, v_out, bound


# ---- the gates ----

T_TOL = 1e-5    # |fp32 t - fp64 t| <= T_TOL max(1, t): test_gpu_trace.py's tolerance


def same_bits(a, b):
    return np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)


def is_anyhit(rays):
    return (np.ascontiguousarray(rays[:, 7]).view(np.int32) & 1) != 0


def gate_exact(g, rays, list_hits, bvh_hits, list_closest_hits=None, label=""):
    """A BVH plan's answers against the list world's on the same rays: both run the same fp32
    tri_intersect / sphere_intersect, so a tree that culls no hit gives the same closest t bit
    for bit, and with the same primitive the same u, v bit for bit.

    exempt   the list hit lies at t <= bvh_tmin(o) (1 + 1e-3), where the BVH's scaled t_min and
             the list's plain EPSILON legitimately part; at most 0.1 % of the rays.  An any-hit ray
             takes the t of the same segment's closest list hit (list_closest_hits).
    ties     the primitive differs at bit-equal t (the list keeps the first in list order, a tree
             the first in its DFS order): accepted only when the fp64 t of the tree's primitive
             on that ray is within 1e-5 max(1, t) of the list's t.  Coincident triangles give
             the same u, v; triangles that meet in the vertex or edge the ray goes through give
             their own, so there u, v are held to the fp64 barycentrics of the tree's primitive
             within prim_hit64's rounding bound instead.
    An any-hit ray has no defined t (any occluder serves): occlusion is compared.
    Returns {"exempt", "ties", "hits"}; raises AssertionError with the first offenders."""
    n = len(rays)
    anyhit = is_anyhit(rays)
    list_hits, bvh_hits = np.ascontiguousarray(list_hits), np.ascontiguousarray(bvh_hits)
    lp, bp = prim_of(list_hits), prim_of(bvh_hits)
    ref = list_hits
    if anyhit.any():
        assert list_closest_hits is not None
        ref = np.ascontiguousarray(np.where(anyhit[:, None], list_closest_hits, list_hits))
    exempt = (prim_of(ref) >= 0) & (ref[:, 0] <= bvh_tmin(rays) * np.float32(1.0 + 1e-3))
    hit_same = (lp >= 0) == (bp >= 0)
    t_same = same_bits(list_hits[:, 0], bvh_hits[:, 0])
    uv_same = same_bits(list_hits[:, 1:3], bvh_hits[:, 1:3]).all(axis=1)
    same = np.where(anyhit, hit_same, hit_same & t_same & (uv_same | (lp != bp)))
    bad = ~same & ~exempt
    assert not bad.any(), (label, "differ from the list answer", int(bad.sum()), "of", n,
                           [(int(i), rays[i].tolist(), list_hits[i].tolist(), int(lp[i]), bvh_hits[i].tolist(), int(bp[i]))
                            for i in np.flatnonzero(bad)[:4]])
    tie = same & ~anyhit & (lp != bp) & ~exempt
    if tie.any():
        idx = np.flatnonzero(tie)
        t64, u64, v64, uvb = prim_hit64(g, rays[idx], bp[idx])
        tl = list_hits[idx, 0].astype(np.float64)
        off = ~(np.abs(t64 - tl) <= T_TOL * np.maximum(1.0, tl))
        off |= ~uv_same[idx] & ~((np.abs(bvh_hits[idx, 1] - u64) <= uvb) & (np.abs(bvh_hits[idx, 2] - v64) <= uvb))
        assert not off.any(), (label, "primitive differs and is no tie", int(off.sum()),
                               [(int(idx[j]), rays[idx[j]].tolist(), list_hits[idx[j]].tolist(), int(lp[idx[j]]),
                                 bvh_hits[idx[j]].tolist(), int(bp[idx[j]]), float(t64[j]), float(u64[j]), float(v64[j]),
                                 float(uvb[j])) for j in np.flatnonzero(off)[:4]])
    counts = {"exempt": int(exempt.sum()), "exempt_differ": int((exempt & ~same).sum()), "ties": int(tie.sum()),
              "hits": int((lp >= 0).sum())}
    print(label, "rays", n, "hits", counts["hits"], "exempt", counts["exempt"], "of which differ", counts["exempt_differ"],
          "ties accepted", counts["ties"])
    assert counts["exempt"] <= 1e-3 * n, (label, counts)
    return counts


def gate_fp64(g, rays, hits, ref=None, label=""):
    """fp32 answers against brute_force (ref = its (t, prim), computed here when None) by
    test_gpu_trace.py's rule: hit-or-miss and the primitive agree on >= 99.8 % of the rays, and
    where they agree t is within 1e-5 max(1, t).  An any-hit ray agrees when occlusion does.
    brute_force names the lowest index among primitives at one t and a tree the first in its DFS
    order, so another primitive agrees when its own fp64 t is within the same tolerance of the
    closest one (gate_exact's tie rule).  Returns {"disagree", "lost", "ties"}."""
    n = len(rays)
    anyhit = is_anyhit(rays)
    t64, p64 = brute_force(g, rays) if ref is None else ref
    hits = np.ascontiguousarray(hits)
    p = prim_of(hits)
    hit_same = (p64 >= 0) == (p >= 0)
    other = hit_same & (p >= 0) & (p != p64) & ~anyhit
    tie = np.zeros(n, bool)
    if other.any():
        idx = np.flatnonzero(other)
        tp = prim_hit64(g, rays[idx], p[idx])[0]
        tie[idx] = np.abs(tp - t64[idx]) <= T_TOL * np.maximum(1.0, t64[idx])
    agree = np.where(anyhit, hit_same, hit_same & ((p < 0) | (p == p64) | tie))
    both = agree & ~anyhit & (p >= 0)
    err = np.abs(hits[both, 0].astype(np.float64) - t64[both])
    off = ~(err <= T_TOL * np.maximum(1.0, t64[both]))
    lost = ~anyhit & (p64 >= 0) & ((p < 0) | (hits[:, 0] > t64 + T_TOL * np.maximum(1.0, np.where(p64 >= 0, t64, 1.0))))
    print(label, "fp64 agree", int(agree.sum()), "of", n, "hits", int((p >= 0).sum()), "ties", int(tie.sum()),
          "lost (a miss or a farther hit)", int(lost.sum()), "max |dt|", float(err.max()) if err.size else 0.0)
    assert not off.any(), (label, "t off the fp64 answer", [(int(i), rays[i].tolist(), hits[i].tolist(), float(t64[i]))
                                                            for i in np.flatnonzero(both)[off][:4]])
    assert agree.sum() >= 0.998 * n, (label, int(agree.sum()), n)
    return {"disagree": n - int(agree.sum()), "lost": int(lost.sum()), "ties": int(tie.sum())}


# families whose every ray goes through a vertex or along an edge: gate_fp64_edge judges them
EDGE_FAMILIES = ("to_vertex", "to_edge", "from_camera")


def gate_fp64_edge(g, rays, hits, ref_robust=None, label=""):
    """gate_fp64 for the rays that go through vertices and along edges.  There every ray is one
    'where rounding decides a silhouette or an edge', the case test_gpu_trace.py's 0.2 % is for:
    whether fp32 barycentrics fall inside is decided in the last bit, the strict fp64 answer and
    the fp32 list world itself part on 5 to 25 % of such rays, and a count of equal primitives
    says nothing.  What must still hold of an fp32 answer, up to uv_bound() in the barycentrics
    and 1e-5 max(1, t) in t:
      a hit    names a primitive that the ray hits in fp64 (inside to within the bound) at that t;
      nothing  is lost: no primitive that the ray hits robustly -- inside by more than the bound,
               whatever the rounding -- lies before the answer, and a miss has none at all.
    >= 99.8 % of the rays as in gate_fp64 (closest-hit rays only)."""
    n = len(rays)
    assert not is_anyhit(rays).any()
    tr, _ = brute_force(g, rays, robust=True) if ref_robust is None else ref_robust
    hits = np.ascontiguousarray(hits)
    p = prim_of(hits)
    t32 = hits[:, 0].astype(np.float64)
    tp = prim_hit64(g, rays, p)[0]
    named = (p < 0) | (np.abs(tp - t32) <= T_TOL * np.maximum(1.0, t32))
    lost = np.isfinite(tr) & ((p < 0) | (t32 > tr + T_TOL * np.maximum(1.0, np.where(np.isfinite(tr), tr, 1.0))))
    agree = named & ~lost
    print(label, "fp64 (edge rule) agree", int(agree.sum()), "of", n, "hits", int((p >= 0).sum()),
          "names no fp64 hit", int((~named).sum()), "lost (a miss or a farther hit)", int(lost.sum()))
    assert agree.sum() >= 0.998 * n, (label, int(agree.sum()), n,
                                      [(int(i), rays[i].tolist(), hits[i].tolist(), int(p[i]), float(tp[i]), float(tr[i]))
                                       for i in np.flatnonzero(~agree)[:4]])
    return {"disagree": n - int(agree.sum()), "lost": int(lost.sum()), "ties": 0}


