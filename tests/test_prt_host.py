"""Precomputed radiance transfer on the host (frt.h "precomputed radiance transfer"):
the SH basis, the environment projection, the corner records, the transfer replay
(frtx_selftest_prt_transfer_host: csrc/frt_prt.hpp, the code the kernels run per lane) against sums
taken here in fp64, a known answer, interreflection against the path integrator, batching, the
refusals, and csrc/tools/prt_host_check.cpp under the sanitizers.  CPU only."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLT_MAX = np.finfo(np.float32).max
NX, NY = 48, 36


# ---- the definitions of frt.h, restated in numpy fp64 ----
def legendre(l, m, x):
    pmm = np.ones_like(x)
    if m > 0:
        s = np.sqrt((1.0 - x) * (1.0 + x))
        odd = 1.0
        for _ in range(m):
            pmm = pmm * (-odd) * s
            odd += 2.0
    if l == m:
        return pmm
    pm1 = x * (2.0 * m + 1.0) * pmm
    if l == m + 1:
        return pm1
    for k in range(m + 2, l + 1):
        pl = ((2.0 * k - 1.0) * x * pm1 - (k + m - 1.0) * pmm) / (k - m)
        pmm, pm1 = pm1, pl
    return pl


def sh_angles(theta, phi):
    """Y (..., 25) at (theta, phi): EstimateSH's real basis, index l (l + 1) + m."""
    out = np.zeros(np.shape(theta) + (25,))
    x = np.cos(theta)
    for l in range(5):
        for m in range(-l, l + 1):
            a = abs(m)
            K = math.sqrt((2.0 * l + 1.0) * math.factorial(l - a) / (4.0 * math.pi * math.factorial(l + a)))
            if m == 0:
                y = K * legendre(l, 0, x)
            elif m > 0:
                y = math.sqrt(2.0) * K * np.cos(m * phi) * legendre(l, m, x)
            else:
                y = math.sqrt(2.0) * K * np.sin(-m * phi) * legendre(l, a, x)
            out[..., l * (l + 1) + m] = y
    return out


def sh_dirs(dirs):
    d = np.asarray(dirs, np.float64)
    theta = np.arccos(np.clip(d[:, 1], -1.0, 1.0))
    phi = np.arctan2(d[:, 0], -d[:, 2])
    phi = np.where(phi < 0.0, phi + 2.0 * math.pi, phi)
    return sh_angles(theta, phi)


def from_srgb(v):
    return np.where(v <= 0.04045, v * (1.0 / 12.92), ((v + 0.055) * (1.0 / 1.055)) ** 2.4)


def texels_of(image):
    """The fp32 texels image_texture's lookup returns, as float64."""
    a = np.asarray(image)
    return (from_srgb(a / 255.0).astype(np.float32) if a.dtype == np.uint8 else a.astype(np.float32)).astype(np.float64)


def view_arrays(view):
    """The scene view's arrays the corner records read."""
    n = int(view.n_tris)

    def arr(ptr, count, dt):
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dt))), shape=(count,)).copy()
    mats = ctypes.cast(view.materials, ctypes.POINTER(frt.Material))
    return {
        "v": arr(view.tri_v, 9 * n, np.float64).reshape(n, 3, 3),
        "n": arr(view.tri_n, 9 * n, np.float64).reshape(n, 3, 3) if view.tri_n else None,
        "geo": arr(view.tri_geometry_normal, n, np.uint8) if view.tri_geometry_normal else np.ones(n, np.uint8),
        "uv": arr(view.tri_uv, 6 * n, np.float64).reshape(n, 3, 2) if view.tri_uv else np.zeros((n, 3, 2)),
        "mat": arr(view.tri_material, n, np.int32),
        "mats": [mats[i] for i in range(int(view.n_materials))],
    }


def corners_np(view):
    """(origin, normal, albedo), each (n_tris, 3, 3) float32: frt.h's corner records from the fp64 view."""
    A = view_arrays(view)
    v = A["v"]
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    c = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
    ng = c / np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2])[:, None]
    n = np.repeat(ng[:, None, :], 3, axis=1)
    if A["n"] is not None:
        smooth = A["geo"] == 0
        n[smooth] = A["n"][smooth]
    o = v + 1e-4 * n
    rho = np.zeros_like(v)
    for t in range(len(v)):
        m = A["mats"][A["mat"][t]]
        if m.type != frt.MAT_TYPES["lambertian"]:
            continue
        for i in range(3):
            col = list(m.albedo)
            if m.texture == frt.FRT_TEX_CHECKER:
                x = 2 * (int(A["uv"][t, i, 0] * m.tex_scale[0] * 2.0) % 2) - 1
                y = 2 * (int(A["uv"][t, i, 1] * m.tex_scale[1] * 2.0) % 2) - 1
                if x * y == 1:
                    col = list(m.tex_odd)
            rho[t, i] = col
    return o.astype(np.float32), n.astype(np.float32), rho.astype(np.float32)


def visibility(scene, o, n, dirs):
    """(cos fp64 (nc, nd), unoccluded (nc, nd) bool for cos > -2^-20): every (corner, direction) ray put to
    selftest_trace_host as frt_trace_device's any-hit record."""
    cos = n.reshape(-1, 3).astype(np.float64) @ dirs.T.astype(np.float64)
    ci, dj = np.nonzero(cos > -2.0 ** -20)
    rays = frt.ray_records(o.reshape(-1, 3)[ci], dirs[dj], t_max=FLT_MAX, streams=np.ones(len(ci), np.uint32))
    hits = frt.selftest_trace_host(scene, rays)
    vis = np.zeros(cos.shape, bool)
    vis[ci, dj] = hits.view(np.int32)[:, 3] < 0
    return cos, vis


def transfer_sum(rho, cos, vis, Y):
    """T^0 (nc, 25, 3) in fp64 and the test's tolerance for the fp32 replay: (terms + 8) 2^-24 S with
    S = rho (4 / n) sum |cos Y| over the sum's terms, plus the terms of directions with |cos| < 2^-20."""
    nd = cos.shape[1]
    w = np.where((cos > 0.0) & vis, cos, 0.0)
    rho = rho.reshape(-1, 3).astype(np.float64)
    T = (4.0 / nd) * (w @ Y)[:, :, None] * rho[:, None, :]
    S = (4.0 / nd) * (w @ np.abs(Y))[:, :, None] * rho[:, None, :]
    terms = np.count_nonzero(w, axis=1)[:, None, None]
    edge = np.where(np.abs(cos) < 2.0 ** -20, np.abs(cos), 0.0)
    tol = (terms + 8) * 2.0 ** -24 * S + (4.0 / nd) * (edge @ np.abs(Y))[:, :, None] * rho[:, None, :]
    return T, tol


# ---- scenes ----
@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, NX / NY)


@pytest.fixture(scope="module")
def textured():
    """Cornell with a checkered quad over the floor and two analytic spheres (rough conductor, dielectric)."""
    return frt.HostScene.from_spec(SS.cornell_textured(), NX / NY)


QUAD_RHO = (0.5, 0.25, 1.0)


def quad_scene():
    spec = {"objects": [{"obj": SS.QUAD_UV_OBJ, "bsdf": {"type": "lambertian", "albedo": QUAD_RHO}, "geo": True}],
            "camera": SS.CORNELL_CAM, "world": "bvh"}
    return frt.HostScene.from_spec(spec, NX / NY)


# ---- the basis ----
def test_basis_table_equals_fp64_restatement():
    rng = np.random.default_rng(1)
    d = rng.normal(size=(4000, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32)
    d[:6] = [[0, 1, 0], [0, -1, 0], [1, 0, 0], [0, 0, -1], [0, 0, 1], [-1, 0, 0]]
    Y = frt.prt_basis(d)
    assert Y.dtype == np.float32 and Y.shape == (4000, 25)
    err = np.abs(Y.astype(np.float64) - sh_dirs(d)).max()
    print("largest |Y - fp64 restatement|", err)
    assert err <= 1e-6
    # the convention is the environment image's: +y is theta = 0, -z is phi = 0
    assert abs(Y[0, 2] - math.sqrt(3 / (4 * math.pi))) < 1e-6 and abs(Y[3, 3] - (-math.sqrt(3 / (4 * math.pi)))) < 1e-6


def test_basis_is_orthonormal_over_a_stratified_set():
    dirs = frt.prt_sample_dirs(64, seed=3)
    assert dirs.shape == (4096, 3) and np.abs(np.linalg.norm(dirs.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    Y = frt.prt_basis(dirs).astype(np.float64)
    n = len(dirs)
    worst = 0.0
    for a in range(25):
        for b in range(a, 25):
            terms = 4.0 * math.pi * Y[:, a] * Y[:, b]
            se = terms.std(ddof=1) / math.sqrt(n)
            # 6 standard errors of the plain estimator (stratification only tightens it), and the
            # rounding of the fp32 table for the pair whose terms do not vary (Y_00^2)
            tol = 6.0 * se + 2.0 ** -21
            dev = abs(terms.mean() - (1.0 if a == b else 0.0))
            worst = max(worst, dev / tol)
            assert dev <= tol, (a, b, dev, tol)
    print("largest deviation over its tolerance", worst)
    # strata: every cell of the 64 x 64 (cos theta, phi) grid holds one direction
    ct, phi = dirs[:, 1].astype(np.float64), np.arctan2(dirs[:, 0].astype(np.float64), -dirs[:, 2].astype(np.float64)) % (2 * math.pi)
    cell = np.minimum(((1.0 - ct) / 2.0 * 64).astype(int), 63) * 64 + np.minimum((phi / (2 * math.pi) * 64).astype(int), 63)
    assert len(np.unique(cell)) >= 4090          # fp32 rounding may move a direction across a cell edge
    assert not np.array_equal(dirs, frt.prt_sample_dirs(64, seed=4))


# ---- the projection ----
@pytest.mark.parametrize("shape,srgb", [((3, 6), True), ((4, 5), False)], ids=["6x3_srgb8", "5x4_f32"])
def test_projection_equals_fp64_sum(shape, srgb):
    ny, nx = shape
    rng = np.random.default_rng(9)
    image = rng.integers(0, 256, (ny, nx, 3), dtype=np.uint8) if srgb else rng.uniform(0.0, 5.0, (ny, nx, 3)).astype(np.float32)
    li = frt.sh_project_image(image)
    theta = math.pi * (np.arange(ny) + 0.5) / ny
    phi = 2.0 * math.pi * (np.arange(nx) + 0.5) / nx
    Y = sh_angles(np.repeat(theta[:, None], nx, axis=1), np.repeat(phi[None, :], ny, axis=0))       # (ny, nx, 25)
    w = np.sin(theta)[:, None] * (2.0 * math.pi / nx) * (math.pi / ny)
    terms = texels_of(image)[:, :, None, :] * Y[:, :, :, None] * w[:, :, None, None]              # (ny, nx, 25, 3)
    want, scale = terms.sum(axis=(0, 1)), np.abs(terms).sum(axis=(0, 1))
    print("largest |li - sum| / sum |terms|", (np.abs(li - want) / scale).max())
    assert li.shape == (25, 3) and np.all(np.abs(li - want) <= 1e-12 * scale)


def test_projection_of_a_constant_colour():
    E = np.array([0.25, 0.5, 0.75])
    li = frt.sh_project_image(None, env_color=E)
    assert np.array_equal(li[0], E * math.sqrt(4.0 * math.pi)) and np.all(li[1:] == 0.0)


# ---- the corner records ----
def check_corners(scene, n_tris=None, smooth=None):
    view = scene.view()
    o, n, rho = frt.prt_corners(scene)
    wo, wn, wr = corners_np(view)
    assert n_tris is None or len(o) == n_tris
    assert o.tobytes() == wo.tobytes() and n.tobytes() == wn.tobytes() and rho.tobytes() == wr.tobytes()
    if smooth is not None:
        A = view_arrays(view)
        assert (A["n"] is not None and np.any(A["geo"] == 0)) == smooth
    return o, n, rho


def test_corner_records_cornell(cornell):
    o, n, rho = check_corners(cornell, 36, smooth=False)                 # flat normals, 108 corners
    assert np.all(np.abs(np.linalg.norm(n.astype(np.float64), axis=2) - 1.0) < 1e-6)
    assert np.count_nonzero(rho.reshape(36, -1).any(axis=1)) == 34         # the light's two triangles carry none


def test_corner_records_smooth_mesh(sphere_obj):
    o, n, rho = check_corners(frt.HostScene("obj_smooth", sphere_obj, NX / NY), smooth=True)
    assert len(np.unique(n.reshape(-1, 3), axis=0)) > 100                  # per-vertex normals, not one a triangle


def test_corner_records_checker(textured):
    check_corners(textured)                                                # every corner of its quad lies in a tex1 cell
    # one cell a unit of uv: the quad's corners (0, 0), (1, 1) take tex1, (1, 0), (0, 1) the albedo
    mat = SS.checker({"type": "lambertian", "albedo": (0.25, 0.5, 0.125)}, (0.75, 0.75, 1.0), (0.5, 0.5))
    spec = {"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}, {"obj": SS.QUAD_UV_OBJ, "bsdf": mat, "geo": True}],
            "camera": SS.CORNELL_CAM, "world": "bvh"}
    scene = frt.HostScene.from_spec(spec, NX / NY)
    o, n, rho = check_corners(scene, 38)
    A = view_arrays(scene.view())
    for t in range(36, 38):
        for i in range(3):
            u, v = A["uv"][t, i]
            assert tuple(rho[t, i]) == ((0.75, 0.75, 1.0) if u == v else (0.25, 0.5, 0.125)), (t, i, u, v, rho[t, i])
    assert len({tuple(c) for c in rho[36:].reshape(-1, 3)}) == 2


# ---- the transfer replay against an independent sum ----
def check_transfer(scene, sqrt_n, flags=0):
    dirs = frt.prt_sample_dirs(sqrt_n, seed=11)
    o, n, rho = frt.prt_corners(scene)
    cos, vis = visibility(scene, o, n, dirs)
    if flags & frt.FRTX_PRT_UNSHADOWED:
        vis[:] = True
    want, tol = transfer_sum(rho, cos, vis, frt.prt_basis(dirs).astype(np.float64))
    T = frt.selftest_prt_transfer_host(scene, dirs, 0, flags).reshape(want.shape).astype(np.float64)
    bad = np.abs(T - want) > tol
    print("n_dirs", len(dirs), "corners", len(want), "largest |T - sum| / tolerance",
          (np.abs(T - want) / np.maximum(tol, 1e-300))[tol > 0].max(), "occluded share", 1.0 - vis[cos > 0].mean())
    assert not bad.any(), (np.argwhere(bad)[:5], T[bad][:5], want[bad][:5])
    assert np.all(T[(rho.reshape(-1, 3) == 0).all(axis=1)] == 0.0)          # corners without an albedo: exactly 0
    return T, vis, cos


@pytest.mark.parametrize("sqrt_n", [7, 13], ids=["49_dirs", "169_dirs"])       # shorter than a chunk; two chunks and a tail
def test_transfer_cornell_bvh(cornell, sqrt_n):
    T, vis, cos = check_transfer(cornell, sqrt_n)
    assert 0.05 < 1.0 - vis[cos > 0].mean() < 0.95                            # the box does occlude
    assert np.all(T.reshape(36, -1)[~frt.prt_corners(cornell)[2].reshape(36, -1).any(axis=1)] == 0.0)   # the emitter


@pytest.mark.parametrize("sqrt_n", [7, 13], ids=["49_dirs", "169_dirs"])
def test_transfer_list_world(sqrt_n):
    check_transfer(frt.HostScene.from_spec(ES.plain_cornell(world="list"), NX / NY), sqrt_n)


@pytest.mark.parametrize("sqrt_n", [7, 13], ids=["49_dirs", "169_dirs"])
def test_transfer_spheres_occlude(textured, sqrt_n):
    assert textured.info.n_spheres == 2
    check_transfer(textured, sqrt_n)


def test_transfer_unshadowed(cornell):
    T, _, _ = check_transfer(cornell, 13, frt.FRTX_PRT_UNSHADOWED)
    assert np.abs(T - frt.selftest_prt_transfer_host(cornell, frt.prt_sample_dirs(13, seed=11), 0).reshape(T.shape)).max() > 0.01


# ---- a known answer: the clamped cosine's zonal coefficients ----
def test_unshadowed_quad_has_the_clamped_cosine_lobe():
    scene = quad_scene()
    dirs = frt.prt_sample_dirs(64, seed=5)
    T = frt.selftest_prt_transfer_host(scene, dirs, 0, frt.FRTX_PRT_UNSHADOWED).astype(np.float64)     # (2, 3, 25, 3)
    A = np.array([math.pi, 2.0 * math.pi / 3.0, math.pi / 4.0, 0.0, -math.pi / 24.0])
    Yn = sh_dirs(np.array([[0.0, 1.0, 0.0]]))[0]
    band = np.array([l for l in range(5) for _ in range(2 * l + 1)])
    want = np.array(QUAD_RHO)[None, :] / math.pi * (A[band] * Yn)[:, None]                              # (25, 3)
    Y = frt.prt_basis(dirs).astype(np.float64)
    terms = 4.0 * np.maximum(dirs[:, 1].astype(np.float64), 0.0)[:, None] * Y                           # per direction, before rho
    se = terms.std(axis=0, ddof=1) / math.sqrt(len(dirs))
    tol = 6.0 * se[:, None] * np.array(QUAD_RHO)[None, :] + 1e-6
    dev = np.abs(T - want[None, None])
    print("largest deviation over its tolerance", (dev / tol).max(), "T[0, 0, :3]", T[0, 0, :3], "want", want[:3])
    assert np.all(dev <= tol)
    assert want[6, 0] > 0.05 and abs(want[2, 1] - 0.25 / math.pi * A[1] * Yn[2]) < 1e-15


# ---- interreflection means something: PRT with B bounces against the path integrator at max_depth = B ----
# The depth correspondence (csrc/frt_path.hpp path_shade): the camera ray's hit is depth 0 and a vertex
# scatters while depth <= max_depth, so max_depth = B gives paths with 1 .. B + 1 scattering vertices before
# they leave to the environment -- the vertices of T^0 .. T^B.  With no emitter the environment is the only light.
# The scene.  A corner's transfer is taken at the vertex itself, and a vertex that lies in the plane of a
# neighbouring wall -- every vertex of the Cornell box -- starts half of its rays in that plane, which they
# then miss: such corners see the environment through the junction (as the reference's vertices do), and the
# gathers carry that light on.  That is a property of per-vertex transfer at junctions, not of the estimator
# under test, and the spec has no edit for it; so this is a builder scene without junctions: a lambertian
# floor under a lambertian box that floats above it, both cut into cells so that T is interpolated over short
# edges, under a constant environment with no emitter.
def grid(origin, du, dv, m):
    """m x m cells of the parallelogram (origin, du, dv) as OBJ vertices and faces; the normal is du x dv."""
    o, du, dv = (np.asarray(x, np.float64) for x in (origin, du, dv))
    v = [o + du * i / m + dv * j / m for j in range(m + 1) for i in range(m + 1)]
    f = []
    for j in range(m):
        for i in range(m):
            a = j * (m + 1) + i
            f += [(a, a + 1, a + m + 2), (a, a + m + 2, a + m + 1)]
    return v, f


def floating_box(tmp_path_factory):
    x0, x1, y0, y1, z0, z1 = -0.4, 0.4, 0.25, 0.85, -0.4, 0.4
    dx, dy, dz = x1 - x0, y1 - y0, z1 - z0
    faces = [((-1, 0, 1), (2, 0, 0), (0, 0, -2), 8),                                                      # the floor
             ((x0, y1, z1), (dx, 0, 0), (0, 0, -dz), 3), ((x0, y0, z0), (dx, 0, 0), (0, 0, dz), 3),       # top, bottom
             ((x1, y0, z1), (0, 0, -dz), (0, dy, 0), 3), ((x0, y0, z0), (0, 0, dz), (0, dy, 0), 3),       # +x, -x
             ((x0, y0, z1), (dx, 0, 0), (0, dy, 0), 3), ((x1, y0, z0), (-dx, 0, 0), (0, dy, 0), 3)]       # +z, -z
    lines, base = [], 1
    for face in faces:
        v, f = grid(*face)
        lines += ["v %.17g %.17g %.17g" % tuple(q) for q in v] + ["f %d %d %d" % tuple(base + k for k in t) for t in f]
        base += len(v)
    path = tmp_path_factory.mktemp("box") / "floating_box.obj"
    path.write_text("\n".join(lines) + "\n")
    spec = {"objects": [{"obj": str(path), "bsdf": {"type": "lambertian", "albedo": (0.8, 0.6, 0.4)}, "geo": True}],
            "camera": SS.CORNELL_CAM, "world": "bvh", "env": (1.0, 0.8, 0.6)}
    return frt.HostScene.from_spec(spec, NX / NY)


def test_interreflection_matches_the_path_integrator(tmp_path_factory):
    B, U = 2, 0.02
    ENV = np.array([1.0, 0.8, 0.6])
    scene = floating_box(tmp_path_factory)
    assert scene.info.n_lights == 0 and scene.info.n_tris == 128 + 6 * 18
    A = view_arrays(scene.view())
    o, n, rho = frt.prt_corners(scene)
    # points just inside corner 0 of: floor cells under and beside the box, its underside, its sides
    c0 = A["v"][:, 0]
    floor = [t for t in range(128) if abs(c0[t, 0]) <= 0.5 and abs(c0[t, 2]) <= 0.5][::5][:4]
    tris = floor + list(range(128 + 18, 128 + 36, 5)) + list(range(128 + 36, 128 + 108, 18))
    p = np.array([(1 - 2 * U) * A["v"][t, 0] + U * A["v"][t, 1] + U * A["v"][t, 2] for t in tris])
    nt = n[tris, 0].astype(np.float64)
    rays = frt.ray_records(p + 0.1 * nt, -nt)
    first = frt.selftest_trace_host(scene, rays)
    assert len(tris) == 12 and np.array_equal(first.view(np.int32)[:, 3], tris)
    # the path side: 8 independent batches of 512 samples; V = the batch-means variance of their mean, taken here
    # (frt.h's V of the chunk means: the host replay returns the means alone, the device call's V needs a GPU)
    batches = []
    for k in range(8):
        q = frt.RenderParams.make(1, 1, 512, seed=21, max_depth=B, sample_offset=512 * k)
        batches.append(frt.selftest_radiance_host(scene, q, rays)[0].astype(np.float64))
    path, V_path = np.mean(batches, axis=0), np.var(batches, axis=0, ddof=1) / len(batches)
    li = frt.sh_project_image(None, env_color=ENV)

    def prt(bounces):
        out, interp = [], []
        for seed in range(4):
            T = frt.selftest_prt_transfer_host(scene, frt.prt_sample_dirs(24, seed=seed), bounces)
            out.append(frt.selftest_prt_rays_host(scene, T, li, rays).astype(np.float64))
            Tq = T[tris].astype(np.float64)                                    # (m, 3, 25, 3)
            u, v = first[:, 1].astype(np.float64)[:, None, None], first[:, 2].astype(np.float64)[:, None, None]
            at = (1 - u - v) * Tq[:, 0] + u * Tq[:, 1] + v * Tq[:, 2]
            interp.append((np.abs(at - Tq[:, 0]) * np.abs(li)[None]).sum(axis=1))
        return np.mean(out, axis=0), np.var(out, axis=0, ddof=1) / len(out), np.mean(interp, axis=0)
    full, V_prt, interp = prt(B)
    tol = 4.0 * np.sqrt(V_path + V_prt) + interp
    print("path", path[:, 0], "\nprt B", full[:, 0], "\ntolerance", tol[:, 0])
    assert np.all(np.abs(full - path) <= tol), (np.abs(full - path) / tol).max()
    direct, V0, interp0 = prt(0)
    miss = np.any(np.abs(direct - path) > 4.0 * np.sqrt(V_path + V0) + interp0, axis=1)
    print("prt 0", direct[:, 0], "points outside the tolerance without the gather:", int(miss.sum()), "of", len(miss))
    assert miss.sum() > len(miss) / 2                                           # a gather that did nothing would not pass


# ---- order and batching ----
def test_batching_changes_no_bit(cornell):
    dirs = frt.prt_sample_dirs(13, seed=2)
    whole = frt.selftest_prt_transfer_host(cornell, dirs, 1)
    parts = frt.selftest_prt_transfer_host(cornell, dirs, 1, budget=1)          # 64 corners a batch: two batches
    assert whole.tobytes() == parts.tobytes() and np.isfinite(whole).all() and whole.any()
    assert not np.array_equal(whole, frt.selftest_prt_transfer_host(cornell, dirs, 0))     # the bounce adds


# ---- refusals ----
def refused(scene, dirs, bounces=0, flags=0):
    """(return code, text, T untouched) of the replay called with a T of sentinels."""
    view = scene.view()
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    T = np.full((int(view.n_tris), 3, 25, 3), 7.0, np.float32)
    rc = frt.lib().frtx_selftest_prt_transfer_host(ctypes.byref(view), dirs.ctypes.data, len(dirs), bounces, flags, T.ctypes.data)
    return rc, frt.lib().frt_last_error(None).decode(), bool(np.all(T == 7.0))


def test_refusals(cornell):
    good = frt.prt_sample_dirs(3)
    for kw, text in ((dict(dirs=np.zeros((0, 3))), "n_dirs"), (dict(dirs=good, bounces=-1), "bounces"),
                     (dict(dirs=good, bounces=17), "bounces"), (dict(dirs=good, flags=1 << 20), "unknown flags"),
                     (dict(dirs=good, flags=frt.FRT_FLAG_SOBOL), "unknown flags")):
        rc, msg, untouched = refused(cornell, **kw)
        assert rc == -1 and text in msg and untouched, (kw, rc, msg)
    bad = good.copy()
    bad[3, 1] = np.nan
    rc, msg, untouched = refused(cornell, bad)
    assert rc == -1 and "direction 3" in msg and "finite" in msg and untouched
    bad = good.copy()
    bad[5] *= 1.01
    rc, msg, untouched = refused(cornell, bad)
    assert rc == -1 and "direction 5" in msg and "unit" in msg and untouched
    bad[5] = good[5] * np.float32(1.0005)                                       # inside the 1e-3 band: accepted
    assert refused(cornell, bad)[0] == 0
    with pytest.raises(frt.FrtError, match="direction 0"):
        frt.prt_basis([[0.0, 0.0, 0.0]])
    with pytest.raises(frt.FrtError, match="sqrt_n"):
        frt.prt_sample_dirs(0)
    with pytest.raises(frt.FrtError, match="negative or not finite"):
        frt.sh_project_image(np.full((2, 2, 3), -1.0, np.float32))
    with pytest.raises(frt.FrtError, match="li"):
        frt.selftest_prt_rays_host(cornell, np.zeros((36, 3, 25, 3), np.float32), np.full((25, 3), np.inf), frt.ray_records([[0, 1, 0]], [[0, 0, -1]]))
    with pytest.raises(frt.FrtError, match="entry 0"):
        frt.selftest_prt_rays_host(cornell, np.zeros((36, 3, 25, 3), np.float32), np.zeros((25, 3)), frt.ray_records([[0, 1, 0]], [[0, 0, 0]]))
    L = frt.lib()
    assert all(n in frt.EXPORTS_X and hasattr(L, n) for n in ("frtx_prt_transfer", "frtx_prt_rays", "frtx_prt_corners"))


def test_rays_replay_shades_by_the_rule(cornell):
    """An emitter shows its emission, a miss the environment (constant or the image's texel), a lambertian
    hit the dot product."""
    T = np.zeros((36, 3, 25, 3), np.float32)
    T[:, :, 0, :] = 2.0
    li = np.zeros((25, 3))
    li[0] = (0.5, 0.25, 0.125)
    rays = frt.ray_records([[0, 1, 0], [0, 1, 0], [0, 1, 0]], [[0, 1, 0], [0, 0, 1], [0, 0, -1]])    # the light, the opening, the back wall
    rgb = frt.selftest_prt_rays_host(cornell, T, li, rays)
    assert np.array_equal(rgb[0], np.float32([17, 12, 4])) and np.array_equal(rgb[1], np.float32([0, 0, 0]))
    assert np.allclose(rgb[2], [1.0, 0.5, 0.25], rtol=1e-6)
    image = ES.random_env(8, 4, seed=4)
    got = frt.selftest_prt_rays_host(cornell, T, li, rays, env_image=image)
    assert np.array_equal(got[1], image[2, 4]) or np.array_equal(got[1], image[1, 4]) or np.array_equal(got[1], image[2, 3])
    assert np.array_equal(got[[0, 2]], rgb[[0, 2]])


# ---- the sanitizer build of the host code ----
def test_prt_host_check_under_sanitizers(tmp_path_factory):
    d = tmp_path_factory.mktemp("asan")
    subprocess.run(["make", "-C", os.path.join(ROOT, "first_raytracer_amd"), "prt_host_asan", "OBJDIR=" + str(d)], check=True, timeout=300)
    r = subprocess.run([str(d / "prt_host_asan")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "prt_host_check: ok" in r.stdout, (r.stdout, r.stderr)
