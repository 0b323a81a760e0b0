"""Shared pieces of the feature-image and denoiser tests (test_features_host.py,
test_denoise_host.py, test_gpu_features.py, test_gpu_denoise.py):

* denoise_ref: an fp64 numpy restatement of the filter of FRT_INTEGRATOR_DENOISE,
  written from the text of DESIGN.md "Denoiser" / include/frt.h; its constants are
  parsed from first_raytracer_amd/csrc/frt_denoise.hpp;
* features_ref: a Python restatement of FRT_INTEGRATOR_ALBEDO and _DEPTH for
  aperture-0 cameras over the oracle's scene (camera, counter RNG, world_hit,
  triangles, materials) and the scene spec's textures;
* the agreement rule of tests/test_gpu_integrators.py, the probe runner and the
  measured probe tolerance."""
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "first_raytracer_amd", "csrc", "frt_denoise.hpp")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SPHERE = 1 << 30

# Largest |probe - restatement| / film maximum over the inputs of
# test_denoise_host.py::test_probe_matches_restatement, measured with the constants now in the
# header: host-replay Cornell features (4 spp, seed 21) with the colour film random_colour(nx, ny)
# at 48 x 36 (3.741e-6, the largest), 41 x 23 (5.4e-7), 5 x 3 (1.0e-6) and 1 x 1 (2e-16), and
# synthetic_inputs at 41 x 23 (3.1e-7), 5 x 3 (7.9e-8) and 1 x 1 (0).  The fp32 depth z enters
# w_z as |z(p) - z(q)| / (0.005 max z): an ulp of z (6e-8 relative) moves the exponent by 1e-5.
# The tests allow 4 x this (expf of the host's and the device's libm differ in the last bits);
# the allowance must stay below 1e-4.
PROBE_MAX_REL_DIFF = 3.75e-6
PROBE_TOLERANCE = 4.0 * PROBE_MAX_REL_DIFF
assert PROBE_TOLERANCE < 1e-4


# ---- the filter ----
def constants(path=HEADER):
    """The five numbers of frt_denoise.hpp: iterations, eps_a, sigma_n, sigma_z, sigma_l0."""
    text = open(path).read()

    def num(name):
        m = re.search(r"constexpr\s+(?:int|float)\s+" + name + r"\s*=\s*([-+0-9.eE]+)f?\s*;", text)
        assert m, name
        return float(m.group(1))
    return {"iterations": int(num("kDenoiseIterations")), "eps_a": num("kDenoiseEpsAlbedo"),
            "sigma_n": num("kDenoiseSigmaN"), "sigma_z": num("kDenoiseSigmaZ"), "sigma_l0": num("kDenoiseSigmaL0")}


H = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def denoise_ref(colour, N, A, D, consts=None):
    """colour, N, A, D: (ny, nx, 3) films (colour noisy; normals, albedo, depth features).
    Returns the filtered (ny, nx, 3) film in float64."""
    K = consts or constants()
    c, N, A, D = (np.asarray(a, np.float64) for a in (colour, N, A, D))
    ny, nx = c.shape[:2]
    k = D[..., 2]
    z = np.where(k > 0, D[..., 0] / np.where(k > 0, k, 1.0), 0.0)
    nlen = np.linalg.norm(N, axis=2)
    nhat = N / np.where(nlen > 0, nlen, 1.0)[..., None]
    guided = (k >= 1) & (nlen > 0)                      # w_n = 1 where either pixel is not
    a_floor = np.maximum(A, K["eps_a"])
    r = c / a_floor
    for i in range(K["iterations"]):
        s = 1 << i
        sigma_l = K["sigma_l0"] * 2.0 ** -i
        lum = 0.2126 * r[..., 0] + 0.7152 * r[..., 1] + 0.0722 * r[..., 2]
        sw = np.zeros((ny, nx))
        sc = np.zeros((ny, nx, 3))
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * s, dy * s
                if abs(ox) >= nx or abs(oy) >= ny:
                    continue
                # p = the pixels whose tap (ox, oy) is inside the frame, q = p + (ox, oy)
                py = slice(max(0, -oy), min(ny, ny - oy))
                px = slice(max(0, -ox), min(nx, nx - ox))
                qy = slice(py.start + oy, py.stop + oy)
                qx = slice(px.start + ox, px.stop + ox)
                both = guided[py, px] & guided[qy, qx]
                cos = np.maximum(0.0, (nhat[py, px] * nhat[qy, qx]).sum(axis=2))
                w_n = np.where(both, cos ** K["sigma_n"], 1.0)
                zp, zq = z[py, px], z[qy, qx]
                w_z = np.exp(-np.abs(zp - zq) / (K["sigma_z"] * np.maximum(zp, zq) + 1e-20))
                w_k = 1.0 - np.abs(k[py, px] - k[qy, qx])
                lp, lq = lum[py, px], lum[qy, qx]
                w_l = np.exp(-np.abs(lp - lq) / (sigma_l * np.maximum(lp, lq) + 1e-20))
                w = H[dx + 2] * H[dy + 2] * w_n * w_z * w_k * w_l
                sw[py, px] += w
                sc[py, px] += w[..., None] * r[qy, qx]
        r = sc / sw[..., None]
    return r * a_floor


def random_colour(nx, ny, seed=11):
    """A random positive colour film, O(1), float32."""
    return np.random.default_rng(seed).uniform(0.05, 2.0, (ny, nx, 3)).astype(np.float32)


def synthetic_inputs(nx, ny, seed=3):
    """Colour and feature films that need no scene: two depth planes with different normals and
    albedos split by a slanted edge, partly covered pixels along it, and a band of misses."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:ny, 0:nx]
    side = (x + 0.5 * y) > 0.55 * (nx + 0.5 * ny)
    cover = np.ones((ny, nx))
    cover[np.abs((x + 0.5 * y) - 0.55 * (nx + 0.5 * ny)) < 0.6] = 0.5
    cover[y >= ny - max(1, ny // 6)] = 0.0
    cover[0, 0] = 1.0
    n0, n1 = np.array([0.0, 0.0, 1.0]), np.array([0.6, 0.0, 0.8])
    N = np.where(side[..., None], n1, n0) * np.ones((ny, nx, 1))
    N[cover < 1] = (0.3, 0.3, 0.3)                        # environment radiance mixed in
    zed = np.where(side, 5.0, 2.0) + 0.01 * x
    D = np.stack([zed * cover, zed * zed * cover, cover], -1)
    A = np.where(side[..., None], np.array([0.7, 0.2, 0.2]), np.array([0.3, 0.6, 0.8])) * np.ones((ny, nx, 1))
    A[cover == 0] = 1.0
    if nx * ny > 4:
        A[ny // 2, nx // 2] = 0.0                         # below eps_a
    colour = A * rng.uniform(0.2, 1.8, (ny, nx, 1)) * rng.uniform(0.8, 1.2, (ny, nx, 3))
    return tuple(np.ascontiguousarray(a, np.float32) for a in (colour, N, A, D))


def build_probe(tmpdir):
    """tests/denoise_probe.hip (its own main over csrc/frt_denoise.hpp) built as host code."""
    exe = os.path.join(str(tmpdir), "denoise_probe")
    subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=on",
                    "-I" + os.path.join(ROOT, "first_raytracer_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "denoise_probe.hip"), "-o", exe], check=True, timeout=300)
    return exe


def run_probe(exe, workdir, colour, N, A, D):
    """The probe's film for (ny, nx, 3) float32 inputs."""
    ny, nx = colour.shape[:2]
    names = []
    for tag, a in (("c", colour), ("n", N), ("a", A), ("d", D)):
        path = os.path.join(str(workdir), tag + ".f32")
        np.ascontiguousarray(a, np.float32).tofile(path)
        names.append(path)
    out = os.path.join(str(workdir), "out.f32")
    subprocess.run([exe, str(nx), str(ny)] + names + [out], check=True, timeout=120)
    return np.fromfile(out, np.float32).reshape(ny, nx, 3)


def rel_diff(film, ref):
    """Largest |film - ref| over the film maximum."""
    return float(np.abs(np.asarray(film, np.float64) - ref).max() / max(float(np.abs(ref).max()), 1e-30))


# ---- host-replay films ----
def host_features(hs, nx, ny, spp, seed):
    """(N, A, D) films (ny, nx, 3) float32 of the host replay of the three feature integrators."""
    import first_raytracer_amd as frt
    pix = np.arange(nx * ny, dtype=np.int32)
    kinds = (frt.FRT_INTEGRATOR_NORMALS, frt.FRT_INTEGRATOR_ALBEDO, frt.FRT_INTEGRATOR_DEPTH)
    return tuple(frt.selftest_path_host(hs, frt.RenderParams.make(nx, ny, spp, seed=seed, integrator=k), pix)[0]
                 .reshape(ny, nx, 3) for k in kinds)


def cornell64_noisy(cornell_obj, spp=4, feature_spp=16, seeds=(300, 301, 302, 303)):
    """[(seed, colour, (N, A, D))]: host-replay path films of Cornell 64 x 64 at spp samples and
    feature_spp-sample host feature films -- the inputs of the "filter helps" test and of the
    tuning sweep (tools/denoise_tune.py)."""
    import first_raytracer_amd as frt
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 1.0)
    pix = np.arange(64 * 64, dtype=np.int32)
    out = []
    for seed in seeds:
        film, _ = frt.selftest_path_host(hs, frt.RenderParams.make(64, 64, spp, seed=seed), pix)
        out.append((seed, film.reshape(64, 64, 3), host_features(hs, 64, 64, feature_spp, seed)))
    return out


def rmse(film, ref):
    return float(np.sqrt(np.mean((np.asarray(film, np.float64).reshape(ref.shape) - ref) ** 2)))


# ---- the agreement rule of the integrator tests ----
def check_close(out, ref, max_frac=0.01):
    """Per-pixel max |diff| <= 1e-3 except where fp32 sends a sample to another primitive (at most
    1 % of the pixels); RMSE < 1e-5 over the others.  Returns the number of excepted pixels."""
    out = np.asarray(out, np.float64).reshape(-1, 3)
    ref = np.asarray(ref, np.float64).reshape(-1, 3)
    d = np.abs(out - ref).max(axis=1)
    bad = d > 1e-3
    assert bad.sum() <= max(1, max_frac * len(d)), (int(bad.sum()), len(d))
    good = ~bad
    assert float(np.sqrt(np.mean((out[good] - ref[good]) ** 2))) < 1e-5
    return int(bad.sum())


def check_depth_close(out, ref, far=False):
    """check_close for a depth film.  far: a scene seen from more than 6 units (veach_mis: 12 to
    19), whose t^2 is 150 to 360 -- one fp32 rounding there is 1.5e-5 to 3e-5, so the rule's 1e-5
    RMSE cannot hold for that channel (measured 4e-5 host against fp64, 3e-5 GPU against host).
    The rule is kept for t and the coverage; t^2 must agree to 1e-6 relative where the coverage
    does (the samples' squares, their sum and the mean: fewer than 16 roundings of 6e-8)."""
    out = np.array(out, np.float64).reshape(-1, 3)
    ref = np.array(ref, np.float64).reshape(-1, 3)
    if far:
        same = out[:, 2] == ref[:, 2]
        assert (np.abs(out[same, 1] - ref[same, 1]) <= 1e-6 * ref[same, 1]).all()
        out[:, 1] = ref[:, 1] = 0.0
    return check_close(out, ref)


# ---- ALBEDO and DEPTH over the oracle's scene ----
def _obj_vertex_uv(path):
    """{rounded vertex position: vt} of an OBJ's faces (no transform)."""
    v, vt, out = [], [], {}
    with open(path) as f:
        for line in f:
            w = line.split()
            if not w:
                continue
            if w[0] == "v":
                v.append(tuple(float(x) for x in w[1:4]))
            elif w[0] == "vt":
                vt.append(tuple(float(x) for x in w[1:3]))
            elif w[0] == "f":
                for corner in w[1:]:
                    idx = corner.split("/")
                    if len(idx) > 1 and idx[1]:
                        out[tuple(round(c, 6) for c in v[int(idx[0]) - 1])] = vt[int(idx[1]) - 1]
    return out


class FeatureScene:
    """What the restatement needs of a scene: the oracle's geometry and materials, and, for a
    scene spec, its spheres' materials and its textures (triangle uv from the OBJ's vt by vertex
    position; such objects carry no to_world in the specs used)."""

    def __init__(self, oscene, spec=None):
        import oracle
        self.o = oscene
        self.tri_v, self.tri_m = oscene.tris()
        self.mats = oscene.materials()
        self.spheres, self.uv, self.images = [], {}, []
        if spec is not None:
            self.images = [np.ascontiguousarray(i["data"]) for i in spec.get("images", ())]
            for ob in spec["objects"]:
                if "sphere" in ob:
                    self.spheres.append(ob)
                elif ob.get("bsdf") and (ob["bsdf"].get("checker") or ob["bsdf"].get("image") is not None):
                    assert ob.get("to_world") is None
                    for pos, t in _obj_vertex_uv(ob["obj"]).items():
                        self.uv[pos] = (t, ob["bsdf"].get("image"))
        cam = oscene.camera()
        self.cam_o, self.llc, self.h, self.v = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
        assert cam[18] == 0.0, "aperture-0 cameras only"
        self.rng = oracle.rng_uniform

    def image_lookup(self, index, u, v):
        import ctypes

        import oracle
        img = self.images[index]
        out = np.zeros(3)
        assert oracle.lib().ora_image_lookup(img.shape[1], img.shape[0], 0 if img.dtype == np.uint8 else 1,
                                             img.ctypes.data, ctypes.c_double(u), ctypes.c_double(v),
                                             out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))) == 0
        return out

    def textured(self, base, tex, odd, scale, image, u, v):
        """texture.h:30-49 / 51-95: the checker's second colour where both cell parities agree,
        the image's nearest texel, or the constant."""
        if tex == 1:
            x = 2 * (int(u * scale[0] * 2) % 2) - 1
            y = 2 * (int(v * scale[1] * 2) % 2) - 1
            return np.asarray(odd, np.float64) if x * y == 1 else base
        if tex == 2:
            return self.image_lookup(image, u, v)
        return base

    def reflectance(self, prim, p):
        """The table of FRT_INTEGRATOR_ALBEDO (include/frt.h) at hit point p of primitive prim."""
        if prim & SPHERE:
            k = prim & ~SPHERE
            if not self.spheres:                          # the reference's own scenes (veach_mis): sphere lights only
                other = [row for m, row in enumerate(self.mats) if m not in set(self.tri_m.tolist())]
                assert other and all(int(row[0]) == 1 for row in other), "a sphere whose material is not known"
                return np.ones(3)
            ob = self.spheres[k]
            m = ob["material"]
            mtype = m["type"]
            albedo = np.asarray(m.get("albedo", (0, 0, 0)), np.float64)
            spec = np.asarray(m.get("specular", (0, 0, 0)), np.float64)
            ck = m.get("checker")
            tex = 1 if ck else 2 if m.get("image") is not None else 0
            odd, scale = (ck["odd"], ck["scale"]) if ck else (None, None)
            image = m.get("image")
            q = p - np.asarray(ob["sphere"], np.float64)
            tu = 1.0 - (math.atan2(q[2], q[0]) + math.pi) / (2 * math.pi)
            tv = (math.asin(q[1]) + 0.5 * math.pi) / math.pi
        else:
            row = self.mats[self.tri_m[prim]]
            mtype = {0: "lambertian", 1: "diffuse_light", 2: "modified_phong", 3: "metal", 4: "dielectric",
                     5: "rough_conductor"}[int(row[0])]
            albedo, spec = row[1:4].copy(), row[7:10].copy()
            tex, odd, scale, image = int(row[20]), row[21:24], row[24:26], None
            tu = tv = 0.0
            if tex:
                v0, v1, v2 = self.tri_v[prim].reshape(3, 3)
                e1, e2, d = v1 - v0, v2 - v0, p - v0
                g = np.array([[e1 @ e1, e1 @ e2], [e1 @ e2, e2 @ e2]])
                bu, bv = np.linalg.solve(g, np.array([d @ e1, d @ e2]))
                uv = [self.uv[tuple(round(c, 6) for c in vert)] for vert in (v0, v1, v2)]
                image = uv[0][1]
                tu = (1 - bu - bv) * uv[0][0][0] + bu * uv[1][0][0] + bv * uv[2][0][0]
                tv = (1 - bu - bv) * uv[0][0][1] + bu * uv[1][0][1] + bv * uv[2][0][1]
        if mtype == "diffuse_light":
            return np.ones(3)
        if mtype in ("lambertian", "modified_phong"):
            albedo = self.textured(albedo, tex, odd, scale, image, tu, tv)
        else:
            spec = self.textured(spec, tex, odd, scale, image, tu, tv)
        if mtype in ("lambertian", "metal"):
            return albedo
        if mtype == "modified_phong":
            return np.minimum(1.0, albedo + spec)
        return spec                                       # dielectric, rough_conductor


def features_ref(oscene, nx, ny, spp, seed, spec=None, sample_offset=0):
    """(albedo, depth) films, each (ny * nx, 3) float64: per pixel the mean over the samples
    s = sample_offset .. + spp of the reflectance colour at the camera ray's hit (1 on a light
    and on a miss) and of (t, t^2, 1) hit, t = |d| t_ray.  Camera rays: DESIGN.md section 4,
    dimensions 0 and 1 the film position (an aperture-0 camera draws no lens point)."""
    S = FeatureScene(oscene, spec)
    alb = np.zeros((nx * ny, 3))
    dep = np.zeros((nx * ny, 3))
    for pix in range(nx * ny):
        px, py = pix % nx, pix // nx
        for s in range(sample_offset, sample_offset + spp):
            u = (px + S.rng(seed, pix, s, 0)) / nx
            v = (py + S.rng(seed, pix, s, 1)) / ny
            d = (S.llc + u * S.h + v * S.v) - S.cam_o
            ok, t, prim, _ = oscene.world_hit(S.cam_o, d, 1e-4, float(np.finfo(np.float32).max))
            if not ok:
                alb[pix] += 1.0
                continue
            te = t * float(np.linalg.norm(d))
            dep[pix] += (te, te * te, 1.0)
            alb[pix] += S.reflectance(prim, S.cam_o + t * d)
    return alb / spp, dep / spp
