"""Shared pieces of the environment-image tests (test_env_image_host.py,
test_gpu_env_image.py, test_gpu_cli_env.py, test_hdr_reader.py): a Radiance
RGBE writer, the direction scene and the oracle-side expectation for it."""
import numpy as np

import scene_specs as SS

SENTINEL = (1000.0, 2000.0, 3000.0)   # constant env of the oracle's pixel selection: no normal or AO value reaches it


# ---- Radiance RGBE files, written by the tests themselves ----
def rgbe_random(nx, ny, seed, zero_exp_at=()):
    """(ny, nx, 4) uint8 RGBE texels: random mantissas, exponents around 128 so the
    values are O(1); texels listed in zero_exp_at (x, y) get e = 0."""
    rng = np.random.default_rng(seed)
    a = np.zeros((ny, nx, 4), np.uint8)
    a[..., :3] = rng.integers(0, 256, (ny, nx, 3))
    a[..., 3] = rng.integers(120, 137, (ny, nx))
    for x, y in zero_exp_at:
        a[y, x, 3] = 0
    return a


def rgbe_decode(a):
    """The independent decode: m * 2^(e - 136), e == 0 -> 0, as float32."""
    m = a[..., :3].astype(np.float64)
    e = a[..., 3:4].astype(np.float64)
    v = np.where(e == 0, 0.0, m * 2.0 ** (e - 136.0))
    return v.astype(np.float32)


def rle_channel(row, run_min=3):
    """New-style RLE of one channel of a scanline: runs (count | 128, value) for
    repeats of >= run_min, literal packets (count, bytes...) otherwise."""
    out = bytearray()
    i, n = 0, len(row)
    lit = bytearray()

    def flush():
        nonlocal lit
        while lit:
            out.append(min(len(lit), 128))
            out.extend(lit[:128])
            lit = lit[128:]
    while i < n:
        j = i
        while j < n and row[j] == row[i] and j - i < 127:
            j += 1
        if j - i >= run_min:
            flush()
            out.append(128 + (j - i))
            out.append(int(row[i]))
            i = j
        else:
            lit.append(int(row[i]))
            i += 1
    flush()
    return bytes(out)


def hdr_bytes(a, rle=False, header_extra=(), magic=b"#?RADIANCE", size_line=None):
    ny, nx = a.shape[:2]
    head = magic + b"\n" + b"".join(h + b"\n" for h in header_extra) + b"FORMAT=32-bit_rle_rgbe\n\n"
    head += (size_line if size_line is not None else b"-Y %d +X %d" % (ny, nx)) + b"\n"
    if not rle:
        return head + a.tobytes()
    body = bytearray()
    for y in range(ny):
        body += bytes([2, 2, nx >> 8, nx & 255])
        for k in range(4):
            body += rle_channel(a[y, :, k])
    return head + bytes(body)


# ---- the direction scene ----
DIR_NX, DIR_NY, DIR_SPP = 64, 48, 4
# Cornell box seen from far enough that it covers the middle of the frame; the camera looks
# down -z, so the u = 0 / 1 seam of the lat-long map runs down the middle column
DIR_CAM = {"lookfrom": (0.0, 1.0, 9.0), "lookat": (0.0, 1.0, 0.0), "vup": (0.0, 1.0, 0.0), "vfov": 40.0,
           "aperture": 0.0, "focus": 10.0}


def plain_cornell(world="bvh", cam=None):
    return {"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": cam or SS.CORNELL_CAM, "world": world}


def direction_spec():
    return plain_cornell(cam=DIR_CAM)


def random_env(nx, ny, seed=3, srgb=False):
    """Distinct random texels: float32 in [0.5, 4], or distinct sRGB bytes."""
    rng = np.random.default_rng(seed)
    if srgb:
        return rng.integers(1, 256, (ny, nx, 3)).astype(np.uint8)
    return rng.uniform(0.5, 4.0, (ny, nx, 3)).astype(np.float32)


def footprint_lookup(oscene, image, nx, ny, pixels):
    """For each listed pixel: ora_env_uv + ora_image_lookup over a 5 x 5 grid of
    camera rays (aperture 0) covering the pixel's footprint enlarged by 2 % of a
    pixel.  Returns (agree: all 25 lookups equal, value: the first lookup)."""
    import ctypes

    import oracle
    L = oracle.lib()
    cam = oscene.camera()
    o, llc, h, v = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    img = np.ascontiguousarray(image)
    fmt = 0 if img.dtype == np.uint8 else 1
    iy, ix = img.shape[:2]
    g = np.linspace(-0.02, 1.02, 5)
    agree = np.zeros(len(pixels), bool)
    value = np.zeros((len(pixels), 3))
    d = np.zeros(3)
    dp = d.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    out = np.zeros(3)
    outp = out.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    uu, vv = ctypes.c_double(), ctypes.c_double()
    for k, pix in enumerate(pixels):
        px, py = pix % nx, pix // nx
        first, same = None, True
        for gy in g:
            for gx in g:
                d[:] = (llc + ((px + gx) / nx) * h + ((py + gy) / ny) * v) - o
                L.ora_env_uv(dp, ctypes.byref(uu), ctypes.byref(vv))
                assert L.ora_image_lookup(ix, iy, fmt, img.ctypes.data, uu.value, vv.value, outp) == 0
                if first is None:
                    first = out.copy()
                elif not np.array_equal(first, out):
                    same = False
        agree[k] = same
        value[k] = first
    return agree, value


def direction_expectation(image, nx=DIR_NX, ny=DIR_NY, spp=DIR_SPP, seed=7):
    """Oracle side of the direction test.  Returns a dict:
      miss     pixels (linear index) all of whose samples missed (normals render
               with the sentinel env equals the sentinel exactly),
      tested   the pixels of `miss` whose 25 footprint lookups agree, value = the texel,
      ao_tested / ao_value   the same for pixels all of whose samples hit (no normals
               component reaches the sentinel) and whose AO value is the sentinel
               exactly: every sample unoccluded, so ao::Li returned the camera ray's
               environment."""
    import oracle
    spec = direction_spec()
    osc = oracle.OracleScene.from_spec(spec, nx / ny)
    osc.set_env(SENTINEL)
    nrm, _ = osc.render(nx, ny, spp, seed=seed, integrator=3)
    ao, _ = osc.render(nx, ny, spp, seed=seed, integrator=2)
    sent = np.asarray(SENTINEL)
    miss = np.flatnonzero((nrm == sent).all(axis=1))
    hit = np.flatnonzero((np.abs(nrm) <= 1.0 + 1e-9).all(axis=1))
    agree, value = footprint_lookup(osc, image, nx, ny, miss)
    ao_clear = hit[(ao[hit] == sent).all(axis=1)]
    ao_agree, ao_value = footprint_lookup(osc, image, nx, ny, ao_clear)
    return {"miss": miss, "tested": miss[agree], "value": value[agree].astype(np.float32),
            "ao_tested": ao_clear[ao_agree], "ao_value": ao_value[ao_agree].astype(np.float32),
            "seed": seed, "nx": nx, "ny": ny, "spp": spp}


def check_direction_conditions(exp):
    """The issue's conditions on the oracle side alone: M >= 25 % of the frame, tested >= 50 % of M."""
    n = exp["nx"] * exp["ny"]
    assert len(exp["miss"]) >= 0.25 * n, (len(exp["miss"]), n)
    assert len(exp["tested"]) >= 0.5 * len(exp["miss"]), (len(exp["tested"]), len(exp["miss"]))
