#!/usr/bin/env python3
"""Digest of everything the host scene pipeline (OBJ import, the builders, frt_host_scene, the
tessellator) computes, one JSON record per scene: a SHA-256 over every array and scalar that
frt_scene_view_get exposes and over frt_scene_info without its two timings, as the scene is built and
again after build_bvh_sah().  The scenes are those of tools/flatten_digest.py, the golden OBJ files as
obj_geo and obj_smooth, and veach_mis; a last record hashes the bytes of a k = 6 tessellated OBJ + MTL.
Two builds whose outputs are equal build every scene to the same bits.  The library is the one
FRT_LIB_PATH names (default: the in-tree one).  No GPU.

  FRT_LIB_PATH=.../libfrt.so python tools/scene_digest.py [--out FILE]
"""
import argparse
import ctypes
import glob
import hashlib
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

# (pointer field, count field, bytes an element) of frt_scene_view
ARRAYS = [("tri_v", "n_tris", 72), ("tri_n", "n_tris", 72), ("tri_uv", "n_tris", 48), ("tri_inv_area", "n_tris", 8),
          ("tri_material", "n_tris", 4), ("tri_geometry_normal", "n_tris", 1), ("sphere", "n_spheres", 32),
          ("sphere_material", "n_spheres", 4), ("materials", "n_materials", None), ("node_box", "n_nodes", 48),
          ("node_child", "n_nodes", 8), ("list", "n_list", 4), ("lights", "n_lights", 4)]
SCALARS = ["world_kind", "root", "cam_origin", "cam_lower_left", "cam_horizontal", "cam_vertical", "cam_u", "cam_v",
           "cam_w", "cam_lens_radius", "cam_half_height", "env_color", "n_images"]


def digest(frt, hs):
    v = hs.view()
    h = hashlib.sha256()
    for ptr, cnt, size in ARRAYS:
        n = getattr(v, cnt)
        size = ctypes.sizeof(frt.Material) if size is None else size
        h.update(("%s %d;" % (ptr, n)).encode())
        if n and getattr(v, ptr):
            h.update(ctypes.string_at(getattr(v, ptr), n * size))
    for name in SCALARS:
        x = getattr(v, name)
        x = list(x) if hasattr(x, "_length_") else [x]
        h.update(("%s %r;" % (name, [e.hex() if isinstance(e, float) else e for e in x])).encode())
    info = frt.HostSceneInfo()
    frt.lib().frt_scene_info(hs.ptr, ctypes.byref(info))
    rec = {n: getattr(info, n) for n, _ in info._fields_ if n not in ("load_ms", "build_ms")}
    h.update(repr(sorted(rec.items())).encode())
    return h.hexdigest(), rec


def scenes(frt, tmp):
    import flatten_digest
    yield from flatten_digest.scenes(frt, tmp)
    golden = os.path.join(ROOT, "tests", "golden", "scenes")
    for obj in sorted(glob.glob(os.path.join(golden, "*.obj"))):
        for kind in ("obj_geo", "obj_smooth"):
            yield "%s_%s" % (os.path.basename(obj)[:-4], kind), frt.HostScene(kind, obj, 1.0)
    yield "veach_mis", frt.HostScene("veach_mis", os.path.join(golden, "veach_mi.obj"), 16 / 9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import first_raytracer_amd as frt

    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, hs in scenes(frt, tmp):
            built, info = digest(frt, hs)
            hs.build_bvh_sah()
            sah, info_sah = digest(frt, hs)
            lines.append(json.dumps({"scene": name, "built": built, "sah": sah, "n_tris": info["n_tris"],
                                     "n_nodes": info["n_nodes"], "depth": info["bvh_depth"],
                                     "sah_depth": info_sah["bvh_depth"]}, sort_keys=True))
            print(lines[-1], flush=True)
        import scene_specs as SS
        obj = os.path.join(tmp, "tess_k6.obj")
        frt.write_tessellated_obj(SS.CORNELL_OBJ, 6, obj)
        h = hashlib.sha256()
        for path in (obj, obj[:-4] + ".mtl"):
            with open(path, "rb") as f:
                # (the header line names the source by the path it was given)
                h.update(f.read().replace(os.path.dirname(SS.CORNELL_OBJ).encode(), b"<scenes>"))
        lines.append(json.dumps({"scene": "tessellated_k6_files", "sha": h.hexdigest()}))
        print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
