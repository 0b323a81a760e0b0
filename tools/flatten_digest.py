#!/usr/bin/env python3
"""Digest of everything scene flattening and the passes over its tree compute on the host, one JSON
record per scene: a SHA-256 of what each of the three counting hooks returns (frtx_selftest_tree_refine,
frtx_selftest_shadow_tree, frtx_selftest_exit_tree in modes 0, 1 and -1) and of a 16 x 16, 4 spp
host-rendered path film with flags 0 and FRT_FLAG_BVH2.  Two builds whose outputs are equal flatten
every scene to the same bits.  The library is the one FRT_LIB_PATH names (default: the in-tree one).
No GPU.

  FRT_LIB_PATH=.../libfrt.so python tools/flatten_digest.py [--out FILE]
"""
import argparse
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def sha(*parts):
    h = hashlib.sha256()
    for p in parts:
        if isinstance(p, np.ndarray):
            h.update(str((p.dtype.str, p.shape)).encode())
            h.update(np.ascontiguousarray(p).tobytes())
        elif isinstance(p, dict):   # an info record: floats by their bits
            for k in sorted(p):
                v = list(p[k]) if hasattr(p[k], "_length_") else p[k]   # (a ctypes array field)
                h.update(k.encode())
                if isinstance(v, np.ndarray):
                    h.update(v.tobytes())
                else:
                    h.update(repr([x.hex() if isinstance(x, float) else x for x in (v if isinstance(v, (list, tuple)) else [v])]).encode())
        else:
            h.update(repr(p).encode())
    return h.hexdigest()


def scenes(frt, tmp):
    import exit_tree_scenes as ETS
    import scene_specs as SS
    import shadow_tree_scenes as STS

    yield "cornell_ref", frt.HostScene("cornell_box_obj", SS.CORNELL_OBJ, 1.0)
    sah = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                   "world": "list"}, 1.0)
    sah.build_bvh_sah()
    yield "cornell_sah", sah
    for k, b in ETS.scenes(os.path.join(tmp, "ets")).items():
        yield "ets_" + k, b.hs
    for k, v in STS.scenes(os.path.join(tmp, "sts")).items():
        yield "sts_" + k, v[0].hs
    for k, spec in (("textured", SS.cornell_textured()), ("conductors", SS.cornell_conductors()),
                    ("image_textured", SS.cornell_image_textured()), ("textured_list", SS.cornell_textured("list"))):
        yield "spec_" + k, frt.HostScene.from_spec(spec, 1.0)
    # an HBM-plan scene: Cornell tessellated as cornell_1m is, at a size the host renders quickly
    obj = os.path.join(tmp, "cornell_k6.obj")
    frt.write_tessellated_obj(SS.CORNELL_OBJ, 6, obj)
    yield "cornell_hbm_k6", frt.HostScene("cornell_box_obj", obj, 1.0)


def record(frt, hs):
    out = {}
    (c0, n0), (c1, n1) = frt.selftest_tree_refine(hs)
    out["tree_refine"] = sha(c0, n0, c1, n1)
    info, dropped, nodes = frt.selftest_shadow_tree(hs)
    out["shadow_tree"] = sha(info, dropped, nodes)
    for mode in (0, 1, -1):
        info, roots, taken, n_off, n_on = frt.selftest_exit_tree(hs, mode)
        out["exit_tree_%d" % mode] = sha(info, roots, taken, n_off, n_on)
        if mode == 1:
            out["exit"] = {k: info[k] for k in ("why_name", "taken", "nodes_added", "lds_bytes", "lds_bytes_oct")}
    pixels = np.arange(16 * 16, dtype=np.int32)
    for name, flags in (("film", 0), ("film_bvh2", frt.FRT_FLAG_BVH2)):
        film, st = frt.selftest_path_host(hs, frt.RenderParams.make(16, 16, 4, seed=3, flags=flags), pixels)
        out[name] = sha(film, st.as_dict())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import first_raytracer_amd as frt

    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, hs in scenes(frt, tmp):
            lines.append(json.dumps({"scene": name, **record(frt, hs)}, sort_keys=True))
            print(lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
