#!/usr/bin/env python3
"""The CPU gate of the tree refinement pass (FRT_TREE_REFINE): node visits V and
primitive tests T per ray, counted on the host by the kernels' visit rule on the
pass's validation rays, without and with the pass, for the trees the bench can
run on, and the pass's cost in seconds on one core.  No GPU.

  python tools/tree_refine_cost.py > profiles/treeopt/host_cost.json
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import first_raytracer_amd as frt  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def build(obj, bvh):
    path = os.path.join(SCENES, obj)
    if bvh == "host":      # the reference's create_bvh topology
        return frt.HostScene("cornell_box_obj", path, 16 / 9)
    hs = frt.HostScene.from_spec({"objects": [{"obj": path, "geo": True}], "camera": frt.CORNELL_CAMERA,
                                  "world": "list"}, 16 / 9)
    hs.build_bvh_sah()     # binned SAH on the host: the rule of the default --bvh gpu builder
    return hs


def flatten_seconds(hs, knob, repeats=5):
    """a host replay of 1 pixel: the flatten dominates; best of `repeats`"""
    os.environ["FRT_TREE_REFINE"] = knob
    best = 1e9
    for _ in range(repeats):
        t0 = time.perf_counter()
        frt.selftest_path_host(hs, frt.RenderParams.make(8, 8, 1), np.zeros(1, np.int32))
        best = min(best, time.perf_counter() - t0)
    del os.environ["FRT_TREE_REFINE"]
    return best


def main():
    out = {"what": "host counter of csrc/host/tree_refine.cpp on the pass's validation rays (a 40 x 40 frame of the "
                   "scene's camera, path + NEE, max_depth 33); J = V + w T", "trees": []}
    for obj, bvh in (("CornellBox-Original.obj", "sah"), ("CornellBox-Original.obj", "host"),
                     ("CornellBox-Sphere.obj", "sah"), ("CornellBox-Sphere.obj", "host")):
        hs = build(obj, bvh)
        (c0, _), (c1, _) = frt.selftest_tree_refine(hs)
        rec = {"scene": obj, "bvh": bvh, "off": c0, "on": c1}
        if c0["applies"]:
            rec["change"] = {k: round(c1[k] / c0[k] - 1.0, 4) for k in ("v", "t", "j")}
            rec["pass_seconds"] = round(flatten_seconds(hs, "1") - flatten_seconds(hs, "0"), 4)
        else:
            rec["note"] = "not LDS-resident: the pass does not run"
        out["trees"].append(rec)
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
