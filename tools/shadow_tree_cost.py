#!/usr/bin/env python3
"""What the shadow-tree pass (FRT_SHADOW_TREE) drops and saves on Cornell, from the host counter
(frtx_selftest_shadow_tree): no GPU.

  python tools/shadow_tree_cost.py > profiles/shadowtree/host_cost.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import first_raytracer_amd as frt  # noqa: E402

OBJ = os.path.join(ROOT, "tests", "golden", "scenes", "CornellBox-Original.obj")


def main():
    out = {"what": "host counter of csrc/host/tree_refine.cpp on the area-light shadow rays of the refinement pass's "
                   "validation replay (40 x 40, one sample a pixel), started at the main root and at the shadow root; "
                   "1e5 segments through tri_intersect of every dropped triangle"}
    ref = frt.HostScene("cornell_box_obj", OBJ, 16 / 9)
    sah = frt.HostScene.from_spec({"objects": [{"obj": OBJ, "geo": True}], "camera": frt.CORNELL_CAMERA, "world": "list"}, 16 / 9)
    sah.build_bvh_sah()
    for name, hs in (("reference_topology", ref), ("binned_sah", sah)):
        info, dropped, _ = frt.selftest_shadow_tree(hs, segments=100000, seed=1)
        info["dropped_triangles"] = [int(i) for i in dropped.nonzero()[0]]
        out[name] = info
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
