#!/usr/bin/env python3
"""Host-side gate of the exit-tree pass (FRT_EXIT_TREE): what frtx_selftest_exit_tree says the pass takes
on CornellBox-Original -- the reference's topology and the binned-SAH tree -- and the node visits V,
primitive tests T and J = V + 1.8 T per ray of the refinement pass's validation replay with the exit
roots ignored and used, over all rays and over the extension rays.  No GPU.

  python tools/exit_tree_cost.py [--out profiles/exittree/host_cost.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exittree", "host_cost.json"))
    a = ap.parse_args()
    import first_raytracer_amd as frt
    import scene_specs as SS

    ref = frt.HostScene("cornell_box_obj", SS.CORNELL_OBJ, 1.0)
    sah = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": SS.CORNELL_CAM,
                                   "world": "list"}, 1.0)
    sah.build_bvh_sah()
    out = {}
    for name, hs in (("cornell_reference_topology", ref), ("cornell_binned_sah", sah)):
        info, roots, taken, _, _ = frt.selftest_exit_tree(hs, 1)
        info = {k: v for k, v in info.items() if k not in ("view_of", "reserved")}
        info["roots"] = roots.tolist()
        info["taken"] = [dict(zip(("sub", "root", "members", "dropped", "added", "shared"), map(int, r))) for r in taken]
        info["j_all_change"] = info["j_all"][1] / info["j_all"][0] - 1.0
        out[name] = info
        print(name, "J", info["j_all"], "ext V", info["v_ext"], "ext T", info["t_ext"], "+%d nodes" % info["nodes_added"])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
