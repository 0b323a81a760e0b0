#!/usr/bin/env python3
"""Same-process A/B of the exit-tree pass (FRT_EXIT_TREE): the bench scene's GPU-built tree uploaded
with the knob off and on, alternated, and the HIP-event kernel ms of every launch at 1080p x 512 spp
for the path integrator, PSS-MLT, AO and normals, with the film sum and ray counts of each, one JSON
line per launch.

  python tools/exit_tree_ab.py [--rounds 3] [--spp 512] [--res 1920x1080] [--out profiles/exittree/ab_exit.jsonl]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--spp", type=int, default=512)
    ap.add_argument("--res", default="1920x1080")
    ap.add_argument("--kinds", default="path,pssmlt,ao,normals")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np

    import first_raytracer_amd as frt
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import scene_specs as SS

    nx, ny = (int(x) for x in a.res.split("x"))
    ctx = frt.Context(0)

    def scene(env=None):   # as bench.py makes it: the OBJ as a list, then the device's binned-SAH tree
        hs = frt.HostScene.from_spec({"objects": [{"obj": SS.CORNELL_OBJ, "geo": True}], "camera": frt.CORNELL_CAMERA,
                                      "world": "list"}, nx / ny)
        if env is not None:
            hs.set_env(env)
        hs.build_bvh_gpu(ctx, "gsah")
        return hs
    plain, white = scene(), scene((1.0, 1.0, 1.0))   # AO: the black environment would make every sample 0
    out = open(a.out, "a") if a.out else None
    kinds = a.kinds.split(",")
    for rnd in range(a.rounds):
        for knob in ("0", "1"):
            os.environ["FRT_EXIT_TREE"] = knob
            for kind in kinds:
                ctx.upload(white if kind == "ao" else plain)
                if kind == "pssmlt":
                    p = frt.RenderParams.pssmlt(nx, ny, 16, 1 << 18, seed=1)
                    film, st = ctx.render(p, np.zeros((ny, nx, 3), np.float32))
                else:
                    integ = {"path": frt.FRT_INTEGRATOR_PATH, "ao": frt.FRT_INTEGRATOR_AO,
                             "normals": frt.FRT_INTEGRATOR_NORMALS}[kind]
                    film, st = ctx.render(frt.RenderParams.make(nx, ny, a.spp, seed=1, integrator=integ))
                rec = {"round": rnd, "exit_tree": int(knob), "kind": kind, "kernel_ms": st.kernel_ms,
                       "film_sum": float(np.asarray(film, np.float64).sum()), "rays": int(st.rays),
                       "extension_rays": int(st.extension_rays), "shadow_rays": int(st.shadow_rays),
                       "scene_bytes": int(st.scene_bytes), "scene_in_lds": int(st.scene_in_lds)}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    ctx.close()


if __name__ == "__main__":
    main()
