#!/usr/bin/env python3
"""The far-origin table of DESIGN.md section 3: rays from distance R of the scene's centre, aimed
at the scene, that the list world hits and a tree plan loses (a miss, or a farther hit), on one
GPU.  Both sides run the same fp32 primitive tests, so every loss is a box culled in error.

    python tools/far_origin_table.py [--rays 20000] [--out table.json]
"""
import argparse
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import first_raytracer_amd as frt  # noqa: E402
import trace_rays as TR  # noqa: E402

SCENES = os.path.join(ROOT, "tests", "golden", "scenes")
PLANS = (("default", 0), ("bvh4q", frt.FRT_FLAG_NO_LDS_SCENE), ("bvh2", frt.FRT_FLAG_NO_LDS_SCENE | frt.FRT_FLAG_BVH2))
ROWS = (("interior", "cornell"), ("interior", "k24"), ("vertex", "cornell"), ("vertex", "k6"))


def trace(ctx, rays, flags=0):
    dev = torch.device("cuda", 0)
    tr = torch.tensor(rays, device=dev)
    th = torch.empty((len(rays), 4), dtype=torch.float32, device=dev)
    ctx.trace_device(tr.data_ptr(), len(rays), th.data_ptr(), flags)
    return th.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=20000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp())
    out, worlds = [], {}
    for what, mesh in ROWS:
        if mesh not in worlds:
            ls, bs = TR.scene_pair(mesh, os.path.join(SCENES, "CornellBox-Original.obj"), os.path.join(SCENES, "veach_mi.obj"), tmp)
            cl, cb = frt.Context(0), frt.Context(0)
            cl.upload(ls)
            cb.upload(bs)
            worlds[mesh] = (TR.Geometry(ls), cl, cb)
        g, cl, cb = worlds[mesh]
        for R in (10, 100, 1000, 10000):
            rays = TR.far(g, a.rays, 1, R, what)
            hl = trace(cl, rays)
            lp = TR.prim_of(hl)
            row = {"target": what, "mesh": mesh, "R": R, "rays": a.rays, "list_hits": int((lp >= 0).sum())}
            for plan, flags in PLANS:
                hb = trace(cb, rays, flags)
                row[plan] = int(((lp >= 0) & ((TR.prim_of(hb) < 0) | (hb[:, 0] > hl[:, 0]))).sum())
            print(json.dumps(row), flush=True)
            out.append(row)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
