"""Measure precomputed radiance transfer on the GPU and write profiles/prt/transfer.json:

  * frtx_prt_transfer on Cornell (100^2 directions) and on the tessellated Cornell box of bench.py
    (cornell_1m, 16^2 directions): kernel ms and rays/s of bounce 0, of one gather bounce (the
    B = 1 call less the B = 0 call), and the whole call with B = 2;
  * the yardstick: frt_trace_device answering the identical ray records -- assembled from
    prt_corners for the corners and directions with cos > 0, any-hit for bounce 0, closest hit for
    the gather -- on the same scene in the same process, best of 5 (on cornell_1m over a prefix of
    the corners: the records of all of them are 12 GB);
  * frtx_prt_rays at 1920 x 1080 against frt_trace_device alone on the same rays.

  python tools/prt_bench.py [--out profiles/prt/transfer.json] [--k 172]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import first_raytracer_amd as frt  # noqa: E402

CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "CornellBox-Original.obj")
REPEATS = 5


def best(fn, n=REPEATS):
    out = [fn() for _ in range(n)]
    ms = [o.kernel_ms for o in out]
    return min(ms), max(ms), out[int(np.argmin(ms))]


def yardstick(ctx, scene, dirs, max_corners, flags):
    """rays/s of frt_trace_device on the transfer's own rays (a prefix of the corners), any-hit and closest."""
    import torch
    o, n, _ = frt.prt_corners(scene)
    o, n = o.reshape(-1, 3)[:max_corners], n.reshape(-1, 3)[:max_corners]
    ci, dj = np.nonzero(n @ dirs.T > 0)
    dev = torch.device("cuda", 0)
    hits = torch.zeros((len(ci), 4), dtype=torch.float32, device=dev)
    res = {"rays": int(len(ci)), "corners": int(len(o))}
    for name, bit in (("anyhit", 1), ("closest", 0)):
        rec = frt.ray_records(o[ci], dirs[dj], streams=np.full(len(ci), bit, np.uint32))
        rays = torch.from_numpy(rec).to(dev)
        lo, hi, _ = best(lambda: ctx.trace_device(rays.data_ptr(), len(ci), hits.data_ptr(), flags))
        res[name] = {"best_ms": lo, "worst_ms": hi, "grays_per_s": len(ci) / lo * 1e-6, "spread": (hi - lo) / lo}
        del rays
    return res


def transfer(ctx, scene, dirs, flags):
    """kernel ms and rays/s of bounce 0, one gather bounce, and the B = 2 call (device entry: no copy of T)."""
    res = {}
    lo0, hi0, s0 = best(lambda: ctx.prt_transfer_device(scene, dirs, 0, flags)[1])
    lo1, hi1, s1 = best(lambda: ctx.prt_transfer_device(scene, dirs, 1, flags)[1])
    lo2, hi2, s2 = best(lambda: ctx.prt_transfer_device(scene, dirs, 2, flags)[1], 3)
    res["bounce0"] = {"best_ms": lo0, "worst_ms": hi0, "rays": s0.shadow_rays, "grays_per_s": s0.shadow_rays / lo0 * 1e-6}
    res["gather"] = {"best_ms": lo1 - lo0, "rays": s1.extension_rays, "grays_per_s": s1.extension_rays / max(lo1 - lo0, 1e-9) * 1e-6}
    res["bounces2"] = {"best_ms": lo2, "worst_ms": hi2, "total_ms": s2.total_ms, "rays": s2.shadow_rays + s2.extension_rays}
    res["plan"] = {"stack_entries": s0.stack_entries, "bvh_depth": s0.bvh_depth}
    return res


def rays_1080p(ctx, scene, T, li):
    import torch
    nx, ny = 1920, 1080
    p = frt.RenderParams.make(nx, ny, 1, seed=1)
    rays = ctx.camera_rays(p, np.arange(nx * ny, dtype=np.int32))
    lo, hi, _ = best(lambda: ctx.prt_rays(T, li, rays)[1])
    dev = torch.device("cuda", 0)
    closest = rays.copy()
    closest.view(np.uint32)[:, 7] = 0
    tr, th = torch.from_numpy(closest).to(dev), torch.zeros((nx * ny, 4), dtype=torch.float32, device=dev)
    tlo, thi, _ = best(lambda: ctx.trace_device(tr.data_ptr(), nx * ny, th.data_ptr(), 0))
    return {"rays": nx * ny, "prt_rays_ms": lo, "prt_rays_worst_ms": hi, "trace_alone_ms": tlo, "trace_alone_worst_ms": thi}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prt", "transfer.json"))
    ap.add_argument("--k", type=int, default=172)
    a = ap.parse_args()
    ctx = frt.Context(0)
    out = {"repeats": REPEATS, "scenes": {}}
    with tempfile.TemporaryDirectory() as tmp:
        big = os.path.join(tmp, "cornell_k.obj")
        frt.write_tessellated_obj(CORNELL, a.k, big)
        for name, obj, sqrt_n, prefix in (("cornell", CORNELL, 100, 108), ("cornell_1m", big, 16, 150000)):
            t0 = time.perf_counter()
            scene = frt.HostScene("cornell_box_obj", obj, 16 / 9)
            if name == "cornell_1m":
                scene.build_bvh_sah()                       # the binned SAH tree: quick to build at this size
            ctx.upload(scene)
            dirs = frt.prt_sample_dirs(sqrt_n, seed=1)
            r = {"n_tris": int(scene.info.n_tris), "n_dirs": len(dirs), "setup_s": time.perf_counter() - t0}
            r["transfer"] = transfer(ctx, scene, dirs, 0)
            r["yardstick"] = yardstick(ctx, scene, dirs, prefix, frt.FRT_FLAG_NO_LDS_SCENE)
            if name == "cornell":
                r["yardstick_default_plan"] = yardstick(ctx, scene, dirs, prefix, 0)   # the LDS-resident plan of the ray queries
                T, _ = ctx.prt_transfer(scene, dirs, 2)
                r["rays_1080p"] = rays_1080p(ctx, scene, T, frt.sh_project_image(None, env_color=(1.0, 1.0, 1.0)))
            out["scenes"][name] = r
            print(name, json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
