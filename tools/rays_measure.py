#!/usr/bin/env python3
"""Timing of the ray-list kernel beside the pixel-list kernel on one GPU, written to
profiles/rays/rays_1080p.json (README and DESIGN.md 5e quote it).

Cornell and cornell_1m (the bench scenes, GPU-built BVH) at 1080p, 64 spp, path: the rays are the
camera's own (Context.camera_rays of every pixel at sample 0), so both kernels run the same
scene, plan and sample count.  Kernel ms (device events around the sparse kernel and its reduce)
of frtx_render_pixels over every pixel and of frtx_radiance_rays over those rays, alternating in
one process, --steps timed pairs after one warm-up pair; the best and the spread (max - min) of
each, and ns per ray-sample.  The two do not trace the same paths: the pixel list jitters its 64
camera rays over the pixel, the ray list repeats one ray 64 times, whose first hits coincide --
less divergence in the first bounces, so the ray figure may come out lower.

  python tools/rays_measure.py [--steps 5] [--out profiles/rays/rays_1080p.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import first_raytracer_amd as frt  # noqa: E402
from adaptive_measure import NX, NY, bench_scene  # noqa: E402


def measure(ctx, steps, spp=64):
    res = {"frame": f"{NX}x{NY}, {spp} spp, seed 0, path", "rays": "camera_rays of every pixel at sample 0", "steps": steps,
           "scenes": {}}
    pixels = np.arange(NX * NY, dtype=np.int32)
    n = NX * NY * spp
    for name in ("cornell", "cornell_1m"):
        ctx.upload(bench_scene(ctx, name))
        p = frt.RenderParams.make(NX, NY, spp)
        rays = ctx.camera_rays(p, pixels)
        pix_ms, ray_ms = [], []
        for _ in range(steps + 1):                      # the first pair warms up
            a, _, sp = ctx.render_pixels(p, pixels)
            b, _, sr = ctx.radiance_rays(p, rays)
            pix_ms.append(sp.kernel_ms)
            ray_ms.append(sr.kernel_ms)
        assert sp.samples == sr.samples == n and sr.camera_rays == n and sp.stack_entries == sr.stack_entries
        d = {"pixels_kernel_ms": pix_ms[1:], "rays_kernel_ms": ray_ms[1:], "pixels_best_ms": min(pix_ms[1:]),
             "rays_best_ms": min(ray_ms[1:]), "pixels_spread_ms": max(pix_ms[1:]) - min(pix_ms[1:]),
             "rays_spread_ms": max(ray_ms[1:]) - min(ray_ms[1:]), "traced_rays_pixels": int(sp.rays),
             "traced_rays_rays": int(sr.rays), "stack_entries": int(sr.stack_entries), "fp64": int(sr.fp64),
             "mean_pixels": float(a.mean()), "mean_rays": float(b.mean())}
        d["pixels_ns_per_sample"] = d["pixels_best_ms"] * 1e6 / n
        d["rays_ns_per_sample"] = d["rays_best_ms"] * 1e6 / n
        d["ratio_rays_over_pixels"] = d["rays_best_ms"] / d["pixels_best_ms"]
        res["scenes"][name] = d
        print(name, json.dumps(d), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rays", "rays_1080p.json"))
    a = ap.parse_args()
    ctx = frt.Context(0)
    res = measure(ctx, a.steps)
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
