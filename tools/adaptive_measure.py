#!/usr/bin/env python3
"""Measurements of the pixel-list kernel and the adaptive driver on one GPU, written to
profiles/adaptive/ (README and DESIGN.md 5d quote them).

  switch    Cornell and cornell_1m (the bench scenes, GPU-built BVH) at 1080p, 64 spp: kernel ms
            of the full render and of frtx_render_pixels over every pixel, the best of --steps
            runs each, alternating; ns per pixel-sample of both; the ratio full / sparse, and
            ADAPTIVE_SWITCH = the smaller ratio rounded down to one decimal.
  adaptive  Cornell 1080p at target 0.1, and the floor under the sun image at 1080p (the image
            sampled): Context.render_until adaptive against uniform -- total samples, kernel
            ms, e, converged, both from a first pass of 16 samples.  There is no 1080p golden
            image: no RMSE.

  python tools/adaptive_measure.py switch|adaptive [--steps 3] [--out-dir profiles/adaptive]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import first_raytracer_amd as frt  # noqa: E402

NX, NY = 1920, 1080
SCENES = os.path.join(ROOT, "tests", "golden", "scenes")


def bench_scene(ctx, name):
    obj = os.path.join(SCENES, "CornellBox-Original.obj")
    if name == "cornell_1m":
        dst = os.path.join(tempfile.gettempdir(), "cornell_1m_k172_adaptive.obj")
        if not os.path.exists(dst):
            frt.write_tessellated_obj(obj, 172, dst)
        obj = dst
    hs = frt.HostScene.from_spec({"objects": [{"obj": obj, "geo": True}], "camera": frt.CORNELL_CAMERA, "world": "list"},
                                 NX / NY)
    hs.build_bvh_gpu(ctx, "gsah")
    return hs


def measure_switch(ctx, steps, spp=64):
    res = {"frame": f"{NX}x{NY}, {spp} spp, seed 0, path", "steps": steps, "scenes": {}}
    pixels = np.arange(NX * NY, dtype=np.int32)
    for name in ("cornell", "cornell_1m"):
        ctx.upload(bench_scene(ctx, name))
        p = frt.RenderParams.make(NX, NY, spp)
        full, sparse = [], []
        film = rgb = None
        for _ in range(steps + 1):                      # the first pair warms up
            film, sf = ctx.render(p)
            rgb, _, ss = ctx.render_pixels(p, pixels)
            full.append(sf.kernel_ms)
            sparse.append(ss.kernel_ms)
        assert sf.samples == ss.samples == NX * NY * spp
        d = {"full_kernel_ms": full[1:], "sparse_kernel_ms": sparse[1:], "full_best_ms": min(full[1:]),
             "sparse_best_ms": min(sparse[1:]), "scene_in_lds_full": int(sf.scene_in_lds), "rays_full": int(sf.rays),
             "rays_sparse": int(ss.rays), "max_abs_diff": float(np.abs(film.reshape(-1, 3) - rgb).max())}
        d["full_ns_per_pixel_sample"] = d["full_best_ms"] * 1e6 / (NX * NY * spp)
        d["sparse_ns_per_pixel_sample"] = d["sparse_best_ms"] * 1e6 / (NX * NY * spp)
        d["ratio_full_over_sparse"] = d["full_best_ms"] / d["sparse_best_ms"]
        res["scenes"][name] = d
        print(name, json.dumps(d), flush=True)
    r = min(d["ratio_full_over_sparse"] for d in res["scenes"].values())
    res["switch"] = min(1.0, np.floor(r * 10) / 10)
    print("switch", res["switch"])
    return res


def run_both(ctx, p, target, cap, switch):
    out = {}
    for kind in ("uniform", "adaptive"):
        if kind == "uniform":
            film, v, spp, e, ok, passes = frt.render_until(lambda q: ctx.render(q), lambda q: ctx.render_error(q)[0], p,
                                                           target, cap, first_spp=16)
            samples = spp * p.nx * p.ny
            plist = [{"spp": a, "e": b, "kernel_ms": c} for a, b, c in passes]
        else:
            film, v, counts, e, ok, passes = frt.render_until(lambda q: ctx.render(q), lambda q: ctx.render_error(q)[0], p,
                                                              target, cap, first_spp=16, adaptive=True, switch=switch,
                                                              render_pixels=lambda q, px: ctx.render_pixels(q, px))
            samples = int(counts.astype(np.int64).sum())
            plist = [{"samples": a, "e": b, "kernel_ms": c, "pixels": d, "sparse": s} for a, b, c, d, s in passes]
            out["counts"] = {str(int(k)): int(n) for k, n in zip(*np.unique(counts, return_counts=True))}
        out[kind] = {"samples": samples, "kernel_ms": sum(x["kernel_ms"] for x in plist), "e": e, "converged": bool(ok),
                     "mean_film": float(np.asarray(film, np.float64).mean()), "passes": plist}
        print(kind, json.dumps({k: x for k, x in out[kind].items() if k != "passes"}), flush=True)
    return out


def measure_adaptive(ctx, switch, target=0.1, cap=1 << 14):
    import env_sampling_specs as E
    res = {"frame": f"{NX}x{NY}, seed 0, path, first_spp 16, max_spp {cap}", "target": target, "switch": switch,
           "note": "no 1080p golden image exists: no RMSE"}
    ctx.upload(bench_scene(ctx, "cornell"))
    ctx.set_env_image(None)
    res["cornell"] = run_both(ctx, frt.RenderParams.make(NX, NY, 1), target, cap, switch)
    ctx.upload(frt.HostScene.from_spec(E.floor_spec(), NX / NY))
    ctx.set_env_image(E.sun_image())
    res["floor_under_sun"] = run_both(ctx, frt.RenderParams.make(NX, NY, 1, flags=frt.FRT_FLAG_ENV_SAMPLING), target, cap,
                                      switch)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["switch", "adaptive"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--switch", type=float, default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "adaptive"))
    a = ap.parse_args()
    ctx = frt.Context(0)
    try:
        if a.what == "switch":
            res, name = measure_switch(ctx, a.steps), "switch.json"
        else:
            res = measure_adaptive(ctx, frt.ADAPTIVE_SWITCH if a.switch is None else a.switch)
            name = "adaptive_1080p.json"
    finally:
        ctx.close()
    os.makedirs(a.out_dir, exist_ok=True)
    with open(os.path.join(a.out_dir, name), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", os.path.join(a.out_dir, name))


if __name__ == "__main__":
    main()
