#!/usr/bin/env python3
"""Calibration of the adaptive render_until on the CPU: does stopping a pixel on its own V
bias the film and its error estimate?  Pixels whose first samples happen to agree stop early
with a V that is too small, so the sum of mean V falls below the sum of the actual mean
squared error.  This tool measures by how much, for the adaptive and for the uniform driver at
the same target, as tools/error_calibration.py does for one render.

Frame: CornellBox-Original 64 x 64 against tests/golden/cornell_64x64_16384spp.pfm, through
the host replay (tests/adaptive_host.py: the kernels' arithmetic), target 0.4 (the uniform
driver ends at 64 spp), max_spp 1024 (an adaptive run that still has active pixels there
returns what it has), switch 1.0.  Per seed r = mean V / mean (film - golden)^2.

The window of a test that sums S seeds is 1 +- 4 sd / sqrt(S), sd the per-seed standard
deviation of r; it may not be wider than +- 25 %, so S is the smallest multiple
of 8 that keeps it inside.  If the adaptive ratio of sums leaves its window at first_spp 16
the tool doubles first_spp until it holds, and records every try: the driver's default
ADAPTIVE_FIRST_SPP is the first that holds.

  python tools/adaptive_calibration.py [--seeds 64] [--jobs 8] [--out profiles/adaptive/calibration.json]
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NX = NY = 64
CAP = 0.25
TARGET, MAX_SPP = 0.4, 1024


def one_seed(job):
    seed, first_spp = job
    import first_raytracer_amd as frt
    import golden_images as G
    from adaptive_host import HostBackend
    hs = frt.HostScene("cornell_box_obj", os.path.join(ROOT, "tests", "golden", "scenes", "CornellBox-Original.obj"), 1.0)
    g = G.cornell64()
    p = frt.RenderParams.make(NX, NY, 1, seed=seed)
    out = {}
    for kind in ("uniform", "adaptive"):
        b = HostBackend(hs, NX, NY)
        r = b.until(p, TARGET, MAX_SPP, first_spp=first_spp, **({"adaptive": True, "switch": 1.0} if kind == "adaptive" else {}))
        film, v = r[0], r[1]
        out[kind] = (float(v.astype(np.float64).mean()), float(((film - g) ** 2).mean()), b.samples, float(r[3]), bool(r[4]),
                     float((film.astype(np.float64) - g).mean()))
    return out


def summary(name, rows, s_test=8):
    v_means, mses = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    r = v_means / mses
    sd = float(r.std(ddof=1))
    s = s_test
    while 4 * sd / np.sqrt(s) > CAP:
        s += 8
    d = {"seeds": len(r), "ratio_of_sums": float(v_means.sum() / mses.sum()), "per_seed_mean": float(r.mean()),
         "per_seed_sd": sd, "test_seeds": s, "half_width": float(4 * sd / np.sqrt(s)),
         "mean_samples": float(np.mean([x[2] for x in rows])), "mean_e": float(np.mean([x[3] for x in rows])),
         "converged": int(sum(x[4] for x in rows)), "mean_film_minus_golden": float(np.mean([x[5] for x in rows])),
         "rmse_of_sums": float(np.sqrt(mses.mean())), "per_seed": [float(x) for x in r]}
    print(f"{name}: ratio of sums {d['ratio_of_sums']:.4f}  per-seed mean {d['per_seed_mean']:.4f} sd {sd:.4f}  "
          f"-> S = {s}, window 1 +- {d['half_width']:.4f}; samples {d['mean_samples']:.0f}, film - golden {d['mean_film_minus_golden']:+.5f}")
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=64)
    ap.add_argument("--first-seed", type=int, default=3000)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive", "calibration.json"))
    a = ap.parse_args()
    res = {"frame": "CornellBox-Original 64x64, max_depth 33, against cornell_64x64_16384spp.pfm, host replay",
           "target": TARGET, "max_spp": MAX_SPP, "switch": 1.0, "first_seed": a.first_seed, "cap": CAP, "tries": []}
    first_spp = 16
    with multiprocessing.Pool(a.jobs) as pool:
        while True:
            rows = pool.map(one_seed, [(a.first_seed + k, first_spp) for k in range(a.seeds)])
            t = {"first_spp": first_spp, "uniform": summary(f"uniform first_spp {first_spp}", [r["uniform"] for r in rows]),
                 "adaptive": summary(f"adaptive first_spp {first_spp}", [r["adaptive"] for r in rows])}
            res["tries"].append(t)
            d = t["adaptive"]
            if (abs(d["ratio_of_sums"] - 1.0) <= d["half_width"] and d["seeds"] >= d["test_seeds"]) or first_spp >= 128:
                break
            first_spp *= 2
    res["first_spp"] = first_spp
    res["uniform"], res["adaptive"] = res["tries"][-1]["uniform"], res["tries"][-1]["adaptive"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
