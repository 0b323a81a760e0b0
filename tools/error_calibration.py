#!/usr/bin/env python3
"""Calibration of the error film (FRT_INTEGRATOR_ERROR) on the CPU: how close is
sum of mean V to the sum of the actual mean squared error against the converged
golden image, and how much does that ratio scatter from seed to seed?  The GPU
tests (tests/test_gpu_error.py) take their windows from the file this writes.

Frame: CornellBox-Original 64 x 64, the parameters of the roulette and Sobol'
golden tests (max_depth 33, no flags), against tests/golden/cornell_64x64_16384spp.pfm.
Everything runs through the host replay (frt_selftest_path_host), one call per
chunk (spp = the chunk's samples, sample_offset = its first sample), and the
chunk films go through frtx_selftest_chunk_variance: the arithmetic of the kernel.

  hash     16 spp in 16 chunks of one sample, per seed r = mean V / mean (film - golden)^2
  sobol    FRT_FLAG_SOBOL, four replicates of 16 spp (seeds b .. b + 3): V = the sample
           variance of the replicate means / 4 (render_until's rule), r as above for the
           mean film
  sobol_error_film
           FRT_FLAG_SOBOL, 64 spp in 64 chunks of one sample: the ERROR film of a
           stratified render, an upper estimate (reported, on fewer seeds)

The window of a test that sums S seeds is 1 +- 4 sd / sqrt(S), sd the per-seed
standard deviation of r; it may not be wider than +- 25 %, so S is the smallest
multiple of 8 that keeps it inside.

  python tools/error_calibration.py [--seeds 32] [--out profiles/error/calibration.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import first_raytracer_amd as frt  # noqa: E402
import golden_images as G  # noqa: E402

NX = NY = 64
CAP = 0.25


def chunk_films(hs, seed, spp, spi, flags):
    """(K, nx ny, 3) chunk means of one render, one host replay call per chunk."""
    pix = np.arange(NX * NY, dtype=np.int32)
    out = []
    for first in range(0, spp, spi):
        n = min(spi, spp - first)
        p = frt.RenderParams.make(NX, NY, n, seed=seed, flags=flags, sample_offset=first)
        out.append(frt.selftest_path_host(hs, p, pix)[0])
    return np.array(out)


def error_film(hs, seed, spp, spi, flags):
    """(film, V) as a render and the ERROR call after it give them: the film from the chunk
    sums (film_reduce: their sum times 1 / spp), V from the hook."""
    films = chunk_films(hs, seed, spp, spi, flags)
    n = np.array([min(spi, spp - f) for f in range(0, spp, spi)], np.float32)[:, None, None]
    partial = films * n
    film = partial.sum(axis=0, dtype=np.float32) * np.float32(1.0 / spp)
    return film, frt.selftest_chunk_variance(partial, spp, spi)


def summary(name, v_means, mses, s_test=8):
    v_means, mses = np.asarray(v_means), np.asarray(mses)
    r = v_means / mses
    sd = float(r.std(ddof=1))
    s = s_test
    while 4 * sd / np.sqrt(s) > CAP:
        s += 8
    d = {"seeds": len(r), "ratio_of_sums": float(v_means.sum() / mses.sum()), "per_seed_mean": float(r.mean()),
         "per_seed_sd": sd, "test_seeds": s, "half_width": float(4 * sd / np.sqrt(s)),
         "per_seed": [float(x) for x in r]}
    print(f"{name}: ratio of sums {d['ratio_of_sums']:.4f}  per-seed mean {d['per_seed_mean']:.4f} sd {sd:.4f}  "
          f"-> S = {s}, window 1 +- {d['half_width']:.4f}")
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=32)
    ap.add_argument("--first-seed", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error", "calibration.json"))
    a = ap.parse_args()
    hs = frt.HostScene("cornell_box_obj", os.path.join(ROOT, "tests", "golden", "scenes", "CornellBox-Original.obj"), 1.0)
    g = G.cornell64().reshape(-1, 3)
    res = {"frame": "CornellBox-Original 64x64, max_depth 33, against cornell_64x64_16384spp.pfm",
           "first_seed": a.first_seed, "cap": CAP}

    vm, ms, es = [], [], []
    for k in range(a.seeds):
        film, v = error_film(hs, a.first_seed + k, 16, 1, 0)
        vm.append(v.astype(np.float64).mean())
        ms.append(((film - g) ** 2).mean())
        es.append(frt.frame_error(film, v))
    res["hash"] = dict(summary("hash 16 spp", vm, ms), spp=16, samples_per_item=1, e_mean=float(np.mean(es)))

    SB = frt.FRT_FLAG_SOBOL
    vm, ms = [], []
    pix = np.arange(NX * NY, dtype=np.int32)
    for k in range(a.seeds):
        b = a.first_seed + 4 * k
        reps = [frt.selftest_path_host(hs, frt.RenderParams.make(NX, NY, 16, seed=b + j, flags=SB), pix)[0] for j in range(4)]
        film, v = frt.replicate_variance(reps)
        vm.append(v.astype(np.float64).mean())
        ms.append(((film - g) ** 2).mean())
    res["sobol"] = dict(summary("sobol 4 x 16 spp replicates", vm, ms), spp=64, first_spp=16, seed_step=4)

    vm, ms = [], []
    for k in range(min(a.seeds, 8)):
        film, v = error_film(hs, a.first_seed + k, 64, 1, SB)
        vm.append(v.astype(np.float64).mean())
        ms.append(((film - g) ** 2).mean())
    r = float(np.sum(vm) / np.sum(ms))
    print(f"sobol 64 spp, ERROR film: sum mean V / sum MSE = {r:.4f} (an upper estimate: > 1)")
    res["sobol_error_film"] = {"seeds": len(vm), "spp": 64, "samples_per_item": 1, "ratio_of_sums": r}

    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
