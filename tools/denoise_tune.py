#!/usr/bin/env python3
"""The CPU sweep the constants of csrc/frt_denoise.hpp were tuned with: the inputs of
tests/test_denoise_host.py::test_filter_helps (host-replay path films of Cornell 64 x 64 at 4 spp,
seeds 300..303, 16-spp host feature films), filtered by the fp64 restatement
(tests/denoise_specs.denoise_ref), mean per-pixel RMSE against golden/cornell_64x64_16384spp.pfm.
One constant is varied at a time around the header's values; sigma_n stays a power of two.

  python tools/denoise_tune.py > profiles/denoise/tuning_cpu.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import denoise_specs as DS  # noqa: E402
import golden_images as G  # noqa: E402

SWEEP = {"iterations": (2, 3, 4, 5, 6), "eps_a": (1e-4, 1e-3, 1e-2), "sigma_n": (16.0, 32.0, 64.0, 128.0),
         "sigma_z": (0.002, 0.003, 0.005, 0.007, 0.01, 0.02, 0.1), "sigma_l0": (1.0, 2.0, 4.0, 8.0, 16.0, 64.0)}


def main():
    gold = G.cornell64()
    films = DS.cornell64_noisy(os.path.join(ROOT, "tests", "golden", "scenes", "CornellBox-Original.obj"))
    base = DS.constants()

    def score(K):
        return float(np.mean([DS.rmse(DS.denoise_ref(f, N, A, D, K), gold) for _, f, (N, A, D) in films]))
    print("inputs: Cornell 64 x 64, host-replay path 4 spp, seeds 300..303, 16-spp host features")
    print(f"unfiltered          rmse {float(np.mean([DS.rmse(f, gold) for _, f, _ in films])):.5f}")
    print(f"header {base} rmse {score(base):.5f}")
    for name, values in SWEEP.items():
        for v in values:
            mark = "  <- header" if base[name] == v else ""
            print(f"{name:10s} = {v:<8g} rmse {score(dict(base, **{name: v})):.5f}{mark}")


if __name__ == "__main__":
    main()
