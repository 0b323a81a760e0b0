"""The workload of a hardware-counter pass over precomputed radiance transfer: on the
tessellated Cornell box (k = 172, 16^2 directions) one frtx_prt_transfer with one gather bounce, then
frt_trace_device over the identical ray records of the first 150,000 corners, any-hit and closest hit.
Run under the profiler, one counter set a run:

  rocprofv3 --pmc SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES SQ_WAVES --output-format csv -d DIR -o run -- python tools/prt_pmc_run.py
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import first_raytracer_amd as frt  # noqa: E402

CORNELL = os.path.join(ROOT, "tests", "golden", "scenes", "CornellBox-Original.obj")


def main():
    import torch
    ctx = frt.Context(0)
    with tempfile.TemporaryDirectory() as tmp:
        big = os.path.join(tmp, "cornell_k.obj")
        frt.write_tessellated_obj(CORNELL, 172, big)
        scene = frt.HostScene("cornell_box_obj", big, 16 / 9)
        scene.build_bvh_sah()
        ctx.upload(scene)
        dirs = frt.prt_sample_dirs(16, seed=1)
        _, st = ctx.prt_transfer_device(scene, dirs, 1)
        print("transfer: shadow rays", st.shadow_rays, "gathers", st.extension_rays, "kernel ms", st.kernel_ms, flush=True)
        o, n, _ = frt.prt_corners(scene)
        o, n = o.reshape(-1, 3)[:150000], n.reshape(-1, 3)[:150000]
        ci, dj = np.nonzero(n @ dirs.T > 0)
        dev = torch.device("cuda", 0)
        hits = torch.zeros((len(ci), 4), dtype=torch.float32, device=dev)
        for bit in (1, 0):
            rays = torch.from_numpy(frt.ray_records(o[ci], dirs[dj], streams=np.full(len(ci), bit, np.uint32))).to(dev)
            st = ctx.trace_device(rays.data_ptr(), len(ci), hits.data_ptr(), frt.FRT_FLAG_NO_LDS_SCENE)
            print("trace: any-hit" if bit else "trace: closest", len(ci), "rays, kernel ms", st.kernel_ms, flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
