"""The context's grow-only buffers (csrc/frt_devbuf.hpp) and the shared launch scaffold
(csrc/frt_render.hip persist_*) under reuse: one context makes a sequence of calls whose sizes grow,
shrink and cross the 64-entry block of the lists and the 256-ray block of the ray queries, so that
every shared buffer is used at a smaller size after a larger one and handed from one entry point to
the next.  Each call's outputs must be the bytes, and its ray counters the numbers, of the same call
on a fresh context."""
import numpy as np
import pytest
import torch

import first_raytracer_amd as frt

pytestmark = pytest.mark.gpu


def counters(st):
    return (st.camera_rays, st.extension_rays, st.shadow_rays, st.samples)


def trace(c, rays):
    dev = torch.device("cuda", 0)
    tr = torch.from_numpy(rays).to(dev)
    th = torch.zeros((len(rays), 4), dtype=torch.float32, device=dev)
    st = c.trace_device(tr.data_ptr(), len(rays), th.data_ptr())
    return th.cpu().numpy(), st


def test_buffers_reused_across_entry_points(cornell_obj):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 1.0)
    small = frt.RenderParams.make(16, 16, 4, seed=5)
    big = frt.RenderParams.make(64, 48, 8, seed=6, samples_per_item=4)
    rng = np.random.default_rng(3)
    px65 = rng.integers(0, 64 * 48, 65).astype(np.int32)
    one_ray = frt.ray_records([[0, 1, 3]], [[0.1, -0.2, -1]])
    rays257 = np.zeros((257, 8), np.float32)
    rays257[:, :3] = rng.uniform(-0.9, 0.9, (257, 3)) + np.array([0.0, 1.0, 0.0])
    rays257[:, 3] = 1e30
    rays257[:, 4:7] = rng.normal(size=(257, 3))
    mlt = frt.RenderParams.pssmlt(16, 16, 4, 64, seed=7, bootstrap=256)
    list_p = frt.RenderParams.make(64, 48, 8, seed=8, samples_per_item=4)
    ray_p = frt.RenderParams.make(1, 1, 4, seed=9)
    small_film = {}

    def denoise(c):
        return c.denoise(np.maximum(small_film["film"], 0).copy(), 16, 16, spp=4, seed=5)

    # (name, the calls a fresh context makes first, the call)
    steps = [
        ("path 16x16", [], lambda c: c.render(small)),
        ("path 64x48", [], lambda c: c.render(big)),
        ("error film", [lambda c: c.render(big)], lambda c: c.render_error(big)),
        ("render_pixels 65", [], lambda c: c.render_pixels(list_p, px65, variance=True)),
        ("radiance_rays 1", [], lambda c: c.radiance_rays(ray_p, one_ray, variance=True)),
        ("pssmlt 16x16", [], lambda c: c.render(mlt)),
        ("path 16x16 again", [], lambda c: c.render(small)),
        ("denoise", [], denoise),
        ("trace_device 257", [], lambda c: trace(c, rays257)),
        ("render_pixels 1", [], lambda c: c.render_pixels(list_p, px65[:1], variance=True)),
    ]
    shared = frt.Context(0)
    shared.upload(hs)
    try:
        for name, before, call in steps:
            got = call(shared)
            if name == "path 16x16":
                small_film["film"] = got[0]
                assert got[0].max() > 0
            fresh = frt.Context(0)
            try:
                fresh.upload(hs)
                for b in before:
                    b(fresh)
                want = call(fresh)
            finally:
                fresh.close()
            assert len(got) == len(want)
            for g, w in zip(got[:-1], want[:-1]):
                assert g.shape == w.shape and g.tobytes() == w.tobytes(), name
            print(name, counters(got[-1]), "kernel ms", got[-1].kernel_ms)
            assert counters(got[-1]) == counters(want[-1]), name
            assert (got[-1].pixels, got[-1].work_items) == (want[-1].pixels, want[-1].work_items), name
            assert name == "error film" or got[-1].camera_rays > 0, name
            assert name.startswith("trace") or np.isfinite(got[0]).all(), name   # a hit record holds primitive bits
    finally:
        shared.close()
