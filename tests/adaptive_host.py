"""The callables of render_until over the host replay (frt.selftest_path_host): a backend
for the CPU tests of the adaptive driver (test_adaptive_host.py) and for
tools/adaptive_calibration.py.  A pass is cut into chunks as frtx_render_pixels cuts it
(samples_per_item, or max(1, spp / chunks) with chunks = 16; the tests take 4, since every
replay call flattens the scene again); one replay call per chunk gives the chunk sums, the
film is their sum times 1 / spp (film_reduce) and V comes from frtx_selftest_chunk_variance:
the arithmetic of the kernels.  A list of all pixels stands in for the full render."""
import contextlib
import os
import types

import numpy as np

import first_raytracer_amd as frt


@contextlib.contextmanager
def plain_flatten():
    """Every replay call flattens the scene again; without the tree refinement and shadow-tree
    passes (FRT_TREE_REFINE, FRT_SHADOW_TREE: they change the traversal's cost, not its hits)
    that takes microseconds instead of 0.15 s."""
    old = {k: os.environ.get(k) for k in ("FRT_TREE_REFINE", "FRT_SHADOW_TREE")}
    os.environ.update({k: "0" for k in old})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class HostBackend:
    def __init__(self, scene, nx, ny, chunks=16):
        self.scene, self.nx, self.ny, self.chunks = scene, nx, ny, chunks
        self.all = np.arange(nx * ny, dtype=np.int32)
        self.samples = 0            # pixel-samples traced so far
        self.calls = []             # (kind, pixels, spp, sample_offset) of every pass
        self._v = None

    def _pass(self, p, pixels):
        spp = p.spp
        spi = min(p.samples_per_item, spp) if p.samples_per_item > 0 else max(1, spp // self.chunks)
        sums = []
        for first in range(0, spp, spi):
            n = min(spi, spp - first)
            q = frt.RenderParams.from_buffer_copy(p)
            q.spp, q.sample_offset, q.samples_per_item = n, p.sample_offset + first, 0
            with plain_flatten():
                sums.append(frt.selftest_path_host(self.scene, q, pixels)[0] * np.float32(n))
        partial = np.array(sums, np.float32)
        rgb = partial.sum(axis=0, dtype=np.float32) * np.float32(1.0 / spp)
        v = frt.selftest_chunk_variance(partial, spp, spi) if len(sums) > 1 else None
        self.samples += len(pixels) * spp
        st = types.SimpleNamespace(work_items=len(pixels) * len(sums), kernel_ms=0.0)
        return rgb, v, st

    def render(self, p):
        rgb, self._v, st = self._pass(p, self.all)
        self.calls.append(("full", len(self.all), p.spp, p.sample_offset))
        # the driver compares work_items with the slot count of the frame's tiles
        st.work_items = frt.lib().frt_shard_slot_count(p) * (st.work_items // len(self.all))
        return rgb.reshape(self.ny, self.nx, 3), st

    def render_error(self, p):
        return self._v.reshape(self.ny, self.nx, 3)

    def render_pixels(self, p, pixels):
        self.calls.append(("sparse", len(pixels), p.spp, p.sample_offset))
        return self._pass(p, np.ascontiguousarray(pixels, np.int32))

    def until(self, p, target, max_spp, **kw):
        if kw.get("adaptive"):
            kw.setdefault("render_pixels", self.render_pixels)
        return frt.render_until(self.render, self.render_error, p, target, max_spp, **kw)
