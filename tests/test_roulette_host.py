"""FRT_FLAG_ROULETTE on the host: Russian roulette in path_shade
(csrc/frt_path.hpp, the kMatsRoulette code) run by the host replay
(frt_selftest_path_host).  The oracle plays no roulette, so the expected values
are the estimator without the flag -- bit for bit where no vertex can play, in
expectation (the oracle's converged golden image) elsewhere."""
import os
import re

import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt
import roulette_specs as RS

ON = RS.ON
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frt.h")


def host_render(hs, nx, ny, env=None):
    pixels = np.arange(nx * ny, dtype=np.int32)
    return lambda p: frt.selftest_path_host(hs, p, pixels, env_image=env)


@pytest.fixture(scope="module")
def cornell(cornell_obj):
    return frt.HostScene("cornell_box_obj", cornell_obj, 1.0)


# ---- 1. the untouched prefix ----
@pytest.mark.parametrize("flags", [0, frt.FRT_FLAG_NO_LDS_SCENE, frt.FRT_FLAG_FP64])
def test_prefix_untouched(cornell_obj, flags):
    hs = frt.HostScene("cornell_box_obj", cornell_obj, 48 / 36)
    RS.check_prefix(host_render(hs, 48, 36), flags)


# ---- 3. fewer rays, same samples ----
def test_fewer_rays_same_samples(cornell):
    RS.check_fewer_rays(host_render(cornell, 64, 64))


# ---- 4. same expectation, against the fp64 golden image ----
def test_golden_expectation(cornell):
    RS.check_golden(host_render(cornell, 64, 64), 16)


# ---- no effect: AO, normals ----
def test_no_effect_on_ao_and_normals():
    nx, ny = 24, 18
    hs = frt.HostScene.from_spec(ES.plain_cornell(), nx / ny)
    render = host_render(hs, nx, ny, env=ES.random_env(16, 8))
    for integrator in (frt.FRT_INTEGRATOR_AO, frt.FRT_INTEGRATOR_NORMALS):
        a, sa = render(frt.RenderParams.make(nx, ny, 4, seed=2, flags=ON, integrator=integrator))
        b, sb = render(frt.RenderParams.make(nx, ny, 4, seed=2, integrator=integrator))
        assert np.array_equal(a, b) and sa.rays == sb.rays


# ---- 9. constants and parameter checks ----
def test_flag_value_matches_header():
    m = re.search(r"FRT_FLAG_ROULETTE\s*=\s*(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == frt.FRT_FLAG_ROULETTE == 4096
    assert frt.lib().frt_get_abi_version() == 9


def test_params_accept_the_flag():
    p = frt.RenderParams.make(40, 24, 2, flags=ON, shard_index=1, shard_count=2)
    q = frt.RenderParams.make(40, 24, 2, shard_index=1, shard_count=2)
    assert np.array_equal(frt.shard_slots(p), frt.shard_slots(q))
    assert len(frt.shard_slots(frt.RenderParams.pssmlt(8, 8, 1, 16, flags=ON))) == 64   # refused at render, not here
    with pytest.raises(frt.FrtError):
        frt.shard_slots(frt.RenderParams.make(8, 8, 1, integrator=7, flags=ON))
