"""frt_render --env-map: the CLI decodes a Radiance .hdr file (frt_read_hdr),
hands it to its contexts through frt::Scene::set_env_map and renders the film
the Python binding renders for the same scene and image.  The file is written
here (tests/env_specs.py); the CLI runs as a child process."""
import os
import subprocess

import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt
from test_gpu_cli import CLI, read_pfm

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("integ,code", [("path", frt.FRT_INTEGRATOR_PATH), ("normals", frt.FRT_INTEGRATOR_NORMALS)])
def test_cli_env_map_matches_binding(cornell_obj, tmp_path, integ, code):
    hdr = tmp_path / "env.hdr"
    hdr.write_bytes(ES.hdr_bytes(ES.rgbe_random(32, 16, seed=6), rle=True))
    out = str(tmp_path / "e.pfm")
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "64x48", "--ns", "8", "--seed", "3",
                        "--integrator", integ, "--env-map", str(hdr), "--out", out],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    img = read_pfm(out)
    image = frt.read_hdr(str(hdr))
    assert np.array_equal(image.view(np.uint32), ES.rgbe_decode(ES.rgbe_random(32, 16, seed=6)).view(np.uint32))
    ctx = frt.Context(0)
    try:
        ctx.upload(frt.HostScene("cornell_box_obj", cornell_obj, 64 / 48))
        plain, _ = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3, integrator=code))
        ctx.set_env_image(image)
        film, _ = ctx.render(frt.RenderParams.make(64, 48, 8, seed=3, integrator=code))
    finally:
        ctx.close()
    assert np.array_equal(img, film)
    assert not np.array_equal(film, plain)          # the map is seen (the box's front is open)


def test_cli_env_flags_exclusive(cornell_obj, tmp_path):
    """No GPU work: the flags are refused before anything is created."""
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--env", "1,1,1", "--env-map", "x.hdr"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "exclude" in r.stderr
    r = subprocess.run([CLI, "--scene", "cornell", "--obj", cornell_obj, "--res", "16x16", "--ns", "1",
                        "--env-map", str(tmp_path / "missing.hdr"), "--out", str(tmp_path / "o.pfm")],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "frt_read_hdr" in r.stderr
    assert not os.path.exists(tmp_path / "o.pfm")
