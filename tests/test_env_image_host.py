"""Environment images on the host: the scene builder's round trip
(frt_scene_set_env_image / frt_scene_env_image, spec key "env_image") and the
lookup itself -- env_eval of csrc/frt_path.hpp run by the host self-test
(frt_selftest_path_host_env reads the image as a render does) against the
oracle hooks ora_env_uv + ora_image_lookup on the direction scene at 32 x 24."""
import ctypes

import numpy as np
import pytest

import env_specs as ES
import first_raytracer_amd as frt
import scene_specs as SS

NX, NY, SPP = 32, 24, 4


def test_builder_round_trip():
    imgs = [{"data": SS.test_image(8, 4, 1)}, {"data": ES.random_env(6, 3)}]
    hs = frt.HostScene.from_spec(dict(ES.plain_cornell(), images=imgs), 1.0)
    assert hs.env_image() is None                       # none set: 0, *out left alone
    L = frt.lib()
    out = frt.Image(7, 7, 7, 7, None)
    assert L.frt_scene_env_image(hs.ptr, ctypes.byref(out)) == 0
    assert (out.nx, out.ny, out.format) == (7, 7, 7)
    hs.set_env_image(1)
    im = hs.env_image()
    assert (im.nx, im.ny, im.format) == (6, 3, frt.FRT_IMAGE_F32)
    got = np.ctypeslib.as_array(ctypes.cast(im.data, ctypes.POINTER(ctypes.c_float)), shape=(3, 6, 3))
    assert np.array_equal(got, imgs[1]["data"])          # the scene's own copy
    hs.set_env_image(0)
    assert hs.env_image().format == frt.FRT_IMAGE_SRGB8
    for bad in (2, -2, 100):
        assert L.frt_scene_set_env_image(hs.ptr, bad) == -1   # FRT_E_INVALID
        with pytest.raises(frt.FrtError):
            hs.set_env_image(bad)
    assert hs.env_image().nx == 8                       # a refused index changes nothing
    hs.set_env_image(None)
    assert hs.env_image() is None
    assert L.frt_scene_set_env_image(None, 0) == -1 and L.frt_scene_env_image(hs.ptr, None) == -1


def test_spec_key():
    imgs = [{"data": SS.test_image(8, 4, 1)}, {"data": ES.random_env(6, 3)}]
    hs = frt.HostScene.from_spec(dict(ES.plain_cornell(), images=imgs, env_image=1), 1.0)
    assert (hs.env_image().nx, hs.env_image().ny) == (6, 3)
    with pytest.raises(frt.FrtError):
        frt.HostScene.from_spec(dict(ES.plain_cornell(), images=imgs, env_image=2), 1.0)
    # the scene view is the one of the scene without the key (ABI 9: no field for it)
    assert frt.HostScene.from_spec(ES.plain_cornell(), 1.0).view().n_images == 0


@pytest.fixture(scope="module")
def expectation():
    image = ES.random_env(32, 16)
    exp = ES.direction_expectation(image, NX, NY, SPP)
    ES.check_direction_conditions(exp)
    return image, exp


@pytest.mark.parametrize("integrator,flags", [
    (frt.FRT_INTEGRATOR_NORMALS, 0), (frt.FRT_INTEGRATOR_PATH, 0), (frt.FRT_INTEGRATOR_PATH, frt.FRT_FLAG_FP64)])
def test_selftest_direction_map(expectation, integrator, flags):
    image, exp = expectation
    hs = frt.HostScene.from_spec(ES.direction_spec(), NX / NY)
    p = frt.RenderParams.make(NX, NY, SPP, seed=exp["seed"], integrator=integrator, flags=flags)
    out, _ = frt.selftest_path_host(hs, p, exp["tested"], env_image=image)
    np.testing.assert_allclose(out, exp["value"], rtol=1e-6, atol=0)


def test_selftest_ao_uses_camera_ray(expectation):
    """ao::Li evaluates the environment with the camera ray (ao.cpp:27), not the visibility ray."""
    image, exp = expectation
    assert len(exp["ao_tested"]) > 0
    hs = frt.HostScene.from_spec(ES.direction_spec(), NX / NY)
    p = frt.RenderParams.make(NX, NY, SPP, seed=exp["seed"], integrator=frt.FRT_INTEGRATOR_AO)
    out, _ = frt.selftest_path_host(hs, p, exp["ao_tested"], env_image=image)
    np.testing.assert_allclose(out, exp["ao_value"], rtol=1e-6, atol=0)
    miss, _ = frt.selftest_path_host(hs, p, exp["tested"], env_image=image)
    np.testing.assert_allclose(miss, exp["value"], rtol=1e-6, atol=0)


def test_selftest_srgb_and_validation(expectation):
    _, exp = expectation
    image = ES.random_env(32, 16, srgb=True)
    e8 = ES.direction_expectation(image, NX, NY, SPP)
    hs = frt.HostScene.from_spec(ES.direction_spec(), NX / NY)
    p = frt.RenderParams.make(NX, NY, SPP, seed=e8["seed"], integrator=frt.FRT_INTEGRATOR_NORMALS)
    out, _ = frt.selftest_path_host(hs, p, e8["tested"], env_image=image)
    np.testing.assert_allclose(out, e8["value"], rtol=1e-6, atol=0)
    for bad in (-0.5, np.nan, np.inf):
        img = ES.random_env(4, 2)
        img[1, 2, 1] = bad
        with pytest.raises(frt.FrtError, match="invalid"):
            frt.selftest_path_host(hs, p, e8["tested"][:1], env_image=img)
    # without an image the self-test is the constant environment, as before
    hs.set_env((0.25, 0.5, 0.75))
    out, _ = frt.selftest_path_host(hs, p, e8["tested"][:4])
    assert np.array_equal(out, np.tile(np.float32([0.25, 0.5, 0.75]), (4, 1)))
