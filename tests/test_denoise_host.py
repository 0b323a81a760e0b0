"""The filter of FRT_INTEGRATOR_DENOISE on the CPU: tests/denoise_probe.hip (its own main over
csrc/frt_denoise.hpp, the functions the kernels compile) against the fp64 numpy restatement
denoise_specs.denoise_ref, its exact properties, and whether it helps -- host-replay path
films of Cornell against the golden image, which is also the harness the header's constants
were tuned with (tools/denoise_tune.py sweeps them over the same films)."""
import numpy as np
import pytest

import denoise_specs as DS
import first_raytracer_amd as frt
import golden_images as G
import scene_specs as SS


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = DS.build_probe(tmp_path_factory.mktemp("probe"))
    work = tmp_path_factory.mktemp("films")
    return lambda c, N, A, D: DS.run_probe(exe, work, c, N, A, D)


@pytest.fixture(scope="module")
def cornell_features(cornell_obj):
    """Host-replay features of Cornell at the sizes the probe tests use, rendered once."""
    out = {}
    for nx, ny in ((48, 36), (1, 1), (5, 3), (41, 23)):
        out[(nx, ny)] = DS.host_features(frt.HostScene("cornell_box_obj", cornell_obj, nx / ny), nx, ny, 4, 21)
    return out


@pytest.fixture(scope="module")
def textured_features():
    nx, ny = 48, 36
    return DS.host_features(frt.HostScene.from_spec(SS.cornell_textured(), nx / ny), nx, ny, 4, 21)


def test_probe_matches_restatement(probe, cornell_features):
    """The inputs PROBE_MAX_REL_DIFF was measured on; the allowance is 4 x that, below 1e-4."""
    worst = 0.0
    for (nx, ny), (N, A, D) in cornell_features.items():
        c = DS.random_colour(nx, ny)
        d = DS.rel_diff(probe(c, N, A, D), DS.denoise_ref(c, N, A, D))
        print(f"probe vs restatement, Cornell {nx} x {ny}: {d:.3e}")
        worst = max(worst, d)
    for nx, ny in ((1, 1), (5, 3), (41, 23)):             # partly covered pixels, misses, an albedo below eps_a
        c, N, A, D = DS.synthetic_inputs(nx, ny)
        d = DS.rel_diff(probe(c, N, A, D), DS.denoise_ref(c, N, A, D))
        print(f"probe vs restatement, synthetic {nx} x {ny}: {d:.3e}")
        worst = max(worst, d)
    print(f"largest: {worst:.3e} (recorded {DS.PROBE_MAX_REL_DIFF:.1e}, allowed {DS.PROBE_TOLERANCE:.1e})")
    assert DS.PROBE_TOLERANCE < 1e-4
    assert worst <= DS.PROBE_TOLERANCE


def test_filter_changes_a_noisy_film(probe, cornell_features):
    """Not the identity: a random film over Cornell's smooth walls comes out smoother."""
    N, A, D = cornell_features[(48, 36)]
    c = DS.random_colour(48, 36)
    out = probe(c, N, A, D)
    assert np.abs(np.diff(out, axis=1)).mean() < 0.5 * np.abs(np.diff(c, axis=1)).mean()


def test_constant_colour_over_constant_albedo_returns_itself(probe, cornell_features):
    """The output is a convex combination of colour / albedo times the pixel's albedo -- one divide
    and one multiply around weights that sum to 1.  Where the albedo film is constant that is the
    colour itself, within 1e-5 relative, whatever the normals and depths are.  Over Cornell's own
    albedo (it differs from wall to wall, so colour / albedo is not constant) the demodulated
    output stays between the smallest and the largest demodulated input."""
    N, A, D = cornell_features[(48, 36)]
    K = DS.constants()
    colour = np.full((36, 48, 3), (0.7, 0.25, 1.5), np.float32)
    flat = np.full_like(A, 0.5)
    out = probe(colour, N, flat, D)
    assert np.abs(out / colour - 1.0).max() <= 1e-5
    out = probe(colour, N, A, D)
    floor = np.maximum(A.astype(np.float64), K["eps_a"])
    r0, r = colour / floor, out / floor
    for ch in range(3):
        assert r[..., ch].min() >= r0[..., ch].min() * (1 - 1e-5) and r[..., ch].max() <= r0[..., ch].max() * (1 + 1e-5)


@pytest.mark.parametrize("scene", ["plain", "checker"])
def test_albedo_as_colour_returns_the_albedo(probe, cornell_features, textured_features, scene):
    """Demodulation keeps texture detail: colour := albedo is 1 everywhere after the divide."""
    N, A, D = cornell_features[(48, 36)] if scene == "plain" else textured_features
    assert A.min() > DS.constants()["eps_a"]
    out = probe(A, N, A, D)
    assert np.abs(out / A - 1.0).max() <= 1e-5
    if scene == "checker":                                # the detail is there to keep
        assert np.abs(np.diff(A, axis=1)).max() > 0.3


def test_zero_in_zero_out_and_range(probe, cornell_features):
    N, A, D = cornell_features[(41, 23)]
    assert not probe(np.zeros((23, 41, 3), np.float32), N, A, D).any()
    c = DS.random_colour(41, 23, seed=5)
    c[3, 4] = 0.0
    c[10, 7] = (1e4, 0.0, 1e-6)                           # a firefly
    out = probe(c, N, A, D)
    assert np.isfinite(out).all() and (out >= 0).all()
    for inputs in (DS.synthetic_inputs(41, 23), DS.synthetic_inputs(5, 3), DS.synthetic_inputs(1, 1)):
        out = probe(*inputs)
        assert np.isfinite(out).all() and (out >= 0).all()


@pytest.fixture(scope="module")
def cornell64_noisy(cornell_obj):
    return DS.cornell64_noisy(cornell_obj)


def test_filter_helps(cornell64_noisy):
    """Per-pixel RMSE against golden/cornell_64x64_16384spp.pfm is lower after the filter than
    before, for every seed.  Printed, not asserted: the spp at which the unfiltered render
    would reach the filtered RMSE -- 4 (before / after)^2, its noise falling as 1 / sqrt(spp)
    (the golden image's own noise, 64 times less, is neglected)."""
    gold = G.cornell64()
    for seed, film, (N, A, D) in cornell64_noisy:
        before = DS.rmse(film, gold)
        after = DS.rmse(DS.denoise_ref(film, N, A, D), gold)
        print(f"seed {seed}: rmse {before:.4f} -> {after:.4f}, ratio {after / before:.3f}, "
              f"equal-error spp about {4 * (before / after) ** 2:.0f}")
        assert after < before
