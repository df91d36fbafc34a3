"""The feature-buffer / denoiser entries of include/ptg.h and the denoiser's
CPU restatement (ptlumi.denoise.atrous_reference).  No GPU work here; the GPU
kernels are compared with this restatement in tests/test_gpu_denoise.py."""
import ctypes as C
import math
import subprocess

import numpy as np
import pytest

from conftest import N

NEW_SYMBOLS = ("ptg_camera_rays", "ptg_render_features", "ptg_denoise_params_default", "ptg_denoise")


def _params(**kw):
    from ptlumi.denoise import DenoiseParams
    return DenoiseParams.default(**kw)


def test_new_symbols_are_exported_and_bound(native_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in N.exported_symbols(), "%s is not declared in ptg.h" % name
        assert getattr(native_lib, name).argtypes is not None
    assert native_lib.ptg_abi_version() == 1


def test_new_entries_reject_null_context(native_lib):
    cfg = N.RenderConfig.make()
    p = _params()
    xy = np.zeros((1, 2), np.uint32)
    js = np.zeros(1, np.int32)
    rays = np.zeros((1, 8), np.float32)
    sub = np.zeros(1, np.uint32)
    assert native_lib.ptg_camera_rays(None, C.byref(cfg), 1, xy.ctypes.data, js.ctypes.data, rays.ctypes.data,
                                      sub.ctypes.data) == -1                          # PTG_E_INVALID
    assert native_lib.ptg_render_features(None, C.byref(cfg), 0, 0, 1, 1, 0, 1, None, None) == -1
    assert native_lib.ptg_denoise(None, 1, 1, C.byref(p), None, None, None, None, None) == -1
    assert native_lib.ptg_last_error()


def test_default_params_are_valid(native_lib):
    from ptlumi.denoise import DenoiseParams
    p = DenoiseParams(99, -1.0, -1.0, -1.0, -1.0, -1.0)
    native_lib.ptg_denoise_params_default(C.byref(p))
    assert 1 <= p.iterations <= 8
    for k in ("sigma_color", "sigma_albedo", "sigma_normal", "sigma_depth", "albedo_floor"):
        v = getattr(p, k)
        assert v > 0 and math.isfinite(v), (k, v)
    p.validate()
    native_lib.ptg_denoise_params_default(None)      # a NULL pointer is ignored
    assert DenoiseParams.default().as_dict() == p.as_dict()


def test_params_validation():
    with pytest.raises(ValueError):
        _params(iterations=9).validate()
    for k in ("sigma_color", "sigma_albedo", "sigma_normal", "sigma_depth"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                _params(**{k: bad}).validate()


def _random_inputs(rng, h, w):
    rad = rng.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    rad[..., 3] = 0
    alb = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    nd = rng.normal(size=(h, w, 4)).astype(np.float32)
    nd[..., 3] = rng.uniform(1.0, 20.0, (h, w)).astype(np.float32)
    return rad, alb, nd


def test_zero_iterations_returns_the_input_bits():
    from ptlumi.denoise import atrous_reference
    rad, alb, nd = _random_inputs(np.random.default_rng(1), 6, 9)
    rad[2, 3, 0] = np.nan
    rad[..., 3] = 7.0
    out = atrous_reference(rad, alb, nd, _params(iterations=0))
    assert out.dtype == np.float32 and out is not rad
    assert np.array_equal(out.view(np.uint32), rad.view(np.uint32))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_pixel_is_repaired(bad):
    from ptlumi.denoise import atrous_reference
    rad, alb, nd = _random_inputs(np.random.default_rng(2), 12, 16)
    # smooth guides, so the bad pixel has neighbours with non-zero weight
    alb[...] = (0.5, 0.4, 0.3, 1.0)
    nd[...] = (0.0, 0.0, 1.0, 4.0)
    rad[5, 7, 1] = bad
    out = atrous_reference(rad, alb, nd, _params(iterations=2))
    assert np.isfinite(out).all()
    assert (out[..., 3] == 0).all()
    # with a constant albedo every output is a weighted mean of finite inputs
    good = rad[..., :3][np.isfinite(rad[..., :3]).all(-1)]
    assert (out[5, 7, :3] >= good.min(0) - 1e-5).all() and (out[5, 7, :3] <= good.max(0) + 1e-5).all()


def test_piecewise_constant_image_is_denoised_without_mixing_the_regions():
    """48x32, two regions that differ in albedo, normal and depth; Gaussian
    noise on the illumination.  The error against the clean image falls, in
    each region the pixels move towards the region's own value, and no
    region's mean ends nearer the other region's value."""
    from ptlumi.denoise import atrous_reference
    h, w = 32, 48
    rng = np.random.default_rng(1234)
    left = np.zeros((h, w), bool)
    left[:, :20] = True
    alb = np.where(left[..., None], np.float32([0.8, 0.3, 0.2, 1.0]), np.float32([0.2, 0.5, 0.9, 1.0])).astype(np.float32)
    nd = np.where(left[..., None], np.float32([0.0, 0.0, 1.0, 5.0]), np.float32([1.0, 0.0, 0.0, 9.0])).astype(np.float32)
    light = np.where(left, np.float32(1.0), np.float32(0.5))
    clean = np.zeros((h, w, 4), np.float32)
    clean[..., :3] = alb[..., :3] * light[..., None]
    noisy = clean.copy()
    noisy[..., :3] = alb[..., :3] * (light[..., None] + rng.normal(0.0, 0.1, (h, w, 3))).astype(np.float32)
    out = atrous_reference(noisy, alb, nd, _params())
    assert out.dtype == np.float32 and out.shape == (h, w, 4)

    def mse(a, b):
        return float(((a[..., :3].astype(np.float64) - b[..., :3]) ** 2).mean())

    assert mse(out, clean) < mse(noisy, clean)
    for own, other in ((left, ~left), (~left, left)):
        own_value = clean[own][0, :3].astype(np.float64)
        other_value = clean[other][0, :3].astype(np.float64)
        before = np.abs(noisy[own][:, :3] - own_value).mean()
        after = np.abs(out[own][:, :3] - own_value).mean()
        assert after < before, (after, before)
        mean = out[own][:, :3].astype(np.float64).mean(0)
        assert np.linalg.norm(mean - own_value) < np.linalg.norm(mean - other_value)
        # and it did not drift towards the other region: no nearer to it than the noisy input's mean was
        mean_in = noisy[own][:, :3].astype(np.float64).mean(0)
        gap = np.linalg.norm(own_value - other_value)
        assert np.linalg.norm(mean - other_value) > np.linalg.norm(mean_in - other_value) - 0.05 * gap
