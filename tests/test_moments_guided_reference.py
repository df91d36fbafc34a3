"""ptg_render_moments / ptg_denoise_guided in include/ptg.h and their CPU
restatements (ptlumi.denoise.moments_reference, atrous_guided_reference).  No
GPU work here; the kernels are compared with these restatements in
tests/test_gpu_moments.py and tests/test_gpu_denoise_guided.py."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, N

NEW_SYMBOLS = ("ptg_render_moments", "ptg_denoise_guided_params_default", "ptg_denoise_guided")
FLOAT_FIELDS = ("sigma_luminance", "sigma_albedo", "sigma_normal", "sigma_depth", "albedo_floor", "variance_floor")
# the values the definition was prototyped with, independent of the library's defaults
START = dict(iterations=4, sigma_luminance=4.0, sigma_albedo=0.05, sigma_normal=1.2, sigma_depth=1.0,
             albedo_floor=0.01, variance_floor=1e-4)


def _params(**kw):
    from ptlumi.denoise import DenoiseGuidedParams
    return DenoiseGuidedParams.default(**kw)


def test_new_symbols_are_exported_and_bound(native_lib):
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for name in NEW_SYMBOLS:
        assert name in exported, name
        assert name in N.exported_symbols(), "%s is not declared in ptg.h" % name
        assert getattr(native_lib, name).argtypes is not None
    assert "ptg_denoise_guided_params" in open(os.path.join(ROOT, "include", "ptg.h")).read()
    assert native_lib.ptg_abi_version() == 1


def test_new_entries_reject_null_context(native_lib):
    cfg = N.RenderConfig.make()
    p = _params()
    assert native_lib.ptg_render_moments(None, C.byref(cfg), 0, 0, 1, 1, 0, 1, None, None, None) == -1   # PTG_E_INVALID
    assert native_lib.ptg_denoise_guided(None, 1, 1, C.byref(p), None, None, None, None, None, None) == -1
    assert native_lib.ptg_last_error()


def test_default_params_are_valid(native_lib):
    from ptlumi.denoise import DenoiseGuidedParams
    p = DenoiseGuidedParams(99, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0)
    native_lib.ptg_denoise_guided_params_default(C.byref(p))
    assert 1 <= p.iterations <= 8
    for k in FLOAT_FIELDS:
        v = getattr(p, k)
        assert v > 0 and math.isfinite(v), (k, v)
    p.validate()
    native_lib.ptg_denoise_guided_params_default(None)      # a NULL pointer is ignored
    assert DenoiseGuidedParams.default().as_dict() == p.as_dict()
    assert list(p.as_dict()) == ["iterations"] + list(FLOAT_FIELDS)
    with pytest.raises(TypeError):
        DenoiseGuidedParams.default(sigma_color=1.0)


def test_params_validation():
    with pytest.raises(ValueError):
        _params(iterations=9).validate()
    for k in FLOAT_FIELDS:
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(ValueError):
                _params(**{k: bad}).validate()


# ---- moments_reference --------------------------------------------------------

def _lum(c):
    f = np.float32
    return f(f(f(f(0.2126) * f(c[0])) + f(f(0.7152) * f(c[1]))) + f(f(0.0722) * f(c[2])))


def _scalar_moments(samples):
    """The definition with float32 scalars, one pixel."""
    f = np.float32
    s1, s2, n = f(0), f(0), 0
    for c in samples:
        if not np.isfinite(c[:3]).all():
            continue
        L = _lum(c)
        s1 = f(s1 + L)
        s2 = f(s2 + f(L * L))
        n += 1
    if n == 0:
        return np.zeros(4, f)
    nf = f(n)
    m1, m2 = f(s1 / nf), f(s2 / nf)
    d = f(m2 - f(m1 * m1))
    var = d if d > 0 else f(0)
    vm = f(var / f(nf - f(1))) if n >= 2 else f(0)
    return np.array([m1, m2, vm, nf], f)


def test_moments_of_one_sample():
    from ptlumi.denoise import moments_reference
    c = np.float32([[[0.3, 0.9, 0.1]], [[2.0, 0.0, 5.0]]])
    out = moments_reference(c)
    assert out.dtype == np.float32 and out.shape == (2, 4)
    for p in range(2):
        L = _lum(c[p, 0])
        assert out[p, 0] == L and out[p, 1] == np.float32(L * L)
        assert out[p, 2] == 0 and out[p, 3] == 1


def test_moments_of_no_finite_sample_are_zero():
    from ptlumi.denoise import moments_reference
    c = np.float32([[[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf]]])
    out = moments_reference(c)
    assert np.array_equal(out.view(np.uint32), np.zeros((1, 4), np.uint32))


def test_one_nan_sample_among_eight_is_left_out():
    from ptlumi.denoise import moments_reference
    rng = np.random.default_rng(5)
    c = rng.uniform(0.0, 3.0, (3, 8, 3)).astype(np.float32)
    c[0, 2, 1] = np.nan
    c[1, 7, 0] = np.nan
    c[2, 0, 2] = np.nan
    out = moments_reference(c)
    for p in range(3):
        want = _scalar_moments(c[p])
        assert want[3] == 7 and want[2] > 0
        assert np.array_equal(out[p].view(np.uint32), want.view(np.uint32)), (p, out[p], want)


def test_constant_samples_have_zero_variance():
    """vm is exactly 0 wherever the sums are exact: black samples, and two
    equal samples of any value (s1 = 2L and s2 = 2 fl(L L) are exact, so
    m1 = L, m2 = fl(L L) and d = m2 - fl(m1 m1) = 0).  Longer runs of one value
    round: 3L already needs two more bits than L has.  There d is bounded by
    the roundings of the two sums, (n - 1) each, the two divisions and the two
    products: below 4 n 2^-24 L^2 to first order."""
    from ptlumi.denoise import moments_reference
    out = moments_reference(np.zeros((2, 16, 3), np.float32))
    assert np.array_equal(out, np.float32([[0, 0, 0, 16]] * 2))
    for value in ((0.5, 0.25, 2.0), (0.3, 0.9, 0.1), (1.0, 1.0, 1.0), (123.0, 0.01, 7.0)):
        L = _lum(value)
        out = moments_reference(np.broadcast_to(np.float32(value), (2, 2, 3)))
        assert (out[:, 0] == L).all() and (out[:, 1] == np.float32(L * L)).all()
        assert (out[:, 2] == 0).all() and (out[:, 3] == 2).all()
        n = 16
        out = moments_reference(np.broadcast_to(np.float32(value), (2, n, 3)))
        assert (out[:, 3] == n).all()
        assert (out[:, 2] >= 0).all() and (out[:, 2] <= 4 * n * 2.0 ** -24 * float(L) ** 2 / (n - 1)).all(), out[:, 2]


# ---- atrous_guided_reference --------------------------------------------------

def _random_inputs(rng, h, w):
    rad = rng.uniform(0.0, 2.0, (h, w, 4)).astype(np.float32)
    rad[..., 3] = 0
    alb = rng.uniform(0.0, 1.0, (h, w, 4)).astype(np.float32)
    nd = rng.normal(size=(h, w, 4)).astype(np.float32)
    nd[..., 3] = rng.uniform(1.0, 20.0, (h, w)).astype(np.float32)
    mom = np.zeros((h, w, 4), np.float32)
    mom[..., 2] = rng.uniform(0.0, 0.05, (h, w)).astype(np.float32)
    return rad, alb, nd, mom


def test_zero_iterations_returns_the_input_bits():
    from ptlumi.denoise import atrous_guided_reference
    rad, alb, nd, mom = _random_inputs(np.random.default_rng(1), 6, 9)
    rad[2, 3, 0] = np.nan
    rad[..., 3] = 7.0
    out = atrous_guided_reference(rad, alb, nd, mom, _params(iterations=0))
    assert out.dtype == np.float32 and out is not rad
    assert np.array_equal(out.view(np.uint32), rad.view(np.uint32))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite_pixel_is_repaired(bad):
    from ptlumi.denoise import atrous_guided_reference
    rad, alb, nd, mom = _random_inputs(np.random.default_rng(2), 12, 16)
    # smooth guides, so the bad pixel has neighbours with non-zero weight
    alb[...] = (0.5, 0.4, 0.3, 1.0)
    nd[...] = (0.0, 0.0, 1.0, 4.0)
    rad[5, 7, 1] = bad
    mom[5, 7, 2] = bad                        # and its variance is as bad
    out = atrous_guided_reference(rad, alb, nd, mom, _params(iterations=2))
    assert np.isfinite(out).all()
    assert (out[..., 3] == 0).all()
    # with a constant albedo every output is a weighted mean of finite inputs
    good = rad[..., :3][np.isfinite(rad[..., :3]).all(-1)]
    assert (out[5, 7, :3] >= good.min(0) - 1e-5).all() and (out[5, 7, :3] <= good.max(0) + 1e-5).all()


def test_guided_filter_keeps_an_edge_the_guides_do_not_mark():
    """The scene the filter exists for: 48x32, 16 samples per pixel, constant
    albedo, normal and depth, an illumination edge 1.0 | 0.3 at column 24,
    per-sample noise sigma 0.4 on rows 0-15 and 0.004 on rows 16-31.  The
    guided filter (the prototype's parameters, not the library's defaults)
    removes the noise of the noisy half and leaves the clean half's edge; the
    fixed-sigma filter with the library's defaults smears that edge."""
    from ptlumi.denoise import DenoiseParams, atrous_guided_reference, atrous_reference, moments_reference
    h, w, n = 32, 48, 16
    rng = np.random.default_rng(1234)
    alb = np.broadcast_to(np.float32([0.6, 0.5, 0.4, 1.0]), (h, w, 4)).copy()
    nd = np.broadcast_to(np.float32([0.0, 0.0, 1.0, 5.0]), (h, w, 4)).copy()
    light = np.where(np.arange(w) < 24, np.float32(1.0), np.float32(0.3))[None, :].repeat(h, 0)
    sigma = np.where(np.arange(h) < 16, 0.4, 0.004)[:, None, None, None]
    clean = np.zeros((h, w, 4), np.float32)
    clean[..., :3] = alb[..., :3] * light[..., None]
    noise = rng.normal(0.0, 1.0, (h, w, n, 1)) * sigma
    per_sample = (alb[:, :, None, :3] * (light[:, :, None, None] + noise)).astype(np.float32)   # [h, w, n, 3]
    raw = np.zeros((h, w, 4), np.float32)
    raw[..., :3] = per_sample.mean(2, dtype=np.float32)
    mom = moments_reference(per_sample.reshape(h * w, n, 3)).reshape(h, w, 4)
    assert (mom[..., 3] == n).all()

    guided = atrous_guided_reference(raw, alb, nd, mom, _params(**START))
    fixed = atrous_reference(raw, alb, nd, DenoiseParams.default())
    assert guided.dtype == np.float32 and guided.shape == (h, w, 4) and (guided[..., 3] == 0).all()

    def mse(a, region):
        return float(((a[region][..., :3].astype(np.float64) - clean[region][..., :3]) ** 2).mean())

    noisy = (slice(0, 14), slice(None))
    edge = (slice(20, 32), slice(22, 26))
    print("noisy rows: raw %.3g fixed %.3g guided %.3g; clean edge: raw %.3g fixed %.3g guided %.3g" % (
        mse(raw, noisy), mse(fixed, noisy), mse(guided, noisy), mse(raw, edge), mse(fixed, edge), mse(guided, edge)))
    assert mse(guided, noisy) < 0.1 * mse(raw, noisy)
    assert mse(guided, edge) <= mse(raw, edge)
    assert mse(fixed, edge) > 100 * mse(raw, edge), "the fixed-sigma filter no longer smears this edge"
