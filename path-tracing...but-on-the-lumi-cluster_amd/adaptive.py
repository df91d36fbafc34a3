"""Adaptive sampling: the parameters of ``ptg_render_adaptive`` and its CPU
restatement.

``AdaptiveParams`` mirrors ``ptg_adaptive_params`` (include/ptg.h).
``adaptive_reference`` is the definition of ``ptg_render_adaptive`` (DESIGN.md
4.14) restated with NumPy over the per-sample radiance: every operation is one
float32 rounding in the order the definition gives, with
``denoise.moments_reference``'s idioms.  It is the documented CPU route and
the tests' checker.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .denoise import _lum, _Params

MAX_PASSES = 16
MAX_DILATE = 2


class AdaptiveParams(_Params, C.Structure):
    """ptg_adaptive_params.  ``AdaptiveParams.default()`` asks the library."""
    _fields_ = [("passes", C.c_uint32), ("min_passes", C.c_uint32), ("dilate", C.c_uint32), ("threshold", C.c_float),
                ("luminance_floor", C.c_float)]
    _default_fn = "ptg_adaptive_params_default"
    _positive = ("threshold", "luminance_floor")

    def validate(self):
        super().validate()
        if not 1 <= self.min_passes <= self.passes <= MAX_PASSES:
            raise ValueError("1 <= min_passes <= passes <= %d, got %d and %d" % (MAX_PASSES, self.min_passes, self.passes))
        if self.dilate > MAX_DILATE:
            raise ValueError("dilate > %d" % MAX_DILATE)


def sample_index(jj, k, passes, m):
    """Sample j of the frame that local index jj of pass k is: pass k owns the
    subframes k, k + passes, k + 2 passes, ... (m samples each)."""
    return ((jj // m) * passes + k) * m + jj % m


def noisy_pixels(s1, s2, n, threshold, luminance_floor):
    """The stopping rule's per-pixel test on the running luminance sums:
    n < 2 or not (variance of the mean <= (threshold * (mean + floor))^2)."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        nf = n.astype(f32)
        m1 = s1 / nf
        m2 = s2 / nf
        d = m2 - m1 * m1
        var = np.where(d > 0, d, f32(0))
        vm = var / (nf - f32(1))
        tol = f32(threshold) * (m1 + f32(luminance_floor))
        return (n < 2) | ~(vm <= tol * tol)


def dilate_window(mask, r):
    """OR over the (2 r + 1)^2 window around each pixel, clipped to the array."""
    h, w = mask.shape
    out = np.zeros_like(mask)
    for dy in range(-r, r + 1):
        y0, y1 = max(0, -dy), min(h, h - dy)
        if y0 >= y1:
            continue
        for dx in range(-r, r + 1):
            x0, x1 = max(0, -dx), min(w, w - dx)
            if x0 >= x1:
                continue
            out[y0:y1, x0:x1] |= mask[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def adaptive_reference(per_sample, m, params: AdaptiveParams = None):
    """ptg_render_adaptive on the CPU.  `per_sample` is the radiance of every
    (pixel, sample) of the rectangle, float32 [h, w, N, >= 3] with N the
    frame's budget in sample-index order; `m` is samples_per_motion_blur_step.
    Returns (accum [h, w, 4], moments [h, w, 4], samples uint32 [h, w],
    active_per_pass: the active pixel count of every pass run)."""
    P = params if params is not None else AdaptiveParams.default()
    P.validate()
    f32 = np.float32
    c = np.ascontiguousarray(per_sample, dtype=f32)
    assert c.ndim == 4 and c.shape[3] >= 3
    h, w, N = c.shape[:3]
    passes, m = int(P.passes), int(m)
    if m < 1 or N < 1 or N % (passes * m):
        raise ValueError("the budget %d is not a multiple of passes * m = %d * %d" % (N, passes, m))
    span = N // passes
    a = np.zeros((h, w, 3), f32)
    s1 = np.zeros((h, w), f32)
    s2 = np.zeros((h, w), f32)
    n = np.zeros((h, w), np.int64)
    taken = np.zeros((h, w), np.int64)
    active = np.ones((h, w), bool)
    active_per_pass = []
    with np.errstate(all="ignore"):
        for k in range(passes):
            if not active.any():
                break
            active_per_pass.append(int(active.sum()))
            for jj in range(span):
                s = c[:, :, sample_index(jj, k, passes, m), :3]
                a = np.where(active[..., None], a + s, a)
                fin = active & np.isfinite(s).all(-1)
                L = _lum(s)
                s1 = np.where(fin, s1 + L, s1)
                s2 = np.where(fin, s2 + L * L, s2)
                n += fin
            taken += active
            if P.min_passes <= k + 1 < passes:
                active = dilate_window(noisy_pixels(s1, s2, n, P.threshold, P.luminance_floor), int(P.dilate))
        ns = taken * span
        accum = np.zeros((h, w, 4), f32)
        accum[..., :3] = a / ns.astype(f32)[..., None]
        nf = n.astype(f32)
        m1 = s1 / nf
        m2 = s2 / nf
        d = m2 - m1 * m1
        var = np.where(d > 0, d, f32(0))
        vm = np.where(n >= 2, var / (nf - f32(1)), f32(0))
        moments = np.zeros((h, w, 4), f32)
        some = n > 0
        moments[some] = np.stack([m1, m2, vm, nf], -1)[some]
    assert accum.dtype == f32 and moments.dtype == f32
    return accum, moments, ns.astype(np.uint32), active_per_pass
