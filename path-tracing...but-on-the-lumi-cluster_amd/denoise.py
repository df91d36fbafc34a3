"""The edge-avoiding a-trous denoiser's parameters and its CPU restatement.

``DenoiseParams`` mirrors ``ptg_denoise_params`` (include/ptg.h).
``atrous_reference`` is the definition of ``ptg_denoise`` ("Feature
buffers and the denoiser") restated with NumPy: every operation is one float32
rounding, in the order the definition gives, and the weight's ``exp`` is the C
library's double ``exp`` called once per tap (``math.exp``; NumPy's vectorised
``exp`` is a different algorithm).  On a glibc host it gives the bits the GPU
kernels give; it is the documented CPU route and the tests' checker.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import native as N

KERNEL = (0.0625, 0.25, 0.375, 0.25, 0.0625)     # the B3 spline {1/16, 1/4, 3/8, 1/4, 1/16}
MAX_ITERATIONS = 8


class DenoiseParams(C.Structure):
    """ptg_denoise_params.  ``DenoiseParams.default()`` asks the library."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("albedo_floor", C.c_float)]

    @classmethod
    def default(cls, **overrides):
        p = cls()
        N.lib().ptg_denoise_params_default(C.byref(p))
        for k, v in overrides.items():
            if k not in dict(cls._fields_):
                raise TypeError("ptg_denoise_params has no field %r" % k)
            setattr(p, k, v)
        return p

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def validate(self):
        if self.iterations > MAX_ITERATIONS:
            raise ValueError("iterations > %d" % MAX_ITERATIONS)
        for k in ("sigma_color", "sigma_albedo", "sigma_normal", "sigma_depth", "albedo_floor"):
            v = getattr(self, k)
            if not (v > 0.0 and math.isfinite(v)):
                raise ValueError("%s must be positive and finite, got %r" % (k, v))


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _exp_neg(e, valid):
    """(float)exp(-(double)e) per valid element through the C library's exp."""
    out = np.zeros(e.shape, np.float64)
    flat_e, flat_v, flat_o = e.reshape(-1), valid.reshape(-1), out.reshape(-1)
    for i in np.nonzero(flat_v)[0]:
        flat_o[i] = math.exp(-float(flat_e[i]))
    return out.astype(np.float32)


def atrous_reference(radiance, albedo, normal_depth, params: DenoiseParams = None):
    """ptg_denoise on the CPU: [h, w, 4] float32 arrays in, the denoised
    [h, w, 4] float32 radiance (w component 0) out."""
    P = params if params is not None else DenoiseParams.default()
    P.validate()
    f32 = np.float32
    rad = np.ascontiguousarray(radiance, dtype=f32)
    alb = np.ascontiguousarray(albedo, dtype=f32)
    nd = np.ascontiguousarray(normal_depth, dtype=f32)
    h, w = rad.shape[:2]
    assert rad.shape == alb.shape == nd.shape == (h, w, 4)
    if P.iterations == 0:
        return rad.copy()
    with np.errstate(all="ignore"):
        m = np.maximum(alb[..., :3], f32(P.albedo_floor))
        I = rad[..., :3] / m                                       # demodulate
        va = f32(P.sigma_albedo) * f32(P.sigma_albedo)
        vn = f32(P.sigma_normal) * f32(P.sigma_normal)
        vz = f32(P.sigma_depth) * f32(P.sigma_depth)
        Z = nd[..., 3]
        for k in range(P.iterations):
            s = 1 << k
            sc = f32(P.sigma_color) * f32(2.0 ** -k)
            vc = sc * sc
            sw = np.zeros((h, w), f32)
            acc = np.zeros((h, w, 3), f32)
            for dy in range(-2, 3):
                y0, y1 = max(0, -s * dy), min(h, h - s * dy)       # rows p whose tap row is inside
                if y0 >= y1:
                    continue
                for dx in range(-2, 3):
                    x0, x1 = max(0, -s * dx), min(w, w - s * dx)
                    if x0 >= x1:
                        continue
                    hw = f32(KERNEL[dy + 2]) * f32(KERNEL[dx + 2])
                    ps = (slice(y0, y1), slice(x0, x1))
                    qs = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
                    Ip, Iq = I[ps], I[qs]
                    valid = np.isfinite(Iq).all(-1)
                    dc = np.where(np.isfinite(Ip).all(-1), _sq3(Ip - Iq), f32(0))
                    d = alb[ps] - alb[qs]
                    da = _sq3(d) + d[..., 3] * d[..., 3]
                    dn = _sq3(nd[ps][..., :3] - nd[qs][..., :3])
                    dz = Z[ps] - Z[qs]
                    dz2 = (dz * dz) / (np.maximum(Z[ps] * Z[ps], Z[qs] * Z[qs]) + f32(1e-12))
                    e = ((dc / vc + da / va) + dn / vn) + dz2 / vz
                    valid &= np.isfinite(e)
                    wgt = hw * _exp_neg(e, valid)
                    sw[ps] = np.where(valid, sw[ps] + wgt, sw[ps])
                    acc[ps] = np.where(valid[..., None], acc[ps] + wgt[..., None] * Iq, acc[ps])
            I = np.where((sw > 0)[..., None], acc / sw[..., None], I)
        out = np.zeros((h, w, 4), f32)
        out[..., :3] = I * m                                       # remodulate
    assert out.dtype == f32
    return out
