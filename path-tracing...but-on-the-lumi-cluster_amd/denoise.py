"""The edge-avoiding a-trous denoiser's parameters and its CPU restatement.

``DenoiseParams`` mirrors ``ptg_denoise_params`` (include/ptg.h).
``atrous_reference`` is the definition of ``ptg_denoise`` ("Feature
buffers and the denoiser") restated with NumPy: every operation is one float32
rounding, in the order the definition gives, and the weight's ``exp`` is the C
library's double ``exp`` called once per tap (``math.exp``; NumPy's vectorised
``exp`` is a different algorithm).  On a glibc host it gives the bits the GPU
kernels give; it is the documented CPU route and the tests' checker.

Further down: the sample moments and the variance-guided filter
(``moments_reference``, ``atrous_guided_reference``), and the temporal
accumulation (``TemporalParams``, ``temporal_reference``: the restatement of
``ptg_temporal_accumulate``), and its form with several
cameras and a history clamp (``TemporalClampParams``,
``temporal_clamped_reference``: ``ptg_temporal_accumulate_clamped``, 4.17).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import native as N

KERNEL = (0.0625, 0.25, 0.375, 0.25, 0.0625)     # the B3 spline {1/16, 1/4, 3/8, 1/4, 1/16}
MAX_ITERATIONS = 8


class _Params:
    """What the parameter structures share; each names the library's
    default function and its fields that must be positive and finite."""

    @classmethod
    def default(cls, **overrides):
        p = cls()
        getattr(N.lib(), cls._default_fn)(C.byref(p))
        for k, v in overrides.items():
            if k not in dict(cls._fields_):
                raise TypeError("%s has no field %r" % (cls._default_fn[:-len("_default")], k))
            setattr(p, k, v)
        return p

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}

    def validate(self):
        if getattr(self, "iterations", 0) > MAX_ITERATIONS:
            raise ValueError("iterations > %d" % MAX_ITERATIONS)
        for k in self._positive:
            v = getattr(self, k)
            if not (v > 0.0 and math.isfinite(v)):
                raise ValueError("%s must be positive and finite, got %r" % (k, v))


class DenoiseParams(_Params, C.Structure):
    """ptg_denoise_params.  ``DenoiseParams.default()`` asks the library."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_color", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("albedo_floor", C.c_float)]
    _default_fn = "ptg_denoise_params_default"
    _positive = ("sigma_color", "sigma_albedo", "sigma_normal", "sigma_depth", "albedo_floor")


def _sq3(d):
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _exp_neg(e, valid):
    """(float)exp(-(double)e) per valid element through the C library's exp."""
    out = np.zeros(e.shape, np.float64)
    flat_e, flat_v, flat_o = e.reshape(-1), valid.reshape(-1), out.reshape(-1)
    for i in np.nonzero(flat_v)[0]:
        flat_o[i] = math.exp(-float(flat_e[i]))
    return out.astype(np.float32)


def _atrous_taps(I, alb, nd, s, P, colour_term, V=None):
    """One iteration's 5 x 5 taps `s` apart over I [h, w, 3], dy outer and dx
    inner: (sw, acc, sv), the sums of the weights, of weight * I and, with the
    variance plane V, of weight^2 * V (else None).  ``colour_term(ps, qs)`` is
    the exponent's first term between the pixels ps and their taps qs, where
    the pixel is finite; the albedo, normal and depth terms, the finiteness
    rules and the weight are the two filters' common definition."""
    f32 = np.float32
    h, w = I.shape[:2]
    va = f32(P.sigma_albedo) * f32(P.sigma_albedo)
    vn = f32(P.sigma_normal) * f32(P.sigma_normal)
    vz = f32(P.sigma_depth) * f32(P.sigma_depth)
    Z = nd[..., 3]
    fin = np.isfinite(I).all(-1)
    sw = np.zeros((h, w), f32)
    acc = np.zeros((h, w, 3), f32)
    sv = np.zeros((h, w), f32) if V is not None else None
    for dy in range(-2, 3):
        y0, y1 = max(0, -s * dy), min(h, h - s * dy)               # rows p whose tap row is inside
        if y0 >= y1:
            continue
        for dx in range(-2, 3):
            x0, x1 = max(0, -s * dx), min(w, w - s * dx)
            if x0 >= x1:
                continue
            hw = f32(KERNEL[dy + 2]) * f32(KERNEL[dx + 2])
            ps = (slice(y0, y1), slice(x0, x1))
            qs = (slice(y0 + s * dy, y1 + s * dy), slice(x0 + s * dx, x1 + s * dx))
            valid = fin[qs].copy()
            ec = np.where(fin[ps], colour_term(ps, qs), f32(0))
            d = alb[ps] - alb[qs]
            da = _sq3(d) + d[..., 3] * d[..., 3]
            dn = _sq3(nd[ps][..., :3] - nd[qs][..., :3])
            dz = Z[ps] - Z[qs]
            dz2 = (dz * dz) / (np.maximum(Z[ps] * Z[ps], Z[qs] * Z[qs]) + f32(1e-12))
            e = ((ec + da / va) + dn / vn) + dz2 / vz
            valid &= np.isfinite(e)
            wgt = hw * _exp_neg(e, valid)
            sw[ps] = np.where(valid, sw[ps] + wgt, sw[ps])
            acc[ps] = np.where(valid[..., None], acc[ps] + wgt[..., None] * I[qs], acc[ps])
            if V is not None:
                sv[ps] = np.where(valid, sv[ps] + (wgt * wgt) * V[qs], sv[ps])
    return sw, acc, sv


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
        for k in range(P.iterations):
            sc = f32(P.sigma_color) * f32(2.0 ** -k)
            vc = sc * sc
            sw, acc, _ = _atrous_taps(I, alb, nd, 1 << k, P, lambda ps, qs: _sq3(I[ps] - I[qs]) / vc)
            I = np.where((sw > 0)[..., None], acc / sw[..., None], I)
        out = np.zeros((h, w, 4), f32)
        out[..., :3] = I * m                                       # remodulate
    assert out.dtype == f32
    return out


# ---- per-pixel sample moments and the variance-guided filter -----------------

PREFILTER = (0.25, 0.5, 0.25)                    # the variance prefilter's {1/4, 1/2, 1/4}


class DenoiseGuidedParams(_Params, C.Structure):
    """ptg_denoise_guided_params.  ``DenoiseGuidedParams.default()`` asks the library."""
    _fields_ = [("iterations", C.c_uint32), ("sigma_luminance", C.c_float), ("sigma_albedo", C.c_float),
                ("sigma_normal", C.c_float), ("sigma_depth", C.c_float), ("albedo_floor", C.c_float),
                ("variance_floor", C.c_float)]
    _default_fn = "ptg_denoise_guided_params_default"
    _positive = ("sigma_luminance", "sigma_albedo", "sigma_normal", "sigma_depth", "albedo_floor", "variance_floor")


def _lum(v):
    """(0.2126f * x + 0.7152f * y) + 0.0722f * z of float32 [..., >= 3]."""
    f32 = np.float32
    return (f32(0.2126) * v[..., 0] + f32(0.7152) * v[..., 1]) + f32(0.0722) * v[..., 2]


def _var_ok(v):
    """A variance the filter may use: >= 0 and finite, else 0."""
    return np.where((v >= 0) & np.isfinite(v), v, np.float32(0))


def moments_reference(per_sample):
    """ptg_render_moments' out_moments on the CPU: the samples' radiance,
    float32 [npix, n, >= 3] in sample order, to [npix, 4] float32
    (m1, m2, variance of the mean, number of finite samples)."""
    f32 = np.float32
    c = np.ascontiguousarray(per_sample, dtype=f32)
    assert c.ndim == 3 and c.shape[2] >= 3
    npix = c.shape[0]
    s1 = np.zeros(npix, f32)
    s2 = np.zeros(npix, f32)
    n = np.zeros(npix, np.int64)
    out = np.zeros((npix, 4), f32)
    with np.errstate(all="ignore"):
        for j in range(c.shape[1]):
            fin = np.isfinite(c[:, j, :3]).all(-1)
            L = _lum(c[:, j])
            s1 = np.where(fin, s1 + L, s1)
            s2 = np.where(fin, s2 + L * L, s2)
            n += fin
        nf = n.astype(f32)
        m1 = s1 / nf
        m2 = s2 / nf
        d = m2 - m1 * m1
        var = np.where(d > 0, d, f32(0))
        vm = np.where(n >= 2, var / (nf - f32(1)), f32(0))
        some = n > 0
        out[some] = np.stack([m1, m2, vm, nf], -1)[some]
    assert out.dtype == f32
    return out


def atrous_guided_reference(radiance, albedo, normal_depth, moments, params: DenoiseGuidedParams = None):
    """ptg_denoise_guided on the CPU: [h, w, 4] float32 arrays in, the denoised
    [h, w, 4] float32 radiance (w component 0) out."""
    P = params if params is not None else DenoiseGuidedParams.default()
    P.validate()
    f32 = np.float32
    rad = np.ascontiguousarray(radiance, dtype=f32)
    alb = np.ascontiguousarray(albedo, dtype=f32)
    nd = np.ascontiguousarray(normal_depth, dtype=f32)
    mom = np.ascontiguousarray(moments, dtype=f32)
    h, w = rad.shape[:2]
    assert rad.shape == alb.shape == nd.shape == mom.shape == (h, w, 4)
    if P.iterations == 0:
        return rad.copy()
    with np.errstate(all="ignore"):
        m = np.maximum(alb[..., :3], f32(P.albedo_floor))
        I = rad[..., :3] / m                                       # demodulate
        ml = _lum(m)
        V = _var_ok(_var_ok(mom[..., 2]) / (ml * ml))
        sl, vf = f32(P.sigma_luminance), f32(P.variance_floor)
        for k in range(P.iterations):
            fin = np.isfinite(I).all(-1)
            gs = np.zeros((h, w), f32)
            gn = np.zeros((h, w), f32)
            for dy in range(-1, 2):                                # the variance prefilter, always at distance 1
                y0, y1 = max(0, -dy), min(h, h - dy)
                if y0 >= y1:
                    continue
                for dx in range(-1, 2):
                    x0, x1 = max(0, -dx), min(w, w - dx)
                    if x0 >= x1:
                        continue
                    gw = f32(PREFILTER[dy + 1]) * f32(PREFILTER[dx + 1])
                    ps = (slice(y0, y1), slice(x0, x1))
                    qs = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                    gs[ps] = np.where(fin[qs], gs[ps] + gw * V[qs], gs[ps])
                    gn[ps] = np.where(fin[qs], gn[ps] + gw, gn[ps])
            g = np.where(gn > 0, gs / gn, f32(0))
            den = sl * np.sqrt(g) + vf
            lum = _lum(I)
            sw, acc, sv = _atrous_taps(I, alb, nd, 1 << k, P, lambda ps, qs: np.abs(lum[ps] - lum[qs]) / den[ps], V)
            some = sw > 0
            I = np.where(some[..., None], acc / sw[..., None], I)
            V = _var_ok(np.where(some, sv / (sw * sw), V))
        out = np.zeros((h, w, 4), f32)
        out[..., :3] = I * m                                       # remodulate
    assert out.dtype == f32
    return out


# ---- temporal accumulation ------------------------------------------------------


class TemporalParams(_Params, C.Structure):
    """ptg_temporal_params.  ``TemporalParams.default()`` asks the library."""
    _fields_ = [("max_history", C.c_float), ("depth_tolerance", C.c_float), ("normal_tolerance", C.c_float),
                ("albedo_tolerance", C.c_float)]
    _default_fn = "ptg_temporal_params_default"
    _positive = ("max_history", "depth_tolerance", "normal_tolerance", "albedo_tolerance")


def _camera_parts(cam):
    """(orientation rows [3][3], position [3], aspect_ratio, inv_focal_length,
    focal_distance) as float32 of a CAMERA_DTYPE record or a ctypes ptg_camera."""
    f32 = np.float32
    if isinstance(cam, C.Structure):
        cam = np.frombuffer(bytes(cam), dtype=N.CAMERA_DTYPE, count=1)[0]
    cam = np.asarray(cam, dtype=N.CAMERA_DTYPE).reshape(())
    ori = np.array(cam["orientation"], f32)[:, :3]
    pos = np.array(cam["position"], f32)[:3]
    return ori, pos, f32(cam["aspect_ratio"]), f32(cam["inv_focal_length"]), f32(cam["focal_distance"])


def _dot3(ax, ay, az, bx, by, bz):
    """The device's dot: (a.x * b.x + a.y * b.y) + a.z * b.z."""
    return (ax * bx + ay * by) + az * bz


def _var_of_mean(m1, m2, n):
    """(max(m2 - m1 * m1, 0) / (n - 1), 0 when n < 2), as moments_reference ends."""
    f32 = np.float32
    d = m2 - m1 * m1
    var = np.where(d > 0, d, f32(0))
    return np.where(n >= 2, var / (n - f32(1)), f32(0)).astype(f32)


def _temporal_images(radiance, moments, albedo, normal_depth, hist):
    """The float32 images of a temporal call, checked: (R, M, A, G), the
    history's (H, HM, HA, HG) or None on a first frame."""
    f32 = np.float32
    cur = tuple(np.ascontiguousarray(a, dtype=f32) for a in (radiance, moments, albedo, normal_depth))
    h, w = cur[0].shape[:2]
    assert all(a.shape == (h, w, 4) for a in cur)
    given = sum(a is not None for a in hist)
    if given not in (0, 5):
        raise ValueError("hist_cam and the four hist_* images are all None or all given")
    if not given:
        return cur, None
    old = tuple(np.ascontiguousarray(a, dtype=f32) for a in hist[1:])
    assert all(a.shape == (h, w, 4) for a in old)
    return cur, old


class _TemporalSums:
    """The seven running sums of the reprojection: sw, sc.xyz, s1, s2, sn."""

    def __init__(self, h, w):
        f32 = np.float32
        self.sw = np.zeros((h, w), f32)
        self.sc = np.zeros((h, w, 3), f32)
        self.s1, self.s2, self.sn = np.zeros((h, w), f32), np.zeros((h, w), f32), np.zeros((h, w), f32)


def _temporal_gather(S, cam, hist_cam, A, G, old, P):
    """Steps 1-4 of DESIGN.md 4.13 for one camera: every valid tap adds into
    the sums S.  A pixel that fails a test through this camera adds nothing."""
    f32 = np.float32
    H, HM, HA, HG = old
    h, w = A.shape[:2]
    ori, pos, aspect, ifl, fd = _camera_parts(cam)
    hori, hpos, haspect, hifl, _ = _camera_parts(hist_cam)
    tz, tn, ta = f32(P.depth_tolerance), f32(P.normal_tolerance), f32(P.albedo_tolerance)
    wf, hf = f32(w), f32(h)
    # 1-2: the pixel's first-hit point
    cov = A[..., 3]
    ok = cov > 0
    z = G[..., 3] / cov
    xs = np.arange(w, dtype=f32)[None, :].repeat(h, 0)
    ys = np.arange(h, dtype=f32)[:, None].repeat(w, 1)
    uvx = ((xs + f32(0.5)) / wf * f32(2) - f32(1)) * aspect
    uvy = -((ys + f32(0.5)) / hf * f32(2) - f32(1))
    dx, dy, dz = uvx * ifl * fd, uvy * ifl * fd, np.full((h, w), f32(-1) * fd, f32)
    ln = np.sqrt(_dot3(dx, dy, dz, dx, dy, dz))
    dx, dy, dz = dx / ln, dy / ln, dz / ln
    # mul_m3v3(ori, d): component c is the dot of (r0.c, r1.c, r2.c) with d
    dirv = [_dot3(ori[0, c], ori[1, c], ori[2, c], dx, dy, dz) for c in range(3)]
    Pw = [pos[c] + dirv[c] * z for c in range(3)]
    # 3: into the history camera
    q = [Pw[c] - hpos[c] for c in range(3)]
    l = [_dot3(hori[r, 0], hori[r, 1], hori[r, 2], q[0], q[1], q[2]) for r in range(3)]   # mul_v3m3(q, ori)
    ok &= l[2] < 0
    t = -l[2]
    sx = (l[0] / t) / hifl / haspect
    sy = -((l[1] / t) / hifl)
    fx = (sx + f32(1)) * f32(0.5) * wf - f32(0.5)
    fy = (sy + f32(1)) * f32(0.5) * hf - f32(0.5)
    ze = np.sqrt((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2])
    ok &= np.isfinite(fx) & np.isfinite(fy)
    # 4: the bilinear taps, b (rows) outer and a (columns) inner
    ix, iy = np.floor(fx), np.floor(fy)
    tx, ty = fx - ix, fy - iy
    for b in (0, 1):
        Y = iy + f32(b)
        wy = ty if b else f32(1) - ty
        for a in (0, 1):
            X = ix + f32(a)
            bw = (tx if a else f32(1) - tx) * wy
            v = ok & (X >= 0) & (X <= f32(w - 1)) & (Y >= 0) & (Y <= f32(h - 1))
            xi = np.where(v, X, f32(0)).astype(np.int64)
            yi = np.where(v, Y, f32(0)).astype(np.int64)
            Hq, HMq, HAq, HGq = H[yi, xi], HM[yi, xi], HA[yi, xi], HG[yi, xi]
            v &= HAq[..., 3] > 0
            v &= np.isfinite(Hq[..., :3]).all(-1)
            v &= HMq[..., 3] > 0
            zh = HGq[..., 3] / HAq[..., 3]
            v &= np.abs(zh - ze) <= tz * np.where(zh > ze, zh, ze)
            v &= _sq3(G[..., :3] - HGq[..., :3]) <= tn
            d = A - HAq
            v &= (_sq3(d) + d[..., 3] * d[..., 3]) <= ta
            S.sw = np.where(v, S.sw + bw, S.sw)
            S.sc = np.where(v[..., None], S.sc + bw[..., None] * Hq[..., :3], S.sc)
            S.s1 = np.where(v, S.s1 + bw * HMq[..., 0], S.s1)
            S.s2 = np.where(v, S.s2 + bw * HMq[..., 1], S.s2)
            S.sn = np.where(v, S.sn + bw * HMq[..., 3], S.sn)


def _temporal_blend(some, Hc, h1, h2, hn, max_history, R, M):
    """Steps 5-7: (out_radiance, out_moments) of the history (Hc, h1, h2, hn)
    where `some`, blended with this frame's R and M."""
    f32 = np.float32
    mh = f32(max_history)
    out_c = R.copy()
    out_c[..., 3] = 0
    nh = np.where(hn < mh, hn, mh)
    nc = M[..., 3]
    both = some & np.isfinite(R[..., :3]).all(-1) & (nc > 0)
    nt = nh + nc
    al = nc / nt
    c6 = Hc + al[..., None] * (R[..., :3] - Hc)
    m1 = h1 + al * (M[..., 0] - h1)
    m2 = h2 + al * (M[..., 1] - h2)
    mom6 = np.stack([m1, m2, _var_of_mean(m1, m2, nt), nt], -1)
    mom7 = np.stack([h1, h2, _var_of_mean(h1, h2, nh), nh], -1)
    out_c[..., :3] = np.where(both[..., None], c6, np.where(some[..., None], Hc, R[..., :3]))
    out_m = np.where(both[..., None], mom6, np.where(some[..., None], mom7, M))
    assert out_c.dtype == f32 and out_m.dtype == f32
    return out_c, np.ascontiguousarray(out_m)


def temporal_reference(cam, hist_cam, radiance, moments, albedo, normal_depth, hist_radiance=None, hist_moments=None,
                       hist_albedo=None, hist_normal_depth=None, params: TemporalParams = None, found=None):
    """ptg_temporal_accumulate on the CPU: [h, w, 4] float32 arrays in,
    (out_radiance, out_moments) out.  `cam` / `hist_cam` are CAMERA_DTYPE
    records or ctypes ptg_camera structures; `hist_cam` and the four hist_*
    arrays are all None (first frame) or all given.  A bool [h, w] array
    passed as `found` is set where a pixel found history."""
    P = params if params is not None else TemporalParams.default()
    P.validate()
    (R, M, A, G), old = _temporal_images(radiance, moments, albedo, normal_depth,
                                         (hist_cam, hist_radiance, hist_moments, hist_albedo, hist_normal_depth))
    h, w = R.shape[:2]
    if found is not None:
        found[...] = False
    if old is None or w * h == 0:
        out_c = R.copy()
        out_c[..., 3] = 0
        return out_c, M.copy()
    with np.errstate(all="ignore"):
        S = _TemporalSums(h, w)
        _temporal_gather(S, cam, hist_cam, A, G, old, P)
        some = S.sw > 0
        out = _temporal_blend(some, S.sc / S.sw[..., None], S.s1 / S.sw, S.s2 / S.sw, S.sn / S.sw, P.max_history, R, M)
    if found is not None:
        found[...] = some
    return out


# ---- temporal accumulation over several cameras, with a history clamp ----------


class TemporalClampParams(_Params, C.Structure):
    """ptg_temporal_clamp_params.  ``TemporalClampParams.default()`` asks the
    library; ``base`` is a TemporalParams."""
    _fields_ = [("base", TemporalParams), ("clamp_radius", C.c_uint32), ("clamp_sigma", C.c_float),
                ("clipped_history", C.c_float)]
    _default_fn = "ptg_temporal_clamp_params_default"
    _positive = ("clamp_sigma", "clipped_history")
    MAX_RADIUS = 2

    def as_dict(self):
        return dict(_Params.as_dict(self), base=self.base.as_dict())

    def validate(self):
        self.base.validate()
        if self.clamp_radius > self.MAX_RADIUS:
            raise ValueError("clamp_radius > %d" % self.MAX_RADIUS)
        _Params.validate(self)


MAX_CAMERAS = 512                                # ptg_temporal_accumulate_clamped's n_cams


def clamp_box(radiance, radius, sigma):
    """The clamp's colour box of every pixel: (n [h, w] int, lo, hi [h, w, 3]
    float32) from the (2 radius + 1)^2 window of `radiance`, dy outer and dx
    inner, taps outside the image or with a non-finite channel left out;
    lo / hi = mean -+ sigma * standard deviation.  Where n is 0 the bounds
    mean nothing."""
    f32 = np.float32
    R = np.ascontiguousarray(radiance, dtype=f32)[..., :3]
    h, w = R.shape[:2]
    fin = np.isfinite(R).all(-1)
    n = np.zeros((h, w), np.int64)
    su = np.zeros((h, w, 3), f32)
    sq = np.zeros((h, w, 3), f32)
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):
            y0, y1 = max(0, -dy), min(h, h - dy)
            if y0 >= y1:
                continue
            for dx in range(-radius, radius + 1):
                x0, x1 = max(0, -dx), min(w, w - dx)
                if x0 >= x1:
                    continue
                ps = (slice(y0, y1), slice(x0, x1))
                qs = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
                v = fin[qs]
                Rq = R[qs]
                n[ps] += v
                su[ps] = np.where(v[..., None], su[ps] + Rq, su[ps])
                sq[ps] = np.where(v[..., None], sq[ps] + Rq * Rq, sq[ps])
        nf = n.astype(f32)[..., None]
        mu = su / nf
        e2 = sq / nf
        d = e2 - mu * mu
        rr = f32(sigma) * np.sqrt(np.where(d > 0, d, f32(0)))
        return n, mu - rr, mu + rr


def temporal_clamped_reference(cams, hist_cam, radiance, moments, albedo, normal_depth, hist_radiance=None,
                               hist_moments=None, hist_albedo=None, hist_normal_depth=None,
                               params: TemporalClampParams = None, found=None, clipped=None):
    """ptg_temporal_accumulate_clamped on the CPU:
    temporal_reference with the reprojection run once per camera of `cams` (a
    sequence of 1 .. 512 CAMERA_DTYPE records or ctypes ptg_camera structures)
    into the same sums, and, with params.clamp_radius > 0, the history clamped
    to this frame's local colour box.  Bool [h, w] arrays passed as `found` /
    `clipped` are set where a pixel found history / had it clipped."""
    P = params if params is not None else TemporalClampParams.default()
    P.validate()
    cams = list(cams) if not isinstance(cams, np.ndarray) else [c for c in cams.reshape(-1)]
    if not 1 <= len(cams) <= MAX_CAMERAS:
        raise ValueError("1 .. %d cameras, got %d" % (MAX_CAMERAS, len(cams)))
    (R, M, A, G), old = _temporal_images(radiance, moments, albedo, normal_depth,
                                         (hist_cam, hist_radiance, hist_moments, hist_albedo, hist_normal_depth))
    h, w = R.shape[:2]
    for flag in (found, clipped):
        if flag is not None:
            flag[...] = False
    if old is None or w * h == 0:
        out_c = R.copy()
        out_c[..., 3] = 0
        return out_c, M.copy()
    f32 = np.float32
    with np.errstate(all="ignore"):
        S = _TemporalSums(h, w)
        for cam in cams:
            _temporal_gather(S, cam, hist_cam, A, G, old, P.base)
        some = S.sw > 0
        Hc, h1, h2, hn = S.sc / S.sw[..., None], S.s1 / S.sw, S.s2 / S.sw, S.sn / S.sw
        clip = np.zeros((h, w), bool)
        if P.clamp_radius > 0:
            n, lo, hi = clamp_box(R, int(P.clamp_radius), P.clamp_sigma)
            below = Hc < lo
            above = ~below & (Hc > hi)
            Hk = np.where(below, lo, np.where(above, hi, Hc))
            clip = some & (n > 0) & (below | above).any(-1)
            dl = _lum(Hk) - _lum(Hc)
            g1 = h1 + dl
            g2 = h2 + (g1 * g1 - h1 * h1)
            ch = f32(P.clipped_history)
            Hc = np.where(clip[..., None], Hk, Hc)
            h2 = np.where(clip, g2, h2)
            h1 = np.where(clip, g1, h1)
            hn = np.where(clip, np.where(hn < ch, hn, ch), hn)
        out = _temporal_blend(some, Hc, h1, h2, hn, P.base.max_history, R, M)
    if found is not None:
        found[...] = some
    if clipped is not None:
        clipped[...] = clip
    return out
