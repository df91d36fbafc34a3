"""CPU expectations for the camera-ray and feature-buffer entries (helpers of
tests/test_gpu_features.py; not a test module).

A float32 scalar restatement of path_trace_pixel's first steps - the seed,
the film jitter and get_camera_ray (path_tracer.hh:659-671, :429-450, with
the samplers of :12-25 and :50-62 and inv_erf, math.hh:455-463) - written
from the reference's operation order.  The random numbers come from the
oracle's pcg4d / generate_uniform_random4; the double-precision library calls
are this host's libm through ``math``.  Every intermediate is an np.float32
scalar, so each operation rounds once.
"""
import math

import numpy as np

import oracle as O

F = np.float32
PI_F = F(math.pi)
MAX_RAY_DIST = F(1e9)


def _signf(v):
    if v < 0:
        return F(-1.0)
    if v > 0:
        return F(1.0)
    return v


def _clampf(v, lo, hi):
    return min(max(v, lo), hi)        # finite arguments only


def _inv_erf(x):
    ln1x2 = F(math.log(float(F(1) - x * x)))
    a = F(0.147)
    p = F(2.0) / (PI_F * a)
    k = p + ln1x2 * F(0.5)
    k2 = k * k
    inner = math.sqrt(float(k2 - ln1x2 * (F(1.0) / a)))
    return F(float(_signf(x)) * math.sqrt(inner - float(k)))


def _sample_gaussian(u, sigma, eps):
    k = u * F(2.0) - F(1.0)
    k = _clampf(k, -(F(1.0) - eps), F(1.0) - eps)
    return sigma * F(1.41421356) * _inv_erf(k)


def _gaussian_disk(ux, uy, sigma):
    r = F(math.sqrt(float(ux)))
    theta = F(2.0) * PI_F * uy
    r = _sample_gaussian(r, sigma, F(1e-6))
    return r * F(math.cos(float(theta))), r * F(math.sin(float(theta)))


def _regular_polygon(ux, uy, angle, sides):
    fs = F(sides)
    side = F(math.floor(float(ux * fs)))
    ux = ux * fs
    ux = F(float(ux) - math.floor(float(ux)))
    side_radians = (F(2.0) * PI_F) / fs
    a1 = side_radians * side + angle
    a2 = side_radians * (side + F(1.0)) + angle
    bx, by = F(math.sin(float(a1))), F(math.cos(float(a1)))
    cx, cy = F(math.sin(float(a2))), F(math.cos(float(a2)))
    if ux + uy > F(1.0):
        ux = F(1.0) - ux
        uy = F(1.0) - uy
    return bx * ux + cx * uy, by * ux + cy * uy


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm3(a):
    n = F(math.sqrt(float(_dot3(a, a))))
    return [a[0] / n, a[1] / n, a[2] / n]


def _mul_m3v3(rows, a):
    """mul_m3v3 (math.hh:227): the dot products of the matrix's columns with a."""
    return [_dot3([rows[0][c], rows[1][c], rows[2][c]], a) for c in range(3)]


def camera_ray(cam, cfg, x, y, sample_index):
    """-> (origin[3], dir[3]) of path_trace_pixel's first ray, np.float32."""
    seed = np.array([[x, y, np.uint32(np.int64(sample_index) & 0xFFFFFFFF), cfg.student_id]], np.uint32)
    _, u = O.pcg(seed)
    u = [F(v) for v in u[0]]
    fx, fy = _gaussian_disk(u[0], u[1], F(0.4))
    fx = fx + F(0.5)
    fy = fy + F(0.5)
    cx, cy = F(x) + fx, F(y) + fy
    uvx = cx / F(cfg.width) * F(2.0) - F(1.0)
    uvy = cy / F(cfg.height) * F(2.0) - F(1.0)
    uvx = uvx * F(cam["aspect_ratio"])
    uvy = -uvy
    apx, apy = F(0), F(0)
    if int(cam["aperture_polygon"]) > 3:
        px, py = _regular_polygon(u[2], u[3], F(cam["aperture_angle"]), int(cam["aperture_polygon"]))
        apx = px * F(cam["aperture_radius"])
        apy = py * F(cam["aperture_radius"])
    origin = [apx, apy, F(0.0)]
    ifl, fd = F(cam["inv_focal_length"]), F(cam["focal_distance"])
    d = [uvx * ifl * fd, uvy * ifl * fd, F(-1.0) * fd]
    d = _norm3([d[0] - origin[0], d[1] - origin[1], d[2] - origin[2]])
    rows = [[F(v) for v in cam["orientation"][r][:3]] for r in range(3)]
    direction = _mul_m3v3(rows, d)
    o = _mul_m3v3(rows, origin)
    pos = cam["position"]
    origin = [o[0] + F(pos[0]), o[1] + F(pos[1]), o[2] + F(pos[2])]
    return origin, direction


def camera_rays(subframes, cfg, xy, js):
    """The expectation of ptg_camera_rays: (rays float32 [n, 8], subframe uint32 [n])."""
    rays = np.zeros((len(js), 8), np.float32)
    sub = np.zeros(len(js), np.uint32)
    with np.errstate(over="ignore"):
        for i, ((x, y), j) in enumerate(zip(xy, js)):
            sub[i] = int(j) // cfg.samples_per_motion_blur_step
            o, d = camera_ray(subframes[sub[i]]["cam"], cfg, int(x), int(y), int(j))
            rays[i] = o + d + [F(0.0), MAX_RAY_DIST]
    return rays, sub


def sample_features(arrays, hit):
    """One traced camera ray's contribution (albedo.rgb, coverage, normal.xyz,
    depth) from its closest hit (a row of Oracle.trace_rays), interpolated in
    hit_info's operation order (path_tracer.hh:369-400)."""
    b = hit[:3].view(np.float32)
    thit = hit[3:4].view(np.float32)[0]
    if thit < 0:
        return [F(1), F(1), F(1), F(0), F(0), F(0), F(0), F(0)]
    inst = arrays["instances"][int(hit[4])]
    ioff, bv = int(inst["mesh"][2]), int(inst["mesh"][3])
    tri = ioff + int(hit[5]) * 3
    v = [bv + int(arrays["indices"][tri + k]) for k in range(3)]
    a = [arrays["albedo"][i] for i in v]
    n = [arrays["normal"][i] for i in v]
    alb = [a[0][c] * b[0] + a[1][c] * b[1] + a[2][c] * b[2] for c in range(3)]
    nn = [(n[0][c] * b[0] + n[1][c] * b[1]) + n[2][c] * b[2] for c in range(3)]
    rows = [[F(x) for x in inst["transform"][r][:3]] for r in range(3)]
    nn = _norm3(_mul_m3v3(rows, nn))
    if hit[6]:
        nn = [-nn[0], -nn[1], -nn[2]]
    return alb + [F(1)] + nn + [thit]


def per_sample_features(arrays, cfg, oracle, rect, samples):
    """Every sample's contribution over rect = (x0, y0, w, h) and samples =
    (j0, j1): float32 [h * w, j1 - j0, 8]: restated camera ray -> the oracle's
    closest hit in the ray's subframe -> sample_features."""
    x0, y0, w, h = rect
    j0, j1 = samples
    yy, xx, jj = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), np.arange(j0, j1), indexing="ij")
    xy = np.stack([xx.reshape(-1), yy.reshape(-1)], 1)
    js = jj.reshape(-1)
    rays, sub = camera_rays(arrays["subframes"], cfg, xy, js)
    hits = np.zeros((len(js), 8), np.uint32)
    for s in np.unique(sub):
        sel = np.nonzero(sub == s)[0]
        hits[sel] = oracle.trace_rays(int(s), rays[sel])
    out = np.array([sample_features(arrays, hit) for hit in hits], np.float32)
    return out.reshape(h * w, j1 - j0, 8)


def fold_features(per_sample, cfg, shape):
    """The expectation of ptg_render_features from per_sample_features' rows
    (already cut to the sample range): each component summed in float32 in
    sample order from +0, then divided by samples_per_pixel.
    -> (albedo+coverage [h, w, 4], normal+depth [h, w, 4])"""
    h, w = shape
    acc = np.zeros((h * w, 8), np.float32)
    for k in range(per_sample.shape[1]):
        acc = acc + per_sample[:, k]
    out = (acc / F(cfg.samples_per_pixel)).reshape(h, w, 8)
    assert out.dtype == np.float32
    return out[..., :4].copy(), out[..., 4:].copy()
