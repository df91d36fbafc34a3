"""Seeded inputs shared by the denoiser tests: the GPU comparisons
(tests/test_gpu_denoise.py, tests/test_gpu_denoise_guided.py) and the pinned
bits of the CPU restatements (tests/test_denoise_reference_bits.py)."""
import hashlib

import numpy as np

SIZES = [(37, 23), (5, 3), (1, 1)]
ITERATIONS = [1, 3, 5]


def fixed_inputs(w, h, seed):
    """Noisy radiance over piecewise-smooth guides (three vertical bands that
    differ in albedo, normal and depth), with one NaN and one +inf pixel where
    the image has room for them."""
    rng = np.random.default_rng(seed)
    band = (np.arange(w) * 3 // max(w, 1))[None, :].repeat(h, 0)
    base_a = np.float32([[0.8, 0.3, 0.2, 1.0], [0.2, 0.5, 0.9, 1.0], [1.0, 1.0, 1.0, 0.0]])
    base_n = np.float32([[0.0, 0.0, 1.0, 5.0], [0.6, 0.0, 0.8, 9.0], [0.0, 0.0, 0.0, 0.0]])
    alb = (base_a[band] + rng.normal(0, 0.01, (h, w, 4))).astype(np.float32)
    nd = (base_n[band] + rng.normal(0, 0.02, (h, w, 4))).astype(np.float32)
    light = np.float32([1.0, 0.5, 2.0])[band][..., None] + rng.normal(0, 0.2, (h, w, 3))
    rad = np.zeros((h, w, 4), np.float32)
    rad[..., :3] = (alb[..., :3] * light).astype(np.float32)
    if w * h >= 15:
        rad[h // 2, w // 3, 1] = np.nan
        rad[h // 3, (2 * w) // 3, 0] = np.inf
    return rad, alb, nd


def guided_inputs(w, h, seed):
    """Noisy radiance over piecewise-smooth guides (three vertical bands that
    differ in albedo, normal, depth and noise level), with one NaN and one
    +inf pixel where the image has room for them; moments whose variance of
    the mean is drawn per band, with a few negative, NaN and infinite entries."""
    rng = np.random.default_rng(seed)
    band = (np.arange(w) * 3 // max(w, 1))[None, :].repeat(h, 0)
    base_a = np.float32([[0.8, 0.3, 0.2, 1.0], [0.2, 0.5, 0.9, 1.0], [1.0, 1.0, 1.0, 0.0]])
    base_n = np.float32([[0.0, 0.0, 1.0, 5.0], [0.6, 0.0, 0.8, 9.0], [0.0, 0.0, 0.0, 0.0]])
    alb = (base_a[band] + rng.normal(0, 0.01, (h, w, 4))).astype(np.float32)
    nd = (base_n[band] + rng.normal(0, 0.02, (h, w, 4))).astype(np.float32)
    noise = np.float32([0.2, 0.02, 0.5])[band]
    light = np.float32([1.0, 0.5, 2.0])[band][..., None] + rng.normal(0, 1, (h, w, 3)) * noise[..., None]
    rad = np.zeros((h, w, 4), np.float32)
    rad[..., :3] = (alb[..., :3] * light).astype(np.float32)
    mom = np.zeros((h, w, 4), np.float32)
    mom[..., 0] = rad[..., 1]
    mom[..., 2] = (noise * noise * rng.uniform(0.5, 1.5, (h, w))).astype(np.float32)
    mom[..., 3] = 16
    if w * h >= 15:
        rad[h // 2, w // 3, 1] = np.nan
        rad[h // 3, (2 * w) // 3, 0] = np.inf
        flat = mom[..., 2].reshape(-1)
        flat[1], flat[4], flat[7], flat[10], flat[13] = -0.5, np.nan, np.inf, -np.inf, 0.0
    return rad, alb, nd, mom


def moments_samples():
    """[64, 9, 3] samples for moments_reference: a few NaN and +-inf samples,
    pixel 5 with no finite sample, pixel 6 with a single finite one."""
    rng = np.random.default_rng(20240)
    c = rng.uniform(0.0, 3.0, (64, 9, 3)).astype(np.float32)
    c[0, 2, 1] = np.nan
    c[1, 8, 0] = np.inf
    c[2, 0, 2] = -np.inf
    c[3, 4, :] = np.nan
    c[5, :, 0] = np.nan
    c[6, :, 1] = np.inf
    c[6, 3, 1] = 0.75
    return c


def bits_digest(a):
    """SHA-256 of a float32 array's bytes, every NaN as 0x7fc00000."""
    u = np.ascontiguousarray(a, np.float32).copy().view(np.uint32)
    u[np.isnan(u.view(np.float32))] = 0x7FC00000
    return hashlib.sha256(u.astype("<u4").tobytes()).hexdigest()


def reference_digest(name, w=None, h=None, iterations=None):
    """The digest of one pinned case: name is "atrous", "atrous_guided"
    (on fixed_inputs / guided_inputs(w, h, 7 * w + h), default parameters but
    for the iterations) or "moments" (on moments_samples())."""
    from ptlumi import denoise as D
    if name == "moments":
        return bits_digest(D.moments_reference(moments_samples()))
    if name == "atrous":
        return bits_digest(D.atrous_reference(*fixed_inputs(w, h, 7 * w + h), D.DenoiseParams.default(iterations=iterations)))
    assert name == "atrous_guided", name
    return bits_digest(D.atrous_guided_reference(*guided_inputs(w, h, 7 * w + h),
                                                 D.DenoiseGuidedParams.default(iterations=iterations)))


def case_key(name, w=None, h=None, iterations=None):
    return name if name == "moments" else "%s_%dx%d_it%d" % (name, w, h, iterations)
