"""Inputs shared by the adaptive-sampling tests: seeded per-sample radiance for
the pinned bits of ptlumi.adaptive.adaptive_reference
(tests/test_adaptive_reference.py) and the oracle cases of the GPU comparison
(tests/test_gpu_adaptive.py)."""
import hashlib

import numpy as np

# (name, h, w, N, m, passes, min_passes, dilate, threshold, luminance_floor)
SYNTHETIC = [
    ("bands_p4_d1", 9, 13, 48, 4, 4, 1, 1, 0.05, 0.01),
    ("bands_p3_d0", 9, 13, 48, 8, 3, 1, 0, 0.08, 0.01),
    ("bands_p6_min2_d2", 7, 5, 48, 2, 6, 2, 2, 0.03, 0.5),
    ("bands_p1", 9, 13, 16, 8, 1, 1, 1, 0.05, 0.01),
    ("bands_p16", 5, 7, 32, 1, 16, 1, 1, 0.1, 0.01),
]


def synthetic_samples(h, w, n, seed):
    """[h, w, n, 3] radiance: three vertical bands of rising noise (the first
    converges at once, the last never), a few NaN and inf samples, one pixel
    with no finite sample and one with a single finite sample."""
    rng = np.random.default_rng(seed)
    band = (np.arange(w) * 3 // max(w, 1))[None, :, None, None]
    sigma = np.float32([0.001, 0.15, 1.5])[band]
    base = np.float32([0.8, 0.3, 2.0])[band]
    c = (base + sigma * rng.normal(0, 1, (h, w, n, 3))).astype(np.float32)
    c = np.abs(c)
    if h * w >= 15:
        c[0, 0, 1, 1] = np.nan
        c[1, 2, n - 1, 0] = np.inf
        c[2, 1, :, 0] = np.nan                 # no finite sample: n = 0
        c[3, 0, :, 1] = np.inf                 # a single finite sample: n = 1
        c[3, 0, n // 2, 1] = 0.75
    return c


def params_of(passes, min_passes, dilate, threshold, luminance_floor):
    from ptlumi.adaptive import AdaptiveParams
    return AdaptiveParams(passes, min_passes, dilate, threshold, luminance_floor)


def bits_digest(*arrays):
    """SHA-256 over the arrays' bytes: float32 with every NaN as 0x7fc00000,
    integers as little-endian uint32."""
    hs = hashlib.sha256()
    for a in arrays:
        a = np.asarray(a)
        if a.dtype == np.float32:
            u = np.ascontiguousarray(a).copy().view(np.uint32)
            u[np.isnan(u.view(np.float32))] = 0x7FC00000
        else:
            u = np.ascontiguousarray(a, np.uint32)
        hs.update(u.astype("<u4").tobytes())
    return hs.hexdigest()


def synthetic_digest(name):
    from ptlumi.adaptive import adaptive_reference
    for case in SYNTHETIC:
        if case[0] == name:
            _, h, w, n, m = case[:5]
            acc, mom, ns, active = adaptive_reference(synthetic_samples(h, w, n, 31 * w + h), m, params_of(*case[5:]))
            return bits_digest(acc, mom, ns, np.array(active, np.uint32))
    raise KeyError(name)


# The GPU comparison's oracle cases (the issue's table):
# (id, w, h, N, bounces, frame, m, passes, dilate, threshold); luminance_floor 0.01, min_passes 1
GPU_CASES = [
    ("f450_p4", 48, 27, 64, 4, 450, 8, 4, 0, 0.2),
    ("f1750_p3", 41, 23, 48, 7, 1750, 8, 3, 1, 0.05),
    ("f450_m4", 48, 27, 32, 4, 450, 4, 4, 1, 0.4),
    ("f0_reawakening", 48, 27, 64, 4, 0, 8, 4, 1, 0.1),
]
