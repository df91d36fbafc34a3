"""Inputs shared by the tests of the temporal accumulation over several cameras
with a history clamp: the CPU tests of the restatement
(tests/test_temporal_clamp_reference.py, with its pinned bits) and the GPU
comparison (tests/test_gpu_temporal_clamp.py).

The images are those of tests/temporal_inputs.py; added here are the lists of
this frame's cameras, a zoom with a dolly as a motion-blurred frame has them,
and the clamp's parameters.  Only +, -, *, / on literals build the cameras, so
they are the same bits on every host.
"""
import numpy as np

import temporal_inputs as T

SUBFRAMES = (1, 3)
RADII = (0, 1, 2)
IFL_SCALE = (1.0, 1.05, 1.1)                     # inv_focal_length of camera s: tan 30 degrees times this
Z_STEP = -0.1                                    # position of camera s: (0, 0, Z_STEP * s) from the case's camera
# The colour box: one standard deviation.  The payloads are uniform noise, so a
# history tap lies outside one deviation of a 3 x 3 or 5 x 5 window in some
# channel for a good part of the pixels and inside for the rest: both branches
# run (tests/test_temporal_clamp_reference.py checks the share).  A clipped
# history keeps 16 samples, below temporal_inputs' max_history of 32 and inside
# the history's 8 .. 100, so the cap binds at some pixels and not at others.
CLAMP = dict(clamp_sigma=1.0, clipped_history=16.0)


def camera_list(w, h, case, subframes):
    """`subframes` cameras of this frame: camera s is the case's current
    camera with inv_focal_length * IFL_SCALE[s], moved by (0, 0, Z_STEP * s).
    Camera 0 is the case's camera itself."""
    cur = T.cameras(w, h, case)[0]
    out = []
    for s in range(subframes):
        c = cur.copy()
        c["inv_focal_length"] = T.TAN_30 * IFL_SCALE[s]
        c["position"][2] = 0.0 + Z_STEP * s
        out.append(c)
    return out


def params(radius, base=None, **overrides):
    """TemporalClampParams over temporal_inputs' PARAMS (`base`: overrides of
    those) with CLAMP (`overrides`: of these)."""
    from ptlumi.denoise import TemporalClampParams
    c = dict(CLAMP, **overrides)
    return TemporalClampParams(T.params(**(base or {})), radius, c["clamp_sigma"], c["clipped_history"])


def case_key(w, h, case, subframes, radius):
    return "temporal_clamp_%dx%d_%s_s%d_r%d" % (w, h, case, subframes, radius)


ALL_CASES = [(w, h, case, s, r) for (w, h) in T.SIZES for case in T.CASES for s in SUBFRAMES for r in RADII]

_reference = {}


def reference(w, h, case, subframes, radius):
    """(out_radiance, out_moments, found, clipped) of the restatement on
    temporal_inputs(w, h, case) through camera_list(..., subframes) with
    params(radius): computed once, read-only."""
    key = (w, h, case, subframes, radius)
    if key not in _reference:
        from ptlumi.denoise import temporal_clamped_reference
        a = T.temporal_inputs(w, h, case)
        found, clipped = np.zeros((h, w), bool), np.zeros((h, w), bool)
        out = temporal_clamped_reference(camera_list(w, h, case, subframes), *a[1:], params=params(radius), found=found,
                                         clipped=clipped) + (found, clipped)
        for o in out:
            o.setflags(write=False)
        _reference[key] = out
    return _reference[key]


def reference_digest(w, h, case, subframes, radius):
    """The digest of one pinned case: the two images, then the found and the
    clipped mask as float32 0 / 1."""
    rad, mom, found, clipped = reference(w, h, case, subframes, radius)
    return T.bits_digest(rad, mom, found.astype(np.float32), clipped.astype(np.float32))
