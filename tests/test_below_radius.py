"""below_radius (csrc/device/ref_math.h): `s < T` in place of
`sqrtf(s) - EARTH_RADIUS < 0` in the atmosphere's below-ground tests.

A correctly rounded square root is monotone, so the equivalence holds for
every non-negative float s once it holds at T and at the float just below it;
numpy's float32 sqrt is correctly rounded (IEEE), like the device's.  The
device side is swept over all 2^32 patterns by tools/exhaustive.hip
(profiles/r08_fastpaths/).
"""
import os
import re

import numpy as np

from conftest import ROOT

CSRC = os.path.join(ROOT, "path-tracing...but-on-the-lumi-cluster_amd", "csrc", "device")


def _constants():
    text = open(os.path.join(CSRC, "ref_math.h")).read()
    bits = int(re.search(r"kBelowEarthBits\s*=\s*(0x[0-9a-fA-F]+)u?\s*;", text).group(1), 16)
    radius = np.float32(float(re.search(r"kBelowEarthRadius\s*=\s*([0-9.eE+]+)f\s*;", text).group(1)))
    return bits, radius


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _want(s, radius):
    """the reference's test: length - EARTH_RADIUS < 0, all in float32"""
    with np.errstate(invalid="ignore"):
        return (np.sqrt(s, dtype=np.float32) - radius) < 0


def test_radius_is_the_path_tracers():
    _, radius = _constants()
    text = open(os.path.join(CSRC, "path_tracer.h")).read()
    earth = np.float32(float(re.search(r"EARTH_RADIUS\s*=\s*([0-9.eE+]+)f\s*;", text).group(1)))
    assert earth == radius == np.float32(6378100.0)
    assert "static_assert(EARTH_RADIUS == kBelowEarthRadius" in text


def test_threshold_brackets_the_radius():
    bits, radius = _constants()
    t, below = _f32(bits), _f32(bits - 1)
    assert np.sqrt(below, dtype=np.float32) < radius <= np.sqrt(t, dtype=np.float32)


def test_equivalence_around_the_threshold_and_at_the_ends():
    bits, radius = _constants()
    t = _f32(bits)
    s = _f32(np.arange(bits - (1 << 16), bits + (1 << 16) + 1, dtype=np.int64).astype(np.uint32))
    assert np.array_equal(s < t, _want(s, radius))
    assert (s < t).sum() == 1 << 16            # the sweep straddles the threshold
    ends = np.array([0.0, np.inf, np.nan], np.float32)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(ends < t, _want(ends, radius))
    assert list(ends < t) == [True, False, False]
