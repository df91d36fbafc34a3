"""ptlumi.adaptive.adaptive_reference, the CPU restatement of
ptg_render_adaptive: its bits are pinned by SHA-256 over
seeded synthetic samples (tests/golden/adaptive_reference_bits.json), and the
properties the definition states are checked on small hand-made inputs.  The
GPU test compares the kernels with the restatement; this keeps the two from
drifting together.  No GPU work here.

`python tests/test_adaptive_reference.py --write` records the digests of the
restatement as it stands (only for a deliberate change of the definition).
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "golden", "adaptive_reference_bits.json")

if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (registers the package as `ptlumi`)

from adaptive_inputs import SYNTHETIC, params_of, synthetic_digest, synthetic_samples  # noqa: E402

NAMES = [c[0] for c in SYNTHETIC]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return ((_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))).all()


@pytest.mark.parametrize("name", NAMES)
def test_reference_bits_are_the_pinned_ones(native_lib, name):
    with open(PINNED) as f:
        pinned = json.load(f)["sha256"]
    assert synthetic_digest(name) == pinned[name], name


def test_every_pinned_case_is_checked():
    with open(PINNED) as f:
        assert sorted(json.load(f)["sha256"]) == sorted(NAMES)


def test_the_entry_points_are_declared_and_the_default_is_valid(native_lib):
    from ptlumi import native as N
    from ptlumi.adaptive import AdaptiveParams
    for name in ("ptg_adaptive_params_default", "ptg_render_adaptive", "ptg_last_adaptive_stats"):
        assert name in N.exported_symbols(), "%s is not declared in ptg.h" % name
    p = AdaptiveParams.default()
    p.validate()
    assert 1 <= p.min_passes <= p.passes <= 16 and p.dilate <= 2
    assert native_lib.ptg_abi_version() == 1


def test_invalid_parameters_are_refused(native_lib):
    from ptlumi.adaptive import adaptive_reference
    c = synthetic_samples(3, 3, 16, 1)
    for bad in ((0, 1, 1, 0.05, 0.01), (4, 0, 1, 0.05, 0.01), (4, 5, 1, 0.05, 0.01), (17, 1, 1, 0.05, 0.01),
                (4, 1, 3, 0.05, 0.01), (4, 1, 1, 0.0, 0.01), (4, 1, 1, float("nan"), 0.01), (4, 1, 1, 0.05, float("inf")),
                (4, 1, 1, 0.05, -1.0)):
        with pytest.raises(ValueError):
            adaptive_reference(c, 2, params_of(*bad))
    with pytest.raises(ValueError):
        adaptive_reference(c, 8, params_of(4, 1, 1, 0.05, 0.01))       # 16 is no multiple of 4 * 8


def test_one_pass_is_the_plain_render_with_moments(native_lib):
    """passes = 1: the moments are moments_reference's bits, the radiance the
    j-ordered float32 sum over N, every pixel took N samples."""
    from ptlumi.adaptive import adaptive_reference
    from ptlumi.denoise import moments_reference
    c = synthetic_samples(9, 13, 16, 5)
    acc, mom, ns, active = adaptive_reference(c, 8, params_of(1, 1, 1, 0.05, 0.01))
    assert _same_bits(mom, moments_reference(c.reshape(9 * 13, 16, 3)).reshape(9, 13, 4))
    s = np.zeros((9, 13, 3), np.float32)
    with np.errstate(all="ignore"):
        for j in range(16):
            s = s + c[:, :, j]
        s = s / np.float32(16)
    assert _same_bits(acc[..., :3], s) and (acc[..., 3] == 0).all()
    assert (ns == 16).all() and ns.dtype == np.uint32 and active == [9 * 13]


@pytest.mark.parametrize("n,m,passes", [(64, 8, 4), (48, 8, 3), (32, 4, 4), (48, 2, 6), (16, 1, 16), (16, 8, 1)])
def test_the_sample_map_is_a_permutation_and_a_pass_owns_its_subframes(n, m, passes):
    from ptlumi.adaptive import sample_index
    span = n // passes
    js = np.array([[sample_index(jj, k, passes, m) for jj in range(span)] for k in range(passes)])
    assert sorted(js.ravel()) == list(range(n))
    for k in range(passes):
        sub = js[k] // m
        assert (sub % passes == k).all()                   # only subframes k, k + passes, ...
        assert (np.diff(js[k]) > 0).all()                  # ascending: a pass adds in sample order
        assert sorted(set(sub)) == list(range(k, n // m, passes))   # and all of them: the whole shutter


def _constant(h, w, n, value=1.0):
    return np.full((h, w, n, 3), value, np.float32)


def test_pixels_with_fewer_than_two_finite_samples_and_nan_sums_stay_active(native_lib):
    from ptlumi.adaptive import adaptive_reference, noisy_pixels
    c = _constant(3, 4, 16)                                 # no variance: every pixel stops after pass 0
    c[0, 0, :, 0] = np.nan                                  # n = 0
    c[1, 1, :, 1] = np.inf                                  # n = 1
    c[1, 1, 9, 1] = 1.0
    c[2, 3, 0] = 3e38                                       # L * L overflows: s2 = inf, m2 - m1 * m1 = NaN -> var 0
    acc, mom, ns, active = adaptive_reference(c, 2, params_of(4, 1, 0, 0.05, 0.01))
    assert active == [12, 2, 2, 2]
    assert ns[0, 0] == 16 and ns[1, 1] == 16 and (np.delete(ns.ravel(), [0, 5]) == 4).all()
    assert mom[0, 0].tolist() == [0, 0, 0, 0] and mom[1, 1, 3] == 1 and mom[1, 1, 2] == 0
    # a NaN mean (s1 = inf - inf) is noisy whatever n is
    s1 = np.float32([np.nan, 4.0])
    assert noisy_pixels(s1, np.float32([1.0, 4.0]), np.array([4, 4]), 0.05, 0.01).tolist() == [True, False]


def test_the_window_is_clipped_at_the_rectangle_edges(native_lib):
    """One noisy pixel in a corner and one on an edge of a still image keep
    exactly their clipped windows awake."""
    from ptlumi.adaptive import adaptive_reference, dilate_window
    rng = np.random.default_rng(3)
    c = _constant(6, 7, 16)
    for (y, x) in ((0, 0), (5, 3)):
        c[y, x] = rng.uniform(0.0, 4.0, (16, 3)).astype(np.float32)
    for r, want in ((0, 2), (1, 4 + 6), (2, 9 + 15)):
        acc, mom, ns, active = adaptive_reference(c, 2, params_of(2, 1, r, 0.01, 0.01))
        assert active == [42, want], (r, active)
        awake = ns == 16
        expect = np.zeros((6, 7), bool)
        expect[0:r + 1, 0:r + 1] = True
        expect[5 - r:6, max(0, 3 - r):3 + r + 1] = True
        assert np.array_equal(awake, expect), r
    m = np.zeros((3, 3), bool)
    m[0, 2] = True
    assert dilate_window(m, 1).tolist() == [[False, True, True], [False, True, True], [False, False, False]]
    assert dilate_window(m, 0).tolist() == m.tolist()


def test_a_stopped_pixel_is_woken_again(native_lib):
    """The rule keeps no state.  In a still row, pixel 5 is noisy throughout
    and keeps pixel 4 awake; pixel 4's samples vary in pass 1 only, which
    makes it noisy from then on, so its neighbour 3 - still, stopped after
    pass 0, absent from pass 1 - takes passes 2 and 3."""
    from ptlumi.adaptive import adaptive_reference, sample_index
    n, m, passes = 32, 2, 4
    span = n // passes
    c = _constant(1, 6, n)
    c[0, 5, ::2] = 9.0
    c[0, 4, [sample_index(jj, 1, passes, m) for jj in range(0, span, 2)]] = 9.0
    acc, mom, ns, active = adaptive_reference(c, m, params_of(passes, 1, 1, 0.05, 0.01))
    assert active == [6, 2, 3, 3]                           # the count rises again
    assert (ns // span).ravel().tolist() == [1, 1, 1, 3, 4, 4]
    # pixel 3's sum is its samples of passes 0, 2 and 3 over its own count
    assert acc[0, 3, :3].tolist() == [1.0, 1.0, 1.0] and mom[0, 3, 3] == 3 * span


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    with open(PINNED, "w") as f:
        json.dump({"canonical_nan": "0x7fc00000", "sha256": {n: synthetic_digest(n) for n in NAMES}}, f, indent=1)
        f.write("\n")
