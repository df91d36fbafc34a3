"""ptlumi.denoise.temporal_clamped_reference, the CPU restatement of
ptg_temporal_accumulate_clamped: that it is
temporal_reference with one camera and no clamp, the clamp's properties on the
plane scene of tests/temporal_inputs.py, and its bits, pinned as SHA-256
digests in tests/golden/temporal_clamp_reference_bits.json so that a later
change cannot move the kernel and the restatement together.  No GPU work here.

`python tests/test_temporal_clamp_reference.py --write` records the digests of
the restatement as it stands (only for a deliberate change of the definition).
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "golden", "temporal_clamp_reference_bits.json")

if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (registers the package as `ptlumi`)

import temporal_clamp_inputs as K  # noqa: E402
import temporal_inputs as T  # noqa: E402
from ptlumi.denoise import (TemporalClampParams, clamp_box, temporal_clamped_reference,  # noqa: E402
                            temporal_reference)
from ptlumi.renderer import TemporalDenoiser  # noqa: E402

f32 = np.float32
W, H = 37, 23


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.parametrize("case", T.CASES)
@pytest.mark.parametrize("w,h", T.SIZES)
def test_one_camera_and_no_clamp_is_temporal_reference(native_lib, w, h, case):
    a = T.temporal_inputs(w, h, case)
    f0, f1, cl = np.zeros((h, w), bool), np.ones((h, w), bool), np.ones((h, w), bool)
    want = temporal_reference(*a, params=T.params(), found=f0)
    got = temporal_clamped_reference([a[0]], *a[1:], params=K.params(0), found=f1, clipped=cl)
    assert T.same_bits(got[0], want[0]).all() and T.same_bits(got[1], want[1]).all()
    assert np.array_equal(f0, f1) and not cl.any()
    # a first frame too
    got = temporal_clamped_reference([a[0]], None, *a[2:6], params=K.params(1), found=f1, clipped=cl)
    want = temporal_reference(a[0], None, *a[2:6], params=T.params())
    assert np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert not f1.any() and not cl.any()


def _box_by_the_definition(R, r, sigma):
    """The colour box of every pixel, pixel by pixel and tap by tap as the
    definition states it: (n, lo, hi)."""
    h, w = R.shape[:2]
    n = np.zeros((h, w), np.int64)
    lo, hi = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                su, sq, cnt = [f32(0)] * 3, [f32(0)] * 3, 0
                for dy in range(-r, r + 1):
                    for dx in range(-r, r + 1):
                        qx, qy = x + dx, y + dy
                        if not (0 <= qx < w and 0 <= qy < h) or not np.isfinite(R[qy, qx, :3]).all():
                            continue
                        cnt += 1
                        for c in range(3):
                            su[c] = su[c] + R[qy, qx, c]
                            sq[c] = sq[c] + R[qy, qx, c] * R[qy, qx, c]
                n[y, x] = cnt
                for c in range(3):
                    mu, e2 = su[c] / f32(cnt), sq[c] / f32(cnt)
                    d = e2 - mu * mu
                    rr = f32(sigma) * np.sqrt(d if d > 0 else f32(0))
                    lo[y, x, c], hi[y, x, c] = mu - rr, mu + rr
    return n, lo, hi


def _history_alone(case, subframes, radius, rad=None, **base):
    """The restatement with a frame that brings no sample (moments all 0), so
    that step 7 hands the history through as it stands after the clamp:
    (Hc', (h1', h2', -, min(hn', max_history)), found, clipped)."""
    a = T.temporal_inputs(W, H, case)
    found, clipped = np.zeros((H, W), bool), np.zeros((H, W), bool)
    out = temporal_clamped_reference(K.camera_list(W, H, case, subframes), a[1], a[2] if rad is None else rad,
                                     np.zeros_like(a[3]), *a[4:], params=K.params(radius, base=base), found=found,
                                     clipped=clipped)
    return out + (found, clipped)


@pytest.mark.parametrize("subframes", K.SUBFRAMES)
@pytest.mark.parametrize("radius", (1, 2))
def test_the_clamp_puts_the_history_inside_the_box_and_keeps_its_variance(native_lib, radius, subframes):
    rad = T.temporal_inputs(W, H, "pan")[2]
    n, lo, hi = _box_by_the_definition(rad, radius, K.CLAMP["clamp_sigma"])
    n_v, lo_v, hi_v = clamp_box(rad, radius, K.CLAMP["clamp_sigma"])
    assert np.array_equal(n, n_v) and (n > 0).all()
    assert np.array_equal(_bits(lo), _bits(lo_v)) and np.array_equal(_bits(hi), _bits(hi_v))
    c0, m0, found0, clipped0 = _history_alone("pan", subframes, 0, max_history=1e6)
    c1, m1, found, clipped = _history_alone("pan", subframes, radius, max_history=1e6)
    assert np.array_equal(found, found0) and not clipped0.any() and found.mean() > 0.8
    assert clipped.any() and (found & ~clipped).any() and not (clipped & ~found).any()
    # inside the box, on the float32 bounds themselves
    assert ((c1[..., :3] >= lo) & (c1[..., :3] <= hi))[found].all()
    # clipped exactly where the unclamped history lay outside
    outside = ((c0[..., :3] < lo) | (c0[..., :3] > hi)).any(-1)
    assert np.array_equal(clipped, found & outside)
    # not clipped: the unclamped bits
    keep = ~clipped
    assert T.same_bits(c1, c0)[keep].all() and T.same_bits(m1, m0)[keep].all()
    # clipped: h2' - h1'^2 is h2 - h1^2 up to the four roundings of h2' = h2 + (h1' h1' - h1 h1), each at
    # most 2^-24 of its result; the sample count is capped
    a1, a2, b1, b2 = (x.astype(np.float64)[clipped] for x in (m0[..., 0], m0[..., 1], m1[..., 0], m1[..., 1]))
    bound = 2.0 ** -24 * (b1 * b1 + a1 * a1 + np.abs(b1 * b1 - a1 * a1) + np.abs(b2))
    assert (np.abs((b2 - b1 * b1) - (a2 - a1 * a1)) <= bound).all()
    assert (np.abs(b1 - a1) > 0).any(), "a clipped history's first moment must have moved somewhere"
    ch = f32(K.CLAMP["clipped_history"])
    assert (m1[..., 3][clipped] <= ch).all() and (m1[..., 3][clipped] == np.minimum(m0[..., 3][clipped], ch)).all()
    assert (m0[..., 3][clipped] > ch).any(), "the cap must bind somewhere"
    if subframes == 1:                            # through three cameras the counts are means of 12 taps: none is that low
        assert (m0[..., 3][clipped] < ch).any(), "and somewhere not"


def test_max_history_applies_after_the_clipped_cap(native_lib):
    _, m, found, clipped = _history_alone("pan", 1, 1, max_history=12.0)
    assert clipped.any() and (m[..., 3][found] <= f32(12)).all()
    _, m, found, clipped = _history_alone("pan", 1, 1, max_history=24.0)
    assert (m[..., 3][clipped] <= f32(16)).all() and (m[..., 3][found & ~clipped] > f32(16)).any()


def test_a_non_finite_neighbour_is_left_out_of_the_window(native_lib):
    """temporal_inputs plants a NaN and a +inf pixel in this frame's radiance:
    their neighbours' windows count one tap less and their boxes are finite."""
    rad = T.temporal_inputs(W, H, "pan")[2]
    bad = np.argwhere(~np.isfinite(rad[..., :3]).all(-1))
    assert len(bad) == 2
    for radius in (1, 2):
        n, lo, hi = clamp_box(rad, radius, 1.0)
        full = (2 * radius + 1) ** 2
        for y, x in bad:
            assert 2 * radius < y < H - 2 * radius and 2 * radius < x < W - 2 * radius
            win = (slice(y - radius, y + radius + 1), slice(x - radius, x + radius + 1))
            assert (n[win] == full - 1).all()
            assert np.isfinite(lo[win]).all() and np.isfinite(hi[win]).all()
        assert (n <= full).all() and (n == full).any()


def test_a_window_without_a_finite_tap_does_not_clamp(native_lib):
    a = T.temporal_inputs(W, H, "pan")
    rad = np.array(a[2])
    rad[4:11, 5:14, 0] = np.nan                   # 7 x 9 pixels: the inner 3 x 5 have no finite tap at radius 2
    for radius in (1, 2):
        n = clamp_box(rad, radius, 1.0)[0]
        empty = n == 0
        assert empty.sum() == (7 - 2 * radius) * (9 - 2 * radius)
        c0, m0, found0, _ = _history_alone("pan", 1, 0, rad=rad)
        c1, m1, found, clipped = _history_alone("pan", 1, radius, rad=rad)
        assert found[empty].any() and not clipped[empty].any() and clipped[~empty].any()
        assert T.same_bits(c1, c0)[empty].all() and T.same_bits(m1, m0)[empty].all()
        assert np.isfinite(c1[found]).all() and np.isfinite(m1[found]).all()


@pytest.mark.parametrize("subframes", K.SUBFRAMES)
@pytest.mark.parametrize("radius", (1, 2))
@pytest.mark.parametrize("case", ["same", "pan", "bigpan"])
def test_the_tests_sigma_runs_both_branches(native_lib, case, radius, subframes):
    """The clipped share among the pixels that found history lies strictly
    between 5% and 95%."""
    _, _, found, clipped = K.reference(W, H, case, subframes, radius)
    share = clipped[found].mean()
    print("%s, %d cameras, radius %d: %.1f%% found, %.1f%% of them clipped" % (case, subframes, radius, 100 * found.mean(),
                                                                              100 * share))
    assert found.mean() > 0.5 and 0.05 < share < 0.95


@pytest.mark.parametrize("case", ["pan", "bigpan"])
def test_more_cameras_find_no_less_history(native_lib, case):
    """Camera 0 of the list is the one-camera list, and every tap adds a
    positive weight: a pixel found through one camera is found through three."""
    one, three = K.reference(W, H, case, 1, 0), K.reference(W, H, case, 3, 0)
    assert not (one[2] & ~three[2]).any()
    assert not T.same_bits(one[0], three[0]).all(), "the other two cameras must have brought taps"


def test_cameras_are_counted_and_a_partial_history_is_refused(native_lib):
    a = T.temporal_inputs(5, 3, "pan")
    for cams in ([], [a[0]] * 513):
        with pytest.raises(ValueError, match="cameras"):
            temporal_clamped_reference(cams, *a[1:], params=K.params(1))
    with pytest.raises(ValueError):
        temporal_clamped_reference([a[0]], None, *a[2:], params=K.params(1))
    out = temporal_clamped_reference(np.stack([a[0]] * 512), *a[1:], params=K.params(1))
    assert out[0].shape == (3, 5, 4)


@pytest.mark.parametrize("field,value", [("clamp_radius", 3), ("clamp_sigma", 0.0), ("clamp_sigma", float("nan")),
                                         ("clamp_sigma", float("inf")), ("clipped_history", -1.0)])
def test_invalid_params_are_refused(native_lib, field, value):
    p = K.params(1)
    setattr(p, field, value)
    with pytest.raises(ValueError, match=field):
        p.validate()
    a = T.temporal_inputs(5, 3, "pan")
    with pytest.raises(ValueError, match=field):
        temporal_clamped_reference([a[0]], *a[1:], params=p)
    with pytest.raises(ValueError, match="max_history"):
        K.params(1, base=dict(max_history=0.0)).validate()
    with pytest.raises(TypeError):
        TemporalClampParams.default(iterations=3)


def test_the_library_defaults_are_valid(native_lib):
    from ptlumi.denoise import TemporalParams
    p = TemporalClampParams.default()
    p.validate()
    d = p.as_dict()
    assert sorted(d) == ["base", "clamp_radius", "clamp_sigma", "clipped_history"]
    assert d["base"] == TemporalParams.default().as_dict()
    assert p.clamp_radius in (1, 2)
    assert TemporalClampParams.default(clamp_radius=0).clamp_radius == 0


def test_blur_subframes_are_evenly_spaced():
    def pick(k, count):
        return TemporalDenoiser(None, None, blur_cameras=k).blur_subframes(count)

    assert [pick(1, s) for s in (1, 2, 3, 8)] == [[0], [1], [1], [4]]          # the middle subframe, as without the option
    assert pick(2, 2) == [0, 1] and pick(8, 2) == [0, 1] and pick(8, 1) == [0]
    assert pick(2, 8) == [2, 6] and pick(4, 8) == [1, 3, 5, 7] and pick(8, 8) == list(range(8))
    assert pick(3, 8) == [1, 4, 6]
    with pytest.raises(ValueError):
        TemporalDenoiser(None, None, blur_cameras=0)
    with pytest.raises(ValueError):
        TemporalDenoiser(None, None, temporal_params=object(), clamp_params=object())


@pytest.mark.parametrize("w,h,case,subframes,radius", K.ALL_CASES, ids=[K.case_key(*c) for c in K.ALL_CASES])
def test_reference_bits_are_the_pinned_ones(native_lib, w, h, case, subframes, radius):
    with open(PINNED) as f:
        pinned = json.load(f)["sha256"]
    assert K.reference_digest(w, h, case, subframes, radius) == pinned[K.case_key(w, h, case, subframes, radius)]


def test_every_pinned_case_is_checked():
    with open(PINNED) as f:
        assert sorted(json.load(f)["sha256"]) == sorted(K.case_key(*c) for c in K.ALL_CASES)


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    with open(PINNED, "w") as f:
        json.dump({"canonical_nan": "0x7fc00000", "sha256": {K.case_key(*c): K.reference_digest(*c) for c in K.ALL_CASES}}, f,
                  indent=1)
        f.write("\n")
