"""ptlumi.denoise.temporal_reference, the CPU restatement of
ptg_temporal_accumulate: its properties on the plane scene of
tests/temporal_inputs.py, and its bits, pinned as SHA-256 digests in
tests/golden/temporal_reference_bits.json so that a later change cannot move
the kernel and the restatement together.  No GPU work here.

`python tests/test_temporal_reference.py --write` records the digests of the
restatement as it stands (only for a deliberate change of the definition).
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
PINNED = os.path.join(HERE, "golden", "temporal_reference_bits.json")

if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (registers the package as `ptlumi`)

import temporal_inputs as T  # noqa: E402
from ptlumi.denoise import TemporalParams, temporal_reference  # noqa: E402

DIGEST_CASES = [(w, h, case) for (w, h) in T.SIZES for case in T.CASES]


def _run(w, h, case, tamper=True, found=None, **overrides):
    return temporal_reference(*T.temporal_inputs(w, h, case, tamper), params=T.params(**overrides), found=found)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("w,h", T.SIZES)
def test_without_history_the_outputs_are_the_input_bits(native_lib, w, h):
    cam, _, rad, mom, alb, nd = T.temporal_inputs(w, h, "pan")[:6]
    c, m = temporal_reference(cam, None, rad, mom, alb, nd, params=T.params())
    assert np.array_equal(_bits(c[..., :3]), _bits(rad[..., :3])) and (_bits(c[..., 3]) == 0).all()
    assert np.array_equal(_bits(m), _bits(mom))


def test_a_partial_history_is_refused(native_lib):
    a = T.temporal_inputs(5, 3, "pan")
    with pytest.raises(ValueError):
        temporal_reference(*a[:6], a[6], None, a[8], a[9], params=T.params())
    with pytest.raises(ValueError):
        temporal_reference(a[0], None, *a[2:], params=T.params())


@pytest.mark.parametrize("w,h", T.SIZES)
def test_a_history_camera_that_looks_away_gives_no_history(native_lib, w, h):
    rad, mom = T.temporal_inputs(w, h, "away")[2:4]
    found = np.ones((h, w), bool)
    c, m = _run(w, h, "away", found=found)
    assert not found.any()
    assert np.array_equal(_bits(c[..., :3]), _bits(rad[..., :3])) and (_bits(c[..., 3]) == 0).all()
    assert np.array_equal(_bits(m), _bits(mom))


@pytest.mark.parametrize("case", ["same", "pan", "bigpan"])
def test_most_pixels_find_history(native_lib, case):
    """What keeps the GPU comparison from passing on "no history" everywhere:
    on the untampered 37 x 23 inputs at least 90% of the pixels come out with
    more samples than the frame brought."""
    mom = T.temporal_inputs(37, 23, case, tamper=False)[3]
    _, m = _run(37, 23, case, tamper=False)
    share = float((m[..., 3] > mom[..., 3]).mean())
    print("%s: %.1f%% of the pixels found history" % (case, 100 * share))
    assert share >= 0.9


def test_the_same_camera_returns_a_noise_free_radiance(native_lib):
    """Radiance that is a function of the world point, the same in both
    frames: whatever the blend factor, the output is that radiance."""
    w, h = 37, 23
    cam, hcam, _, mom, alb, nd, _, hmom, halb, hnd = T.temporal_inputs(w, h, "same", tamper=False)
    pw = T.plane_hits(cam, w, h)[2]
    rad = np.zeros((h, w, 4), np.float32)
    rad[..., 0] = 0.8 + 0.1 * pw[..., 0]
    rad[..., 1] = 0.6 + 0.05 * pw[..., 1]
    rad[..., 2] = 0.7 + 0.02 * pw[..., 0] * pw[..., 1]
    found = np.zeros((h, w), bool)
    c, _ = temporal_reference(cam, hcam, rad, mom, alb, nd, rad, hmom, halb, hnd, params=T.params(), found=found)
    assert found.all()
    assert np.allclose(c[..., :3], rad[..., :3], rtol=1e-5, atol=0)


@pytest.mark.parametrize("case", ["pan", "bigpan"])
def test_a_pan_lands_on_the_same_world_point(native_lib, case):
    """Radiance 0.8 + 0.1 * world x in both frames, each through its own
    camera.  The valid taps lie in the 2 x 2 block of history pixels around
    the reprojected point and the function is monotone across the image, so
    the history differs from the pixel's own value by less than the widest
    range of such a block.  A reprojection that is off by more than a pixel,
    or mirrored, would miss this under the big pan, where the frames differ by more."""
    w, h = 37, 23
    cam, hcam, _, mom, alb, nd, _, hmom, halb, hnd = T.temporal_inputs(w, h, case, tamper=False)

    def image(c):
        rad = np.zeros((h, w, 4), np.float32)
        rad[..., :3] = (0.8 + 0.1 * T.plane_hits(c, w, h)[2][..., 0])[..., None]
        return rad

    cur, hist = image(cam), image(hcam)
    blocks = np.stack([hist[:-1, :-1, 0], hist[1:, :-1, 0], hist[:-1, 1:, 0], hist[1:, 1:, 0]])
    bound = float((blocks.max(0) - blocks.min(0)).max())
    found = np.zeros((h, w), bool)
    c, _ = temporal_reference(cam, hcam, cur, mom, alb, nd, hist, hmom, halb, hnd, params=T.params(), found=found)
    assert found.mean() >= 0.9
    err = float(np.abs(c[..., :3] - cur[..., :3])[found].max())
    print("%s: history off by %.4f at most, a block spans %.4f, the frames differ by %.4f" % (
        case, err, bound, np.abs(hist - cur).max()))
    assert err <= bound
    if case == "bigpan":
        assert np.abs(hist - cur).max() > 1.5 * bound, "the two frames must differ by more than the bound"


@pytest.mark.parametrize("case", ["same", "pan"])
def test_sample_counts_add_up_to_the_cap(native_lib, case):
    """nt = min(hn, max_history) + nc: hn is a weighted mean of the taps'
    counts (8 .. 100 here) and nc is 8."""
    w, h = 37, 23
    a = T.temporal_inputs(w, h, case, tamper=False)
    mom, hmom = a[3], a[7]
    found = np.zeros((h, w), bool)
    _, m = _run(w, h, case, tamper=False, found=found, max_history=20.0)
    nt = m[..., 3]
    assert found.any() and (nt[found] >= 16).all() and (nt[found] <= 28).all()
    assert np.array_equal(nt[~found], mom[..., 3][~found])
    if case == "same":
        # the point lands on its own pixel to a few ulp of a coordinate below 37 (2e-5 of a
        # pixel), so a neighbour with 12 times the count moves hn by less than 1e-3 relative
        assert np.allclose(nt, np.minimum(hmom[..., 3], np.float32(20)) + mom[..., 3], rtol=1e-3)
    _, mu = _run(w, h, case, tamper=False, max_history=1e6)
    assert (mu[..., 3][found] <= np.float32(108) * np.float32(1 + 1e-5)).all() and (mu[..., 3] >= nt).all()
    assert (mu[..., 3] > nt).any(), "the cap of 20 must have bound somewhere"


def test_a_nan_pixel_with_history_comes_out_finite(native_lib):
    w, h = 37, 23
    rad = T.temporal_inputs(w, h, "pan")[2]
    found = np.zeros((h, w), bool)
    c, m = _run(w, h, "pan", found=found)
    bad = ~np.isfinite(rad[..., :3]).all(-1)
    assert bad.sum() == 2 and found[bad].all(), "the NaN and the +inf pixel must lie where history is found"
    assert np.isfinite(c[bad]).all() and np.isfinite(m[bad]).all()
    assert np.isfinite(c[found]).all() and np.isfinite(m[found]).all(), "no non-finite history tap may be used"
    # the history's sample count alone, capped
    assert (m[bad][:, 3] <= np.float32(T.PARAMS["max_history"])).all()


def _far_from_the_band_edges(w, h, margin):
    pw = T.plane_hits(T.cameras(w, h, "pan")[0], w, h)[2]
    return np.all([np.abs(pw[..., 0] - e) > margin for e in T.BAND_EDGES], axis=0)


@pytest.mark.parametrize("field", ["normal_tolerance", "albedo_tolerance"])
def test_a_tight_guide_tolerance_removes_history_across_a_band_edge(native_lib, field):
    """Within a band the guides are equal bits, across an edge they differ:
    a tolerance of 1e-9 changes pixels next to an edge and no others.  At
    depth 5 a pixel is 0.25 world units wide and `pan` shifts the image by
    about a pixel, so pixels farther than 1 unit from both edges have all
    four taps in their own band."""
    w, h = 37, 23
    loose = _run(w, h, "pan", tamper=False)
    tight = _run(w, h, "pan", tamper=False, **{field: 1e-9})
    changed = ~(T.same_bits(loose[0], tight[0]).all(-1) & T.same_bits(loose[1], tight[1]).all(-1))
    assert changed.any()
    assert not (changed & _far_from_the_band_edges(w, h, 1.0)).any()


def test_a_tight_depth_tolerance_removes_history_under_a_pan(native_lib):
    """A tap's depth is that of the tap's own pixel, the expected depth that of
    the reprojected point between the taps: under a pan they differ by far
    more than 1e-9 relative."""
    w, h = 37, 23
    found = np.zeros((h, w), bool)
    _run(w, h, "pan", tamper=False, found=found)
    assert found.mean() >= 0.9
    _run(w, h, "pan", tamper=False, found=found, depth_tolerance=1e-9)
    assert found.mean() < 0.1


@pytest.mark.parametrize("field,value", [("max_history", 0.0), ("depth_tolerance", -1.0), ("normal_tolerance", float("nan")),
                                         ("albedo_tolerance", float("inf"))])
def test_invalid_params_are_refused(native_lib, field, value):
    with pytest.raises(ValueError, match=field):
        T.params(**{field: value}).validate()
    with pytest.raises(ValueError, match=field):
        _run(5, 3, "pan", **{field: value})
    with pytest.raises(TypeError):
        TemporalParams.default(iterations=3)


def test_the_library_defaults_are_valid(native_lib):
    p = TemporalParams.default()
    p.validate()
    assert sorted(p.as_dict()) == ["albedo_tolerance", "depth_tolerance", "max_history", "normal_tolerance"]


@pytest.mark.parametrize("w,h,case", DIGEST_CASES, ids=[T.case_key(*c) for c in DIGEST_CASES])
def test_reference_bits_are_the_pinned_ones(native_lib, w, h, case):
    with open(PINNED) as f:
        pinned = json.load(f)["sha256"]
    assert T.reference_digest(w, h, case) == pinned[T.case_key(w, h, case)]


def test_every_pinned_case_is_checked():
    with open(PINNED) as f:
        assert sorted(json.load(f)["sha256"]) == sorted(T.case_key(*c) for c in DIGEST_CASES)


if __name__ == "__main__" and sys.argv[1:] == ["--write"]:
    with open(PINNED, "w") as f:
        json.dump({"canonical_nan": "0x7fc00000", "sha256": {T.case_key(*c): T.reference_digest(*c) for c in DIGEST_CASES}}, f,
                  indent=1)
        f.write("\n")
