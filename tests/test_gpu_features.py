"""ptg_camera_rays and ptg_render_features against their CPU expectations
(tests/feature_helpers.py), bit for bit.

160x90, 16 spp (two motion-blur subframes), frames 0 and 450.  The camera
rays are compared with a float32 scalar restatement of the seed, the film
jitter and get_camera_ray; the feature buffers with: restated camera rays ->
the oracle's closest hit in each ray's subframe -> hit_info's interpolation in
NumPy float32 -> the ordered sum.
"""
import numpy as np
import pytest

from conftest import arrays_copy, scene_for
from oracle import Oracle

import feature_helpers as FH

W, H, SPP = 160, 90, 16
# 29 x 19 rectangles that hold geometry, sky and silhouette pixels
RECTS = {0: (60, 5, 29, 19), 450: (0, 0, 29, 19)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _pairs(frame):
    """64 (pixel, sample) pairs: the image corners, the subframe boundary
    (samples 7 and 8) and seeded random ones."""
    rng = np.random.default_rng(100 + frame)
    xy = np.stack([rng.integers(0, W, 64), rng.integers(0, H, 64)], 1).astype(np.uint32)
    js = rng.integers(0, SPP, 64).astype(np.int32)
    xy[0], xy[1], xy[2], xy[3] = (0, 0), (W - 1, H - 1), (0, 0), (W - 1, H - 1)
    js[0], js[1], js[2], js[3] = 7, 8, 8, 7
    js[4], js[5], js[6] = 0, SPP - 1, 7
    return xy, js


def _arrays(assets_dir, frame, hexagon):
    s = scene_for(assets_dir, W, H, SPP, frame=frame)
    arr = arrays_copy(s)
    if hexagon:
        cam = arr["subframes"]["cam"]
        cam["aperture_polygon"] = 6
        cam["aperture_radius"] = np.float32(0.05)
        cam["aperture_angle"] = np.float32(0.3)
    return s, arr


@pytest.mark.gpu
@pytest.mark.parametrize("hexagon", [False, True], ids=["scene_camera", "hexagon_aperture"])
@pytest.mark.parametrize("frame", [0, 450])
def test_camera_rays_match_the_restatement(gpu, assets_dir, frame, hexagon):
    s, arr = _arrays(assets_dir, frame, hexagon)
    gpu.upload_arrays(arr)
    xy, js = _pairs(frame)
    rays, sub = gpu.camera_rays(s.cfg, xy, js)
    want_rays, want_sub = FH.camera_rays(arr["subframes"], s.cfg, xy, js)
    assert np.array_equal(sub, want_sub)
    assert set(sub.tolist()) == {0, 1}
    if hexagon:
        # the aperture moves the origins off the camera position
        assert len(np.unique(want_rays[want_sub == 0, :3], axis=0)) > 1
    bad = np.nonzero((_bits(rays) != _bits(want_rays)).any(1))[0]
    assert len(bad) == 0, "frame %d: %d/64 rays differ, first: pixel %s sample %d got %s want %s" % (
        frame, len(bad), xy[bad[0]], js[bad[0]], rays[bad[0]], want_rays[bad[0]])
    assert (rays[:, 6] == 0).all() and (rays[:, 7] == np.float32(1e9)).all()


_expect = {}


def _per_sample(arr, cfg, frame):
    """Every sample's contribution over the frame's rectangle, computed once."""
    if frame not in _expect:
        _expect[frame] = FH.per_sample_features(arr, cfg, Oracle(arr, cfg), RECTS[frame], (0, SPP))
        _expect[frame].setflags(write=False)
    return _expect[frame]


@pytest.mark.gpu
@pytest.mark.parametrize("samples", [(0, SPP), (8, SPP)], ids=["all_samples", "samples_8_16"])
@pytest.mark.parametrize("frame", [0, 450])
def test_features_match_the_cpu_expectation(gpu, assets_dir, frame, samples):
    s, arr = _arrays(assets_dir, frame, False)
    gpu.upload_arrays(arr)
    rect = RECTS[frame]
    albedo, normal_depth = gpu.render_features(s.cfg, rect=rect, samples=samples)
    gpu.synchronize()
    ps = _per_sample(arr, s.cfg, frame)
    want_a, want_n = FH.fold_features(ps[:, samples[0]:samples[1]], s.cfg, (rect[3], rect[2]))
    # the expectation itself holds geometry, sky and partly covered pixels
    full = np.float32(samples[1] - samples[0]) / np.float32(SPP)
    cov = want_a[..., 3]
    assert (cov == full).any() and (cov == 0).any() and ((cov > 0) & (cov < full)).any()
    assert (want_a[cov == 0][:, :3] == full).all() and (want_n[cov == 0] == 0).all()
    assert (want_n[cov > 0][:, 3] > 0).all()
    got_a, got_n = albedo.cpu().numpy(), normal_depth.cpu().numpy()
    assert got_a.shape == (rect[3], rect[2], 4) and got_n.shape == (rect[3], rect[2], 4)
    for name, got, want in (("albedo+coverage", got_a, want_a), ("normal+depth", got_n, want_n)):
        bad = np.argwhere((_bits(got) != _bits(want)).any(-1))
        assert len(bad) == 0, "frame %d %s: %d/%d pixels differ, first (row, col) %s: got %s want %s" % (
            frame, name, len(bad), rect[2] * rect[3], bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.gpu
def test_features_argument_checks(gpu, assets_dir, native_lib):
    import ctypes as C
    s, arr = _arrays(assets_dir, 0, False)
    gpu.upload_arrays(arr)
    with pytest.raises(Exception, match="rectangle outside"):
        gpu.render_features(s.cfg, rect=(150, 0, 29, 19))
    with pytest.raises(Exception, match="subframes"):
        gpu.render_features(s.cfg, samples=(0, 4 * SPP))
    assert native_lib.ptg_render_features(gpu._ctx, C.byref(s.cfg), 0, 0, 4, 4, 0, SPP, None, None) == -1
