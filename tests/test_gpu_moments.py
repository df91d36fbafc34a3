"""ptg_render_moments against its definition: ptlumi.denoise.moments_reference
over the oracle's per-sample radiance, bit for bit; its radiance and BGRA
outputs against ptg_render's for the same call."""
import numpy as np
import pytest

from conftest import arrays_copy, scene_for
from oracle import Oracle
from ptlumi.denoise import moments_reference

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    """Equal bit patterns; two NaNs count as equal (x86 and gfx950 quiet NaNs
    carry different sign and payload bits)."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))


def _oracle_samples(arr, cfg, rect, samples):
    """[h, w, n, 4]: the oracle's path_trace_pixel of every (pixel, sample)."""
    x0, y0, w, h = rect
    j0, j1 = samples
    ys, xs, js = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), np.arange(j0, j1), indexing="ij")
    out = Oracle(arr, cfg).samples(np.stack([xs.ravel(), ys.ravel()], 1), js.ravel())
    return out.reshape(h, w, j1 - j0, 4)


def _expected(per_sample):
    h, w, n = per_sample.shape[:3]
    want = moments_reference(per_sample.reshape(h * w, n, 4)).reshape(h, w, 4)
    want.setflags(write=False)
    return want


def _assert_moments(got, want, what):
    got = got.cpu().numpy()
    bad = np.argwhere(~_same_bits(got, want).all(-1))
    assert len(bad) == 0, "%s: %d pixels differ, first (row, col) %s: got %s want %s" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


_reference = {}


def _frame450(assets_dir):
    """48x27x16 spp, frame 450: the arrays and the expected moments, computed once."""
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    if "f450" not in _reference:
        arr = arrays_copy(s)
        _reference["f450"] = (arr, _expected(_oracle_samples(arr, s.cfg, (0, 0, 48, 27), (0, 16))))
    return (s,) + _reference["f450"]


def test_moments_of_a_whole_image_in_two_chunks(gpu, assets_dir):
    """A span of 16 samples is split over both chunk pipelines at the default
    concurrency, so the running sums cross a chunk border."""
    s, arr, want = _frame450(assets_dir)
    gpu.upload_arrays(arr)
    bgra, acc, mom = gpu.render_moments(s.cfg, want_accum=True)
    bgra_r, acc_r = gpu.render(s.cfg, want_accum=True)
    gpu.synchronize()
    _assert_moments(mom, want, "48x27x16")
    assert (want[..., 3] == 16).all() and (want[..., 2] > 0).any()
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_r.cpu().numpy()))
    assert np.array_equal(bgra.cpu().numpy(), bgra_r.cpu().numpy())


def test_moments_of_a_rectangle_and_an_unaligned_sample_range(gpu, assets_dir):
    """A rectangle off the origin and samples 3..20 of 24, which fold as 16 + 2;
    the moments are normalised by the 18 samples rendered, the radiance by 24."""
    rect, samples = (7, 3, 31, 19), (3, 21)
    s = scene_for(assets_dir, 41, 23, 24, bounces=7, frame=1750)
    arr = arrays_copy(s)
    gpu.upload_arrays(arr)
    bgra, acc, mom = gpu.render_moments(s.cfg, rect=rect, samples=samples, want_accum=True)
    bgra_r, acc_r = gpu.render(s.cfg, rect=rect, samples=samples, want_accum=True)
    gpu.synchronize()
    want = _expected(_oracle_samples(arr, s.cfg, rect, samples))
    assert (want[..., 3] == 18).all()
    _assert_moments(mom, want, "41x23 rect %s samples %s" % (rect, samples))
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_r.cpu().numpy()))
    assert np.array_equal(bgra.cpu().numpy(), bgra_r.cpu().numpy())


def test_moments_are_the_same_in_every_pipeline(gpu, assets_dir):
    s, arr, want = _frame450(assets_dir)
    gpu.upload_arrays(arr)
    try:
        gpu.set_pipeline("megakernel")
        _, _, mega = gpu.render_moments(s.cfg)
        gpu.set_pipeline("wavefront")
        gpu.set_concurrency(0)
        _, _, serial = gpu.render_moments(s.cfg)
        gpu.synchronize()
    finally:
        gpu.set_pipeline("wavefront")
        gpu.set_concurrency(2)
    _assert_moments(mega, want, "megakernel")
    _assert_moments(serial, want, "concurrency 0")


def test_one_sample_has_no_variance(gpu, assets_dir):
    s = scene_for(assets_dir, 33, 17, 1, frame=0)
    arr = arrays_copy(s)
    gpu.upload_arrays(arr)
    _, _, mom = gpu.render_moments(s.cfg)
    gpu.synchronize()
    per_sample = _oracle_samples(arr, s.cfg, (0, 0, 33, 17), (0, 1))
    want = _expected(per_sample)
    _assert_moments(mom, want, "33x17x1")
    finite = np.isfinite(per_sample[:, :, 0, :3]).all(-1)
    got = mom.cpu().numpy()
    assert finite.any()
    assert (got[finite][:, 2] == 0).all() and (got[finite][:, 3] == 1).all()


def test_non_finite_samples_are_left_out_of_the_moments(gpu, assets_dir):
    """Subframe 1 (samples 8-15) gets a light colour of (NaN, 4, 4): the
    pixels it lights have fewer than 16 finite samples."""
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    arr = arrays_copy(s)
    arr["subframes"]["light"]["color"][1, :3] = np.array((np.nan, 4.0, 4.0), np.float32)
    per_sample = _oracle_samples(arr, s.cfg, (0, 0, 48, 27), (0, 16))
    n = np.isfinite(per_sample[..., :3]).all(-1).sum(-1)
    assert ((n > 0) & (n < 16)).any(), "the oracle has no pixel with some but not all samples finite"
    want = _expected(per_sample)
    assert np.array_equal(want[..., 3], n.astype(np.float32))
    gpu.upload_arrays(arr)
    bgra, acc, mom = gpu.render_moments(s.cfg, want_accum=True)
    bgra_r, acc_r = gpu.render(s.cfg, want_accum=True)
    gpu.synchronize()
    _assert_moments(mom, want, "NaN light in subframe 1")
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_r.cpu().numpy()))
    assert np.array_equal(bgra.cpu().numpy(), bgra_r.cpu().numpy())


def test_null_out_moments_is_refused(gpu, assets_dir):
    import ctypes as C
    from ptlumi import native as N
    s, arr, _ = _frame450(assets_dir)
    gpu.upload_arrays(arr)
    assert N.lib().ptg_render_moments(gpu._ctx, C.byref(s.cfg), 0, 0, 48, 27, 0, 16, None, None, None) == -1
    assert b"out_moments" in N.lib().ptg_last_error()
