"""ptg_render_with_features: radiance, moments and first-hit features in one
pass.  Its definition is "as if ptg_render_moments and ptg_render_features
had been called", so every check is bit for bit: against the CPU expectations
of the two entries (tests/feature_helpers.py, ptlumi.denoise.moments_reference
over the oracle's samples) and against the two entries themselves, across
chunk borders, chunk sizes, concurrency levels and both pipelines, in the
counting build, and for the arguments it must refuse.
"""
import ctypes as C
import time

import numpy as np
import pytest

from conftest import N, arrays_copy, scene_for
from oracle import Oracle
from ptlumi.denoise import moments_reference

import feature_helpers as FH

pytestmark = pytest.mark.gpu

W, H, SPP = 160, 90, 16
# the 29 x 19 rectangles of tests/test_gpu_features.py: geometry, sky and silhouette pixels
RECTS = {0: (60, 5, 29, 19), 450: (0, 0, 29, 19)}
NAMES = ("bgra", "accum", "moments", "albedo+coverage", "normal+depth")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a if a.dtype == np.uint8 else a.view(np.uint32)


def _host(tensors):
    return [t.cpu().numpy() for t in tensors]


def _separate(gpu, cfg, rect=None, samples=None):
    """The two-call route, in the fused call's order of outputs."""
    bgra, acc, mom = gpu.render_moments(cfg, rect=rect, samples=samples, want_accum=True)
    alb, nd = gpu.render_features(cfg, rect=rect, samples=samples)
    gpu.synchronize()
    return _host((bgra, acc, mom, alb, nd))


def _fused(gpu, cfg, rect=None, samples=None):
    out = gpu.render_with_features(cfg, rect=rect, samples=samples)
    gpu.synchronize()
    return _host(out)


def _assert_same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name)
        differ = _bits(g) != _bits(w)
        if g.dtype == np.float32:   # two NaNs count as equal: x86 and gfx950 quiet NaNs differ in sign and payload
            differ &= ~(np.isnan(g) & np.isnan(w))
        bad = np.argwhere(differ.any(-1))
        assert len(bad) == 0, "%s, %s: %d/%d pixels differ, first (row, col) %s: got %s want %s" % (
            what, name, len(bad), g.shape[0] * g.shape[1], bad[0], g[tuple(bad[0])], w[tuple(bad[0])])


# ---- 2. bits against the CPU expectation ---------------------------------------

_expect = {}


def _expectation(assets_dir, frame):
    """(scene, arrays, per-sample features [h*w, 16, 8], the oracle's per-sample
    radiance [h*w, 16, 4]) over the frame's rectangle, computed once."""
    s = scene_for(assets_dir, W, H, SPP, frame=frame)
    if frame not in _expect:
        arr = arrays_copy(s)
        x0, y0, w, h = RECTS[frame]
        oracle = Oracle(arr, s.cfg)
        feats = FH.per_sample_features(arr, s.cfg, oracle, RECTS[frame], (0, SPP))
        ys, xs, js = np.meshgrid(np.arange(y0, y0 + h), np.arange(x0, x0 + w), np.arange(SPP), indexing="ij")
        rad = oracle.samples(np.stack([xs.ravel(), ys.ravel()], 1), js.ravel()).reshape(h * w, SPP, 4)
        for a in (feats, rad):
            a.setflags(write=False)
        _expect[frame] = (arr, feats, rad)
    return (s,) + _expect[frame]


@pytest.mark.parametrize("samples", [(0, SPP), (8, SPP)], ids=["all_samples", "samples_8_16"])
@pytest.mark.parametrize("frame", [0, 450])
def test_fused_outputs_match_the_cpu_expectation(gpu, assets_dir, frame, samples):
    s, arr, feats, rad = _expectation(assets_dir, frame)
    gpu.upload_arrays(arr)
    rect = RECTS[frame]
    h, w = rect[3], rect[2]
    j0, j1 = samples
    want_a, want_n = FH.fold_features(feats[:, j0:j1], s.cfg, (h, w))
    # the expectation itself holds geometry, sky and partly covered pixels
    full = np.float32(j1 - j0) / np.float32(SPP)
    cov = want_a[..., 3]
    assert (cov == full).any() and (cov == 0).any() and ((cov > 0) & (cov < full)).any()
    assert (want_a[cov == 0][:, :3] == full).all() and (want_n[cov == 0] == 0).all()
    assert (want_n[cov > 0][:, 3] > 0).all()
    want_m = moments_reference(rad[:, j0:j1]).reshape(h, w, 4)
    got = _fused(gpu, s.cfg, rect, samples)
    what = "frame %d samples %s" % (frame, samples)
    _assert_same(got[2:], [want_m, want_a, want_n], what + " against the CPU expectation")
    _assert_same(got, _separate(gpu, s.cfg, rect, samples), what + " against the separate entries")


def test_without_moments_the_radiance_is_ptg_renders(gpu, assets_dir):
    s, arr, _, _ = _expectation(assets_dir, 450)
    gpu.upload_arrays(arr)
    rect = RECTS[450]
    bgra, acc, mom, alb, nd = gpu.render_with_features(s.cfg, rect=rect, want_moments=False)
    bgra_r, acc_r = gpu.render(s.cfg, rect=rect, want_accum=True)
    alb_r, nd_r = gpu.render_features(s.cfg, rect=rect)
    gpu.synchronize()
    assert mom is None
    _assert_same(_host((bgra, acc, alb, nd)), _host((bgra_r, acc_r, alb_r, nd_r)), "want_moments=False")


# ---- 3. chunk borders, chunk sizes, concurrency levels, both pipelines ----------

def test_whole_image_in_two_chunks(gpu, assets_dir):
    """48x27x16 at the default concurrency: the span splits over the two chunk
    pipelines, so the eight feature sums cross a chunk border."""
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    _assert_same(_fused(gpu, s.cfg), _separate(gpu, s.cfg), "48x27x16")


def test_rectangle_off_the_origin_and_an_unaligned_sample_range(gpu, assets_dir):
    """Samples 3..20 of 24 fold as 16 + 2; seven bounces."""
    rect, samples = (7, 3, 31, 19), (3, 21)
    s = scene_for(assets_dir, 41, 23, 24, bounces=7, frame=1750)
    gpu.upload_arrays(arrays_copy(s))
    _assert_same(_fused(gpu, s.cfg, rect, samples), _separate(gpu, s.cfg, rect, samples), "41x23 %s %s" % (rect, samples))


@pytest.mark.parametrize("bounces", [0, 4])
def test_several_chunks_per_slot(gpu, assets_dir, bounces):
    """64x36x64 in chunks of at most 2^16 paths: several chunks per slot, so a
    slot's next camera runs beside a round that stores features (with no
    bounce, round 0 is that last round) and a slot's feature buffer is reused."""
    s = scene_for(assets_dir, 64, 36, 64, frame=450)
    cfg = N.RenderConfig.make(64, 36, 64, bounces)
    gpu.upload_arrays(arrays_copy(s))
    want = _separate(gpu, cfg)
    try:
        gpu.set_chunk_paths(16)
        got = _fused(gpu, cfg)
    finally:
        gpu.set_chunk_paths(27)
    _assert_same(got, want, "64x36x64, %d bounces, 2^16-path chunks" % bounces)


def test_every_concurrency_level_and_the_megakernel(gpu, assets_dir):
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    want = _separate(gpu, s.cfg)
    got = {}
    try:
        for level in (0, 1, 2):
            gpu.set_concurrency(level)
            got["concurrency %d" % level] = _fused(gpu, s.cfg)
        gpu.set_pipeline("megakernel")
        got["megakernel"] = _fused(gpu, s.cfg)
    finally:
        gpu.set_pipeline("wavefront")
        gpu.set_concurrency(2)
    for what, g in got.items():
        _assert_same(g, want, what)


# ---- 4. counting build ---------------------------------------------------------

def test_counting_build_same_bits_and_no_walk_of_its_own(gpu, assets_dir):
    """The counting twins give the same bits, and the fused render's samples,
    node visits, ray queries and shades and its closest-hit walk launches are
    render_moments': it walks no primary ray a second time."""
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    want = _separate(gpu, s.cfg)
    try:
        gpu.enable_counters(True)
        gpu.enable_timing(True)
        gpu.render_moments(s.cfg, want_accum=True)
        gpu.synchronize()
        cnt_m, extend_m = gpu.counters(), gpu.kernel_times()["extend"][1]
        got = _fused(gpu, s.cfg)
        cnt_f, extend_f = gpu.counters(), gpu.kernel_times()["extend"][1]
    finally:
        gpu.enable_timing(False)
        gpu.enable_counters(False)
    _assert_same(got, want, "counting build")
    assert cnt_m[0] == 48 * 27 * 16 and cnt_m[4] > cnt_m[0] and cnt_m[5] > 0
    for k in (0, 1, 4, 5):
        assert cnt_f[k] == cnt_m[k], "counter %d: fused %d, render_moments %d" % (k, cnt_f[k], cnt_m[k])
    assert extend_f == extend_m > 0


# ---- 6. argument checks ----------------------------------------------------------

def test_argument_checks_write_nothing(gpu, assets_dir, native_lib):
    import torch
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    dev = torch.device("cuda", gpu.device)
    acc, mom, alb, nd = (torch.full((27, 48, 4), -7.0, dtype=torch.float32, device=dev) for _ in range(4))
    bgra = torch.full((27, 48, 4), 93, dtype=torch.uint8, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(rect, samples, outs):
        return native_lib.ptg_render_with_features(gpu._ctx, C.byref(s.cfg), *rect, *samples, *outs)
    whole, all_samples = (0, 0, 48, 27), (0, 16)
    ok = (p(acc), p(bgra), p(mom), p(alb), p(nd))
    assert call(whole, all_samples, ok[:3] + (None, p(nd))) == -1          # PTG_E_INVALID
    assert b"null feature output" in native_lib.ptg_last_error()
    assert call(whole, all_samples, ok[:4] + (None,)) == -1
    assert call(whole, all_samples, (p(acc), p(bgra), p(mom), p(alb), p(alb))) == -1
    assert b"same buffer" in native_lib.ptg_last_error()
    assert call(whole, all_samples, (p(acc), p(bgra), p(alb), p(alb), p(nd))) == -1
    assert call(whole, all_samples, (p(nd), p(bgra), p(mom), p(alb), p(nd))) == -1
    assert call((40, 0, 29, 19), all_samples, ok) != 0
    assert b"rectangle outside" in native_lib.ptg_last_error()
    assert call(whole, (0, 64), ok) != 0
    assert b"subframes" in native_lib.ptg_last_error()
    assert call(whole, (8, 8), ok) == -1
    gpu.synchronize()
    for t in (acc, mom, alb, nd):
        assert (t == -7.0).all().item()
    assert (bgra == 93).all().item()
    # the optional outputs may all be absent
    assert call(whole, all_samples, (None, None, None, p(alb), p(nd))) == 0
    alb_r, nd_r = gpu.render_features(s.cfg)
    gpu.synchronize()
    _assert_same(_host((alb, nd)), _host((alb_r, nd_r)), "features alone")
    assert (acc == -7.0).all().item() and (mom == -7.0).all().item() and (bgra == 93).all().item()


# ---- 7. time -------------------------------------------------------------------

def test_fused_pass_saves_the_second_walk(gpu, assets_dir):
    """Frame 450 at 320x180x64, synchronised wall time after one warm-up each,
    median of 5: the fused call must beat render_moments + render_features by
    at least half of the feature pass's time (DESIGN.md 4.13's habit: assert
    half of a measured gain on a shared machine).  The two separate entries
    are the parent's unchanged code, so they are the yardstick.

    Measured on an MI355X (two repetitions in one process, ms): render_moments
    12.26 / 12.31, render_features 3.69 / 3.68, render_with_features 12.36 /
    12.27: the saving is 0.97 / 1.01 of the feature pass, so the bound holds
    with 1.7 ms to spare.  (160x90x64: 4.70, 3.04, 4.73; 640x360x64: 42.94,
    11.11, 42.97.)"""
    s = scene_for(assets_dir, 320, 180, 64, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    cfg = s.cfg

    def median_ms(fn):
        fn()
        gpu.synchronize()
        ts = []
        for _ in range(5):
            t = time.perf_counter()
            fn()
            gpu.synchronize()
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts))
    t_moments = median_ms(lambda: gpu.render_moments(cfg, want_accum=True))
    t_features = median_ms(lambda: gpu.render_features(cfg))
    t_fused = median_ms(lambda: gpu.render_with_features(cfg))
    print("320x180x64 frame 450: render_moments %.3f ms, render_features %.3f ms, render_with_features %.3f ms"
          % (t_moments, t_features, t_fused))
    assert t_fused < t_moments + 0.5 * t_features, (t_moments, t_features, t_fused)
