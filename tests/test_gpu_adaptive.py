"""ptg_render_adaptive against its definition: ptlumi.adaptive.adaptive_reference
over the oracle's per-sample radiance, bit for bit (radiance, BGRA, moments,
sample counts and the active count of every pass), on cases whose later passes
are real, ragged pixel lists; then the entry's other promises."""
import ctypes as C

import numpy as np
import pytest

from adaptive_inputs import GPU_CASES, params_of
from conftest import arrays_copy, scene_for
from oracle import Oracle, tonemap
from ptlumi import native as N
from ptlumi.adaptive import adaptive_reference

pytestmark = pytest.mark.gpu

FLOOR = 0.01


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(got, want):
    """Equal bit patterns; two NaNs count as equal (x86 and gfx950 quiet NaNs
    carry different sign and payload bits)."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (_bits(g) == _bits(w)) | (np.isnan(g) & np.isnan(w))


def _oracle_samples(arr, cfg, w, h, n):
    """[h, w, n, 4]: the oracle's path_trace_pixel of every (pixel, sample) of the image."""
    ys, xs, js = np.meshgrid(np.arange(h), np.arange(w), np.arange(n), indexing="ij")
    out = Oracle(arr, cfg).samples(np.stack([xs.ravel(), ys.ravel()], 1), js.ravel())
    out = out.reshape(h, w, n, 4)
    out.setflags(write=False)
    return out


_scenes = {}
_cases = {}


def _scene(assets_dir, w, h, n, bounces, frame, m):
    if m == 8:
        return scene_for(assets_dir, w, h, n, bounces=bounces, frame=frame)
    key = (w, h, n, bounces, m)
    if key not in _scenes:
        _scenes[key] = N.Scene(assets_dir, N.RenderConfig.make(w, h, n, bounces, blur_step=m))
    s = _scenes[key]
    if s.frame != frame:
        s.setup_frame(frame)
    return s


def _case(assets_dir, name):
    """(scene, arrays, per-sample radiance of the whole image, params) of a
    GPU_CASES row; the arrays and the oracle's samples are computed once."""
    row = [c for c in GPU_CASES if c[0] == name][0]
    _, w, h, n, bounces, frame, m, passes, dilate, threshold = row
    s = _scene(assets_dir, w, h, n, bounces, frame, m)
    if name not in _cases:
        arr = arrays_copy(s)
        _cases[name] = (arr, _oracle_samples(arr, s.cfg, w, h, n))
    arr, per_sample = _cases[name]
    return s, arr, per_sample, params_of(passes, 1, dilate, threshold, FLOOR)


def _expected(per_sample, m, params):
    """The restatement's outputs plus the BGRA of its radiance."""
    acc, mom, ns, active = adaptive_reference(per_sample, m, params)
    h, w = ns.shape
    return acc, tonemap(acc.reshape(h * w, 4)).reshape(h, w, 4), mom, ns, active


def _assert_ragged(active, npix):
    """Every pass after the first has between 5% and 95% of the pixels active:
    the lists are real and ragged (from the restatement alone)."""
    assert len(active) >= 2 and active[0] == npix, active
    for a in active[1:]:
        assert 0.05 * npix <= a <= 0.95 * npix, (active, npix)


def _assert_outputs(gpu, got, want, what):
    bgra, acc, mom, ns = (t.cpu().numpy() for t in got)
    w_acc, w_bgra, w_mom, w_ns, w_active = want
    active = gpu.adaptive_stats()
    print("%s: active per pass %s of %d pixels" % (what, w_active, w_ns.size))
    assert active == w_active, "%s: active counts %s, want %s" % (what, active, w_active)
    assert np.array_equal(ns.view(np.uint32), w_ns), "%s: %d sample counts differ" % (what, (ns.view(np.uint32) != w_ns).sum())
    for name, g, w in (("radiance", acc, w_acc), ("moments", mom, w_mom)):
        bad = np.argwhere(~_same_bits(g, w).all(-1))
        assert len(bad) == 0, "%s %s: %d pixels differ, first (row, col) %s: got %s want %s" % (
            what, name, len(bad), bad[0], g[tuple(bad[0])], w[tuple(bad[0])])
    assert np.array_equal(bgra, w_bgra), "%s: tonemapped bytes differ" % what


@pytest.mark.parametrize("name", [c[0] for c in GPU_CASES])
def test_adaptive_render_is_the_restatement_bit_for_bit(gpu, assets_dir, name):
    s, arr, per_sample, params = _case(assets_dir, name)
    want = _expected(per_sample, s.cfg.samples_per_motion_blur_step, params)
    _assert_ragged(want[4], s.cfg.width * s.cfg.height)
    if name == "f0_reawakening":
        assert any(b > a for a, b in zip(want[4][1:], want[4][2:])), want[4]   # the count rises again
    gpu.upload_arrays(arr)
    got = gpu.render_adaptive(s.cfg, params)
    gpu.synchronize()
    _assert_outputs(gpu, got, want, name)


def test_a_rectangle_off_the_origin_with_odd_sizes(gpu, assets_dir):
    """The window is clipped to the rectangle, not to the image: the
    restatement sees the rectangle's samples alone.  The threshold is the first
    of a fixed list that leaves every later pass 5%-95% of the rectangle."""
    x0, y0, w, h = rect = (7, 3, 31, 19)
    s, arr, per_sample, params = _case(assets_dir, "f1750_p3")
    sub = per_sample[y0:y0 + h, x0:x0 + w]
    want = None
    for threshold in (0.05, 0.1, 0.03, 0.2, 0.02, 0.4):
        params.threshold = threshold
        want = _expected(sub, 8, params)
        if len(want[4]) >= 2 and all(0.05 * w * h <= a <= 0.95 * w * h for a in want[4][1:]):
            break
    _assert_ragged(want[4], w * h)
    gpu.upload_arrays(arr)
    got = gpu.render_adaptive(s.cfg, params, rect=rect)
    gpu.synchronize()
    _assert_outputs(gpu, got, want, "rect %s threshold %g" % (rect, params.threshold))


def test_one_pass_is_render_moments(gpu, assets_dir):
    s, arr, _, _ = _case(assets_dir, "f450_p4")
    gpu.upload_arrays(arr)
    bgra, acc, mom, ns = gpu.render_adaptive(s.cfg, params_of(1, 1, 1, 0.05, FLOOR))
    bgra_r, acc_r, mom_r = gpu.render_moments(s.cfg, want_accum=True)
    gpu.synchronize()
    assert np.array_equal(_bits(acc.cpu().numpy()), _bits(acc_r.cpu().numpy()))
    assert np.array_equal(_bits(mom.cpu().numpy()), _bits(mom_r.cpu().numpy()))
    assert np.array_equal(bgra.cpu().numpy(), bgra_r.cpu().numpy())
    assert (ns.cpu().numpy() == 64).all() and gpu.adaptive_stats() == [48 * 27]


def test_a_huge_threshold_stops_everything_after_min_passes(gpu, assets_dir):
    s, arr, per_sample, _ = _case(assets_dir, "f450_p4")
    finite = np.isfinite(per_sample[..., :3]).all()
    assert finite, "a pixel without finite samples would stay active"
    gpu.upload_arrays(arr)
    _, _, _, ns = gpu.render_adaptive(s.cfg, params_of(4, 2, 1, 1e30, FLOOR))
    gpu.synchronize()
    assert gpu.adaptive_stats() == [48 * 27, 48 * 27]      # passes_run == 2
    assert (ns.cpu().numpy() == 2 * 64 // 4).all()


def test_every_concurrency_level_gives_the_same_bits(gpu, assets_dir):
    """f450_p4: a pass is 16 samples, which the default level splits over both
    chunk pipelines (the parametrised test above ran at that level)."""
    s, arr, per_sample, params = _case(assets_dir, "f450_p4")
    want = _expected(per_sample, 8, params)
    gpu.upload_arrays(arr)
    try:
        for level in (0, 1, 2):
            gpu.set_concurrency(level)
            got = gpu.render_adaptive(s.cfg, params)
            gpu.synchronize()
            _assert_outputs(gpu, got, want, "concurrency %d" % level)
    finally:
        gpu.set_concurrency(2)


def test_pixels_with_fewer_than_two_finite_samples_stay_active(gpu, assets_dir):
    """Subframe 0 - pass 0 of 4 - gets a light colour of (NaN, 4, 4).  With a
    threshold nothing else misses, pass 1 is exactly the pixels that have
    fewer than 2 finite samples after pass 0; they then have 8 and stop."""
    s = scene_for(assets_dir, 48, 27, 32, frame=450)
    arr = arrays_copy(s)
    arr["subframes"]["light"]["color"][0, :3] = np.array((np.nan, 4.0, 4.0), np.float32)
    per_sample = _oracle_samples(arr, s.cfg, 48, 27, 32)
    few = np.isfinite(per_sample[:, :, :8, :3]).all(-1).sum(-1) < 2
    assert 0 < few.sum() < few.size, "the oracle has no pixel the NaN light leaves with fewer than 2 finite samples"
    params = params_of(4, 1, 0, 1e30, FLOOR)
    want = _expected(per_sample, 8, params)
    assert want[4] == [48 * 27, int(few.sum())]
    assert np.array_equal(want[3] == 16, few)
    gpu.upload_arrays(arr)
    got = gpu.render_adaptive(s.cfg, params)
    gpu.synchronize()
    _assert_outputs(gpu, got, want, "NaN light in subframe 0")
    assert np.array_equal(got[3].cpu().numpy() == 16, few)


def test_render_is_untouched_by_an_adaptive_call(gpu, assets_dir):
    s, arr, _, params = _case(assets_dir, "f450_p4")
    gpu.upload_arrays(arr)
    bgra0, acc0 = gpu.render(s.cfg, want_accum=True)
    gpu.render_adaptive(s.cfg, params)
    bgra1, acc1 = gpu.render(s.cfg, want_accum=True)
    gpu.synchronize()
    assert np.array_equal(_bits(acc0.cpu().numpy()), _bits(acc1.cpu().numpy()))
    assert np.array_equal(bgra0.cpu().numpy(), bgra1.cpu().numpy())


def test_invalid_calls_are_refused_with_a_message(gpu, assets_dir):
    import torch
    s, arr, _, _ = _case(assets_dir, "f450_p4")           # N = 64, m = 8
    gpu.upload_arrays(arr)
    L = N.lib()
    out = torch.empty((27, 48, 4), dtype=torch.float32, device="cuda:%d" % gpu.device)

    def call(p, accum=out, cfg=s.cfg):
        return L.ptg_render_adaptive(gpu._ctx, C.byref(cfg), 0, 0, 48, 27, C.byref(p) if p is not None else None,
                                     C.c_void_p(accum.data_ptr()) if accum is not None else None, None, None, None)

    good = (4, 1, 1, 0.05, FLOOR)
    assert call(params_of(*good)) == 0
    bad = [(0, 1, 1, 0.05, FLOOR), (4, 0, 1, 0.05, FLOOR), (4, 5, 1, 0.05, FLOOR), (17, 1, 1, 0.05, FLOOR),
           (4, 1, 3, 0.05, FLOOR), (4, 1, 1, 0.0, FLOOR), (4, 1, 1, -1.0, FLOOR), (4, 1, 1, float("nan"), FLOOR),
           (4, 1, 1, float("inf"), FLOOR), (4, 1, 1, 0.05, 0.0), (4, 1, 1, 0.05, float("inf")),
           (3, 1, 1, 0.05, FLOOR), (16, 1, 1, 0.05, FLOOR)]          # 64 is no multiple of 3 * 8 or 16 * 8
    for b in bad:
        L.ptg_render(None, None, 0, 0, 0, 0, 0, 0, None, None)      # sets another message
        assert call(params_of(*b)) == -1, b
        assert b"ptg_render_adaptive" in L.ptg_last_error(), (b, L.ptg_last_error())
    assert call(None) == -1 and b"params" in L.ptg_last_error()
    assert call(params_of(*good), accum=None) == -1 and b"no output" in L.ptg_last_error()
    try:
        gpu.set_pipeline("megakernel")
        assert call(params_of(*good)) == -1
        assert b"wavefront" in L.ptg_last_error()
    finally:
        gpu.set_pipeline("wavefront")
    assert call(params_of(*good)) == 0
    gpu.synchronize()


def test_the_denoiser_and_the_temporal_step_take_adaptive_moments(gpu, assets_dir):
    """passes = 1 is render_moments, so the composed calls give the bits of
    their render_moments versions; a real adaptive render goes through both
    with a sample count that varies per pixel."""
    from ptlumi.renderer import TemporalDenoiser
    s, arr, _, params = _case(assets_dir, "f450_p4")
    one = params_of(1, 1, 1, 0.05, FLOOR)
    gpu.upload(s, include_static=True)
    bgra_a, out_a = gpu.render_adaptive_denoised(s.cfg, one)
    bgra_g, out_g = gpu.render_denoised_guided(s.cfg)
    gpu.synchronize()
    assert np.array_equal(_bits(out_a.cpu().numpy()), _bits(out_g.cpu().numpy()))
    assert np.array_equal(bgra_a.cpu().numpy(), bgra_g.cpu().numpy())
    plain = TemporalDenoiser(gpu, s.cfg).step(s)[1].cpu().numpy()
    same = TemporalDenoiser(gpu, s.cfg, adaptive_params=one).step(s)[1].cpu().numpy()
    assert np.array_equal(_bits(plain), _bits(same))
    td = TemporalDenoiser(gpu, s.cfg, adaptive_params=params)
    td.step(s)
    out = td.step(s)[1].cpu().numpy()
    n = td.history[2].cpu().numpy()[..., 3]
    assert np.isfinite(out).all() and len(np.unique(n)) > 1


def test_adaptive_beats_uniform_sampling_of_the_same_cost_on_frame_0(gpu, assets_dir):
    """Frame 0 at 160 x 90 with a budget of 64 and the default parameters,
    against this renderer's own 256-spp render (validator PSNR, no downscale),
    beside ptg_render at the smallest multiple of 8 spp that takes at least as
    many samples, on a scene set up for that count.
    Measured on one MI355X (threshold 0.025, dilate 2): 33% of the pixels stay
    active after the first pass and 30% after the others, 39% of the budget
    is taken; adaptive 36.93 dB,
    uniform at 32 spp 33.18 dB, a gain of 3.75 dB; half of it is asserted."""
    from ptlumi import validator as V
    from ptlumi.adaptive import AdaptiveParams
    w, h, budget = 160, 90, 64

    def rgb(spp, adaptive):
        s = scene_for(assets_dir, w, h, spp, frame=0)
        gpu.upload_arrays(arrays_copy(s))
        bgra = gpu.render_adaptive(s.cfg, AdaptiveParams.default())[0] if adaptive else gpu.render(s.cfg)[0]
        gpu.synchronize()
        return V.bgra_to_rgb(bgra.cpu().numpy())

    ref = rgb(256, False)
    own = rgb(budget, True)
    active = gpu.adaptive_stats()
    taken = sum(active) * (budget // AdaptiveParams.default().passes)
    spp = max(8, -(-taken // (8 * w * h)) * 8)
    assert spp < budget, "the adaptive render took the whole budget: %s" % active
    p_adaptive, p_uniform = V.psnr(ref, own), V.psnr(ref, rgb(spp, False))
    print("frame 0 160x90 budget 64 vs 256 spp: %d samples, adaptive %.2f dB, uniform at %d spp %.2f dB" % (
        taken, p_adaptive, spp, p_uniform))
    assert p_adaptive > p_uniform + HALF_OF_THE_MEASURED_GAIN, "%.2f dB against %.2f dB" % (p_adaptive, p_uniform)


# half of the gain measured on one MI355X (the test's docstring), in dB
HALF_OF_THE_MEASURED_GAIN = 1.87


def test_counting_and_timing_cover_the_adaptive_launches(gpu, assets_dir):
    """The counting instantiations give the same bits and count the samples
    taken; the timing record holds a camera launch per chunk and a fold each."""
    s, arr, per_sample, params = _case(assets_dir, "f450_p4")
    want = _expected(per_sample, 8, params)
    gpu.upload_arrays(arr)
    try:
        gpu.enable_counters(True)
        gpu.enable_timing(True)
        got = gpu.render_adaptive(s.cfg, params)
        gpu.synchronize()
        _assert_outputs(gpu, got, want, "counting")
        assert int(gpu.counters()[0]) == sum(want[4]) * (64 // 4)
        times = gpu.kernel_times()
        chunks = 2 * len(want[4])                          # a pass of 16 samples is two chunks
        assert times["camera"][1] == chunks and times["accumulate"][1] == chunks
    finally:
        gpu.enable_counters(False)
        gpu.enable_timing(False)
