"""ptg_temporal_accumulate_clamped against its CPU restatement
(ptlumi.denoise.temporal_clamped_reference), bit for bit, on the seeded plane
scene of tests/temporal_clamp_inputs.py and on two rendered frames; against
ptg_temporal_accumulate where the two are one definition; its contract; the
TemporalDenoiser options that reach it; and what it does to frame 450, the
first frame of a fast zoom, end to end."""
import ctypes as C

import numpy as np
import pytest

import temporal_clamp_inputs as K
import temporal_inputs as T
from conftest import arrays_copy, scene_for
from ptlumi import native as N
from ptlumi import validator as V
from ptlumi.denoise import TemporalClampParams, temporal_clamped_reference
from ptlumi.renderer import GpuRenderer, TemporalDenoiser

pytestmark = pytest.mark.gpu


def _device(arrays):
    import torch
    return [torch.from_numpy(np.array(a)).to("cuda:0") for a in arrays]


def _run(gpu, w, h, case, subframes, radius, alias_radiance=False, alias_moments=False, sync=True):
    a = T.temporal_inputs(w, h, case)
    d = _device(a[2:])
    out = gpu.temporal_accumulate_clamped(K.camera_list(w, h, case, subframes), *d[:4], history=(a[1],) + tuple(d[4:]),
                                          params=K.params(radius), want_bgra=True, want_flags=True,
                                          out_radiance=d[0] if alias_radiance else None,
                                          out_moments=d[1] if alias_moments else None)
    if sync:
        gpu.synchronize()
    assert not alias_radiance or out[0].data_ptr() == d[0].data_ptr()
    assert not alias_moments or out[1].data_ptr() == d[1].data_ptr()
    return out


def _assert_same(got, want, what):
    same = T.same_bits(got, want).all(-1)
    bad = np.argwhere(~same)
    assert len(bad) == 0, "%s: %d pixels differ, first (row, col) %s: got %s want %s" % (
        what, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


def _assert_matches(gpu, out, want, what):
    """out: the wrapper's (radiance, moments, bgra, flags) after a synchronize;
    want: (radiance, moments, found, clipped) of the restatement."""
    import torch
    rad, mom, bgra, flags = out
    _assert_same(rad.cpu().numpy(), want[0], what + " out_radiance")
    _assert_same(mom.cpu().numpy(), want[1], what + " out_moments")
    assert (rad.cpu().numpy()[..., 3] == 0).all()
    found, clipped = GpuRenderer.split_flags(flags.cpu().numpy())
    assert np.array_equal(found, want[2]), what + " found"
    assert np.array_equal(clipped, want[3]), what + " clipped"
    assert (flags.cpu().numpy() <= 3).all()
    tm = gpu.tonemap_device(torch.from_numpy(np.array(want[0])).to("cuda:0"), torch.empty_like(bgra))
    gpu.synchronize()
    assert torch.equal(bgra, tm), what + ": out_bgra is not the tonemap of the expected radiance"


@pytest.mark.parametrize("w,h,case,subframes,radius", K.ALL_CASES, ids=[K.case_key(*c) for c in K.ALL_CASES])
def test_matches_the_reference_bit_for_bit(gpu, w, h, case, subframes, radius):
    """37 x 23 is more than one wave and no multiple of one; 5 x 3 and 1 x 1
    put taps and most of the window outside the image."""
    _assert_matches(gpu, _run(gpu, w, h, case, subframes, radius), K.reference(w, h, case, subframes, radius),
                    K.case_key(w, h, case, subframes, radius))


@pytest.mark.parametrize("case", T.CASES)
@pytest.mark.parametrize("w,h", T.SIZES)
def test_one_camera_and_no_clamp_is_ptg_temporal_accumulate(gpu, w, h, case):
    a = T.temporal_inputs(w, h, case)
    d = _device(a[2:])
    old = gpu.temporal_accumulate(a[0], *d[:4], history=(a[1],) + tuple(d[4:]), params=T.params(), want_bgra=True)
    new = _run(gpu, w, h, case, 1, 0)
    for o, n, what in zip(old, new, ("out_radiance", "out_moments")):
        _assert_same(n.cpu().numpy(), o.cpu().numpy(), "%dx%d %s %s" % (w, h, case, what))
    assert np.array_equal(old[2].cpu().numpy(), new[2].cpu().numpy())


@pytest.mark.parametrize("radius,alias_radiance", [(0, True), (1, False), (2, False)])
def test_allowed_aliasing_gives_the_same_bits(gpu, radius, alias_radiance):
    """out_moments == moments always; out_radiance == radiance without a clamp."""
    out = _run(gpu, 37, 23, "pan", 3, radius, alias_radiance=alias_radiance, alias_moments=True)
    _assert_matches(gpu, out, K.reference(37, 23, "pan", 3, radius), "in place, radius %d" % radius)


def _call(gpu, w, h, params, cams, hist_cam, pointers, n_cams=None):
    arr = (N.Camera * max(len(cams), 1))(*(N.Camera.of(c) for c in cams))
    hc = N.Camera.of(hist_cam) if hist_cam is not None else None
    ptr = [C.c_void_p(t.data_ptr()) if t is not None else None for t in pointers]
    return N.lib().ptg_temporal_accumulate_clamped(gpu._ctx, w, h, C.byref(params), len(cams) if n_cams is None else n_cams,
                                                   arr, C.byref(hc) if hc is not None else None, *ptr)


def test_refusals(gpu):
    import torch
    w, h = 5, 3
    a = T.temporal_inputs(w, h, "pan")
    cams = K.camera_list(w, h, "pan", 3)
    d = _device(a[2:])
    out_r, out_m = torch.empty_like(d[0]), torch.empty_like(d[1])
    tail = [out_r, out_m, None, None]
    p0, p1 = K.params(0), K.params(1)
    assert _call(gpu, w, h, p1, cams, a[1], d + tail) == 0
    other = [torch.empty_like(d[0]), torch.empty_like(d[1]), None, None]
    assert _call(gpu, w, h, p1, [cams[0]] * 512, a[1], d + other) == 0
    # the radiance in place under a clamp; without one it is allowed, and the moments always
    assert _call(gpu, w, h, p1, cams, a[1], d + [d[0], out_m, None, None]) == -1
    assert _call(gpu, w, h, K.params(2), cams, a[1], d + [d[0], out_m, None, None]) == -1
    scratch = _device(a[2:4])
    assert _call(gpu, w, h, p1, cams, a[1], [d[0], scratch[1]] + d[2:] + [other[0], scratch[1], None, None]) == 0
    assert _call(gpu, w, h, p0, cams, a[1], scratch + d[2:] + [scratch[0], scratch[1], None, None]) == 0
    # the number of cameras
    assert _call(gpu, w, h, p1, cams, a[1], d + tail, n_cams=0) == -1
    assert _call(gpu, w, h, p1, [cams[0]] * 513, a[1], d + tail) == -1
    # the clamp's parameters
    for field, value in (("clamp_radius", 3), ("clamp_sigma", 0.0), ("clamp_sigma", float("nan")),
                         ("clamp_sigma", float("inf")), ("clipped_history", -1.0)):
        p = K.params(1)
        setattr(p, field, value)
        assert _call(gpu, w, h, p, cams, a[1], d + tail) == -1, (field, value)
        with pytest.raises(N.PtgError, match=r"\(-1\)"):
            gpu.temporal_accumulate_clamped(cams, *d[:4], history=(a[1],) + tuple(d[4:]), params=p)
    assert _call(gpu, w, h, K.params(1, base=dict(depth_tolerance=0.0)), cams, a[1], d + tail) == -1
    # ptg_temporal_accumulate's own: an output in the history, a partial history, one output buffer
    for k in range(4, 8):
        assert _call(gpu, w, h, p1, cams, a[1], d + [d[k], out_m, None, None]) == -1
        assert _call(gpu, w, h, p1, cams, a[1], d + [out_r, d[k], None, None]) == -1
        assert _call(gpu, w, h, p1, cams, a[1], d[:k] + [None] + d[k + 1:] + tail) == -1
    assert _call(gpu, w, h, p1, cams, None, d + tail) == -1
    assert _call(gpu, w, h, p1, cams, a[1], d[:4] + [None] * 4 + tail) == -1
    assert _call(gpu, w, h, p1, cams, a[1], d + [out_r, out_r, None, None]) == -1
    assert _call(gpu, w, h, p1, cams, a[1], d + [None, out_m, None, None]) == -1
    gpu.synchronize()
    # nothing was launched by a refused call: the first call's outputs are still its outputs
    _assert_same(out_r.cpu().numpy(), K.reference(w, h, "pan", 3, 1)[0], "after the refusals")


def test_back_to_back_calls_keep_their_cameras(gpu):
    """Two calls with different camera lists, queued before either has run
    to completion, then one synchronize: each result is its own restatement."""
    first = _run(gpu, 37, 23, "bigpan", 3, 1, sync=False)
    second = _run(gpu, 37, 23, "bigpan", 1, 1, sync=False)
    third = _run(gpu, 37, 23, "pan", 3, 2, sync=False)
    gpu.synchronize()
    _assert_matches(gpu, first, K.reference(37, 23, "bigpan", 3, 1), "first of three calls")
    _assert_matches(gpu, second, K.reference(37, 23, "bigpan", 1, 1), "second of three calls")
    _assert_matches(gpu, third, K.reference(37, 23, "pan", 3, 2), "third of three calls")
    assert not T.same_bits(first[0].cpu().numpy(), second[0].cpu().numpy()).all()


def _frame(gpu, scene, cfg):
    gpu.upload_arrays(arrays_copy(scene))
    sub = scene.view()["subframes"]
    cams = [N.Camera.of(s["cam"]) for s in sub]
    _, acc, mom = gpu.render_moments(cfg, want_accum=True)
    alb, nd = gpu.render_features(cfg)
    return cams, acc, mom, alb, nd


def test_two_rendered_frames_match_the_reference_bit_for_bit(gpu, assets_dir):
    """Frames 449 and 450 at 160 x 90 x 16 spp, two subframes each: frame 450
    through both its cameras, radius 1 and the library's sigma, equals the
    restatement on the same downloaded inputs, and every branch ran."""
    s = scene_for(assets_dir, 160, 90, 16, frame=449)
    hist = _frame(gpu, s, s.cfg)
    s = scene_for(assets_dir, 160, 90, 16, frame=450)
    cur = _frame(gpu, s, s.cfg)
    assert len(cur[0]) == 2 and len(hist[0]) == 2
    p = TemporalClampParams.default(clamp_radius=1)
    history = (hist[0][1],) + hist[1:]
    out = gpu.temporal_accumulate_clamped(*cur, history=history, params=p, want_bgra=True, want_flags=True)
    gpu.synchronize()
    host = lambda ts: [t.cpu().numpy() for t in ts]                                     # noqa: E731
    found, clipped = np.zeros((90, 160), bool), np.zeros((90, 160), bool)
    want = temporal_clamped_reference(cur[0], history[0], *host(cur[1:]), *host(history[1:]), params=p, found=found,
                                      clipped=clipped)
    _assert_matches(gpu, out, want + (found, clipped), "frames 449 -> 450")
    print("frames 449 -> 450 at 160x90x16, 2 cameras: %.1f%% of the pixels found history, %.1f%% of those were clipped" % (
        100 * found.mean(), 100 * clipped[found].mean()))
    assert found.any() and not found.all()
    assert clipped.any() and (found & ~clipped).any()


def test_temporal_denoiser_with_the_options_is_the_calls_made_by_hand(gpu, assets_dir):
    import torch
    s = scene_for(assets_dir, 160, 90, 16, frame=449)
    p = TemporalClampParams.default(clamp_radius=2, clamp_sigma=1.5)
    td = TemporalDenoiser(gpu, s.cfg, seed_stride=3, clamp_params=p, blur_cameras=2)
    first = td.step(s)
    s.setup_frame(450)
    second = td.step(s)
    gpu.synchronize()

    cfg1 = N.RenderConfig.make(160, 90, 16, 4, student_id=(s.cfg.student_id + 3) & 0xFFFFFFFF)
    s.setup_frame(449)
    h = _frame(gpu, s, s.cfg)
    assert len(h[0]) == 2
    h_rad, h_mom, _ = gpu.temporal_accumulate_clamped(*h, history=None, params=p)
    want_first = gpu.denoise_guided(h_rad, h[3], h[4], h_mom)
    s.setup_frame(450)
    c = _frame(gpu, s, cfg1)
    rad, mom, _ = gpu.temporal_accumulate_clamped(*c, history=(h[0][1], h_rad, h_mom, h[3], h[4]), params=p)
    want_second = gpu.denoise_guided(rad, c[3], c[4], mom)
    gpu.synchronize()
    for got, want, what in ((first, want_first, "first step"), (second, want_second, "second step")):
        assert torch.equal(got[0], want[1]), what + ": bgra"
        assert T.same_bits(got[1].cpu().numpy(), want[0].cpu().numpy()).all(), what + ": radiance"
    # one camera of the two is another result: the option reached the kernel
    one, _, _ = gpu.temporal_accumulate_clamped(c[0][1:], *c[1:], history=(h[0][1], h_rad, h_mom, h[3], h[4]), params=p)
    gpu.synchronize()
    assert not torch.equal(one, rad)


def test_temporal_denoiser_with_the_defaults_is_todays(gpu, assets_dir):
    import torch
    s = scene_for(assets_dir, 160, 90, 16, frame=449)
    a, b = TemporalDenoiser(gpu, s.cfg), TemporalDenoiser(gpu, s.cfg, clamp_params=None, blur_cameras=1)
    calls = []
    real = gpu.temporal_accumulate_clamped
    gpu.temporal_accumulate_clamped = lambda *x, **k: calls.append(1) or real(*x, **k)
    try:
        outs = []
        for td in (a, b):
            s.setup_frame(449)
            td.step(s)
            s.setup_frame(450)
            outs.append(td.step(s))
        gpu.synchronize()
    finally:
        del gpu.temporal_accumulate_clamped
    assert not calls, "the default step must not call the new entry"
    assert torch.equal(outs[0][0], outs[1][0]) and T.same_bits(outs[0][1].cpu().numpy(), outs[1][1].cpu().numpy()).all()
    # blur_cameras alone goes through the new entry with the clamp off; on a frame of one subframe that is today's result
    s1 = scene_for(assets_dir, 160, 90, 8, frame=449)
    outs = []
    for td in (TemporalDenoiser(gpu, s1.cfg), TemporalDenoiser(gpu, s1.cfg, blur_cameras=8)):
        s1.setup_frame(449)
        td.step(s1)
        s1.setup_frame(450)
        outs.append(td.step(s1))
    gpu.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and T.same_bits(outs[0][1].cpu().numpy(), outs[1][1].cpu().numpy()).all()


def test_frame_450_at_64spp_end_to_end(gpu, assets_dir):
    """Frames 447 .. 450 at 320 x 180 x 64 spp (eight subframes), the sample
    count at which the plain accumulation loses most on the first frame of
    the zoom; frame 450 against this renderer's own 256-spp render of it
    (validator PSNR, no downscale).  Printed: render_denoised_guided of frame
    450 alone, today's TemporalDenoiser, and the new one (the library's
    TemporalClampParams, blur_cameras 8), with the two arms on their own.
    Measured on one MI355X: 27.49 dB alone, 25.71 dB today's, 27.25 dB the new
    one (cameras only 25.15 dB, clamp only 27.09 dB): a gain of 1.54 dB over
    today's, of which half is asserted, so that noise in nothing but the
    inputs cannot flip the check.  The new one is still 0.24 dB below the
    single frame's filter: that is reported, not asserted."""
    s = scene_for(assets_dir, 320, 180, 256, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    ref, _ = gpu.render(s.cfg)
    gpu.synchronize()
    ref = V.bgra_to_rgb(ref.cpu().numpy())
    s = scene_for(assets_dir, 320, 180, 64, frame=447)
    arms = {"today": {}, "cameras": dict(blur_cameras=8), "clamp": dict(clamp_params=TemporalClampParams.default()),
            "both": dict(clamp_params=TemporalClampParams.default(), blur_cameras=8)}
    psnr = {}
    for name, options in arms.items():
        td = TemporalDenoiser(gpu, s.cfg, **options)
        for f in (447, 448, 449, 450):
            s.setup_frame(f)
            bgra, radiance = td.step(s)
        gpu.synchronize()
        psnr[name] = V.psnr(ref, V.bgra_to_rgb(bgra.cpu().numpy()))
        assert np.isfinite(radiance.cpu().numpy()).all(), name
    single, _ = gpu.render_denoised_guided(s.cfg)
    gpu.synchronize()
    p_single = V.psnr(ref, V.bgra_to_rgb(single.cpu().numpy()))
    print("frame 450 320x180x64 vs 256 spp: guided alone %.2f dB, today's TemporalDenoiser %.2f dB, new %.2f dB "
          "(cameras only %.2f dB, clamp only %.2f dB)" % (p_single, psnr["today"], psnr["both"], psnr["cameras"], psnr["clamp"]))
    assert psnr["both"] >= psnr["today"] + HALF_OF_THE_MEASURED_GAIN, "%.2f dB against %.2f dB" % (psnr["both"], psnr["today"])


# half of the gain of the new denoiser over today's measured on one MI355X (the test's docstring), in dB
HALF_OF_THE_MEASURED_GAIN = 0.77
