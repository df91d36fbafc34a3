"""Progressive rendering (ptg_accum_begin / _add / _resolve, renderer.Accumulator):
a frame rendered in steps, resolved between them, saved and continued in
another context ends on the bits of the one-shot ptg_render_with_features, and
the state's planes are the running sums ptg.h says they are.  Every
comparison is bit for bit, two NaNs counting as equal
(tests/test_gpu_fused_features.py, whose shapes and CPU expectation are reused).
"""
import ctypes as C

import numpy as np
import pytest

from conftest import N, arrays_copy, scene_for
from ptlumi.renderer import Accumulator, GpuRenderer

from test_gpu_fused_features import RECTS, SPP, _assert_same, _bits, _expectation, _host

pytestmark = pytest.mark.gpu

F = np.float32


def _one_shot(gpu, cfg, rect=None, samples=None):
    out = gpu.render_with_features(cfg, rect=rect, samples=samples)
    gpu.synchronize()
    return _host(out)


def _resolved(gpu, acc, by_samples=False):
    out = acc.resolve(by_samples=by_samples)
    gpu.synchronize()
    return [t.cpu().numpy() if t is not None else None for t in out]


def _state(gpu, acc):
    """The state's planes on the host, float32 [planes, h, w, 4]."""
    gpu.synchronize()
    return acc.state.cpu().numpy()


def _same_plane(got, want, what):
    differ = (_bits(got) != _bits(want)) & ~(np.isnan(got) & np.isnan(want))
    bad = np.argwhere(differ.any(-1))
    assert len(bad) == 0, "%s: %d/%d pixels differ, first (row, col) %s: got %s want %s" % (
        what, len(bad), got.shape[0] * got.shape[1], bad[0], got[tuple(bad[0])], want[tuple(bad[0])])


# ---- 1. resumed equals one-shot ------------------------------------------------

@pytest.mark.parametrize("frame", [0, 450])
def test_resumed_equals_one_shot(gpu, assets_dir, frame):
    """Adds to 5, 8 and 16: a border that is no multiple of 8 and one inside a
    motion-blur group; after each, resolve() is the one-shot render of [0, done)."""
    s, arr, _, _ = _expectation(assets_dir, frame)
    gpu.upload_arrays(arr)
    rect = RECTS[frame]
    done = []
    for n, acc in gpu.render_progressive(s.cfg, (5, 8, SPP), rect=rect):
        assert n == acc.samples_done
        _assert_same(_resolved(gpu, acc), _one_shot(gpu, s.cfg, rect, (0, n)), "frame %d after %d samples" % (frame, n))
        done.append(n)
    assert done == [5, 8, SPP]


# ---- 2. the planes are what the header says --------------------------------------

@pytest.mark.parametrize("frame", [0, 450])
def test_the_planes_are_the_running_sums(gpu, assets_dir, frame):
    s, arr, feats, rad = _expectation(assets_dir, frame)
    gpu.upload_arrays(arr)
    x0, y0, w, h = RECTS[frame]
    acc = Accumulator(gpu, s.cfg, rect=RECTS[frame])
    acc.add(5).add(SPP)
    planes = _state(gpu, acc)
    assert planes.shape == (4, h, w, 4) and planes.dtype == np.float32
    assert acc.state.numel() * 4 == N.lib().ptg_accum_state_bytes(w, h, 3)
    # plane 0: the oracle's per-sample radiance summed in sample order in float32
    want = np.zeros((h * w, 4), F)
    s1, s2, n = np.zeros(h * w, F), np.zeros(h * w, F), np.zeros(h * w, np.uint32)
    fsum = np.zeros((h * w, 8), F)
    with np.errstate(all="ignore"):
        for j in range(SPP):
            c = rad[:, j]
            want[:, :3] = want[:, :3] + c[:, :3]
            fin = np.isfinite(c[:, :3]).all(-1)
            L = (F(0.2126) * c[:, 0] + F(0.7152) * c[:, 1]) + F(0.0722) * c[:, 2]
            s1 = np.where(fin, s1 + L, s1)
            s2 = np.where(fin, s2 + L * L, s2)
            n += fin
            fsum = fsum + feats[:, j]
    assert want.dtype == F and s1.dtype == F and s2.dtype == F and fsum.dtype == F
    assert (n > 0).all() and (want[:, 3] == 0).all()
    _same_plane(planes[0], want.reshape(h, w, 4), "frame %d radiance sums" % frame)
    mom = np.zeros((h * w, 4), F)
    mom[:, 0], mom[:, 1] = s1, s2
    mom.view(np.uint32)[:, 2] = n
    _same_plane(planes[1], mom.reshape(h, w, 4), "frame %d moments plane (s1, s2, n)" % frame)
    assert np.array_equal(planes[1].view(np.uint32)[..., 2].reshape(-1), n)
    _same_plane(planes[2], fsum[:, :4].reshape(h, w, 4), "frame %d albedo + coverage sums" % frame)
    _same_plane(planes[3], fsum[:, 4:].reshape(h, w, 4), "frame %d normal + depth sums" % frame)


# ---- 3. chunk borders inside a step and between steps ---------------------------------

@pytest.mark.parametrize("steps", [(24, 40, 64), (8, 64)], ids=["24_40_64", "8_64"])
@pytest.mark.parametrize("bounces", [0, 4])
def test_chunk_borders_inside_and_between_steps(gpu, assets_dir, bounces, steps):
    """64x36x64 in chunks of at most 2^16 paths (24 samples): every add is
    split over the two chunk pipelines, and the add of samples 8..63 has two
    chunks per slot, so a slot's next camera is hoisted into the chunk before it."""
    s = scene_for(assets_dir, 64, 36, 64, frame=450)
    cfg = N.RenderConfig.make(64, 36, 64, bounces)
    gpu.upload_arrays(arrays_copy(s))
    want = _one_shot(gpu, cfg)
    try:
        gpu.set_chunk_paths(16)
        acc = Accumulator(gpu, cfg)
        for end in steps:
            acc.add(end)
        got = _resolved(gpu, acc)
    finally:
        gpu.set_chunk_paths(27)
    _assert_same(got, want, "64x36x64, %d bounces, adds to %s in 2^16-path chunks" % (bounces, steps))


# ---- 4. off-origin rectangle, sample_begin > 0, seven bounces ---------------------------

def test_rectangle_off_the_origin_from_sample_3(gpu, assets_dir):
    rect = (7, 3, 31, 19)
    s = scene_for(assets_dir, 41, 23, 24, bounces=7, frame=1750)
    gpu.upload_arrays(arrays_copy(s))
    acc = Accumulator(gpu, s.cfg, rect=rect, sample_begin=3)
    assert acc.samples_done == 3 and acc.rect == rect
    acc.add(11)
    _assert_same(_resolved(gpu, acc), _one_shot(gpu, s.cfg, rect, (3, 11)), "41x23 %s samples 3..10" % (rect,))
    acc.add(21)
    assert acc.samples_done == 21 and acc.sample_begin == 3
    _assert_same(_resolved(gpu, acc), _one_shot(gpu, s.cfg, rect, (3, 21)), "41x23 %s samples 3..20" % (rect,))


# ---- 5. every concurrency level and the megakernel ------------------------------------

def test_every_concurrency_level_and_the_megakernel(gpu, assets_dir, native_lib):
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    want = _one_shot(gpu, s.cfg)
    bgra_m, acc_m, mom_m = gpu.render_moments(s.cfg, want_accum=True)
    gpu.synchronize()
    want_moments = _host((bgra_m, acc_m, mom_m))
    got = {}
    try:
        for level in (0, 1, 2):
            gpu.set_concurrency(level)
            got["concurrency %d" % level] = _resolved(gpu, Accumulator(gpu, s.cfg).add(8).add(16))
        gpu.set_pipeline("megakernel")
        mega = _resolved(gpu, Accumulator(gpu, s.cfg, features=False).add(8).add(16))
        # with the feature planes the megakernel cannot add: refused, nothing written
        acc = Accumulator(gpu, s.cfg)
        gpu.set_pipeline("wavefront")
        acc.add(8)
        gpu.set_pipeline("megakernel")
        before, header = _state(gpu, acc).copy(), bytes(acc.header)
        assert native_lib.ptg_accum_add(gpu._ctx, C.byref(acc.header), C.c_void_p(acc.state.data_ptr()), 16) == -1
        assert b"wavefront pipeline" in native_lib.ptg_last_error()
        assert bytes(acc.header) == header and acc.samples_done == 8
        assert np.array_equal(_bits(_state(gpu, acc)), _bits(before))
        # and back on the wavefront pipeline it goes on
        gpu.set_pipeline("wavefront")
        got["wavefront after the refused add"] = _resolved(gpu, acc.add(16))
    finally:
        gpu.set_pipeline("wavefront")
        gpu.set_concurrency(2)
    for what, g in got.items():
        _assert_same(g, want, what)
    assert mega[3] is None and mega[4] is None
    _assert_same(mega[:3], want_moments, "megakernel, no features, against render_moments")


# ---- 6. counting build --------------------------------------------------------------

def test_counting_build_same_bits_and_each_add_counts_its_samples(gpu, assets_dir):
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    want = _one_shot(gpu, s.cfg)
    counted = []
    try:
        gpu.enable_counters(True)
        acc = Accumulator(gpu, s.cfg)
        for end, step in ((5, 5), (8, 3), (16, 8)):
            acc.add(end)
            gpu.synchronize()
            counted.append((step, int(gpu.counters()[0])))
        got = _resolved(gpu, acc)
    finally:
        gpu.enable_counters(False)
    for step, samples in counted:
        assert samples == 48 * 27 * step, counted
    _assert_same(got, want, "counting build")


# ---- 7. by_samples ------------------------------------------------------------------

def test_by_samples_divides_by_the_samples_taken(gpu, assets_dir):
    s, arr, _, _ = _expectation(assets_dir, 0)
    gpu.upload_arrays(arr)
    rect = RECTS[0]
    h, w = rect[3], rect[2]
    acc = Accumulator(gpu, s.cfg, rect=rect).add(8)
    planes = _state(gpu, acc)
    budget = _resolved(gpu, acc)
    preview = _resolved(gpu, acc, by_samples=True)
    with np.errstate(all="ignore"):
        radiance = planes[0] / F(8)
        want = [None, radiance, budget[2], planes[2] / F(8), planes[3] / F(8)]
    assert radiance.dtype == F and (radiance[..., 3] == 0).all()
    want[0] = gpu.tonemap(radiance.reshape(-1, 4)).reshape(h, w, 4)
    _assert_same(preview, want, "8 of 16 samples by_samples")
    # half the budget: the preview is brighter than the budget-mode image, which divides by 16
    finite = np.isfinite(budget[1])
    assert (preview[1][finite] >= budget[1][finite]).all() and (preview[1][finite] > budget[1][finite]).any()
    acc.add(SPP)
    _assert_same(_resolved(gpu, acc, by_samples=True), _resolved(gpu, acc), "16 of 16: both modes")


# ---- 8. checkpoint into another context ---------------------------------------------

def test_checkpoint_into_another_context(gpu, assets_dir, tmp_path):
    s, arr, _, _ = _expectation(assets_dir, 450)
    gpu.upload_arrays(arr)
    rect = RECTS[450]
    want = _one_shot(gpu, s.cfg, rect)
    path = str(tmp_path / "frame450.npz")
    acc = Accumulator(gpu, s.cfg, rect=rect).add(8)
    acc.save(path)
    del acc
    other = GpuRenderer(0)
    try:
        other.upload_arrays(arr)
        resumed = Accumulator.load(other, path)
        assert resumed.samples_done == 8 and resumed.rect == rect and resumed.moments and resumed.features
        assert resumed.cfg.as_dict() == s.cfg.as_dict()
        resumed.add(SPP)
        got = _resolved(other, resumed)
    finally:
        other.close()
    _assert_same(got, want, "saved after 8 samples, continued to 16 in a second context")


# ---- 9. resolve leaves the state alone ------------------------------------------------

def test_resolve_leaves_the_state_alone(gpu, assets_dir):
    s, arr, _, _ = _expectation(assets_dir, 450)
    gpu.upload_arrays(arr)
    rect = RECTS[450]
    acc = Accumulator(gpu, s.cfg, rect=rect).add(8)
    before = _state(gpu, acc).copy()
    for by_samples in (False, True):
        assert all(t is not None for t in acc.resolve(by_samples=by_samples))
    assert np.array_equal(_bits(_state(gpu, acc)), _bits(before))
    acc.add(SPP)
    _assert_same(_resolved(gpu, acc), _one_shot(gpu, s.cfg, rect), "continued after two resolves")


# ---- 10. argument checks --------------------------------------------------------------

def test_argument_checks_write_nothing(gpu, assets_dir, native_lib):
    import torch
    L = native_lib
    s = scene_for(assets_dir, 48, 27, 16, frame=450)
    gpu.upload_arrays(arrays_copy(s))
    dev = torch.device("cuda", gpu.device)
    acc, mom, alb, nd = (torch.full((27, 48, 4), -7.0, dtype=torch.float32, device=dev) for _ in range(4))
    bgra = torch.full((27, 48, 4), 93, dtype=torch.uint8, device=dev)
    state = torch.full((4, 27, 48, 4), -7.0, dtype=torch.float32, device=dev)
    small = torch.full((1, 27, 48, 4), -7.0, dtype=torch.float32, device=dev)    # a state without moments and features
    p = lambda t: C.c_void_p(t.data_ptr())
    outs = (p(acc), p(bgra), p(mom), p(alb), p(nd))
    whole = (0, 0, 48, 27)

    def untouched():
        gpu.synchronize()
        return all((t == -7.0).all().item() for t in (acc, mom, alb, nd)) and (bgra == 93).all().item()

    # begin: a rectangle outside the image, unknown flag bits - header and state stay as they were
    hdr = N.Accum.from_buffer_copy(b"\xab" * 64)
    assert L.ptg_accum_begin(gpu._ctx, C.byref(s.cfg), 40, 0, 29, 19, 3, 0, C.byref(hdr), p(state)) != 0
    assert b"rectangle outside" in L.ptg_last_error()
    assert L.ptg_accum_begin(gpu._ctx, C.byref(s.cfg), *whole, 4, 0, C.byref(hdr), p(state)) == -1
    assert b"flag" in L.ptg_last_error()
    assert L.ptg_accum_begin(gpu._ctx, C.byref(s.cfg), *whole, 3, 0, None, p(state)) == -1
    gpu.synchronize()
    assert bytes(hdr) == b"\xab" * 64 and (state == -7.0).all().item()
    # a header begin has not written is no header
    assert L.ptg_accum_add(gpu._ctx, C.byref(hdr), p(state), 8) == -1
    assert b"magic" in L.ptg_last_error()

    assert L.ptg_accum_begin(gpu._ctx, C.byref(s.cfg), *whole, 3, 0, C.byref(hdr), p(state)) == 0
    plain = N.Accum()
    assert L.ptg_accum_begin(gpu._ctx, C.byref(s.cfg), *whole, 0, 0, C.byref(plain), p(small)) == 0
    gpu.synchronize()
    assert (state == 0).all().item() and (small == 0).all().item()
    assert (hdr.magic, hdr.version, hdr.flags, hdr.sample_begin, hdr.sample_next, hdr.reserved) == (N.ACCUM_MAGIC, 1, 3, 0, 0, 0)

    def refused(call, text, code=-1):
        before = bytes(hdr)
        rc = call()
        assert (rc == code) if code is not None else (rc != 0), rc
        assert text in L.ptg_last_error(), L.ptg_last_error()
        assert bytes(hdr) == before

    # the empty state: nothing to add below its end, nothing to resolve
    refused(lambda: L.ptg_accum_add(gpu._ctx, C.byref(hdr), p(state), 0), b"adds nothing")
    refused(lambda: L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 0, *outs), b"holds no sample")
    # beyond the frame's subframes (16 samples: 2 subframes)
    refused(lambda: L.ptg_accum_add(gpu._ctx, C.byref(hdr), p(state), 64), b"subframes", code=-6)
    bad = N.Accum.from_buffer_copy(bytes(hdr))
    bad.magic ^= 1
    assert L.ptg_accum_add(gpu._ctx, C.byref(bad), p(state), 8) == -1 and b"magic" in L.ptg_last_error()
    bad = N.Accum.from_buffer_copy(bytes(hdr))
    bad.version = 2
    assert L.ptg_accum_add(gpu._ctx, C.byref(bad), p(state), 8) == -1 and b"version" in L.ptg_last_error()
    assert untouched() and (state == 0).all().item()

    assert L.ptg_accum_add(gpu._ctx, C.byref(hdr), p(state), 8) == 0
    assert L.ptg_accum_add(gpu._ctx, C.byref(plain), p(small), 8) == 0
    gpu.synchronize()
    held, held_small = state.clone(), small.clone()
    refused(lambda: L.ptg_accum_add(gpu._ctx, C.byref(hdr), p(state), 8), b"adds nothing")
    refused(lambda: L.ptg_accum_add(gpu._ctx, C.byref(hdr), p(state), 5), b"adds nothing")
    bad = N.Accum.from_buffer_copy(bytes(hdr))
    bad.magic = 0
    assert L.ptg_accum_resolve(gpu._ctx, C.byref(bad), p(state), 0, *outs) == -1 and b"magic" in L.ptg_last_error()
    # a moments or feature output of a state that keeps none
    assert L.ptg_accum_resolve(gpu._ctx, C.byref(plain), p(small), 0, p(acc), p(bgra), p(mom), None, None) == -1
    assert b"PTG_ACCUM_MOMENTS" in L.ptg_last_error()
    assert L.ptg_accum_resolve(gpu._ctx, C.byref(plain), p(small), 0, p(acc), p(bgra), None, p(alb), None) == -1
    assert b"PTG_ACCUM_FEATURES" in L.ptg_last_error()
    # two equal outputs, no output, an output inside the state
    refused(lambda: L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 0, p(acc), p(bgra), p(mom), p(alb), p(alb)),
            b"same buffer")
    refused(lambda: L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 1, p(mom), p(bgra), p(mom), p(alb), p(nd)),
            b"same buffer")
    refused(lambda: L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 0, None, None, None, None, None), b"no output")
    inside = C.c_void_p(state.data_ptr() + 2 * 27 * 48 * 16)
    refused(lambda: L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 0, inside, p(bgra), p(mom), p(alb), p(nd)),
            b"inside the state")
    last_byte = C.c_void_p(state.data_ptr() + 4 * 27 * 48 * 16 - 1)
    refused(lambda: L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 0, None, last_byte, None, None, None),
            b"inside the state")
    assert untouched()
    assert torch.equal(state.view(torch.int32), held.view(torch.int32))
    assert torch.equal(small.view(torch.int32), held_small.view(torch.int32))

    # what is allowed: any subset of the outputs, and the state goes on to the one-shot bits
    assert L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 0, None, None, p(mom), None, None) == 0
    gpu.synchronize()
    assert (acc == -7.0).all().item() and (alb == -7.0).all().item() and (nd == -7.0).all().item() and (bgra == 93).all().item()
    assert not (mom == -7.0).any().item()
    assert L.ptg_accum_add(gpu._ctx, C.byref(hdr), p(state), 16) == 0
    assert L.ptg_accum_add(gpu._ctx, C.byref(plain), p(small), 16) == 0
    assert L.ptg_accum_resolve(gpu._ctx, C.byref(hdr), p(state), 0, *outs) == 0
    gpu.synchronize()
    got = _host((bgra, acc, mom, alb, nd))
    _assert_same(got, _one_shot(gpu, s.cfg), "after the refused calls")
    # without the moments flag the radiance and the bytes are ptg_render's
    assert L.ptg_accum_resolve(gpu._ctx, C.byref(plain), p(small), 0, p(acc), p(bgra), None, None, None) == 0
    bgra_r, acc_r = gpu.render(s.cfg, want_accum=True)
    gpu.synchronize()
    _assert_same(_host((bgra, acc)), _host((bgra_r, acc_r)), "a state of one plane against ptg_render")
