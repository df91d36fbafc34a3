"""The deferred resolve, output by output (k_resolve, csrc/pt_kernels.hip).

ptg_render_adaptive's closing division and ptg_accum_resolve are one kernel
whose every output may be null, and the plane behind a null output is not
loaded.  The contract, through the C ABI: an output requested alone has the
bits it has in the call that requests them all, and every buffer that was not
requested keeps what it held.  On an off-origin odd rectangle of frames 0 and
450; comparisons are on the bit patterns.
"""
import ctypes as C

import pytest

from conftest import arrays_copy, scene_for
from ptlumi.adaptive import AdaptiveParams
from ptlumi.renderer import Accumulator

pytestmark = pytest.mark.gpu

W, H, SPP = 48, 27, 16
RECT = (5, 3, 37, 19)
FRAMES = [0, 450]
SENTINEL_F, SENTINEL_B, SENTINEL_N = -7.0, 93, -5
NAMES = ("accum", "bgra", "moments", "albedo", "normal_depth", "samples")


def _buffers(gpu):
    """Sentinel-filled buffers of the rectangle, by NAMES."""
    import torch
    dev = torch.device("cuda", gpu.device)
    h, w = RECT[3], RECT[2]
    b = {k: torch.full((h, w, 4), SENTINEL_F, dtype=torch.float32, device=dev)
         for k in ("accum", "moments", "albedo", "normal_depth")}
    b["bgra"] = torch.full((h, w, 4), SENTINEL_B, dtype=torch.uint8, device=dev)
    b["samples"] = torch.full((h, w), SENTINEL_N, dtype=torch.int32, device=dev)
    return b


def _bits(t):
    import torch
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _alone_equals_all(gpu, call, names, what):
    """`call(buffers, wanted)` runs the entry with the outputs named in
    `wanted` (the others null).  Each of `names` alone: the bits of the call
    with all of `names`, and no other buffer touched."""
    import torch
    full = _buffers(gpu)
    call(full, names)
    gpu.synchronize()
    fresh = _buffers(gpu)
    for k in NAMES:
        if k in names:
            assert not torch.equal(_bits(full[k]), _bits(fresh[k])), "%s: all outputs: %s was not written" % (what, k)
        else:
            assert torch.equal(_bits(full[k]), _bits(fresh[k])), "%s: all outputs: %s was written" % (what, k)
    for one in names:
        b = _buffers(gpu)
        call(b, (one,))
        gpu.synchronize()
        for k in NAMES:
            want = full[k] if k == one else fresh[k]
            differ = int((_bits(b[k]) != _bits(want)).sum().item())
            assert differ == 0, "%s: %s alone: %d words of %s differ from %s" % (
                what, one, differ, k, "the all-outputs call" if k == one else "the sentinel")


def _ptrs(b, wanted, names):
    return [C.c_void_p(b[k].data_ptr()) if k in wanted else None for k in names]


@pytest.mark.parametrize("frame", FRAMES)
def test_adaptive_each_output_alone(gpu, assets_dir, native_lib, frame):
    s = scene_for(assets_dir, W, H, SPP, frame=frame)
    gpu.upload_arrays(arrays_copy(s))
    p = AdaptiveParams.default(passes=2, min_passes=1)
    order = ("accum", "bgra", "moments", "samples")

    def call(b, wanted):
        rc = native_lib.ptg_render_adaptive(gpu._ctx, C.byref(s.cfg), *RECT, C.byref(p), *_ptrs(b, wanted, order))
        assert rc == 0, native_lib.ptg_last_error()

    _alone_equals_all(gpu, call, order, "frame %d ptg_render_adaptive, 2 passes" % frame)


@pytest.mark.parametrize("by_samples", [0, 1])
@pytest.mark.parametrize("frame", FRAMES)
def test_accum_resolve_each_output_alone(gpu, assets_dir, native_lib, frame, by_samples):
    s = scene_for(assets_dir, W, H, SPP, frame=frame)
    gpu.upload_arrays(arrays_copy(s))
    acc = Accumulator(gpu, s.cfg, rect=RECT).add(8)       # all flags; half the budget, so the two divisors differ
    assert acc.moments and acc.features
    order = ("accum", "bgra", "moments", "albedo", "normal_depth")

    def call(b, wanted):
        rc = native_lib.ptg_accum_resolve(gpu._ctx, C.byref(acc.header), C.c_void_p(acc.state.data_ptr()), by_samples,
                                          *_ptrs(b, wanted, order))
        assert rc == 0, native_lib.ptg_last_error()

    _alone_equals_all(gpu, call, order, "frame %d ptg_accum_resolve, by_samples %d" % (frame, by_samples))


@pytest.mark.parametrize("frame", FRAMES)
def test_accum_resolve_plain_state(gpu, assets_dir, native_lib, frame):
    """A state of the radiance sums alone (no mom, no feat plane behind it)
    resolves accum alone and bgra alone."""
    s = scene_for(assets_dir, W, H, SPP, frame=frame)
    gpu.upload_arrays(arrays_copy(s))
    acc = Accumulator(gpu, s.cfg, rect=RECT, moments=False, features=False).add(SPP)
    assert tuple(acc.state.shape) == (1, RECT[3], RECT[2], 4)
    order = ("accum", "bgra", "moments", "albedo", "normal_depth")

    def call(b, wanted):
        rc = native_lib.ptg_accum_resolve(gpu._ctx, C.byref(acc.header), C.c_void_p(acc.state.data_ptr()), 0,
                                          *_ptrs(b, wanted, order))
        assert rc == 0, native_lib.ptg_last_error()

    _alone_equals_all(gpu, call, ("accum", "bgra"), "frame %d ptg_accum_resolve of a plain state" % frame)
    # and they are ptg_render's bits
    import torch
    b = _buffers(gpu)
    call(b, ("accum", "bgra"))
    bgra, accum = gpu.render(s.cfg, rect=RECT, want_accum=True)
    gpu.synchronize()
    assert torch.equal(_bits(b["accum"]), _bits(accum)) and torch.equal(b["bgra"], bgra)
