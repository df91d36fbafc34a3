"""ptg_denoise against its CPU restatement (ptlumi.denoise.atrous_reference),
bit for bit, on seeded synthetic inputs; and the end-to-end claim: a denoised
16-spp frame is nearer the reference's frame than the raw 16-spp frame."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, arrays_copy, scene_for
from denoise_inputs import fixed_inputs as _inputs
from ptlumi import validator as V
from ptlumi.denoise import DenoiseParams, atrous_reference


def _same_bits(got, want):
    """Equal bit patterns; two NaNs count as equal (the definition fixes no
    NaN payload, and a CPU and the GPU generate different ones)."""
    g, w = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    return (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))


_reference = {}


def _want(w, h, iterations):
    key = (w, h, iterations)
    if key not in _reference:
        rad, alb, nd = _inputs(w, h, 7 * w + h)
        _reference[key] = atrous_reference(rad, alb, nd, DenoiseParams.default(iterations=iterations))
        _reference[key].setflags(write=False)
    return _reference[key]


def _run(gpu, w, h, iterations, alias=False):
    import torch
    rad, alb, nd = (torch.from_numpy(a).to("cuda:0") for a in _inputs(w, h, 7 * w + h))
    out, bgra = gpu.denoise(rad, alb, nd, DenoiseParams.default(iterations=iterations), want_bgra=True,
                            out_radiance=rad if alias else None)
    gpu.synchronize()
    if alias:
        assert out.data_ptr() == rad.data_ptr()
    return out, bgra


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("w,h", [(37, 23), (5, 3), (1, 1)])
def test_denoise_matches_the_reference_bit_for_bit(gpu, w, h, iterations):
    """37 < 2 * 16, the reach of step 16, so every border branch runs."""
    import torch
    out, bgra = _run(gpu, w, h, iterations)
    want = _want(w, h, iterations)
    got = out.cpu().numpy()
    same = _same_bits(got, want)
    bad = np.argwhere(~same.all(-1))
    assert len(bad) == 0, "%dx%d, %d iterations: %d pixels differ, first (row, col) %s: got %s want %s" % (
        w, h, iterations, len(bad), bad[0], got[tuple(bad[0])], want[tuple(bad[0])])
    if w * h >= 15:
        assert np.isfinite(got).all(), "the NaN and +inf pixels have finite neighbours and must come out finite"
    assert (got[..., 3] == 0).all()
    tm = torch.empty_like(bgra)
    gpu.tonemap_device(out, tm)
    gpu.synchronize()
    assert torch.equal(bgra, tm), "out_bgra is not tonemap_device(out_radiance)"


@pytest.mark.gpu
def test_denoise_in_place(gpu):
    out, _ = _run(gpu, 37, 23, 3, alias=True)
    assert _same_bits(out.cpu().numpy(), _want(37, 23, 3)).all()


@pytest.mark.gpu
def test_zero_iterations_copies_the_bits(gpu):
    import torch
    rad, alb, nd = _inputs(37, 23, 5)
    rad[..., 3] = 3.0
    d = [torch.from_numpy(a).to("cuda:0") for a in (rad, alb, nd)]
    out, bgra = gpu.denoise(*d, DenoiseParams.default(iterations=0))
    gpu.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), rad.view(np.uint32))
    tm = gpu.tonemap_device(out, torch.empty_like(bgra))
    gpu.synchronize()
    assert torch.equal(bgra, tm)


@pytest.mark.gpu
@pytest.mark.parametrize("field,value", [("iterations", 9), ("sigma_color", 0.0), ("sigma_albedo", -1.0),
                                         ("sigma_normal", float("nan")), ("sigma_depth", float("inf"))])
def test_invalid_params_are_refused(gpu, field, value):
    import torch
    from ptlumi.native import PtgError
    d = [torch.from_numpy(a).to("cuda:0") for a in _inputs(5, 3, 1)]
    with pytest.raises(PtgError, match=r"\(-1\)"):
        gpu.denoise(*d, DenoiseParams.default(**{field: value}))


@pytest.mark.gpu
def test_denoised_16spp_frame_is_nearer_the_reference_frame(gpu, assets_dir):
    """Frame 0 at 640x360 x 16 spp against the reference's own 256-spp frame
    (tests/golden/frame_0000_ref.npz): render_denoised with the default
    parameters must score strictly higher than the raw render."""
    s = scene_for(assets_dir, 640, 360, 16, frame=0)
    gpu.upload_arrays(arrays_copy(s))
    raw, _ = gpu.render(s.cfg)
    den, radiance = gpu.render_denoised(s.cfg)
    gpu.synchronize()
    ref = np.load(os.path.join(GOLDEN, "frame_0000_ref.npz"))["rgb"]
    p_raw = V.psnr(ref, V.bgra_to_rgb(raw.cpu().numpy()))
    p_den = V.psnr(ref, V.bgra_to_rgb(den.cpu().numpy()))
    print("frame 0 640x360x16 vs output/frame_0000.bmp: raw %.2f dB, denoised %.2f dB" % (p_raw, p_den))
    assert np.isfinite(radiance.cpu().numpy()).all()
    assert p_den > p_raw, "denoised %.2f dB <= raw %.2f dB" % (p_den, p_raw)
