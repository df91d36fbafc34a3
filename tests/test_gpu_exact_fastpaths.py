"""The exact fast paths of the atmosphere and the certified surface pass:
below_radius in place of the sqrt-and-compare below-ground tests, and
pow5_d / pow_quarter_d in place of the generic pow in k_wf_shade<MathFast>
(csrc/device/ref_math.h).  Results must stay the oracle's bit for bit:

  * frame 0 is night (the sun below the horizon: every shadowed branch of the
    light-step loops), frame 450 is day (NEE live, unshadowed steps, so the
    heights feed exp), frame 1400 a third view;
  * both pipelines: the wavefront kernels use the certified forms (MathFast),
    the megakernel the exact ones (MathExact), and both share below_radius;
  * libptg_certfail.so shades every surface path again in the exact pass
    (glibc's restated pow): its frames must equal the default build's.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, N, scene_for
from oracle import Oracle

pytestmark = pytest.mark.gpu

W, H, SPP, BOUNCES = 64, 36, 16, 4
FRAMES = [0, 450, 1400]
CERTFAIL = os.path.join(os.path.dirname(N.LIB_PATH), "libptg_certfail.so")

_oracle = {}


def oracle_frame(assets_dir, frame):
    """(radiance bits [H][W][3], BGRA [H][W][4]) of the CPU restatement, computed once per frame."""
    if frame not in _oracle:
        s = scene_for(assets_dir, W, H, SPP, BOUNCES, frame=frame)
        acc, bgra = Oracle(s.view(), s.cfg).render_rect(0, 0, W, H)
        _oracle[frame] = (np.ascontiguousarray(acc[..., :3]).view(np.uint32).copy(), np.array(bgra))
    return _oracle[frame]


def test_selftest_mask_is_zero(gpu):
    assert gpu.selftest() == 0


@pytest.mark.parametrize("pipeline", ["wavefront", "megakernel"])
@pytest.mark.parametrize("frame", FRAMES)
def test_frames_bit_identical_to_oracle(gpu, assets_dir, frame, pipeline):
    want_acc, want_bgra = oracle_frame(assets_dir, frame)
    s = scene_for(assets_dir, W, H, SPP, BOUNCES, frame=frame)
    gpu.set_pipeline(pipeline)
    try:
        gpu.upload(s)
        bgra, acc = gpu.render(s.cfg, want_accum=True)
        gpu.synchronize()
    finally:
        gpu.set_pipeline("wavefront")
    got = np.ascontiguousarray(acc.cpu().numpy()[..., :3]).view(np.uint32)
    mism = int((got != want_acc).any(-1).sum())
    assert mism == 0, "%d/%d pixels differ from the oracle" % (mism, W * H)
    assert np.array_equal(bgra.cpu().numpy(), want_bgra)


def test_forced_exact_pass_equals_default_build(gpu, assets_dir, tmp_path):
    out = str(tmp_path / "certfail.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fastpaths_render.py"),
                        ",".join(map(str, FRAMES)), str(W), str(H), str(SPP), out],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env=dict(os.environ, PTG_LIB=CERTFAIL), timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    d = np.load(out)
    assert str(d["lib"]) == "libptg_certfail.so"
    for f in FRAMES:
        s = scene_for(assets_dir, W, H, SPP, BOUNCES, frame=f)
        gpu.upload(s)
        bgra, acc = gpu.render(s.cfg, want_accum=True)
        gpu.synchronize()
        got = np.ascontiguousarray(acc.cpu().numpy()[..., :3]).view(np.uint32)
        assert np.array_equal(d["acc_%d" % f], got), f
        assert np.array_equal(d["bgra_%d" % f], bgra.cpu().numpy()), f
