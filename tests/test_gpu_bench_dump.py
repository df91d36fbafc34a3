"""bench.py's plain run: --steps sets the timed steps, the line carries
ms_per_step, nothing beside the headline figure is measured, and
--dump-outputs writes what the last timed step computed - the arrays a
caller of GpuRenderer.render receives - as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, N, scene_for

pytestmark = pytest.mark.gpu

W, H, SPP, FRAME = 67, 43, 16, 300   # ragged against the 32x16 tiles and the wave size


def test_plain_run_dumps_last_step(gpu, assets_dir, tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--width", str(W), "--height", str(H), "--spp", str(SPP), "--frame", str(FRAME),
                        "--gpu-memory", "shared", "--dump-outputs", str(out)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(W * H * SPP / d["ms_per_step"] / 1e3, rel=1e-2)
    for leg in ("heavy_frame", "animation", "roofline", "cpu_baseline", "with_frame_setup", "value_survey_def",
                "frame_check", "strong"):
        assert d[leg] is None, leg
    assert sorted(os.listdir(out)) == ["accum.npy", "image.npy"]
    image, accum = np.load(out / "image.npy"), np.load(out / "accum.npy")
    assert image.dtype == np.float32 and accum.dtype == np.float32
    assert image.shape == (H, W, 4) and accum.shape == (H, W, 4)
    assert image.nbytes + accum.nbytes <= 64 << 20

    cfg = N.RenderConfig.make(W, H, SPP, 4)
    gpu.upload(scene_for(assets_dir, W, H, SPP, frame=FRAME))
    bgra, acc = gpu.render(cfg, want_accum=True)
    gpu.synchronize()
    assert np.array_equal(image, bgra.cpu().numpy().astype(np.float32))
    assert np.array_equal(accum.view(np.uint32), acc.cpu().numpy().view(np.uint32))
