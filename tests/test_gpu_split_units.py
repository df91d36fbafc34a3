"""libptg.so is linked from three HIP units, each with its own device code
object (csrc/pt_kernels.hip, image_ops.hip, upload.hip).  A fresh process
whose first GPU work is in the image-space unit - no scene uploaded, nothing
rendered - must find that unit's kernels and compute the pinned bits
(tests/split_units_check.py)."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_image_unit_runs_first_in_a_fresh_process():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "split_units_check.py")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["tonemap_n"] == 2 * 4096 + 4
    assert out["tonemap_equal"], "ptg_tonemap differs from the oracle"
    assert out["denoise_differ"] == 0, "%d components differ from atrous_reference" % out["denoise_differ"]
    assert out["denoise_finite"]
