"""ptg_render_with_features under the forced redo pass (libptg_certfail.so,
tests/test_gpu_redo.py): a surface path of round 0 stores its features before
any rounding certificate is consulted, returns SH_REDO and is shaded again by
the plain MathExact instantiation, which stores none.  The fused outputs must
still be the separate entries' bit for bit."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT, N

CERTFAIL = os.path.join(os.path.dirname(N.LIB_PATH), "libptg_certfail.so")


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_fused_features_while_every_surface_path_is_redone():
    env = dict(os.environ, PTG_LIB=CERTFAIL)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fused_redo_check.py"), "450"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["lib"] == "libptg_certfail.so"
    assert all(out["equal"].values()), out["equal"]
    assert all(out["counted_equal"].values()), out["counted_equal"]
    assert out["covered"], "the frame shows no surface"
    # every surface shade of the certified pass that evaluated a certified
    # expression was listed and shaded again (tests/test_gpu_redo.py)
    redo = out["redo"]
    first = out["shades"] - redo["surface"]
    assert redo["surface"] > 0 and redo["sky"] == 0
    assert redo["surface"] <= first and redo["surface"] >= 0.99 * first, (out["shades"], redo)
