"""Every text-patch variant under tools/variants/ still finds its anchors in
csrc/ (tools/variant_build.sh applies them to a scratch copy and compiles the
result).  A variant whose anchor has moved fails its own assert here, at the
commit that moved it, instead of at the next experiment that needs it.  No
compile: only that the script runs and edits the copy."""
import glob
import hashlib
import os
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "path-tracing...but-on-the-lumi-cluster_amd", "csrc")
# at_commit.py replaces the sources with a commit's (it needs the git history)
VARIANTS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "tools", "variants", "*.py"))
                  if os.path.basename(p) != "at_commit.py")
# variants that take their value from the environment and have no default
ENV = {"PTG_RUN": "2", "PTG_BANDS": "512"}


def _digest(top):
    out = {}
    for d, _, files in os.walk(top):
        for f in files:
            p = os.path.join(d, f)
            out[os.path.relpath(p, top)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def test_every_variant_is_covered():
    assert "noop.py" in VARIANTS and len(VARIANTS) > 1


@pytest.mark.parametrize("name", VARIANTS)
def test_variant_applies(name, tmp_path):
    work = str(tmp_path / "csrc")
    shutil.copytree(CSRC, work)
    before = _digest(work)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "variants", name), work], capture_output=True,
                       text=True, env=dict(os.environ, **ENV), cwd=str(tmp_path))
    assert r.returncode == 0, "%s no longer applies:\n%s%s" % (name, r.stdout, r.stderr)
    if name != "noop.py":
        assert _digest(work) != before, name + " changed nothing"
