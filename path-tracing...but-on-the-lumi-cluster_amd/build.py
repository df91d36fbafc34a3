"""In-tree build of libptg.so (gfx950) and of the test oracle.

``build()`` is what ``__graft_entry__.build()`` runs: it compiles the HIP
kernels for gfx950 and the host C++ (make -C csrc), prepares the scene assets
and, for the tests only, builds the oracle (oracle/Makefile) - and, when the
reference tree is present (this container, not the GPU box), the reference
renderer from its sources as the oracle's checker - and the user-kernel test
library built against include/ptg_device.h.  Built files stay in the
tree (git-ignored) so they travel to the GPU box with the snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
ORACLE = os.path.join(ROOT, "oracle")
REFERENCE = "/root/reference"

# Reference builds the tests and the bench use: (mode, W, H, SPP, BOUNCES)
REF_CONFIGS = [
    ("strict", 640, 360, 32, 4),     # parity goldens (scene arrays, rays, samples)
    ("strict", 160, 90, 32, 4),      # small whole-frame golden
    ("strict", 1280, 720, 256, 4),   # bench workload: per-sample spot checks
    ("v3", 1280, 720, 16, 4),        # CPU baseline (reference flags, portable -march)
    ("v3", 640, 360, 32, 4),         # CPU baseline configs[0] (one core); strict-vs-shipped statistics
]
# reference host code + ptg_render in place of baseline_render (oracle/dropin_main.cc),
# and + ptg_render_gather over an RCCL communicator (oracle/dropin_rccl.cc)
DROPIN_CONFIGS = [("strict", 160, 90, 32, 4)]


def _run(cmd, cwd, verbose):
    if verbose:
        print("+", " ".join(cmd), "(in %s)" % cwd, flush=True)
    r = subprocess.run(cmd, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("command failed: %s" % " ".join(cmd))
    return r.stdout


def build_native(verbose=False, jobs=8):
    _run(["make", "-j%d" % jobs, "all", "certfail"], os.path.join(PKG, "csrc"), verbose)
    return os.path.join(PKG, "_build", "libptg.so")


def build_oracle(verbose=False, jobs=8, with_reference=None):
    _run(["make", "oracle"], ORACLE, verbose)
    if with_reference is None:
        with_reference = os.path.isdir(REFERENCE)
    if with_reference:
        for mode, w, h, spp, b in REF_CONFIGS:
            _run(["make", "-j%d" % jobs, "ref", "REF_MODE=%s" % mode, "REF_W=%d" % w, "REF_H=%d" % h,
                  "REF_SPP=%d" % spp, "REF_BOUNCES=%d" % b], ORACLE, verbose)
        for mode, w, h, spp, b in DROPIN_CONFIGS:   # needs libptg.so: build_native first
            _run(["make", "-j%d" % jobs, "dropin", "dropin_rccl", "REF_MODE=%s" % mode, "REF_W=%d" % w,
                  "REF_H=%d" % h, "REF_SPP=%d" % spp, "REF_BOUNCES=%d" % b], ORACLE, verbose)


def build_test_kernels(verbose=False):
    """The user-kernel library of tests/test_gpu_device_dropin.py: a HIP kernel
    built against include/ptg_device.h alone (test infrastructure); and the math
    probe library of tests/test_gpu_math_probe.py: the rounding certificates and
    the glibc restatement behind C entry points, with their host-libm reference.
    The probe library belongs to the tests beside it: where tests/ is an older
    suite without tests/math_probe (run against this build), nothing uses it,
    and the rest of the build must not stop there."""
    _run(["make"], os.path.join(ROOT, "tests", "device_dropin"), verbose)
    probe = os.path.join(ROOT, "tests", "math_probe")
    if os.path.exists(os.path.join(probe, "Makefile")):
        _run(["make"], probe, verbose)
    elif verbose:
        print("tests/math_probe is not in this tree: the probe library is not built", flush=True)


def build_tools(verbose=False):
    """tools/_bin/walk_sim: the CPU model of the block walk over the upload's own
    packing (tests/test_block_bvh.py), tests/frame_records/_bin/records_test,
    the CPU test of the upload's per-frame records (tests/test_frame_records.py),
    and tests/plane_set/_bin/plane_set_test, the CPU test of the outputs check and
    the tile pack carving (tests/test_plane_set.py; like tests/math_probe it
    belongs to the tests beside it and is built where they are)."""
    _run(["make", "walk_sim"], os.path.join(ROOT, "tools"), verbose)
    _run(["make"], os.path.join(ROOT, "tests", "frame_records"), verbose)
    if os.path.exists(os.path.join(ROOT, "tests", "plane_set", "Makefile")):
        _run(["make"], os.path.join(ROOT, "tests", "plane_set"), verbose)


def prepare_assets():
    from . import assets
    return assets.prepare(assets.default_dir(ROOT))


def build(verbose=False):
    prepare_assets()
    build_native(verbose)
    build_test_kernels(verbose)
    build_tools(verbose)
    build_oracle(verbose)
