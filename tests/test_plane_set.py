"""The plane set's host half, on the CPU.

csrc/host/planes.h holds what every entry that takes caller-given outputs
shares: check_planes (outputs distinct, present, aligned, outside a forbidden
byte range - ptg_render_with_features, ptg_assemble_tile_packs and
ptg_accum_resolve refuse through it) and the carving of a tile pack into its
five planes (ptg_render_tiles_packed writes through it, k_assemble_tile_packs
reads through it).  Through the C ABI the check runs only behind a bound GPU
context; it is pure host code, so tests/plane_set/plane_set_test.cpp calls it
directly: every rule alone, every pair of rules at once with the message that
wins, the range at its first and last byte and just outside both, bgra's 4-byte
element, no output, one output; and the pack's plane offsets and bytes against
include/ptg.h's stated layout, with the refusals at 2^31 slots.
"""
import os
import subprocess

from conftest import ROOT

DIR = os.path.join(ROOT, "tests", "plane_set")


def _run(tool):
    r = subprocess.run([tool], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "plane_set_test: all passed" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_plane_set(native_lib):
    subprocess.run(["make", "-s"], cwd=DIR, check=True)
    _run(os.path.join(DIR, "_bin", "plane_set_test"))


def test_plane_set_sanitized():
    """The same program as a stand-alone host build under AddressSanitizer and
    UBSan (without libptg.so: no HIP runtime in the process)."""
    r = subprocess.run(["make", "-s", "plane_set_test_host", "EXTRA=-fsanitize=address,undefined -fno-sanitize-recover=all"],
                       cwd=DIR, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    _run(os.path.join(DIR, "_bin", "plane_set_test_host"))
