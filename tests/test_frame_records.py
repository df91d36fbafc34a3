"""The per-frame records of a frame upload, on the CPU.

BlockCache::pack_frame (csrc/host/block_bvh.cpp) is the host half of
ptg_upload_frame: besides the blocks it builds the per-instance records
(InstTrav, InstShade, InstBox) and the list of meshes whose triangles the
device still has to pack.  The any-hit walk trusts InstBox without walking
the TLAS (BlockWalker::try_candidate), and a wrong one only changes which
occluder is found first, so the GPU tests cannot tell it from a right one.

tests/frame_records/records_test.cpp runs pack_frame on frames made with the
project's own BVH builder (every class of instance, a TLAS that names an
instance twice, the leaf-box gate and its memo, a failed frame, the mesh
jobs), and on the real scene, whose record arrays must hash to what the code
computed before it moved out of pt_kernels.hip (tests/golden/frame_records.json).
"""
import json
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

DIR = os.path.join(ROOT, "tests", "frame_records")
TOOL = os.path.join(DIR, "_bin", "records_test")


@pytest.fixture(scope="module")
def records_test(native_lib):
    subprocess.run(["make", "-s"], cwd=DIR, check=True)
    return TOOL


def test_synthetic_frames(records_test):
    r = subprocess.run([records_test], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "records_test: all passed" in r.stdout, r.stdout + r.stderr
    assert "FAILED" not in r.stdout, r.stdout


def test_real_scene_records_unchanged(records_test, assets_dir):
    with open(os.path.join(GOLDEN, "frame_records.json")) as f:
        want = json.load(f)["frames"]
    r = subprocess.run([records_test, "real", assets_dir], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = {}
    for frame, name, digest in re.findall(r"^frame (\d+) (\w+) ([0-9a-f]{64})$", r.stdout, re.M):
        got.setdefault(frame, {})[name] = digest
    counts = {m[0]: [int(x) for x in m[1:]] for m in re.findall(
        r"^frame (\d+): instances (\d+) subframes (\d+) all (\d+) one (\d+) never (\d+) tri0 (\d+) jobs (\d+)$",
        r.stdout, re.M)}
    assert sorted(got) == sorted(want) == ["0", "1400", "450"], r.stdout
    for frame, w in want.items():
        assert got[frame] == w["sha256"], (frame, r.stdout)
        assert counts[frame] == [w["instances"], w["subframes"], w["all_subframes"], w["one_subframe"], w["never"],
                                 w["no_triangle_candidates"], w["mesh_jobs_count"]], (frame, r.stdout)
    # what the fixture covers: static and dynamic instances on every frame (the
    # other classes only in test_synthetic_frames)
    assert all(w["all_subframes"] > 100 and w["one_subframe"] > 100 for w in want.values())
