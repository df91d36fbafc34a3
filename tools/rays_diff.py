#!/usr/bin/env python3
"""Diagnostics: ptg_trace_rays on the golden rays of frame 450 vs the golden
hits (tests/golden/rays_f450.npz); prints the rays whose records differ.

--walk [--round R]: the same rays (origin and direction; the walk kernels
bring their own tmin and tmax for bounce round R, default 1) through
ptg_walk_rays, against the oracle asked with that range, compared on the
words tests/test_gpu_walk_rays.py compares."""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa
import conftest
from conftest import scene_for, arrays_copy
from ptlumi.renderer import GpuRenderer
walk = "--walk" in sys.argv
rnd = int(sys.argv[sys.argv.index("--round") + 1]) if "--round" in sys.argv else 1
g = np.load(os.path.join(ROOT, "tests", "golden", "rays_f450.npz"))
s = scene_for(conftest.ASSETS, 640, 360, 32, frame=int(g["frame"]))
r = GpuRenderer(0)
r.upload_arrays(arrays_copy(s))
if walk:
    import walk_ray_inputs as R
    fr = R.frame_for(conftest.ASSETS, int(g["frame"]), int(g["subframe"]))
    rays = np.ascontiguousarray(g["rays"][:, :6])
    hits, _ = r.walk_rays(fr.subframe, rays, round=rnd)
    want = R.expect(fr, rays, rnd)
    bad = R.differing_rows(hits, want)
else:
    hits = r.trace_rays(int(g["subframe"]), g["rays"])
    want = g["hits"]
    bad = np.nonzero((hits != want).any(1))[0]
print("lib", os.environ.get("PTG_LIB", "default"), "walk round %d," % rnd if walk else "", "rays differing:", len(bad), "of", len(want))
for i in bad[:12]:
    print(i, "got", hits[i].tolist(), "want", want[i].tolist())
