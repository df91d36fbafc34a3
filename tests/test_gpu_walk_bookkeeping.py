"""The wavefront walk's per-iteration bookkeeping (k_wf_walk through
ptg_walk_rays) against the oracle, word for word, on inputs built for each
piece of it (tests/walk_bookkeeping_inputs.py; tests/test_walk_bookkeeping_inputs.py
checks those inputs on the CPU):

  the LDS stack's two 4-byte planes   deep stacks, through the spill to HBM and back
  the finite flags kept in `oct`       waves that mix finite and non-finite levels
  the one finish site                  short queues of walks that end in every phase
  the chunk pipeline on the new loop   the smoke shape at both concurrency levels

Comparisons are those of tests/test_gpu_walk_rays.py: words 0, 1, 3, 4, 5, 6
on a hit, 3 and 4 on a miss, word 7 always.
"""
import numpy as np
import pytest

import walk_bookkeeping_inputs as B
import walk_ray_inputs as R
from conftest import N, scene_for
from oracle import Oracle

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fr(gpu, assets_dir):
    """Frame 450, subframe 1, uploaded."""
    f = R.frame_for(assets_dir, 450, 1)
    gpu.upload_arrays(f.arrays)
    return f


def _assert_rows(got, want, rays, what):
    bad = R.differing_rows(got, want)
    assert len(bad) == 0, "%s: %d/%d rows differ, first row %d ray %s: gpu %s oracle %s" % (
        what, len(bad), len(want), bad[0], rays[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


@pytest.mark.parametrize("grid", [1, 8])
def test_stack_planes_across_the_window(gpu, fr, grid):
    """The deep-stack fixture (stacks up to 23 entries; the reference alone
    needs more than the window's 16) on 1 and on 8 blocks: the closest-hit
    words equal the oracle's and ptg_trace_rays' (the private stack), and the
    counted run's past-window tally says the spill to HBM and the way back
    ran on the two-plane window."""
    rays = R.family(fr, "deep")
    want = R.expected(fr, "deep", 1)
    counted, stats = gpu.walk_rays(1, rays, round=1, grid_blocks=grid, counted=True)
    plain, _ = gpu.walk_rays(1, rays, round=1, grid_blocks=grid)
    print("deep on %d blocks: %d rays, stats %s" % (grid, len(rays), stats.tolist()))
    assert np.array_equal(counted, plain)
    _assert_rows(plain, want, rays, "deep grid %d" % grid)
    per_ray = fr.memo("deep k_rays", lambda: R.as_walk_record(gpu.trace_rays(1, R.with_range(rays, *R.closest_range(1)))))
    hit = R.hit_mask(per_ray)
    assert np.array_equal(hit, R.hit_mask(plain))
    assert np.array_equal(plain[hit][:, [0, 1, 3, 4, 5, 6]], per_ray[hit][:, [0, 1, 3, 4, 5, 6]])
    assert np.array_equal(plain[~hit][:, [3, 4]], per_ray[~hit][:, [3, 4]])
    assert stats[0][0] == len(rays)
    assert stats[0][1] > 0 and stats[0][2] > 16           # walks past the closest-hit window, and how far


@pytest.mark.parametrize("grid", [0, 1, 8])
def test_finite_flags_in_mixed_waves(gpu, fr, grid):
    """Groups of 64 in which one lane, or every other lane, has a level whose
    reciprocal direction is not finite (world only, object space only, axis
    rays, denormals), beside plain camera rays: both walks equal the oracle."""
    rays, flagged = B.flag_waves(fr)
    want = fr.memo("flag_waves expect", lambda: R.expect(fr, rays, 1))
    got, _ = gpu.walk_rays(1, rays, round=1, grid_blocks=grid)
    _assert_rows(got, want, rays, "flag waves grid %d" % grid)
    _assert_rows(got[flagged], want[flagged], rays[flagged], "flagged lanes grid %d" % grid)


@pytest.mark.parametrize("rnd", [0, 1])
def test_level_changes_with_flags(gpu, fr, rnd):
    """The two constructed sets alone, in both rounds' ranges: every ray
    enters a BLAS whose finite flag differs from the world's, and leaves it
    for a TLAS that still holds entries."""
    a, _ = B.world_only_nonfinite(fr)
    b, _ = B.object_only_nonfinite(fr)
    rays = np.concatenate([a, b])
    want = fr.memo(("level sets expect", rnd), lambda: R.expect(fr, rays, rnd))
    for grid in (0, 1):
        got, _ = gpu.walk_rays(1, rays, round=rnd, grid_blocks=grid)
        _assert_rows(got, want, rays, "level sets round %d grid %d" % (rnd, grid))


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("n", B.FINISH_LENGTHS)
def test_one_finish_site(gpu, fr, n, grid):
    """Queues of 1 .. 129 walks that end in different phases - at the pop
    after the root's block step, deep in a walk, at an occluder in a leaf
    phase - on 1 and 3 blocks: every row is written (a sentinel left fails the
    call) and equals the oracle's."""
    mix = B.finish_mix(fr)
    want = fr.memo("finish mix expect", lambda: R.expect(fr, mix, 1))
    got, _ = gpu.walk_rays(1, mix[:n], round=1, grid_blocks=grid)
    _assert_rows(got, want[:n], mix[:n], "finish n %d grid %d" % (n, grid))


def test_finish_after_a_resumed_tlas_walk(gpu, fr):
    """One block: each of its waves walks a group of shadowed sun-ward rays,
    then comes back for unshadowed ones with an occluder as its candidate.  A
    walk that took a candidate and ends unshadowed has walked the candidate's
    instance whole and then the TLAS from its root: the counted run says that
    candidates were taken, the oracle that no tail ray is shadowed."""
    rays, tail = B.resume_queue(fr)
    want = fr.memo("resume expect", lambda: R.expect(fr, rays, 1))
    assert (want[:tail, 7] == 1).all() and (want[tail:, 7] == 0).all()
    got, stats = gpu.walk_rays(1, rays, round=1, grid_blocks=1, counted=True)
    print("resume: stats %s" % stats.tolist())
    _assert_rows(got, want, rays, "resume")
    assert stats[1][0] == len(rays)
    assert stats[1][3] >= 1
    plain, _ = gpu.walk_rays(1, rays, round=1, grid_blocks=1)
    assert np.array_equal(plain, got)


@pytest.mark.parametrize("frame,spp", [(0, 16), (450, 8)])
def test_smoke_shape_at_both_concurrency_levels(assets_dir, frame, spp):
    """64x36 renders of frame 0 (16 spp) and frame 450 (8 spp) through the
    chunk pipeline, one stream and two chunks in flight: the accumulated
    planes and the tonemapped bytes equal the oracle's."""
    from ptlumi.renderer import GpuRenderer
    scene = scene_for(assets_dir, 64, 36, spp, frame=frame)
    cfg = scene.cfg
    acc_o, bgra_o = Oracle(scene.view(), cfg).render_rect(0, 0, 64, 36)
    r = GpuRenderer(0)
    try:
        r.upload(scene)
        for level in (0, 2):
            r.set_concurrency(level)
            bgra, acc = r.render(cfg, want_accum=True)
            r.synchronize()
            got = acc.cpu().numpy()[..., :3].view(np.uint32)
            mism = int((got != acc_o[..., :3].view(np.uint32)).any(-1).sum())
            assert mism == 0, "frame %d concurrency %d: %d/%d pixels differ" % (frame, level, mism, 64 * 36)
            assert np.array_equal(bgra.cpu().numpy(), bgra_o), "frame %d concurrency %d: tonemapped bytes differ" % (frame, level)
    finally:
        r.close()
