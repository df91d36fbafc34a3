"""The wavefront walk kernels (k_wf_walk, through ptg_walk_rays) against the
oracle, ray by ray, on families built to land on the branches a render's own
rays reach only by luck (tests/walk_ray_inputs.py; tests/test_walk_ray_inputs.py
checks on the CPU that each family does what it claims).

Every comparison is exact equality of the record words: words 0, 1, 3, 4, 5, 6
on a hit, words 3 and 4 on a miss, word 7 (shadowed) always.  The oracle is
asked with the tmin and tmax the kernels use in that bounce round: closest hit
0 (round 0) or 1e-4 .. 1e9, any hit 1e-4 .. 1e9.
"""
import numpy as np
import pytest

import walk_ray_inputs as R
from conftest import N

PtgError = N.PtgError

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def on_gpu(gpu, assets_dir):
    """on_gpu(frame, subframe) -> that Frame, uploaded (again only when the frame changes)."""
    state = {"key": None}

    def use(frame=450, subframe=1):
        fr = R.frame_for(assets_dir, frame, subframe)
        if state["key"] != frame:
            gpu.upload_arrays(fr.arrays)
            state["key"] = frame
        return fr
    return use


def _assert_rows(got, want, rays, what):
    bad = R.differing_rows(got, want)
    assert len(bad) == 0, "%s: %d/%d rows differ, first row %d ray %s: gpu %s oracle %s" % (
        what, len(bad), len(want), bad[0], rays[bad[0]].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist())


CASES = [("axis", 450, 1, 1), ("scaled", 450, 1, 1), ("scaled", 450, 1, 0), ("seams", 450, 1, 1), ("nonfinite", 450, 1, 1),
         ("restart", 450, 1, 0), ("restart", 450, 1, 1), ("axis", 0, 0, 1), ("restart", 0, 0, 0), ("restart", 0, 0, 1)]


@pytest.mark.parametrize("name,frame,subframe,rnd", CASES)
def test_walk_kernels_match_the_oracle(gpu, on_gpu, name, frame, subframe, rnd):
    """k_wf_walk<false> and k_wf_walk<true>, default grid, per family and round
    (scaled also in round 0, where the upscaled rays' hits pass tmin)."""
    fr = on_gpu(frame, subframe)
    rays = R.family(fr, name)
    got, stats = gpu.walk_rays(subframe, rays, round=rnd)
    assert stats is None
    _assert_rows(got, R.expected(fr, name, rnd), rays, "%s frame %d round %d" % (name, frame, rnd))
    assert (got[:, 2] == 0).all() and (got[~R.hit_mask(got), :3] == 0).all()


@pytest.mark.parametrize("name,frame,subframe,rnd", CASES)
def test_per_ray_kernel_matches_the_oracle(gpu, on_gpu, name, frame, subframe, rnd):
    """ptg_trace_rays (k_rays, the private-stack walker) on the same families
    with the same tmin and tmax: one query, so the shadow word has the
    closest-hit range too, and the oracle is asked the same."""
    fr = on_gpu(frame, subframe)
    rays = R.with_range(R.family(fr, name), *R.closest_range(rnd))
    got = gpu.trace_rays(subframe, rays)
    want = fr.memo(("k_rays", name, rnd), lambda: fr.oracle.trace_rays(subframe, rays))
    _assert_rows(got, want, rays, "k_rays %s frame %d round %d" % (name, frame, rnd))
    hit = R.hit_mask(want)
    assert np.array_equal(got[hit, 2], want[hit, 2])


def test_deep_rays_spill_and_match(gpu, on_gpu):
    """Rays whose stacks outgrow the LDS windows (the committed fixture
    tests/golden/walk_deep_rays_f450.npz): a counted and a plain pass give the
    same records, the oracle's; at least 64 closest-hit walks and 16 any-hit
    walks passed their window (16 entries of LdsStack, 16 slots of
    LdsSlotStack<false> in the default build), so reserve()'s spill and the
    pop's read-back ran; and no stack went past the lane's HBM area (the
    frame's stack bound in entries, twice that in slots: ptg_walk_rays
    compares in the stack's own units and fails a counted run that did).

    How the fixture was found: 2^20 candidate rays (walk_ray_inputs.deep_candidates,
    seeds 0..7, 131072 each: near-horizontal unit rays from points in the lower
    third of frame 450's scene box) went through counted ptg_walk_rays calls of
    16 rays on an MI355X; 1617 closest-hit and 1497 any-hit walks passed their
    window.  The groups with such a walk were then walked ray by ray, and the
    fixture keeps every ray whose own walk passed its window: 1617 rays, all
    of them in the closest-hit walk, 1497 also in the any-hit walk; the
    largest stack was 23 in both."""
    fr = on_gpu(450, 1)
    rays = R.family(fr, "deep")
    want = R.expected(fr, "deep", 1)
    counted, stats = gpu.walk_rays(1, rays, round=1, counted=True)
    plain, none = gpu.walk_rays(1, rays, round=1)
    print("deep: %d rays, stats %s" % (len(rays), stats.tolist()))
    assert none is None
    assert np.array_equal(counted, plain)
    _assert_rows(plain, want, rays, "deep")
    assert stats[0][0] == len(rays) and stats[1][0] == len(rays)
    assert stats[0][1] >= 64
    assert stats[1][1] >= 16
    assert 16 < stats[0][2] and 16 < stats[1][2]      # past both windows


@pytest.mark.parametrize("grid", [0, 1, 3, 8, 24])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 8192])
def test_dealing_reaches_every_position(gpu, on_gpu, n, grid):
    """The queue's dealing (band, local, rl, t) for queue lengths around a
    64-entry group and grids of 1, 3 (one XCD), 8 and 24 (eight XCDs) blocks:
    every row equals the oracle's, and no position keeps ptg_walk_rays'
    sentinel (that fails the call)."""
    fr = on_gpu(450, 1)
    rays = R.family(fr, "shuffled")[:n]
    got, _ = gpu.walk_rays(1, rays, round=1, grid_blocks=grid)
    _assert_rows(got, R.expected(fr, "shuffled", 1)[:n], rays, "n %d grid %d" % (n, grid))


def test_dealing_runs_of_the_any_hit_walk(gpu, on_gpu):
    """196 700 rays on 8 blocks: 3074 groups, so a band is 4 groups = kAnyRun
    and the any-hit walk deals runs (rl > 0).  Every row equals ptg_trace_rays'
    and, on a seeded 2048-row subset, the oracle's."""
    fr = on_gpu(450, 1)
    rays = R.shuffled_tiled(fr, 196700)
    got, _ = gpu.walk_rays(1, rays, round=1, grid_blocks=8)
    per_ray = R.as_walk_record(gpu.trace_rays(1, R.with_range(rays, *R.closest_range(1))))
    _assert_rows(got, per_ray, rays, "196700 rays against k_rays")
    sel = np.sort(np.random.default_rng(4508).permutation(len(rays))[:2048])
    _assert_rows(got[sel], R.expect(fr, rays[sel], 1), rays[sel], "196700 rays against the oracle")


@pytest.mark.parametrize("grid", [1, 8])
def test_candidates_carried_between_unrelated_rays(gpu, on_gpu, grid):
    """On 1 or 8 blocks every wave walks many groups of the shuffled rays, so
    the occluder one ray found is tried first by rays that have nothing to do
    with it (try_candidate, resume_tlas): the shadow words still equal the
    oracle's and the closest-hit words are untouched.  stats[1][3] counts the
    any-hit walks that took a candidate: at least n / 8."""
    fr = on_gpu(450, 1)
    rays = R.family(fr, "shuffled")
    got, stats = gpu.walk_rays(1, rays, round=1, grid_blocks=grid, counted=True)
    print("candidates: grid %d stats %s" % (grid, stats.tolist()))
    _assert_rows(got, R.expected(fr, "shuffled", 1), rays, "candidates grid %d" % grid)
    assert stats[1][0] == len(rays)
    assert stats[1][3] >= len(rays) // 8
    assert stats[0][3] == 0


def test_bad_arguments_are_errors(gpu, on_gpu):
    from ptlumi.renderer import GpuRenderer
    rays = np.zeros((4, 6), np.float32)
    rays[:, 5] = 1
    fresh = GpuRenderer(0)
    try:
        with pytest.raises(PtgError, match="not uploaded"):
            fresh.walk_rays(0, rays)
    finally:
        fresh.close()
    fr = on_gpu(450, 1)
    with pytest.raises(PtgError, match="subframe"):
        gpu.walk_rays(len(fr.arrays["subframes"]), rays)
    with pytest.raises(PtgError, match="round"):
        gpu.walk_rays(1, rays, round=255)
    with pytest.raises(PtgError, match="grid_blocks"):
        gpu.walk_rays(1, rays, grid_blocks=1 << 20)
    hits, stats = gpu.walk_rays(1, np.zeros((0, 6), np.float32), counted=True)
    assert hits.shape == (0, 8) and stats.tolist() == [[0] * 4] * 2
    got, _ = gpu.walk_rays(1, rays, round=254)       # the last round the entry takes
    assert got.shape == (4, 8)
