"""The ray families of tests/walk_ray_inputs.py do what they claim, checked
with the oracle alone (no GPU): a GPU pass over a family that had lost its
zeros, its hits or its ties would be vacuous.  Frame 450, 640x360x32,
subframe 1, as tests/test_gpu_walk_rays.py uses them."""
import numpy as np
import pytest

import walk_ray_inputs as R


@pytest.fixture(scope="module")
def fr(assets_dir):
    return R.frame_for(assets_dir, 450, 1)


def test_families_are_seeded_float32_rays(fr):
    for name in ("axis", "scaled", "restart", "seams", "nonfinite", "shuffled"):
        a, b = R.FAMILIES[name](fr), R.FAMILIES[name](fr)
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 6, name
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    assert 1400 <= len(R.family(fr, "axis")) <= 1600
    assert 1400 <= len(R.family(fr, "scaled")) <= 1600
    assert 2700 <= len(R.family(fr, "restart")) <= 3 * 1024
    assert 900 <= len(R.family(fr, "seams")) <= 1024
    assert 64 <= len(R.family(fr, "nonfinite")) <= 128
    assert len(R.family(fr, "shuffled")) == 8192


def test_axis_has_both_zeros_and_hits(fr):
    d = R.family(fr, "axis")[:, 3:]
    zero = d == 0
    assert zero.any(1).all()
    assert (zero & np.signbit(d)).any(0).all() and (zero & ~np.signbit(d)).any(0).all()   # -0 and +0 in every component
    assert set(zero.sum(1)) == {1, 2}
    assert R.hit_mask(R.expected(fr, "axis", 1)).mean() >= 0.25


def test_scaled_covers_the_exponent_classes_and_hits(fr):
    e = R.biased_exponents(R.family(fr, "scaled")[:, 3:])
    for c in R.EXPONENT_CLASSES:
        assert (e == c).any(1).sum() >= 100, c
    assert R.hit_mask(R.expected(fr, "scaled", 1)).sum() >= 200
    # the upscaled rays' hits lie below MIN_RAY_DIST: round 0 (tmin 0) sees them
    assert R.hit_mask(R.expected(fr, "scaled", 0)).sum() >= R.hit_mask(R.expected(fr, "scaled", 1)).sum() + 200


def test_restart_lands_on_the_tmin_edge(fr):
    _, kind = R.restart(fr)
    e0, e1 = R.expected(fr, "restart", 0), R.expected(fr, "restart", 1)
    near = R.hit_mask(e0) & (e0[:, 3].view(np.float32) < R.MIN_RAY_DIST)
    assert near.mean() >= 0.05
    a = kind == 0
    assert len(R.differing_rows(e0[a], e1[a])) >= 0.05 * a.sum()


def test_seams_meet_vertices_and_edges_exactly(fr):
    e = R.expected(fr, "seams", 1)
    hit = R.hit_mask(e)
    assert hit.mean() >= 0.9
    b = e[hit][:, :2].view(np.float32)
    assert ((b == 0) | (b == 1)).any(1).mean() >= 0.10


def test_nonfinite_rays_are_not_finite(fr):
    r = R.family(fr, "nonfinite")
    assert (~np.isfinite(r)).any(1).all()
    assert np.isnan(r[:, 3:]).any() and np.isinf(r[:, 3:]).any() and np.isnan(r[:, :3]).any() and np.isinf(r[:, :3]).any()
    assert {1, 2, 3} <= set(np.isnan(r[:, 3:]).sum(1))


def test_shuffled_is_half_shadowed(fr):
    e = R.expected(fr, "shuffled", 1)
    assert 0.25 <= e[:, 7].mean() <= 0.75
    tiled = R.shuffled_tiled(fr, 20000)
    assert np.array_equal(tiled[:8192], R.family(fr, "shuffled")) and not np.array_equal(tiled[8192:16384], tiled[:8192])


def test_deep_fixture_is_rays_from_the_search_pool(fr):
    r = R.deep()
    assert r.dtype == np.float32 and r.ndim == 2 and r.shape[1] == 6 and 0 < len(r) <= 8192
    assert np.isfinite(r).all()
    # every fixture ray is, bit for bit, a ray of the 2^20-candidate pool (seeds 0..7)
    pool = np.concatenate([R.deep_candidates(fr, 131072, seed) for seed in range(8)])
    row = np.dtype((np.void, 24))
    assert np.isin(np.ascontiguousarray(r).view(row).ravel(), pool.view(row).ravel()).all()
    assert len(np.unique(np.ascontiguousarray(r).view(row).ravel())) == len(r)
