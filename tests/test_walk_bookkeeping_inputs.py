"""The ray sets of tests/walk_bookkeeping_inputs.py do what they claim, checked
on the CPU with the host scene and the oracle alone: a GPU pass over waves
that had lost their non-finite lanes, or over a queue whose walks all end in
the same phase, would be vacuous.  Frame 450, subframe 1."""
import numpy as np
import pytest

import walk_bookkeeping_inputs as B
import walk_ray_inputs as R


@pytest.fixture(scope="module")
def fr(assets_dir):
    return R.frame_for(assets_dir, 450, 1)


def test_world_only_nonfinite_rays(fr):
    rays, inst = B.world_only_nonfinite(fr)
    assert len(rays) == 96 and len(set(inst.tolist())) >= 8
    d = rays[:, 3:]
    assert (~B.recip_finite(d)).sum(1).tolist() == [1] * 96                # one zero or denormal component
    assert (d == 0).any() and ((d != 0) & ~B.recip_finite(d)).any()        # both kinds
    for r, i in zip(rays, inst):
        assert B.recip_finite(B.object_dir(fr, i, r[3:])).all()
    e = R.expect(fr, rays, 1)
    assert (e[R.hit_mask(e), 4] == inst[R.hit_mask(e)]).mean() >= 0.5      # the aimed-at BLAS is entered: the hit is in it
    assert (B.boxes_crossed(fr, rays) >= 2).mean() >= 0.9                  # and another one: a BLAS is left for a TLAS with entries


def test_object_only_nonfinite_rays(fr):
    rays, inst = B.object_only_nonfinite(fr)
    assert len(rays) == 96 and len(set(inst.tolist())) >= 8
    assert B.recip_finite(rays[:, 3:]).all()
    for r, i in zip(rays, inst):
        od = B.object_dir(fr, i, r[3:])
        assert od[0] == 0 and B.recip_finite(od[1:]).all()
    e = R.expect(fr, rays, 1)
    assert (e[R.hit_mask(e), 4] == inst[R.hit_mask(e)]).mean() >= 0.5
    assert (B.boxes_crossed(fr, rays) >= 2).mean() >= 0.9


def test_flag_waves_layout(fr):
    rays, flagged = B.flag_waves(fr)
    assert rays.shape == (80 * 64, 6) and rays.dtype == np.float32
    f = flagged.reshape(80, 64)
    assert all(f[g].sum() == 1 and f[g, g] for g in range(64))
    assert all(f[g].sum() == 32 and f[g, g % 2] and not f[g, 1 - g % 2] for g in range(64, 80))
    # an unflagged lane is finite in the world and stays so in every instance it could enter only by luck;
    # a flagged lane is non-finite in the world, or in the space of the instance it is aimed at
    assert B.recip_finite(rays[~flagged][:, 3:]).all()
    pool = B.flagged_rays(fr)
    world_bad = ~B.recip_finite(pool[:, 3:]).all(1)
    assert world_bad[:96].all() and not world_bad[96:192].any() and world_bad[192:].all()
    assert R.hit_mask(R.expect(fr, pool, 1)).mean() >= 0.4


def test_finish_mix_ends_in_every_phase(fr):
    mix = B.finish_mix(fr)
    assert mix.shape == (192, 6) and np.isfinite(mix).all()
    e = R.expect(fr, mix, 1)
    assert not R.hit_mask(e[1::4]).any() and (e[1::4, 7] == 0).all()       # escape rays meet nothing
    assert (e[2::4, 7] == 1).all() and (e[3::4, 7] == 0).all()             # shadowed / unshadowed sun-ward rays
    assert R.hit_mask(e[0::4]).any() and not R.hit_mask(e[0::4]).all()
    # the escape rays start above the scene's box and point away from it
    assert (mix[1::4, 1] > fr.hi[1]).all() and (mix[1::4, 4] > 0).all()
    # every queue length of the GPU test holds each kind it has room for
    for n in B.FINISH_LENGTHS:
        assert n >= 1 and n <= len(mix)


def test_resume_queue(fr):
    rays, tail = B.resume_queue(fr)
    assert tail == 256 and len(rays) == 256 + 129
    e = R.expect(fr, rays, 1)
    assert (e[:tail, 7] == 1).all() and (e[tail:, 7] == 0).all()
    assert (B.boxes_crossed(fr, rays[tail:]) >= 1).all()
    assert B.sun_ward(fr, rays).all()
