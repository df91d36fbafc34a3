"""Ray sets for tests/test_gpu_walk_bookkeeping.py (a helper, not a test
module; tests/test_walk_bookkeeping_inputs.py checks on the CPU that each set
does what it claims).  CPU only: numpy, the host scene and the oracle, on the
Frame of tests/walk_ray_inputs.py (frame 450, subframe 1).

  flag_waves   64-ray groups in which one lane, or every other lane, walks with
               a reciprocal direction that is not finite at some level, next
               to lanes whose levels are all finite
  finish_mix   rays that end their walk in different phases of an iteration,
               side by side from the queue's first entries on
  resume_queue a queue whose tail is walked by waves that already carry an
               occluder, and is not occluded itself
"""
import numpy as np

import walk_ray_inputs as R

F32 = np.float32


# ---- instances -----------------------------------------------------------------

def object_dir(fr, inst, d):
    """The direction d in instance `inst`'s space, in float32 and in the order
    BlockWalker::enter() adds the terms: (M0 * d.x + M1 * d.y) + M2 * d.z, each
    product and sum rounded (row vectors times inv_transform)."""
    M = fr.arrays["instances"][int(inst)]["inv_transform"].astype(F32)
    d = np.asarray(d, F32)
    return np.array([F32(F32(F32(M[0, c] * d[0]) + F32(M[1, c] * d[1])) + F32(M[2, c] * d[2])) for c in range(3)], F32)


def recip_finite(d):
    """Per component: whether 1 / d is a finite float (false for +-0, for the
    denormals whose reciprocal overflows, and for NaN)."""
    d = np.asarray(d, F32)
    with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
        return np.isfinite(F32(1.0) / d)


def instance_boxes(fr):
    """World-space bounds of every instance's vertices: (lo, hi), float64 [n, 3]."""
    def make():
        ins = fr.arrays["instances"]
        lo, hi = np.zeros((len(ins), 3)), np.zeros((len(ins), 3))
        local = {}
        for i, rec in enumerate(ins):
            key = tuple(int(v) for v in rec["mesh"])
            if key not in local:
                verts, _, _, bv = key     # (vertex_count, triangle_count, index_offset, base_vertex_offset)
                p = fr.arrays["pos"][bv: bv + verts][:, :3].astype(np.float64)
                local[key] = np.array([[p[:, 0].min(), p[:, 1].min(), p[:, 2].min()], [p[:, 0].max(), p[:, 1].max(), p[:, 2].max()]])
            b = local[key]
            corners = np.array([[b[(k >> 0) & 1, 0], b[(k >> 1) & 1, 1], b[(k >> 2) & 1, 2]] for k in range(8)])
            T = rec["transform"].astype(np.float64)
            w = corners @ T[:3, :3] + T[3, :3]
            lo[i], hi[i] = w.min(0), w.max(0)
        return lo, hi
    return fr.memo("instance_boxes", make)


def boxes_crossed(fr, rays6, shrink=0.02):
    """How many instances' boxes (each shrunk by `shrink` of its size on every
    side, so that a count does not hang on rounding) each ray's positive half
    line crosses; float64 slab test, a zero component handled as the planes it
    lies between."""
    lo, hi = instance_boxes(fr)
    pad = (hi - lo) * shrink
    lo, hi = lo + pad, hi - pad
    o, d = rays6[:, None, :3].astype(np.float64), rays6[:, None, 3:6].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo[None] - o) / d, (hi[None] - o) / d
    inside = (o >= lo[None]) & (o <= hi[None])
    zero = d == 0
    tn = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1)).max(2)
    tf = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1)).min(2)
    return ((tn <= tf) & (tf > 0)).sum(1)


def _rotated_about_y(fr):
    """Instances whose inverse rotation mixes x and z alone (M1.x = M1.z = 0,
    M0.x, M0.z, M2.x, M2.z all non-zero), largest meshes first."""
    ins = fr.arrays["instances"]
    M = ins["inv_transform"]
    ok = (M[:, 1, 0] == 0) & (M[:, 1, 2] == 0) & (M[:, 0, 0] != 0) & (M[:, 0, 2] != 0) & (M[:, 2, 0] != 0) & (M[:, 2, 2] != 0)
    idx = np.nonzero(ok)[0]
    return idx[np.argsort(-ins["mesh"][idx, 1].astype(np.int64), kind="stable")]


def _aimed(fr, inst, prim, d, back=40.0):
    """A ray along d through the centroid of triangle `prim` of `inst`, starting `back` units before it."""
    c = R.world_triangle(fr, inst, prim).mean(0)
    d = np.asarray(d, F32)
    n = d.astype(np.float64) / np.linalg.norm(d.astype(np.float64))
    return np.concatenate([(c - back * n).astype(F32), d]).astype(F32)


# ---- finite flags ----------------------------------------------------------------

def world_only_nonfinite(fr, n=96):
    """Rays whose world direction has a zero or denormal x or z component,
    aimed at a triangle of an instance rotated about y, in whose space every
    component's reciprocal is finite: (rays [n, 6], instance [n])."""
    rng = np.random.default_rng(4601)
    insts = _rotated_about_y(fr)[:24]
    rays, who = [], []
    k = 0
    while len(rays) < n:
        inst = int(insts[k % len(insts)])
        tiny = [F32(0.0), F32(-0.0), F32(3e-42), F32(-3e-42)][k % 4]
        d = rng.normal(size=3)
        d[1] = -abs(d[1]) - 0.3
        d = (d / np.linalg.norm(d)).astype(F32)
        d[(k // 4) % 2 * 2] = tiny
        k += 1
        if not recip_finite(object_dir(fr, inst, d)).all():
            continue
        prim = int(rng.integers(0, int(fr.arrays["instances"][inst]["mesh"][1])))
        rays.append(_aimed(fr, inst, prim, d))
        who.append(inst)
    return np.array(rays, F32), np.array(who)


def object_only_nonfinite(fr, n=96):
    """Rays whose world direction has three normal components while the x
    component in the aimed-at instance's space is exactly zero: d = (M2.x,
    dy, -M0.x) gives M0.x * M2.x - M2.x * M0.x there: (rays [n, 6], instance [n])."""
    rng = np.random.default_rng(4602)
    insts = _rotated_about_y(fr)[:24]
    rays, who = [], []
    k = 0
    while len(rays) < n:
        inst = int(insts[k % len(insts)])
        k += 1
        M = fr.arrays["instances"][inst]["inv_transform"].astype(F32)
        s = F32(1.0) if k % 2 else F32(-1.0)
        d = np.array([s * M[2, 0], F32(-rng.uniform(0.2, 1.5)), -s * M[0, 0]], F32)
        if not recip_finite(d).all() or recip_finite(object_dir(fr, inst, d))[0]:
            continue
        prim = int(rng.integers(0, int(fr.arrays["instances"][inst]["mesh"][1])))
        rays.append(_aimed(fr, inst, prim, d))
        who.append(inst)
    return np.array(rays, F32), np.array(who)


def plain_rays(fr):
    """Camera rays of the frame: three normal direction components."""
    rays = R.camera_hits(fr)[0][:, :6].astype(F32)
    return rays[recip_finite(rays[:, 3:]).all(1)]


def flagged_rays(fr):
    """The pool of rays with a non-finite reciprocal at some level: the two
    sets above, axis rays and the scaled family's zero / denormal tail."""
    def make():
        a, _ = world_only_nonfinite(fr)
        b, _ = object_only_nonfinite(fr)
        ax = R.family(fr, "axis")[::6]
        sc = R.family(fr, "scaled")[-240:][1::4]      # the tail's denormal components (3e-42)
        return np.concatenate([a, b, ax, sc]).astype(F32)
    return fr.memo("flagged_rays", make)


def flag_waves(fr):
    """(rays [80 * 64, 6], flagged [80 * 64] bool): 64 groups of 64 with one
    flagged ray, in lane g of group g, then 16 groups whose even (8 groups) or
    odd (8 groups) lanes are flagged."""
    def make():
        f, p = flagged_rays(fr), plain_rays(fr)
        rays = np.zeros((80, 64, 6), F32)
        flag = np.zeros((80, 64), bool)
        for g in range(64):
            flag[g, g] = True
        for g in range(64, 80):
            flag[g, (g % 2)::2] = True
        nf, npl = 0, 0
        for g in range(80):
            for l in range(64):
                if flag[g, l]:
                    rays[g, l] = f[nf % len(f)]
                    nf += 1
                else:
                    rays[g, l] = p[npl % len(p)]
                    npl += 1
        return rays.reshape(-1, 6), flag.reshape(-1)
    return fr.memo("flag_waves", make)


# ---- one finish site -----------------------------------------------------------------

FINISH_LENGTHS = (1, 23, 24, 25, 63, 64, 65, 129)


def escape_rays(fr, n):
    """Rays that start above the scene box and point away from it: no block of the TLAS root is met."""
    rng = np.random.default_rng(4603)
    o = R._box_points(fr, rng, n)
    o[:, 1] = fr.hi[1] + F32(5.0) + rng.uniform(0, 5, n).astype(F32)
    d = rng.normal(size=(n, 3))
    d[:, 1] = np.abs(d[:, 1]) + 0.2
    return np.concatenate([o, R._unit(d)], 1).astype(F32)


def finish_mix(fr):
    """192 rays, four kinds taking turns from the first entry on: a shuffled
    ray (walks for many iterations), an escape ray (its closest-hit walk
    steps the root block and ends at the pop of the next node phase), a
    sun-ward ray the oracle finds shadowed (its any-hit walk ends in a leaf
    phase) and one it finds unshadowed."""
    def make():
        sh = R.family(fr, "shuffled")
        e = R.expected(fr, "shuffled", 1)
        sunny = sun_ward(fr, sh)
        dark, lit = sh[sunny & (e[:, 7] == 1)], sh[sunny & (e[:, 7] == 0)]
        esc = escape_rays(fr, 48)
        out = np.zeros((192, 6), F32)
        out[0::4], out[1::4], out[2::4], out[3::4] = sh[:48], esc, dark[:48], lit[:48]
        return out
    return fr.memo("finish_mix", make)


def sun_ward(fr, rays6):
    """Rows whose direction is within ~11 degrees of the subframe's light."""
    sun = np.array(fr.arrays["subframes"][fr.subframe]["light"]["direction"][:3], np.float64)
    sun /= np.linalg.norm(sun)
    d = rays6[:, 3:6].astype(np.float64)
    return (d @ sun) / np.linalg.norm(d, axis=1) > 0.98


def resume_queue(fr, blocks_waves=4, tail=129):
    """(rays, first_tail_row): `blocks_waves` groups of 64 sun-ward rays the
    oracle finds shadowed - one group per wave of a one-block grid, so every
    wave holds an occluder when it comes back for more - and then `tail`
    sun-ward rays that are not shadowed and start inside the box of at least
    one instance.  A tail walk that takes its wave's candidate ends
    unshadowed, so it walked that instance whole and then the TLAS from the
    root (BlockWalker::resume_tlas)."""
    def make():
        sh = R.family(fr, "shuffled")
        e = R.expected(fr, "shuffled", 1)
        sunny = sun_ward(fr, sh)
        dark = sh[sunny & (e[:, 7] == 1)][: 64 * blocks_waves]
        lit = sh[sunny & (e[:, 7] == 0)]
        lit = lit[boxes_crossed(fr, lit) >= 1][:tail]
        assert len(dark) == 64 * blocks_waves and len(lit) == tail
        return np.concatenate([dark, lit]).astype(F32), len(dark)
    return fr.memo(("resume_queue", blocks_waves, tail), make)
