"""Ray families for the walk-kernel parity tests (helpers of
tests/test_walk_ray_inputs.py and tests/test_gpu_walk_rays.py; not a test
module).  CPU only: numpy, the host scene and the oracle.

Every family is a seeded function of a Frame returning float32 [n, 6] rays
(origin.xyz, direction.xyz), each built to land on a branch of the walk that
a render's own rays reach only by luck:

  axis       zero direction components, both signs of zero: `fin == false`,
             the min/max slab test
  scaled     direction components at both ends of the float exponent range:
             the `!ok` fallback of BlockWalker::enter()
  restart    rays leaving a surface point, along the old direction, into the
             hemisphere and in the triangle's plane: `t > tmin`, `det == 0`
  seams      rays at mesh vertices and edge midpoints: ties between adjacent
             triangles, decided by the reference's leaf order
  nonfinite  NaN and infinite components
  shuffled   unrelated rays side by side: candidates carried between them
  deep       rays that hold many stack entries (a committed fixture)

expect() is the oracle's answer in ptg_walk_rays' record, with the tmin and
tmax the walk kernels use in a bounce round.
"""
import os

import numpy as np

from conftest import GOLDEN, arrays_copy, scene_for
from feature_helpers import camera_rays
from oracle import Oracle

W, H, SPP = 640, 360, 32
MIN_RAY_DIST, MAX_RAY_DIST = np.float32(1e-4), np.float32(1e9)
DEEP_FIXTURE = os.path.join(GOLDEN, "walk_deep_rays_f450.npz")


class Frame:
    """One frame's arrays (reference layout), its oracle and the subframe the rays are traced in."""

    def __init__(self, assets_dir, frame, subframe):
        s = scene_for(assets_dir, W, H, SPP, frame=frame)
        self.frame, self.subframe, self.cfg = frame, subframe, s.cfg
        self.arrays = arrays_copy(s)
        self.oracle = Oracle(self.arrays, s.cfg)
        count, offset = (int(v) for v in self.arrays["subframes"][subframe]["tlas"])
        root = self.arrays["nodes"][offset]
        self.lo, self.hi = np.array(root["min"], np.float32), np.array(root["max"], np.float32)
        self._memo = {}

    def memo(self, key, make):
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]


_frames = {}


def frame_for(assets_dir, frame=450, subframe=1):
    """Session-cached Frame (the arrays are a copy: a later setup_frame of the shared scene leaves them alone)."""
    key = (frame, subframe)
    if key not in _frames:
        _frames[key] = Frame(assets_dir, frame, subframe)
    return _frames[key]


def with_range(rays6, tmin, tmax):
    """[n, 6] -> ptg_trace_rays' [n, 8] layout."""
    rays6 = np.asarray(rays6, np.float32).reshape(-1, 6)
    n = len(rays6)
    return np.concatenate([rays6, np.full((n, 1), tmin, np.float32), np.full((n, 1), tmax, np.float32)], 1)


def closest_range(rnd):
    """The closest-hit walk's (tmin, tmax) in bounce round `rnd` (k_wf_walk)."""
    return (np.float32(0.0) if rnd == 0 else MIN_RAY_DIST), np.float32(1e9)


def as_walk_record(hits):
    """A ptg_trace_rays / Oracle.trace_rays record as ptg_walk_rays returns it:
    word 2 is 0, and words 0-2 are 0 on a miss (thit < 0)."""
    out = np.array(hits, np.uint32)
    out[:, 2] = 0
    miss = out[:, 3].view(np.float32) < 0
    out[miss, :3] = 0
    return out


def expect(fr, rays6, rnd):
    """The oracle's record for ptg_walk_rays(round=rnd): the closest-hit words
    from a query with the closest-hit walk's range, the shadow word from one
    with the any-hit walk's (MIN_RAY_DIST, MAX_RAY_DIST)."""
    tmin, tmax = closest_range(rnd)
    out = fr.oracle.trace_rays(fr.subframe, with_range(rays6, tmin, tmax))
    if rnd == 0:
        out[:, 7] = fr.oracle.trace_rays(fr.subframe, with_range(rays6, MIN_RAY_DIST, MAX_RAY_DIST))[:, 7]
    return as_walk_record(out)


def differing_rows(got, want):
    """Rows whose compared words differ: words 0, 1, 3, 4, 5, 6 on a hit, 3 and
    4 on a miss, word 7 always (exact equality; `want` says hit or miss)."""
    got, want = np.asarray(got, np.uint32), np.asarray(want, np.uint32)
    hit = want[:, 3].view(np.float32) >= 0
    ne = got != want
    bad = ne[:, 7] | ne[:, 3] | ne[:, 4] | (hit & (ne[:, 0] | ne[:, 1] | ne[:, 5] | ne[:, 6]))
    return np.nonzero(bad)[0]


def hit_mask(rec):
    return np.asarray(rec)[:, 3].view(np.float32) >= 0


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def _box_points(fr, rng, n, margin=0.0):
    lo, hi = fr.lo.astype(np.float64), fr.hi.astype(np.float64)
    pad = (hi - lo) * margin
    return rng.uniform(lo - pad, hi + pad, (n, 3)).astype(np.float32)


def _down_grid(fr, k):
    """k x k origins above the scene box, over the inner 80% of its footprint."""
    xs = np.linspace(fr.lo[0] * 0.8 + fr.hi[0] * 0.2, fr.lo[0] * 0.2 + fr.hi[0] * 0.8, k)
    zs = np.linspace(fr.lo[2] * 0.8 + fr.hi[2] * 0.2, fr.lo[2] * 0.2 + fr.hi[2] * 0.8, k)
    gx, gz = np.meshgrid(xs, zs)
    y = np.full(k * k, float(fr.hi[1]) + 10.0)
    return np.stack([gx.reshape(-1), y, gz.reshape(-1)], 1).astype(np.float32)


# ---- axis -----------------------------------------------------------------

def axis(fr):
    """~1500 rays with one or two zero direction components, each zero as +0.0
    and as -0.0: the six axis directions from points of the scene box, in-plane
    diagonals (a, 0, b) from such points, and a grid above the scene looking
    straight down."""
    rng = np.random.default_rng(4501)
    pz, nz = np.float32(0.0), np.float32(-0.0)
    dirs = []
    for ax in range(3):
        for s in (1.0, -1.0):
            for z0 in (pz, nz):
                for z1 in (pz, nz):
                    d = [z0, z1]
                    d.insert(ax, np.float32(s))
                    dirs.append(d)
    dirs = np.array(dirs, np.float32)                       # 24 axis directions
    o1 = _box_points(fr, rng, 25 * len(dirs))
    r1 = np.concatenate([o1, np.tile(dirs, (25, 1))], 1)
    n2 = 500
    d2 = rng.normal(size=(n2, 3)).astype(np.float32)
    d2[np.arange(n2), np.arange(n2) % 3] = np.where(np.arange(n2) % 2 == 0, pz, nz)
    r2 = np.concatenate([_box_points(fr, rng, n2), d2], 1)
    o3 = _down_grid(fr, 20)
    d3 = np.zeros((len(o3), 3), np.float32)
    d3[:, 1] = -1.0
    d3[:, 0] = np.where(np.arange(len(o3)) % 2 == 0, pz, nz)
    d3[:, 2] = np.where(np.arange(len(o3)) % 4 < 2, pz, nz)
    r3 = np.concatenate([o3, d3], 1)
    return np.concatenate([r1, r2, r3]).astype(np.float32)


# ---- scaled ---------------------------------------------------------------

# unit directions times m * 2^k.  A component of a unit vector in [0.5, 1) has
# the biased exponent 126, so it lands at 126 + k: 1 (k = -125), 252 (126), 253
# (127) and, times 1.9, 254; smaller components fall below, into the denormals
# (exponent 0) for k = -125 and -120.  rcp_nr's range is [1, 252].
SCALES = [(-125, 1.0), (-120, 1.0), (-100, 1.0), (100, 1.0), (125, 1.0), (126, 1.0), (127, 1.0), (127, 1.9)]
EXPONENT_CLASSES = (0, 1, 252, 253, 254)


def biased_exponents(d):
    """The biased exponent of every direction component (0: zero or denormal)."""
    return (np.ascontiguousarray(d, np.float32).view(np.uint32) >> 23) & 0xFF


def scaled(fr):
    """~1500 rays from a grid just above the scene box, looking down at a
    seeded tilt, so that the unit ray hits the terrain: 1280 with the
    direction scaled by SCALES, and 240 unit directions with one denormal or
    1e-30 component beside normal ones.  t scales inversely: an upscaled ray
    hits at a tiny t (below MIN_RAY_DIST: only round 0, tmin 0, takes it), a
    downscaled one misses against tmax 1e9; the mixed ones hit."""
    rng = np.random.default_rng(4502)
    n = 1280
    o = _down_grid(fr, 36)[rng.permutation(36 * 36)[:n]]
    o[:, 1] = fr.hi[1] + np.float32(1.0)
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.6                       # downwards: the unit ray hits the terrain
    d = _unit(d)
    k, m = np.array(SCALES)[np.arange(n) % len(SCALES)].T
    d = (d.astype(np.float64) * (m * np.exp2(k))[:, None]).astype(np.float32)
    assert np.isfinite(d).all()
    n2 = 240
    o2 = _down_grid(fr, 16)[rng.permutation(256)[:n2]]
    d2 = rng.normal(size=(n2, 3))
    d2[:, 1] = -np.abs(d2[:, 1]) - 0.6
    d2 = _unit(d2)
    tiny = np.where(np.arange(n2) % 2 == 0, np.float32(1e-30), np.float32(3e-42))   # 3e-42: a denormal
    tiny = tiny * np.where(np.arange(n2) % 4 < 2, 1, -1).astype(np.float32)
    d2[np.arange(n2), (np.arange(n2) % 2) * 2] = tiny                               # x or z; y stays normal
    return np.concatenate([np.concatenate([o, d], 1), np.concatenate([o2, d2], 1)]).astype(np.float32)


# ---- camera hits (restart, seams, shuffled) -----------------------------------

def camera_hits(fr, n=1024):
    """n camera rays of the frame's subframe (feature_helpers.camera_rays, a
    seeded pixel set) with the oracle's closest hits: (rays [n, 8], hits [n, 8])."""
    def make():
        rng = np.random.default_rng(4503)
        xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1)
        step = fr.cfg.samples_per_motion_blur_step
        js = fr.subframe * step + rng.integers(0, step, n)
        rays, sub = camera_rays(fr.arrays["subframes"], fr.cfg, xy, js)
        assert (sub == fr.subframe).all()
        return rays, fr.oracle.trace_rays(fr.subframe, rays)
    return fr.memo(("camera_hits", n), make)


def world_triangle(fr, inst, prim):
    """The three world-space vertices of triangle `prim` of instance `inst`
    (float64; row vectors times the instance's transform, as the reference
    transforms a point)."""
    rec = fr.arrays["instances"][int(inst)]
    ioff, bv = int(rec["mesh"][2]), int(rec["mesh"][3])
    idx = fr.arrays["indices"][ioff + 3 * int(prim): ioff + 3 * int(prim) + 3].astype(np.int64) + bv
    p = fr.arrays["pos"][idx][:, :3].astype(np.float64)
    T = rec["transform"].astype(np.float64)
    return p @ T[:3, :3] + T[3, :3]


def _hit_points(rays, hits):
    """o + t * d in float32 for the rows that hit: (rows, points)."""
    rows = np.nonzero(hit_mask(hits))[0]
    t = hits[rows, 3].view(np.float32)
    return rows, (rays[rows, :3] + t[:, None] * rays[rows, 3:6]).astype(np.float32)


def restart(fr):
    """3 x (the camera rays that hit) rays starting at the hit point o + t * d
    (float32): (a) along the same d, (b) into a seeded hemisphere direction
    about the geometric normal, (c) along an edge of the hit triangle, in its
    plane.  -> (rays [3m, 6], kind [3m] in 0..2)"""
    rays, hits = camera_hits(fr)
    rows, p = _hit_points(rays, hits)
    rng = np.random.default_rng(4504)
    da = rays[rows, 3:6]
    db, dc = np.zeros_like(da), np.zeros_like(da)
    for k, r in enumerate(rows):
        v = world_triangle(fr, hits[r, 4], hits[r, 5])
        nrm = np.cross(v[1] - v[0], v[2] - v[0])
        nrm /= np.linalg.norm(nrm)
        if np.dot(nrm, da[k].astype(np.float64)) > 0:      # the side the ray came from
            nrm = -nrm
        h = rng.normal(size=3)
        h /= np.linalg.norm(h)
        db[k] = (h if np.dot(h, nrm) > 0 else -h).astype(np.float32)
        e = v[(k + 1) % 3] - v[k % 3]
        dc[k] = (e / np.linalg.norm(e)).astype(np.float32)
    out = np.concatenate([np.concatenate([p, d], 1) for d in (da, db, dc)]).astype(np.float32)
    return out, np.repeat(np.arange(3), len(rows))


def seams(fr):
    """~1024 rays from one origin aimed at world-space vertices (two in three)
    and edge midpoints (float32) of the triangles the camera rays hit; the
    direction is p - o, not normalised, so the hit is at t ~ 1.  The origin is
    the camera position rounded to whole units: p - o then rounds less, and
    more rays meet a vertex or an edge exactly (a barycentric of 0 or 1: 22%
    of the vertex rays, 6% of the midpoint rays; 16% and 5% from the camera
    position itself)."""
    rays, hits = camera_hits(fr)
    rows = np.nonzero(hit_mask(hits))[0]
    o = np.round(np.array(fr.arrays["subframes"][fr.subframe]["cam"]["position"][:3], np.float32))
    pts = []
    for k, r in enumerate(rows):
        v = world_triangle(fr, hits[r, 4], hits[r, 5])
        a, b = v[k % 3], v[(k + 1) % 3]
        pts.append(a if k % 3 != 2 else 0.5 * (a + b))
    pts = np.array(pts).astype(np.float32)[:1024]
    d = (pts - o).astype(np.float32)
    return np.concatenate([np.broadcast_to(o, d.shape), d], 1).astype(np.float32)


# ---- nonfinite --------------------------------------------------------------

def nonfinite(fr):
    """96 rays with NaN or infinite components: one, two or three NaN direction
    components, a +inf or -inf direction component, an inf or NaN origin
    component; the rest of each ray is a ray that would hit the terrain."""
    rng = np.random.default_rng(4505)
    n = 96
    o = _down_grid(fr, 10)[:n].copy()
    d = rng.normal(size=(n, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.6
    d = _unit(d)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for i in range(n):
        kind, c = i % 6, (i // 6) % 3
        if kind == 0:
            d[i, c] = nan
        elif kind == 1:
            d[i, c] = d[i, (c + 1) % 3] = nan
        elif kind == 2:
            d[i, :] = nan
        elif kind == 3:
            d[i, c] = inf if (i // 18) % 2 == 0 else -inf
        elif kind == 4:
            o[i, c] = inf if (i // 18) % 2 == 0 else -inf
        else:
            o[i, c] = nan
    return np.concatenate([o, d], 1).astype(np.float32)


# ---- shuffled ---------------------------------------------------------------

def shuffled(fr):
    """8192 rays permuted with a fixed seed, so that neighbouring lanes and a
    wave's successive groups share nothing: random rays through the scene box,
    sun-ward rays from surface points (the camera rays' hits and points under
    the down-grid), and camera rays."""
    def make():
        rng = np.random.default_rng(4506)
        rays, hits = camera_hits(fr)
        n1 = 3072
        d1 = rng.normal(size=(n1, 3))
        d1[::3, 1] = -np.abs(d1[::3, 1])                   # one in three looks down, the others up: most of those leave the scene
        d1[1::3, 1] = np.abs(d1[1::3, 1])
        d1[2::3, 1] = np.abs(d1[2::3, 1])
        r1 = np.concatenate([_box_points(fr, rng, n1), _unit(d1)], 1)
        # surface points: the camera hits, and the terrain under a grid; each several times with a jittered sun direction
        _, p = _hit_points(rays, hits)
        down = with_range(np.concatenate([_down_grid(fr, 32), np.tile(np.float32([0, -1, 0]), (1024, 1))], 1), 0.0, 1e9)
        _, pd = _hit_points(down, fr.oracle.trace_rays(fr.subframe, down))
        pts = np.concatenate([p, pd])
        n2 = 4096
        pts = pts[rng.integers(0, len(pts), n2)]
        sun = np.array(fr.arrays["subframes"][fr.subframe]["light"]["direction"][:3], np.float64)   # points at the light
        d2 = _unit(sun / np.linalg.norm(sun) + 0.05 * rng.normal(size=(n2, 3)))
        o2 = (pts + np.float32(1e-3) * d2).astype(np.float32)
        r2 = np.concatenate([o2, d2], 1)
        r3 = rays[:, :6]
        out = np.concatenate([r1, r2, r3]).astype(np.float32)
        assert len(out) == 8192
        return out[rng.permutation(len(out))]
    return fr.memo("shuffled", make)


def shuffled_tiled(fr, n=196700):
    """The shuffled set tiled to n rays, the origins of every copy jittered by
    up to a millimetre (seeded)."""
    base = shuffled(fr)
    rng = np.random.default_rng(4507)
    out = np.tile(base, ((n + len(base) - 1) // len(base), 1))[:n].copy()
    out[len(base):, :3] += rng.uniform(-1e-3, 1e-3, (n - len(base), 3)).astype(np.float32)
    return out


# ---- deep -------------------------------------------------------------------

def deep_candidates(fr, n, seed):
    """The pool the deep fixture was searched in: long grazing rays through
    the vegetation and along the terrain - origins near the ground on the
    scene box's rim and inside it, directions within a few degrees of
    horizontal."""
    rng = np.random.default_rng(seed)
    o = _box_points(fr, rng, n)
    ground = float(fr.lo[1])
    o[:, 1] = (ground + rng.uniform(0.0, 0.35, n) * float(fr.hi[1] - fr.lo[1])).astype(np.float32)
    d = rng.normal(size=(n, 3))
    d[:, 1] = rng.normal(scale=0.08, size=n)
    return np.concatenate([o, _unit(d)], 1).astype(np.float32)


def deep(fr=None):
    """The committed fixture: float32 [n <= 8192, 6]."""
    return np.load(DEEP_FIXTURE)["rays"].astype(np.float32)


# ---- shared, computed once per frame ------------------------------------------

FAMILIES = {"axis": axis, "scaled": scaled, "restart": lambda fr: restart(fr)[0], "seams": seams,
            "nonfinite": nonfinite, "shuffled": shuffled, "deep": deep}


def family(fr, name):
    """The named family's rays for `fr`, built once."""
    return fr.memo(("family", name), lambda: FAMILIES[name](fr))


def expected(fr, name, rnd):
    """expect() of the named family in round `rnd`, computed once; treat as read-only."""
    return fr.memo(("expect", name, rnd), lambda: expect(fr, family(fr, name), rnd))
