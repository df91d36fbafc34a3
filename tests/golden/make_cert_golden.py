"""Makes tests/golden/cert_midpoints.npz: arguments of the seven MathFast
wrappers (csrc/device/ref_math.h) whose reference double lies within 64 double
ulps of a float rounding midpoint - the cases a rounding certificate exists
for, which random inputs meet about once in 10^7.

Method: with the other arguments fixed, one argument runs over all 2^23 floats
of a binade through the probe library's host reference (math_ref_scan,
tests/math_probe/math_ref.cpp: the reference's plain expression with this
host's libm); about 2 of them land that close.  Scans go on, in a fixed seeded
order, until every wrapper has at least 256 cases, 64 of them at distance
<= 12 and 64 at distance >= 53.  The scanned argument and its binades:
  acc_exp                   x over [-8, -1/4), acc in [0, 50]
  exp_times                 s over a binade of (2^-4, 2^20), x = -h / H
  add_mul_pow               x over [1/8, 1), a, b in [0, 1], y = 5
  div_mul_pow               x over [1/16, 4) (the Mie phase's 1 + g^2 - 2 g mu
                            spans [0.04, 3.24]), a one of its numerators,
                            b = 2 + g^2, y = 1.5; mu itself has too few floats
                            for 256 cases
  times_cos, times_sin      phi over [1/4, 2 pi], s in [0, 1]
  times_one_minus_div_pow   bpdf over a binade of [2^-10, 2^14), r in (0, 1]
The file holds arguments and recorded results only: per wrapper NAME,
NAME_args (n, 4) float64, NAME_v (n) uint64 the reference double's bits,
NAME_dist (n) uint32 its distance from the midpoint in double ulps.

Usage: python tests/golden/make_cert_golden.py   (after build())
"""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import math_inputs as M  # noqa: E402

F32, F64, U32 = np.float32, np.float64, np.uint32
MAX_DIST = 64
NEED_ALL, NEED_NEAR, NEED_FAR = 256, 64, 64
NEAR, FAR = 12, 53
BATCH = 32


def _fbits(x):
    return int(np.array(x, F32).view(U32))


def plan(name, i):
    """Scan i of a wrapper: (fixed args, scanned argument, first float's bits, count)."""
    rng = np.random.default_rng([M.SEED, M.SITE[name], i])
    unit = lambda: float(M._unit(rng, 1)[0])
    full = 1 << 23
    if name == "acc_exp":
        k = int(rng.integers(-2, 3))
        return [float(F32(50.0 * unit())), 0, 0, 0], 1, _fbits(-(2.0 ** k)), full
    if name == "exp_times":
        return [float(M._height_x(rng, 1)[0]), 0, 0, 0], 1, _fbits(2.0 ** int(rng.integers(-4, 20))), full
    if name == "add_mul_pow":
        return [unit(), unit(), 0, 5.0], 2, _fbits(2.0 ** int(rng.integers(-3, 0))), full
    if name == "div_mul_pow":
        a = M.mie_args(np.array([2.0 * unit() - 1.0], F32))
        return [float(a[0, 0]), float(a[1, 0]), 0, 1.5], 2, _fbits(2.0 ** int(rng.integers(-4, 2))), full
    if name in ("times_cos", "times_sin"):
        k = int(rng.integers(-2, 3))
        count = full if k < 2 else _fbits(M.TWO_PI_F) - _fbits(4.0) + 1
        return [unit(), 0, 0, 0], 1, _fbits(2.0 ** k), count
    return [float(F32(1.0) - F32(unit())), M.GAMMA, 0, 0.25], 2, _fbits(2.0 ** int(rng.integers(-10, 14))), full


def scan(name, i):
    fixed, arg, base, count = plan(name, i)
    fx = np.array(fixed, F64)
    bits = np.zeros(64, U32)
    dist = np.zeros(64, U32)
    n = M.lib().math_ref_scan(M.SITE[name], fx.ctypes.data, arg, base, count, MAX_DIST, 64, bits.ctypes.data, dist.ctypes.data)
    n = min(n, 64)
    args = np.tile(fx[:, None], (1, n))
    args[arg] = bits[:n].view(F32).astype(F64)
    return args, dist[:n]


def collect(name, pool):
    args, dist, i = [], [], 0
    while True:
        for a, d in pool.map(lambda j: scan(name, j), range(i, i + BATCH)):
            args.append(a)
            dist.append(d)
        i += BATCH
        d = np.concatenate(dist)
        if len(d) >= NEED_ALL and (d <= NEAR).sum() >= NEED_NEAR and (d >= FAR).sum() >= NEED_FAR:
            break
    a = np.concatenate(args, axis=1)
    _, v, _, _ = M.ref_wrapper(M.SITE[name], a)
    print("%-26s %4d scans, %4d cases, %3d at <= %d, %3d at >= %d" % (name, i, len(d), (d <= NEAR).sum(), NEAR,
                                                                  (d >= FAR).sum(), FAR), flush=True)
    return a.T.copy(), v, d


def main():
    out = {}
    with ThreadPoolExecutor(max_workers=8) as pool:
        for name in M.SITES:
            a, v, d = collect(name, pool)
            out[name + "_args"], out[name + "_v"], out[name + "_dist"] = a, v, d.astype(U32)
    np.savez_compressed(M.FIXTURE, **out)
    print("wrote", M.FIXTURE, os.path.getsize(M.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
