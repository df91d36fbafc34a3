"""Inputs and host-side models for the math probe tests (CPU).

tests/test_math_inputs.py checks this file against itself and against the
probe library's host reference (tests/math_probe/math_ref.cpp: the reference's
plain expressions with this host's libm); tests/test_gpu_math_probe.py feeds
the same inputs to the device code of csrc/device/{ref_math,glibc_math}.h.

Contents:
  * a model of float_certain on integer bit patterns (model_certain);
  * the constructed float_certain cases (certain_cases);
  * per wrapper: the ordinary cases from the path's own domains, the edge
    cases, and the committed near-midpoint fixture (tests/golden/
    cert_midpoints.npz, made by tests/golden/make_cert_golden.py);
  * must_certify: which cases the device has to certify, from the reference
    alone;
  * the arguments of the library-function comparison (lib_cases).

A wrapper's cases are a float64 array of shape (4, n): row k is argument k in
the wrapper's own order (math_probe.hip), float arguments widened.
"""
import ctypes as C
import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "tests", "math_probe", "_build", "libmath_probe.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "cert_midpoints.npz")

SITES = ["acc_exp", "exp_times", "add_mul_pow", "div_mul_pow", "times_cos", "times_sin", "times_one_minus_div_pow"]
SITE = {name: k for k, name in enumerate(SITES)}
TOMDP = SITE["times_one_minus_div_pow"]
# ref_math.h: kCertUlps, kMaxLibDist (the GPU test checks them against the library's)
CERT_ULPS = 32
MAX_LIB_DIST = 4
# each wrapper's own bound K on |v_fast - v_glibc| in double ulps, from its
# comment with D = kMaxLibDist: 2 (D + 1), 2 (2 D + 1), 2 (2 D + 2), 4 (D + 1),
# and times_one_minus_div_pow's margin at s <= 0
K_BOUND = {"acc_exp": 10, "exp_times": 18, "times_cos": 18, "times_sin": 18, "add_mul_pow": 20, "div_mul_pow": 20,
           "times_one_minus_div_pow": 42}
LIB_FNS = ["exp", "pow", "sin", "cos", "pow5_d", "pow_quarter_d"]
POW_YS = [5.0, 0.25, 1.5, float(np.float32(1.0) / np.float32(2.4))]
N_ORDINARY = 1 << 17
SEED = 20240611

GAMMA = float(np.float32(0.15))                      # REGULARIZATION_GAMMA widened
BPDF_EDGE = np.float32(GAMMA ** 4)                  # (float)(0.15^4): q crosses 1 here
BPDF_MUST = 2.0 * 0.15 ** 4                          # must_certify's restriction of times_one_minus_div_pow

U64, U32, F64, F32 = np.uint64, np.uint32, np.float64, np.float32
SIGN = U64(1 << 63)
MAG = U64((1 << 63) - 1)
INF = U64(0x7ff0 << 48)


# ---------------------------------------------------------------- the library
_lib = None


def lib():
    """The probe library (host reference and device entry points)."""
    global _lib
    if _lib is None:
        assert os.path.exists(LIB_PATH), "build it first: __graft_entry__.build() (tests/math_probe/Makefile)"
        L = C.CDLL(LIB_PATH)
        P, u32, i32 = C.c_void_p, C.c_uint32, C.c_int
        L.math_ref_wrapper.argtypes = [i32, u32, P, P, P, P]
        L.math_ref_wrapper.restype = None
        L.math_ref_lib.argtypes = [i32, u32, P, C.c_double, P]
        L.math_ref_lib.restype = None
        L.math_ref_mie_args.argtypes = [u32, P, P]
        L.math_ref_mie_args.restype = None
        L.math_ref_scan.argtypes = [i32, P, i32, u32, u32, u32, u32, P, P]
        L.math_ref_scan.restype = u32
        L.math_probe_float_certain.argtypes = [u32, P, P, P]
        L.math_probe_wrapper.argtypes = [i32, u32, P, P, P, P]
        L.math_probe_wrapper_lds.argtypes = [i32, u32, u32, P, P]
        L.math_probe_lib.argtypes = [i32, u32, P, C.c_double, P]
        for f in (L.math_probe_float_certain, L.math_probe_wrapper, L.math_probe_wrapper_lds, L.math_probe_lib):
            f.restype = i32
        for f in (L.math_probe_cert_ulps, L.math_probe_max_lib_dist, L.math_probe_args):
            f.restype = u32
        _lib = L
    return _lib


def ref_wrapper(site, args):
    """The host reference of a wrapper: (float bits, double bits, q, w); q and
    w only for times_one_minus_div_pow (zeros otherwise)."""
    args = np.ascontiguousarray(args, F64)
    n = args.shape[1]
    f = np.zeros(n, U32)
    v = np.zeros(n, U64)
    qw = np.zeros((2, n), F64)
    lib().math_ref_wrapper(site, n, args.ctypes.data, f.ctypes.data, v.ctypes.data, qw.ctypes.data)
    return f, v, qw[0], qw[1]


def ref_lib(fn, x_bits, y=0.0):
    x_bits = np.ascontiguousarray(x_bits, U64)
    out = np.zeros(len(x_bits), U64)
    lib().math_ref_lib(fn, len(x_bits), x_bits.ctypes.data, y, out.ctypes.data)
    return out


# ------------------------------------------------------ float_certain's model
def f32_of(u):
    """float bits of the double with bits u, round to nearest even."""
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(u, U64).view(F64).astype(F32).view(U32)


def is_nan64(u):
    return (u & MAG) > INF


def interval(u, m):
    """[u - m, u + m] on the pattern line, clipped at +-0 and +-inf of u's sign."""
    mag, sign, m = u & MAG, u & SIGN, np.asarray(m).astype(U64)
    lo = np.where(mag > m, mag - m, U64(0))
    hi = np.minimum(mag + m, INF)
    return lo | sign, hi | sign


def model_certain(u, m):
    """Every double within m patterns of u rounds to u's float: rounding is
    monotone, so the two end points decide.  NaN is never certain."""
    lo, hi = interval(u, m)
    return (f32_of(lo) == f32_of(hi)) & ~is_nan64(u)


def model_certain_enumerated(u, m):
    """The same by rounding every pattern of the interval (m a scalar)."""
    mag, sign = u & MAG, u & SIGN
    ok = ~is_nan64(u)
    f0 = f32_of(u)
    for d in range(-m, m + 1):
        p = np.clip(mag.astype(np.int64) + d, 0, int(INF)).astype(U64) | sign
        ok &= f32_of(p) == f0
    return ok


def wrapper_margin(s):
    """times_one_minus_div_pow's margin for exponent difference s."""
    return 4 * (((2 * MAX_LIB_DIST + 1) << max(int(s), 0)) + 1) + 2


MARGINS = [10, 18, 20, CERT_ULPS] + [wrapper_margin(s) for s in range(17)]
SMALL_MARGIN = 64     # up to here every offset -(m+2)..(m+2); beyond, -2..2 about anchor-m, anchor, anchor+m


def _offsets(m):
    if m <= SMALL_MARGIN:
        return np.arange(-(m + 2), m + 3, dtype=np.int64)
    d = np.arange(-2, 3, dtype=np.int64)
    return np.concatenate([d - m, d, d + m])


def _q_of(e):
    """Bits below float's quantum in the binade of double exponent e, as
    float_certain has them; 29 outside float's range too (any anchor will do)."""
    return np.where((e >= 1023 - 151) & (e < 1023 - 126), 926 - e, 29)


def certain_anchors():
    """Magnitude patterns (int64) the float_certain cases are built around."""
    rng = np.random.default_rng(SEED)
    e = np.arange(2048, dtype=np.int64)
    q = _q_of(e)
    top = rng.integers(0, 1 << 52, size=2048, dtype=np.int64)
    m52 = (1 << 52) - 1
    value = (top >> q << q) & m52                                         # a float: the low q bits zero
    half = np.where(q <= 52, np.int64(1) << np.minimum(q - 1, 62), 0)
    mid_even = ((top >> (q + 1) << (q + 1)) | (np.int64(1) << np.minimum(q, 62)) | half) & m52   # lower float odd
    mid_odd = ((top >> (q + 1) << (q + 1)) | half) & m52                  # lower float even
    first = np.zeros(2048, np.int64)
    last = np.full(2048, m52, np.int64)
    per_e = np.stack([value, mid_even, mid_odd, first, last]) | (e << 52)[None, :]
    d = lambda x: int(np.array(x, F64).view(np.int64))
    flt_max = float(np.finfo(F32).max)
    edges = [d(2.0 ** -151), d(2.0 ** -150), d(2.0 ** -149), d(1.5 * 2.0 ** -149), d(2.0 ** -126), d(flt_max),
             d(flt_max + 2.0 ** 103), d(2.0 ** 128), d(np.inf), 0x7ff8000000000000, 0x7ff0000000000001,
             0x7ff4000000000000, 0x7fffffffffffffff, 0, 1, (1 << 52) - 1]
    a = np.concatenate([per_e.reshape(-1), np.array(edges, np.int64)])
    return np.minimum(a, (1 << 63) - 1 - (1 << 22))       # room for the largest offset


_certain_cases = None


def certain_cases():
    """(patterns uint64, margins uint32): every anchor x both signs x every
    margin x that margin's offsets, and 2^16 random patterns."""
    global _certain_cases
    if _certain_cases is None:
        a = certain_anchors()
        us, ms = [], []
        for m in MARGINS:
            mag = np.clip(a[:, None] + _offsets(m)[None, :], 0, (1 << 63) - 1).reshape(-1).astype(U64)
            for sign in (U64(0), SIGN):
                us.append(mag | sign)
                ms.append(np.full(len(mag), m, U32))
        rng = np.random.default_rng(SEED + 1)
        us.append(rng.integers(0, 1 << 64, size=1 << 16, dtype=U64))
        ms.append(np.array(MARGINS, U32)[rng.integers(0, len(MARGINS), size=1 << 16)])
        _certain_cases = (np.concatenate(us), np.concatenate(ms))
    return _certain_cases


# --------------------------------------------------------- the wrappers' cases
def _cols(*cols):
    n = max(np.size(c) for c in cols)
    out = np.zeros((4, n), F64)
    for k, c in enumerate(cols):
        out[k] = np.asarray(c, F64)
    return out


def _unit(rng, n):
    """floats in [0, 1) on the 2^-24 grid, as the path's uniform4 gives them."""
    return (rng.integers(0, 1 << 24, size=n).astype(F32) * F32(2.0 ** -24)).astype(F32)


def _height_x(rng, n):
    """x = -h / H as a float: h in [0, 1e5], H one of the two scale heights."""
    h = (_unit(rng, n) * F32(1.0e5)).astype(F32)
    H = np.where(rng.integers(0, 2, size=n) == 0, F32(7994.0), F32(1200.0)).astype(F32)
    return ((-h) / H).astype(F32)


def mie_args(mu):
    mu = np.ascontiguousarray(mu, F32)
    out = np.zeros((4, len(mu)), F64)
    lib().math_ref_mie_args(len(mu), mu.ctypes.data, out.ctypes.data)
    return out


TWO_PI_F = F32(2.0) * F32(math.pi)

_ordinary = {}


def ordinary_cases(name, n=N_ORDINARY):
    """Seeded cases from the domain the path gives the wrapper."""
    if (name, n) in _ordinary:
        return _ordinary[(name, n)]
    rng = np.random.default_rng(SEED + 16 + SITE[name])
    if name == "acc_exp":
        a = _cols((_unit(rng, n) * F32(50.0)).astype(F32), _height_x(rng, n))
    elif name == "exp_times":
        a = _cols(_height_x(rng, n), ((F32(1.0) - _unit(rng, n)) * F32(1.0e6)).astype(F32))
    elif name == "add_mul_pow":
        a = _cols(_unit(rng, n), _unit(rng, n), _unit(rng, n), np.full(n, 5.0))
    elif name == "div_mul_pow":
        a = mie_args((F32(2.0) * _unit(rng, n) - F32(1.0)).astype(F32))
    elif name in ("times_cos", "times_sin"):
        a = _cols(_unit(rng, n), (TWO_PI_F * _unit(rng, n)).astype(F32))
    else:
        bpdf = np.power(10.0, 8.0 * rng.random(n) - 4.0).astype(F32)
        a = _cols((F32(1.0) - _unit(rng, n)).astype(F32), np.full(n, GAMMA), bpdf, np.full(n, 0.25))
    _ordinary[(name, n)] = a
    return a


def fixture_cases(name):
    """(args, v_bits, dist) of the committed near-midpoint cases."""
    g = np.load(FIXTURE)
    return g[name + "_args"], g[name + "_v"], g[name + "_dist"]


def bpdf_sweep():
    """times_one_minus_div_pow: every float bpdf within 2^17 float ulps either
    side of (float)(0.15^4), at r in {1, 0.37, 2^-120}."""
    c = int(BPDF_EDGE.view(U32))
    bpdf = np.arange(c - (1 << 17), c + (1 << 17) + 1, dtype=U32).view(F32).astype(F64)
    parts = [_cols(np.full(len(bpdf), float(F32(r))), np.full(len(bpdf), GAMMA), bpdf, np.full(len(bpdf), 0.25))
             for r in (1.0, 0.37, 2.0 ** -120)]
    return np.concatenate(parts, axis=1)


_SPECIAL = np.array([-1.0, -0.37, -2.0 ** -130, -0.0, 0.0, np.inf, -np.inf, np.nan, 1.0, 0.25, 2.0 ** -24, 1.0 + 2.0 ** -23,
                     3.0 * 2.0 ** -25, 2.0 ** -149, float(np.finfo(F32).max)], F64)


def _grid(*axes):
    g = np.meshgrid(*[np.asarray(a, F64) for a in axes], indexing="ij")
    return [x.reshape(-1) for x in g]


def exact_arg_cases(name):
    """The exact-argument shortcuts (x = 0, phi = 0, pow_exact_arg's x = 1 and
    x = +-0 with y > 0) with other arguments of every kind: exact float ties
    (1 + 2^-24, 2^-24 + 1), negatives, -0, inf, NaN.  fail_mask must be 0."""
    sp = _SPECIAL
    if name == "acc_exp":
        acc, x = _grid(sp, [0.0, -0.0])
        return _cols(acc, x)
    if name == "exp_times":
        x, s = _grid([0.0, -0.0], sp)
        return _cols(x, s)
    if name == "add_mul_pow":
        a, b, x = _grid(sp, sp, [1.0, 0.0, -0.0])
        return _cols(a, b, x, np.full(len(a), 5.0))
    if name == "div_mul_pow":
        a, b, x = _grid(sp, [2.640000104904175, 1.0, 3.0, -3.0, 0.0, np.nan], [1.0, 0.0, -0.0])
        return _cols(a, b, x, np.full(len(a), 1.5))
    if name in ("times_cos", "times_sin"):
        s, phi = _grid(sp, [0.0, -0.0])
        return _cols(s, phi)
    r, x = _grid(sp, [1.0, 0.0, -0.0])
    return _cols(r, np.full(len(r), GAMMA), x, np.full(len(r), 0.25))


def edge_cases(name, n=1 << 14):
    """Negative / -0 / inf / NaN in each checked argument with ordinary others,
    and results in float's subnormal range [2^-151, 2^-126) and at overflow."""
    rng = np.random.default_rng(SEED + 64 + SITE[name])
    o = ordinary_cases(name)[:, :n].copy()
    sp = _SPECIAL[rng.integers(0, len(_SPECIAL), size=n)]
    tiny = np.ldexp(1.0 + _unit(rng, n).astype(F64), rng.integers(-153, -120, size=n)).astype(F32).astype(F64)
    huge = np.ldexp(1.0 + _unit(rng, n).astype(F64), rng.integers(100, 128, size=n)).astype(F32).astype(F64)
    parts = []
    if name == "acc_exp":
        parts.append(_cols(sp, o[1]))
        parts.append(_cols(np.where(rng.integers(0, 2, size=n) == 0, 0.0, tiny), -(87.0 + 18.0 * _unit(rng, n)).astype(F32)))
        parts.append(_cols(huge, o[1]))
        parts.append(_cols(o[0], (88.0 + 2.0 * _unit(rng, n)).astype(F32)))
    elif name == "exp_times":
        parts.append(_cols(o[0], sp))
        parts.append(_cols(o[0], -o[1]))
        parts.append(_cols(o[0], tiny))
        parts.append(_cols(-(60.0 + 40.0 * _unit(rng, n)).astype(F32), np.ldexp(o[1], -20).astype(F32)))
        parts.append(_cols((F32(80.0) * _unit(rng, n)).astype(F32), huge))
    elif name == "add_mul_pow":
        parts.append(_cols(sp, o[1], o[2], o[3]))
        parts.append(_cols(o[0], sp, o[2], o[3]))
        parts.append(_cols(-o[0], o[1], o[2], o[3]))
        parts.append(_cols(o[0], -o[1], o[2], o[3]))
        parts.append(_cols(np.where(rng.integers(0, 2, size=n) == 0, 0.0, tiny), tiny, o[2], o[3]))
        parts.append(_cols(0.0, o[1], np.ldexp(o[2], -27).astype(F32), o[3]))
        parts.append(_cols(huge, huge, o[2], o[3]))
    elif name == "div_mul_pow":
        parts.append(_cols(sp, o[1], o[2], o[3]))
        parts.append(_cols(tiny, o[1], o[2], o[3]))
        parts.append(_cols(huge, o[1], np.ldexp(o[2], -10), o[3]))
        parts.append(_cols(o[0], o[1], sp, o[3]))
    elif name in ("times_cos", "times_sin"):
        parts.append(_cols(sp, o[1]))
        parts.append(_cols(-o[0], o[1]))
        parts.append(_cols(tiny, o[1]))
        parts.append(_cols(huge, o[1]))
        parts.append(_cols(o[0], np.ldexp(o[1], -rng.integers(20, 150, size=n)).astype(F32)))
    else:
        parts.append(_cols(sp, o[1], o[2], o[3]))
        parts.append(_cols(-o[0], o[1], o[2], o[3]))
        parts.append(_cols(tiny, o[1], o[2], o[3]))
        parts.append(_cols(huge, o[1], o[2], o[3]))
        parts.append(_cols(o[0], o[1], sp, o[3]))
    return np.concatenate(parts, axis=1)


def all_cases(name):
    """{class: args} of every case of a wrapper."""
    c = {"ordinary": ordinary_cases(name), "fixture": fixture_cases(name)[0].T.copy(), "exact": exact_arg_cases(name),
         "edge": edge_cases(name)}
    if name == "times_one_minus_div_pow":
        c["sweep"] = bpdf_sweep()
    return c


# ------------------------------------------------- what the reference implies
def exact_arg(name, args):
    """The wrapper's exact-argument shortcut applies (ref_math.h)."""
    if name in ("acc_exp", "times_cos", "times_sin"):
        return args[1] == 0.0
    if name == "exp_times":
        return args[0] == 0.0
    x, y = args[2], args[3]
    return (x == 1.0) | ((x == 0.0) & (y > 0.0))


def precondition(name, args):
    """The sign preconditions the wrapper's bound needs (NaN fails them)."""
    with np.errstate(invalid="ignore"):
        if name == "acc_exp":
            return args[0] >= 0.0
        if name == "add_mul_pow":
            return (args[0] >= 0.0) & (args[1] >= 0.0)
        if name == "times_one_minus_div_pow":
            return args[0] >= 0.0
    return np.ones(args.shape[1], bool)


def _exponent(x):
    return (np.ascontiguousarray(x, F64).view(U64) >> U64(52) & U64(0x7ff)).astype(np.int64)


def tomdp_state(args):
    """times_one_minus_div_pow from the reference's q and w alone, allowing the
    fast q its (2 D + 1) ulps: `zero` - the fast q certainly exceeds 1 + 2^-48;
    `big_s` - the fast s certainly exceeds 16 (or its w is 0 with q <= 1 + 2^-48);
    `margin_hi` - an upper bound of the device's margin where s may be <= 16
    (the fast q and w may each sit one binade off the reference's: s + 2)."""
    _, _, q, w = ref_wrapper(TOMDP, args)
    dq = (2 * MAX_LIB_DIST + 1) * 2.0 ** -52
    with np.errstate(invalid="ignore"):
        zero = q > 1.0 + 2.0 ** -48 + dq
        big_s = (q <= 1.0) & (q >= 0.5) & (w + dq < 2.0 ** -18)
    s = _exponent(q) - _exponent(w)
    s_hi = np.clip(s + 2, 0, 40)
    margin_hi = 4 * (((2 * MAX_LIB_DIST + 1) << s_hi) + 1) + 2
    return zero, big_s, s_hi, margin_hi


def must_certify(name, args):
    """Cases the device has to certify, judged from the reference alone: the
    preconditions hold and the reference double is farther than margin + K
    patterns from every float rounding boundary.  The fast double is within K
    of it, so the whole interval the device checks rounds to one float, and a
    tight float_certain says so.  times_one_minus_div_pow: the device's margin
    is at most margin_hi, and K is the wrapper's own bound at s + 2 where that
    exceeds 42; only bpdf >= 2 * 0.15^4 is judged, where s stays small."""
    _, v, _, _ = ref_wrapper(SITE[name], args)
    ok = precondition(name, args) & ~is_nan64(v)
    if name != "times_one_minus_div_pow":
        return ok & model_certain(v, np.full(len(v), CERT_ULPS + K_BOUND[name], U64))
    _, _, s_hi, margin_hi = tomdp_state(args)
    k = np.maximum(margin_hi, K_BOUND[name])
    return ok & (args[2] >= BPDF_MUST) & (s_hi <= 16) & model_certain(v, (margin_hi + k).astype(U64))


def must_refuse_fixture(name, dist):
    """Fixture cases the device cannot certify: the fast double is within K of
    the reference's, so within 32 of the midpoint when dist <= 32 - K (no case
    for times_one_minus_div_pow, whose K exceeds 32)."""
    return dist.astype(np.int64) <= CERT_ULPS - K_BOUND[name]


# ------------------------------------------------------ the library functions
SINCOS_MAX = 105414350.0


def _d(x):
    return int(np.array(x, F64).view(U64))


def _around(centres, below=64, above=64, signs=(0,)):
    out = []
    for c in centres:
        p = np.arange(c - below, c + above + 1, dtype=np.int64)
        p = p[(p >= 0)].astype(U64)
        for s in signs:
            out.append(p | (SIGN if s else U64(0)))
    return np.concatenate(out)


def _nonfloat(u):
    """Make sure no pattern is a float widened: some bit below float's 24 set."""
    return np.where((u & U64(0x1fffffff)) == 0, u | U64(1), u)


def _in_sincos_domain(u):
    mag = u & MAG
    return (mag < U64(_d(SINCOS_MAX))) | (mag >= INF)


_lib_cases = {}


def strided_floats():
    """Every 4099th float bit pattern, widened to double (bits)."""
    with np.errstate(invalid="ignore"):      # signalling NaNs among them
        return np.arange(0, 1 << 32, 4099, dtype=np.int64).astype(U32).view(F32).astype(F64).view(U64)


def lib_cases(fn):
    """{class: uint64 patterns} for exp / pow / sin / cos: every 4099th float
    widened, the 64 doubles either side of each branch threshold of
    glibc_math.h, and 2^20 doubles that are not floats (half of them random
    patterns, half with an exponent in the function's working range)."""
    if fn in _lib_cases:
        return _lib_cases[fn]
    floats = strided_floats()
    rng = np.random.default_rng(SEED + 128 + LIB_FNS.index(fn))
    n = 1 << 19
    rand = rng.integers(0, 1 << 64, size=n, dtype=U64)
    mant = rng.integers(0, 1 << 52, size=n, dtype=U64)
    sign = rng.integers(0, 2, size=n, dtype=U64) << U64(63)
    if fn == "exp":
        edges = _around([_d(2.0 ** -54), _d(512.0), _d(1024.0), _d(709.782712893384), _d(708.3964185322641),
                         _d(745.1332191019412)], signs=(0, 1))
        work = sign | (rng.integers(1023 - 60, 1023 + 11, size=n, dtype=U64) << U64(52)) | mant
    elif fn in ("sin", "cos"):
        edges = _around([_d(2.0 ** -27), _d(2.0 ** -26), 0x3fc020c49ba5e354, 0x3feb600000000000, 0x400368fd00000000],
                        signs=(0, 1))
        edges = np.concatenate([edges, _around([0x419921fb00000000 - 1], below=63, above=0, signs=(0, 1))])
        work = sign | (rng.integers(1023 - 30, 1023 + 27, size=n, dtype=U64) << U64(52)) | mant
    else:
        edges = _around([0, 1 << 52, _d(1.0), int(INF)], signs=(0, 1))
        work = (sign & (rand << U64(60))) | (rng.integers(1023 - 20, 1023 + 21, size=n, dtype=U64) << U64(52)) | mant
    c = {"floats": floats, "edges": edges, "doubles": _nonfloat(np.concatenate([rand, work]))}
    if fn in ("sin", "cos"):
        c = {k: u[_in_sincos_domain(u)] for k, u in c.items()}
    _lib_cases[fn] = c
    return c


def fast_pow_cases():
    """pow5_d / pow_quarter_d: float arguments (their stated domain): every
    4099th float, and zeros, ones, infinities, NaN and float's extremes."""
    floats = strided_floats()
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 2.0 ** -149, 2.0 ** -126, float(np.finfo(F32).max)], F64)
    return np.concatenate([floats, sp.view(U64)])


def ulp_distance(a, b):
    """Distance of two doubles' bit patterns on the ordered line (same sign)."""
    a, b = (a & MAG).astype(np.int64), (b & MAG).astype(np.int64)
    return np.abs(a - b)
