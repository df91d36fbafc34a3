"""The rounding certificates and the glibc restatement, called directly.

Every whole-frame parity pin rests on csrc/device/ref_math.h (float_certain,
the seven MathFast wrappers) and csrc/device/glibc_math.h (exp / pow / sin /
cos restated).  Here the probe library (tests/math_probe/) calls them on
constructed inputs (tests/math_inputs.py) and the results are compared with
an integer model of float_certain and with this host's libm through the
library's host reference - the reference's plain expressions.

  sound    certified => the fast float is the reference's, bit for bit
  tight    whatever the reference alone shows certifiable is certified
  exact    MathExact (and MathExactLds, table in LDS) == the reference, always
"""
import ctypes as C

import numpy as np
import pytest

import math_inputs as M

pytestmark = pytest.mark.gpu

U64, U32 = np.uint64, np.uint32


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).to("cuda:0")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _same_float(a, b):
    """Equal float bits, any NaN matching any NaN."""
    nan = lambda x: (x & U32(0x7fffffff)) > U32(0x7f800000)
    return (a == b) | (nan(a) & nan(b))


def _same_double(a, b):
    return (a == b) | (M.is_nan64(a) & M.is_nan64(b))


def _first(bad, fmt, *cols):
    i = int(np.nonzero(bad)[0][0])
    return "%d cases, first at %d: " % (bad.sum(), i) + fmt % tuple(c[i] for c in cols)


# ------------------------------------------------------------- float_certain
def test_float_certain_is_sound_and_tight(gpu):
    """Against the model on the whole constructed set: every double exponent,
    both signs, float values / both kinds of midpoint / binade ends, every
    offset within each margin, the 2^-151 / 2^-150 / 2^128 edges."""
    import torch
    L = M.lib()
    assert L.math_probe_cert_ulps() == M.CERT_ULPS and L.math_probe_max_lib_dist() == M.MAX_LIB_DIST
    u, m = M.certain_cases()
    du, dm = _dev(u, np.int64), _dev(m, np.int32)
    out = torch.zeros(len(u), dtype=torch.uint8, device="cuda:0")
    assert L.math_probe_float_certain(len(u), _ptr(du), _ptr(dm), _ptr(out)) == 0
    got = out.cpu().numpy().astype(bool)
    print("float_certain: %d patterns, %d certified" % (len(u), got.sum()))
    unsound = got & ~M.model_certain(u, m)
    assert not unsound.any(), "certified, yet the interval rounds to two floats: " + _first(unsound, "0x%016x margin %d", u, m)
    slack = ~got & ~M.is_nan64(u) & M.model_certain(u, m.astype(U64) + U64(1))
    assert not slack.any(), "refused, yet even margin + 1 rounds to one float: " + _first(slack, "0x%016x margin %d", u, m)
    assert not got[M.is_nan64(u)].any()


# ------------------------------------------------------------------ wrappers
_results = {}


def _run_wrapper(name):
    """Device and reference results of every case of a wrapper, computed once."""
    if name in _results:
        return _results[name]
    import torch
    L, site = M.lib(), M.SITE[name]
    cases = M.all_cases(name)
    kinds = list(cases)
    args = np.ascontiguousarray(np.concatenate([cases[k] for k in kinds], axis=1))
    n = args.shape[1]
    assert L.math_probe_args() == args.shape[0]
    kind =np.concatenate([np.full(cases[k].shape[1], i) for i, k in enumerate(kinds)])
    d_args = _dev(args.reshape(-1), np.float64)
    outs = [torch.zeros(n, dtype=torch.int32, device="cuda:0") for _ in range(5)]
    assert L.math_probe_wrapper(site, n, _ptr(d_args), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2])) == 0
    assert L.math_probe_wrapper_lds(site, 64, n, _ptr(d_args), _ptr(outs[3])) == 0
    assert L.math_probe_wrapper_lds(site, 256, n, _ptr(d_args), _ptr(outs[4])) == 0
    fast, mask, exact, lds64, lds256 = (o.cpu().numpy().view(U32) for o in outs)
    ref, v, _, _ = M.ref_wrapper(site, args)
    r = dict(name=name, site=site, args=args, kind=kind, kinds=kinds, fast=fast, mask=mask, exact=exact, lds64=lds64,
             lds256=lds256, ref=ref, v=v, bit=U32(1 << site))
    _results[name] = r
    return r


def _describe(r, bad):
    i = int(np.nonzero(bad)[0][0])
    return "%s: %d cases, first (%s) args %s = %s: reference %08x (double %016x), exact %08x, fast %08x, fail_mask %x" % (
        r["name"], bad.sum(), r["kinds"][r["kind"][i]], [float(x).hex() for x in r["args"][:, i]], list(r["args"][:, i]),
        r["ref"][i], r["v"][i], r["exact"][i], r["fast"][i], r["mask"][i])


@pytest.mark.parametrize("name", M.SITES)
def test_math_exact_equals_host_reference(gpu, name):
    """MathExact's float == the reference's on every case (ordinary, fixture,
    exact-argument, edge, sweep); MathExactLds the same at block sizes 64 and
    256 (exp's table read from LDS: acc_exp and exp_times use it)."""
    r = _run_wrapper(name)
    bad = ~_same_float(r["exact"], r["ref"])
    assert not bad.any(), _describe(r, bad)
    for k in ("lds64", "lds256"):
        bad = ~_same_float(r[k], r["ref"])
        assert not bad.any(), k + " " + _describe(r, bad)


@pytest.mark.parametrize("name", M.SITES)
def test_certified_fast_float_is_the_reference(gpu, name):
    """Soundness: fail_mask 0 => MathFast's float is the reference's, on every
    case, the near-midpoint fixture and the bpdf sweep included."""
    r = _run_wrapper(name)
    certified = r["mask"] == 0
    bad = certified & ~_same_float(r["fast"], r["ref"])
    assert not bad.any(), _describe(r, bad)
    for i, k in enumerate(r["kinds"]):
        sel = r["kind"] == i
        print("%s %s: %d cases, %d not certified" % (name, k, sel.sum(), (sel & ~certified).sum()))


@pytest.mark.parametrize("name", M.SITES)
def test_fail_mask_has_only_the_sites_bit(gpu, name):
    r = _run_wrapper(name)
    bad = (r["mask"] & ~r["bit"]) != 0
    assert not bad.any(), _describe(r, bad)


@pytest.mark.parametrize("name", M.SITES)
def test_preconditions_refuse(gpu, name):
    """Outside the exact-argument shortcuts: a NaN result, a negative acc / a /
    b / r (or a NaN one) and fixture cases within 32 - K of a midpoint set the
    site's bit."""
    r = _run_wrapper(name)
    a = r["args"]
    checked = ~M.exact_arg(name, a)
    refuse = M.is_nan64(r["v"]) | ~M.precondition(name, a)
    fx = r["kind"] == r["kinds"].index("fixture")
    dist = np.zeros(a.shape[1], np.int64)
    dist[fx] = M.fixture_cases(name)[2]
    refuse |= fx & M.must_refuse_fixture(name, dist)
    if name == "times_one_minus_div_pow":
        zero, big_s, _, _ = M.tomdp_state(a)
        with np.errstate(invalid="ignore"):
            refuse &= ~(zero & (a[0] >= 0.0))      # r * 0: certified even when it is NaN (inf * 0)
        refuse |= big_s
        assert (checked & big_s).sum() > 300
    refuse &= checked
    assert refuse.sum() > 50
    bad = refuse & (r["mask"] == 0)
    assert not bad.any(), _describe(r, bad)


def test_zero_branch_certifies(gpu):
    """times_one_minus_div_pow, q > 1 + 2^-48 and r >= 0: certified, r * 0's bits."""
    r = _run_wrapper("times_one_minus_div_pow")
    a = r["args"]
    zero, _, _, _ = M.tomdp_state(a)
    with np.errstate(invalid="ignore"):
        sel = zero & (a[0] >= 0.0)
        want = (a[0].astype(np.float32) * np.float32(0.0)).view(U32)
    assert sel.sum() > 1000
    bad = sel & ((r["mask"] != 0) | ~_same_float(r["fast"], want) | ~_same_float(r["ref"], want))
    assert not bad.any(), _describe(r, bad)


@pytest.mark.parametrize("name", M.SITES)
def test_certificates_are_tight(gpu, name):
    """Every case the reference alone shows certifiable is certified (at least
    99.9% of the ordinary set: tests/test_math_inputs.py), and the
    exact-argument cases whatever their other arguments are."""
    r = _run_wrapper(name)
    must = M.must_certify(name, r["args"]) | M.exact_arg(name, r["args"])
    ordinary = r["kind"] == r["kinds"].index("ordinary")
    print("%s: %d of %d ordinary cases not certified" % (name, (ordinary & (r["mask"] != 0)).sum(), ordinary.sum()))
    bad = must & (r["mask"] != 0)
    assert not bad.any(), _describe(r, bad)


# --------------------------------------------------------- library functions
def _device_lib(fn, x, y=0.0):
    import torch
    dx = _dev(x, np.int64)
    out = torch.zeros(len(x), dtype=torch.int64, device="cuda:0")
    assert M.lib().math_probe_lib(M.LIB_FNS.index(fn), len(x), _ptr(dx), y, _ptr(out)) == 0
    return out.cpu().numpy().view(U64)


@pytest.mark.parametrize("fn,y", [("exp", 0.0), ("sin", 0.0), ("cos", 0.0)] + [("pow", y) for y in M.POW_YS])
def test_restatement_equals_libm(gpu, fn, y):
    """dexp / dpow / dsin / dcos == this host's libm bit for bit: every 4099th
    float, 64 doubles either side of each branch threshold, and 2^20 doubles
    that are not floats."""
    for kind, x in M.lib_cases(fn).items():
        got, want = _device_lib(fn, x, y), M.ref_lib(M.LIB_FNS.index(fn), x, y)
        bad = ~_same_double(got, want)
        assert not bad.any(), "%s(%s) %s: " % (fn, y if fn == "pow" else "", kind) + _first(
            bad, "x 0x%016x: device 0x%016x libm 0x%016x", x, got, want)


@pytest.mark.parametrize("fn", ["pow5_d", "pow_quarter_d"])
def test_fast_pow_is_within_the_certificates_distance(gpu, fn):
    """MathFast's constant-exponent powers on float arguments: within
    kMaxLibDist ulps of libm's pow with its sign (or NaN as it is), and
    identical at 0 and 1."""
    x = M.fast_pow_cases()
    got, want = _device_lib(fn, x), M.ref_lib(M.LIB_FNS.index(fn), x)
    nan_g, nan_w = M.is_nan64(got), M.is_nan64(want)
    assert np.array_equal(nan_g, nan_w), _first(nan_g != nan_w, "x 0x%016x: device 0x%016x libm 0x%016x", x, got, want)
    ok = ~nan_w
    bad = ok & ((got ^ want) >> U64(63) != 0)
    assert not bad.any(), "sign: " + _first(bad, "x 0x%016x: device 0x%016x libm 0x%016x", x, got, want)
    dist = np.where(ok, M.ulp_distance(got, want), 0)
    print("%s: largest distance from libm's pow %d ulps over %d float arguments" % (fn, dist.max(), len(x)))
    bad = dist > M.MAX_LIB_DIST
    assert not bad.any(), _first(bad, "x 0x%016x: device 0x%016x libm 0x%016x", x, got, want)
    xv = x.view(np.float64)
    exact = (xv == 0.0) | (xv == 1.0)
    assert exact.sum() >= 3 and np.array_equal(got[exact], want[exact])
