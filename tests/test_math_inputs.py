"""The math probe's inputs are what they claim to be (CPU; no device work).

tests/test_gpu_math_probe.py drives the rounding certificates and the glibc
restatement (csrc/device/ref_math.h, glibc_math.h) with the inputs of
tests/math_inputs.py.  Here: the float_certain model agrees with a plain
enumeration, the committed near-midpoint fixture reproduces from the host
reference, and the ordinary sets are such that the device cannot pass by
refusing to certify.
"""
import numpy as np
import pytest

import math_inputs as M

U64 = np.uint64


def test_model_endpoints_equal_enumeration():
    """Rounding is monotone: the end points of [u - 32, u + 32] decide for the
    whole interval.  2^16 cases drawn from the constructed set (so most sit at
    a rounding boundary or an edge), every pattern of each rounded."""
    u, m = M.certain_cases()
    sel = np.nonzero(m == M.CERT_ULPS)[0]
    pick = sel[np.random.default_rng(M.SEED).integers(0, len(sel), size=1 << 16)]
    got = M.model_certain(u[pick], np.full(len(pick), M.CERT_ULPS, U64))
    want = M.model_certain_enumerated(u[pick], M.CERT_ULPS)
    assert np.array_equal(got, want)
    assert got.sum() > 1000 and (~got).sum() > 1000          # both answers well represented


def test_constructed_set_covers_what_it_lists():
    u, m = M.certain_cases()
    e = (u >> U64(52) & U64(0x7ff)).astype(np.int64)
    assert len(np.unique(e)) == 2048
    assert set(np.unique(m).tolist()) == set(M.MARGINS)
    assert M.MARGINS[4] == 42 and M.MARGINS[-1] == 4 * ((9 << 16) + 1) + 2
    assert ((u >> U64(63)) == 1).any() and ((u >> U64(63)) == 0).any()
    for x in (2.0 ** -151, 2.0 ** -150, 2.0 ** -149, 2.0 ** -126, float(np.finfo(np.float32).max), 2.0 ** 128, np.inf, 0.0):
        assert (u == np.array(x).view(U64)).any(), x
    assert M.is_nan64(u).any()
    # the subnormal-float branch: patterns within every margin of a midpoint, q = 30..54
    sub = (e >= 1023 - 151) & (e < 1023 - 126) & ~M.model_certain(u, m)
    assert len(np.unique(e[sub])) == 25
    assert 1 << 21 < len(u) < 1 << 24


@pytest.mark.parametrize("name", M.SITES)
def test_fixture_reproduces_from_the_host_reference(name):
    args, v, dist = M.fixture_cases(name)
    assert args.shape == (len(v), 4) and len(dist) == len(v)
    _, v_now, _, _ = M.ref_wrapper(M.SITE[name], args.T)
    assert np.array_equal(v_now, v), "the host libm's doubles differ from the recorded ones"
    e = (v >> U64(52) & U64(0x7ff)).astype(np.int64)
    assert ((e >= 1023 - 126) & (e <= 1023 + 127)).all()
    low = (v & U64(0x1fffffff)).astype(np.int64)
    assert np.array_equal(np.abs(low - (1 << 28)), dist.astype(np.int64))
    assert dist.max() <= 64
    assert len(v) >= 256 and (dist <= 12).sum() >= 64 and (dist >= 53).sum() >= 64, \
        (len(v), (dist <= 12).sum(), (dist >= 53).sum())
    assert len(np.unique(args, axis=0)) == len(args)
    # distance >= 53 > 32 + K: these the device must certify (K <= 20; the last
    # wrapper's K is its own margin, its fixture cases serve soundness)
    if name != "times_one_minus_div_pow":
        assert M.must_certify(name, args.T)[dist >= 53].all()


@pytest.mark.parametrize("name", M.SITES)
def test_ordinary_cases_must_be_certified(name):
    """At least 99.9% of each ordinary set is must_certify (a condition on the
    inputs: the expected free share is about (2 (32 + K) + 1) / 2^29), so a
    device that refuses certificates fails the tightness test."""
    a = M.ordinary_cases(name)
    assert a.shape == (4, M.N_ORDINARY)
    must = M.must_certify(name, a)
    judged = a[2] >= M.BPDF_MUST if name == "times_one_minus_div_pow" else np.ones(a.shape[1], bool)
    share = must[judged].mean()
    print("%s: must_certify %d of %d judged (%.5f%%)" % (name, must[judged].sum(), judged.sum(), 100 * share))
    assert judged.sum() >= 0.8 * a.shape[1]
    assert share >= 0.999, share


def test_sweep_and_edges_reach_the_branches():
    """The bpdf sweep crosses q = 1 and takes s past 16; the edge sets reach
    float's subnormal range and overflow for every wrapper."""
    sw = M.bpdf_sweep()
    zero, big_s, s_hi, _ = M.tomdp_state(sw)
    # w < 2^-18 within about 2^7 float ulps of the edge, at each of the three r
    assert zero.sum() > 1000 and big_s.sum() > 300
    assert (s_hi <= 16).sum() > 1000 and ((s_hi > 10) & (s_hi <= 16)).sum() > 100
    for name in M.SITES:
        f, v, _, _ = M.ref_wrapper(M.SITE[name], M.edge_cases(name))
        mag = (f & np.uint32(0x7fffffff)).astype(np.int64)
        assert ((mag > 0) & (mag < 0x00800000)).sum() > 100, name            # subnormal floats
        assert (mag == 0x7f800000).sum() > 10, name                          # overflow / inf
        assert M.is_nan64(v).sum() > 10, name
        ex = M.exact_arg_cases(name)
        assert M.exact_arg(name, ex).all()


def test_library_inputs():
    for fn in ("exp", "pow", "sin", "cos"):
        c = M.lib_cases(fn)
        d = c["doubles"]
        assert ((d & U64(0x1fffffff)) != 0).all()                            # none is a float widened
        assert len(c["floats"]) > (1 << 19) and len(d) > (1 << 19)
    assert len(M.lib_cases("exp")["floats"]) == -(-(1 << 32) // 4099)
    mag = M.lib_cases("sin")["edges"] & M.MAG
    assert mag.max() < np.array(M.SINCOS_MAX).view(U64)
