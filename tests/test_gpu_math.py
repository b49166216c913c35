"""The device math primitives of frei_amd/csrc/frei_math.h against exact arithmetic, one value
per lane through the test-only probe tests/csrc/frei_math_probe.hip (built by
frei_amd.build.build_probe() with the library's flags): fm::div, fm::sqrt, fm::sqrt_pos,
fm::rcp_nr, fm::exp_neg, fm::exp_neg_nf, fm::exp_neg_unclamped and the formulas planck,
planck_em, exp_em and shell_step built on them.

References (tests/mathref.py): Fraction, Python integers and 60-digit decimal; NumPy's IEEE
``/`` and ``sqrt`` as the bulk reference, cross-checked against Fraction / math.isqrt on a subset
in the same test.  ulp errors are in units of the ulp of the exact result.  The near-midpoint
operands (quotients within 2^-53 ulp and roots within 2^-44 ulp of a rounding midpoint) are the
constructions pinned without a GPU by tests/test_math_hardcases_host.py.

Bounds, each from the operation count and none from the code under test:
  div, sqrt, sqrt_pos   bit-identical to the correctly rounded result on random operands and on
                        the operand families the kernels form; faithful on the near-midpoint sets
  rcp_nr                <= 1 ulp of the exact 1 / b
  exp_neg*              mutually bit-identical and equal to the in-kernel ::exp; <= 1 ulp of
                        exp(x) (ocml's documented bound)
  planck                relative error <= (4 + 1 / x) 2^-52: 1 ulp in e; the subtraction 1 - e
                        (exact or half an ulp) amplified by e / (1 - e) <= 1 / x; one multiply;
                        one faithfully rounded quotient; one unit of margin
  planck_em             <= 6 2^-52 for x in [2^-40, 700]: 1 ulp in e; <= 2.42 2^-52 from 1 - e at
                        e <= 2^-1/2 (or the cancellation-free -y (1 + y q)); one multiply; one
                        quotient
  shell_step            e, u, v each within 4 2^-52 absolutely (every intermediate is in [0, 1]);
                        u, v within 16 2^-52 relatively on the x <= ln2 / 2 branch (em ~ x, v ~ x / 2:
                        em - v amplifies by about 3); e, u, v >= 0; |e + u + v - 1| <= 4 2^-52

Measured on MI355X (each test prints its figures, pytest -s):
  div        0 differences on every random and family set; on 25 000 near-midpoint quotients
             2762 are the other bracketing double (one ulp off), none is further — so the
             near-midpoint tests assert faithful rounding and report the count, as frei_math.h
             and DESIGN.md now state.  This test found div(-0, b > 0) = +0; div now copies its
             quotient estimate's sign onto the result.
  sqrt*      0 differences on every random set and at the specials; 5 of 326 near-midpoint roots
             one ulp off, none further (sqrt and sqrt_pos alike)
  rcp_nr     0.500 ulp: all 2^20 + 2^16 results are the correctly rounded reciprocal
  exp_neg*   identical to each other and to ::exp on every set; 0.7953 ulp worst, 0.6209 where
             the result is subnormal
  planck     0.295 of the bound (worst at x = 13.7); 1.379 2^-52 for x >= 1; rel - 2^-52 / x <= 1.128 2^-52
  planck_em  1.826 2^-52 (1.523 on the series branch, 1.725 at the branch point); non-increasing
             over the 16 doubles around the branch
  shell_step absolute e 0.383 u 1.615 v 1.232 2^-52; relative on x <= ln2 / 2 u 12.983 v 11.843
             2^-52; |e + u + v - 1| 0.250 2^-52
Two mutations of a scratch copy of frei_math.h each turn this file red: one bit of exp_neg's 1/6
coefficient (1176 of 2^20 results differ from ::exp), and div returning its quotient estimate
without the residual correction (525 882 of 2^20 quotients misrounded; five tests fail)."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import mathref as M

pytestmark = pytest.mark.gpu

FN = {"div": 0, "sqrt": 1, "sqrt_pos": 2, "rcp_nr": 3, "exp_neg": 4, "exp_neg_nf": 5,
      "exp_neg_unclamped": 6, "planck": 7, "planck_em": 8, "shell_step": 9}
EXPS = ("exp_neg", "exp_neg_nf", "exp_neg_unclamped")
N_BULK = 1 << 20
N_EXACT = 4096
EPS = M.EPS
LOG2E = float.fromhex("0x1.71547652b82fep+0")      # the reduction's constant (0x3ff71547652b82fe)

# cgs: B_lambda = c1 / expm1(hcl / T), c1 = 2 h c^2 / lam^5, hcl = h c / (lam k)
H, C, KB = 6.62607015e-27, 2.99792458e10, 1.380649e-16


@pytest.fixture(scope="module")
def probe():
    """run(name, a, b=None, c=None) -> (out, dev_ref); out is (3, n) for shell_step.  A missing
    probe or one built from other sources is a failure, not a skip."""
    from frei_amd import build
    assert os.path.exists(build.PROBE_LIB), (
        f"{build.PROBE_LIB} is missing: frei_amd.build.build() builds it")
    assert build.probe_stamp_matches(), (
        "libfrei_mathprobe.so was built from another frei_math.h, probe source or flags: rebuild")
    lib = ctypes.CDLL(build.PROBE_LIB)
    dp = ctypes.POINTER(ctypes.c_double)
    lib.frei_mathprobe.restype = ctypes.c_int
    lib.frei_mathprobe.argtypes = [ctypes.c_int, ctypes.c_int64, dp, dp, dp, dp, dp]

    def run(name, a, b=None, c=None):
        ins = [None if v is None else np.ascontiguousarray(v, dtype=np.float64)
               for v in (a, b, c)]
        n = ins[0].size
        assert 0 < n <= N_BULK and all(v is None or v.size == n for v in ins)
        out = np.full((3 if name == "shell_step" else 1, n), np.nan)
        ref = np.full(n, np.nan)
        ptr = [None if v is None else v.ctypes.data_as(dp) for v in ins]
        err = lib.frei_mathprobe(FN[name], n, *ptr, out.ctypes.data_as(dp), ref.ctypes.data_as(dp))
        assert err == 0, f"frei_mathprobe({name}): HIP error {err}"
        return (out if name == "shell_step" else out[0]), ref
    return run


def _logu(rng, n, lo, hi, signs=True):
    """Magnitudes log-uniform in 2^[lo, hi] with a full random significand, random signs."""
    x = np.ldexp(1.0 + rng.random(n), rng.integers(lo, hi, n).astype(np.int32))
    return x * rng.choice([-1.0, 1.0], n) if signs else x


def _subset(rng, n, k=N_EXACT):
    return np.arange(n) if n <= k else rng.choice(n, k, replace=False)


def _assert_bits(got, want, what, *operands):
    bad = np.flatnonzero(~M.same_bits(got, want))
    if bad.size:
        i = bad[0]
        ops = ", ".join(float(o[i]).hex() for o in operands)
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, e.g. ({ops}) -> "
                             f"{float(got[i]).hex()}, want {float(want[i]).hex()}")


# ------------------------------------------------------------------ division
def _check_div(probe, rng, a, b, what):
    with np.errstate(all="ignore"):
        want = a / b
    idx = _subset(rng, a.size)
    for i in idx.tolist():      # NumPy's quotient is the correctly rounded one
        assert M.same_bits(want[i], M.round_div(float(a[i]), float(b[i]))), (what, a[i], b[i])
    got, ref = probe("div", a, b)
    _assert_bits(ref, want, f"{what}: the in-kernel a / b against IEEE", a, b)
    _assert_bits(got, want, f"{what}: fm::div against the correctly rounded quotient", a, b)


def test_div_random_operands_are_correctly_rounded(probe):
    rng = np.random.default_rng(101)
    _check_div(probe, rng, _logu(rng, N_BULK, -450, 451), _logu(rng, N_BULK, -450, 451),
               "|a|, |b| in 2^[-450, 450]")


def _planck_c1(rng, n):
    lam = 1e-4 * 10 ** rng.uniform(math.log10(0.3), math.log10(500.0), n)     # cm
    return 2 * H * C * C / lam ** 5, H * C / (lam * KB)


def test_div_operand_families_of_the_kernels_are_correctly_rounded(probe):
    rng = np.random.default_rng(102)
    n = 1 << 16
    # (B1 - B2) / dtau, B1 and B2 agreeing to 1 .. 50 bits
    B1 = 10 ** rng.uniform(-60, 10, n)
    B2 = B1 * (1.0 + rng.choice([-1.0, 1.0], n) * np.ldexp(0.5 + 0.5 * rng.random(n),
                                                          -rng.integers(0, 50, n).astype(np.int32)))
    _check_div(probe, rng, B1 - B2, 10 ** rng.uniform(-14, 4, n), "(B1 - B2) / dtau")
    # Emw / E and pi (1 - w0) / Emw, w0 in (0.1, 0.5], E from the kernel's polynomial
    w0 = np.concatenate([0.5 - 0.4 * rng.random(n - 2), [0.5, np.nextafter(0.1, 1.0)]])
    E = (1.225 - 0.1777 * w0) - 0.05582 * (w0 * w0)
    Emw = E - w0
    _check_div(probe, rng, Emw, E, "Emw / E")
    _check_div(probe, rng, math.pi * (1.0 - w0), Emw, "pi (1 - w0) / Emw")
    # c1 e / (1 - e), e from 2^-1000 up to 1 - 2^-53
    e = np.concatenate([
        np.ldexp(1.0 + rng.random(n // 2), -rng.integers(1, 1001, n // 2).astype(np.int32)),
        1.0 - np.ldexp(1.0 + rng.random(n // 2 - 2), -rng.integers(2, 54, n // 2 - 2).astype(np.int32)),
        [2.0 ** -1000, 1.0 - 2.0 ** -53]])
    c1, _ = _planck_c1(rng, n)
    assert e.min() == 2.0 ** -1000 and e.max() == 1.0 - 2.0 ** -53
    _check_div(probe, rng, c1 * e, 1.0 - e, "c1 e / (1 - e)")
    # divisors that are powers of two; a zero numerator of either sign
    _check_div(probe, rng, _logu(rng, n, -450, 451),
               np.ldexp(rng.choice([-1.0, 1.0], n), rng.integers(-450, 451, n).astype(np.int32)),
               "a / 2^k")
    zeros = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    _check_div(probe, rng, zeros, _logu(rng, n, -450, 451), "+-0 / b")


def test_div_special_divisors_give_nan(probe):
    """The dropped div_fixup's other cases, as frei_math.h states them: a zero, infinite or NaN
    divisor gives NaN (IEEE: +-inf, +-0, NaN)."""
    b = np.array([0.0, -0.0, np.inf, -np.inf, np.nan])
    got, _ = probe("div", np.full(b.size, 3.0), b)
    assert np.isnan(got).all(), got


def test_div_near_midpoint_quotients_are_faithful(probe):
    cases = M.div_midpoint_cases(12500, seed=5)
    assert len(cases) >= 20000
    a = np.array([float(A) for A, _, _, _ in cases])
    b = np.array([float(B) for _, B, _, _ in cases])
    want = np.array([M.div_midpoint_expected(N, k) for _, _, N, k in cases])
    other = np.array([math.ldexp((N - 1) // 2 if k > 0 else (N + 1) // 2, -53)
                      for _, _, N, k in cases])
    assert M.same_bits(a / b, want).all()
    got, ref = probe("div", a, b)
    _assert_bits(ref, want, "the in-kernel a / b on near-midpoint quotients", a, b)
    off = np.flatnonzero(~M.same_bits(got, want))
    print(f"div near-midpoint: {off.size} of {got.size} one ulp off the correctly rounded "
          f"quotient (closest case {min(abs(k) / (2 * B) for _, B, _, k in cases):.2e} ulp "
          f"from its midpoint)"
          + "".join(f"\n  e.g. {a[i].hex()} / {b[i].hex()} -> {got[i].hex()}, correctly "
                    f"rounded {want[i].hex()}" for i in off[:3]))
    # faithful: one of the two doubles bracketing the exact quotient
    faithful = M.same_bits(got, want) | M.same_bits(got, other)
    assert faithful.all(), (f"{(~faithful).sum()} results outside the bracketing doubles, e.g. "
                            f"{a[~faithful][0].hex()} / {b[~faithful][0].hex()}")


# ------------------------------------------------------------------ square roots
def _check_sqrt(probe, rng, name, x, what):
    with np.errstate(all="ignore"):
        want = np.sqrt(x)
    for i in _subset(rng, x.size).tolist():
        if x[i] > 0 and math.isfinite(x[i]):
            assert want[i] == M.round_sqrt(float(x[i])), (what, x[i])
    got, ref = probe(name, x)
    _assert_bits(ref, want, f"{what}: the in-kernel ::sqrt against IEEE", x)
    _assert_bits(got, want, f"{what}: fm::{name} against the correctly rounded root", x)


def test_sqrt_is_correctly_rounded_over_its_range_and_at_the_specials(probe):
    rng = np.random.default_rng(103)
    _check_sqrt(probe, rng, "sqrt", _logu(rng, N_BULK, -767, 1024, signs=False),
                "x in 2^[-767, 1023]")
    specials = np.array([0.0, -0.0, np.inf, np.nan, -1.0, -2.5e-300, 2.0 ** -767,
                         np.finfo(float).max, 1.0, 4.0])
    got, ref = probe("sqrt", specials)
    with np.errstate(all="ignore"):
        want = np.sqrt(specials)
    _assert_bits(got, want, "fm::sqrt at +-0, inf, NaN, negative arguments and the range ends",
                 specials)
    _assert_bits(ref, want, "::sqrt at the specials", specials)
    assert math.copysign(1.0, got[1]) == -1.0 and np.isnan(got[3:6]).all()


@pytest.mark.parametrize("name", ["sqrt", "sqrt_pos"])
def test_sqrt_forms_are_correctly_rounded_on_the_sweeps_domain(probe, name):
    rng = np.random.default_rng(104)
    x = np.concatenate([0.5 + 0.71 * rng.random(N_BULK - 3), [np.nextafter(0.5, 1.0), 1.0, 1.21]])
    assert x.min() > 0.5 and x.max() <= 1.21
    _check_sqrt(probe, rng, name, x, "x in (0.5, 1.21]")


@pytest.mark.parametrize("name", ["sqrt", "sqrt_pos"])
def test_sqrt_near_midpoint_roots_are_faithful(probe, name):
    xs, want, other = [], [], []
    counts = []
    for binade in (0, 1):
        cases, scale = M.sqrt_midpoint_cases(binade)
        counts.append(len(cases))
        for x, m, c in cases:
            xs.append(x)
            want.append(M.sqrt_midpoint_expected(m, c, scale))
            other.append(math.ldexp(m + 1 if c >= 0 else m, -scale))
    assert counts[0] >= 200 and counts[1] >= 20, counts
    xs, want, other = np.array(xs), np.array(want), np.array(other)
    assert M.same_bits(np.sqrt(xs), want).all()
    got, ref = probe(name, xs)
    _assert_bits(ref, want, "the in-kernel ::sqrt on near-midpoint roots", xs)
    off = np.flatnonzero(~M.same_bits(got, want))
    print(f"{name} near-midpoint: {off.size} of {xs.size} one ulp off the correctly rounded root "
          f"({counts[0]} in [1/4, 1), {counts[1]} in [1, 1.21])"
          + "".join(f"\n  e.g. {xs[i].hex()} -> {got[i].hex()}, correctly rounded {want[i].hex()}"
                    for i in off[:3]))
    faithful = M.same_bits(got, want) | M.same_bits(got, other)
    assert faithful.all(), f"{(~faithful).sum()} roots outside the bracketing doubles"


# ------------------------------------------------------------------ reciprocal
def test_rcp_nr_is_within_one_ulp_of_the_exact_reciprocal(probe):
    rng = np.random.default_rng(105)
    worst, n_inexact = 0.5, 0
    for what, b in (("|b| in 2^[-450, 450]", _logu(rng, N_BULK, -450, 451)),
                    ("chi in [-1, -0.2]", np.concatenate([-0.2 - 0.8 * rng.random((1 << 16) - 2),
                                                          [-1.0, -0.2]]))):
        got, ref = probe("rcp_nr", b)
        rn = 1.0 / b
        _assert_bits(ref, rn, f"{what}: the in-kernel 1.0 / b against IEEE", b)
        for i in _subset(rng, b.size).tolist():
            assert rn[i] == M.round_div(1.0, float(b[i]))
        # where it is the correctly rounded reciprocal the error is at most half an ulp; every
        # other element is measured exactly
        rest = np.flatnonzero(~M.same_bits(got, rn))
        n_inexact += rest.size
        for i in rest.tolist():
            ok, err = M.rcp_within_one_ulp(float(got[i]), float(b[i]))
            worst = max(worst, err)
            assert ok, f"{what}: rcp_nr({float(b[i]).hex()}) = {float(got[i]).hex()}, {err} ulp"
    print(f"rcp_nr: worst error {worst:.3f} ulp; {n_inexact} of {N_BULK + (1 << 16)} not the "
          f"correctly rounded reciprocal")


# ------------------------------------------------------------------ exponentials
def _exp_boundaries():
    """x = (k + 1/2) ln2 for k = -1 .. -1076 (where the reduction's n steps) and the 4 doubles on
    each side of each."""
    out = []
    for k in range(-1, -1077, -1):
        x = float(M.CTX.multiply(M.D(k) + M.D("0.5"), M.LN2))
        lo = hi = x
        out.append(x)
        for _ in range(4):
            lo, hi = math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf)
            out += [lo, hi]
    return np.array(out)


EXP_EDGES = np.array([0.0, -0.0, -1e-300, -1.0, -745.1, -745.2, -1074.9, -1075.0, -1075.1,
                      -1100.0, -1100.5, -1e6])


def test_exp_neg_forms_are_identical_and_equal_the_compilers_exp(probe):
    rng = np.random.default_rng(106)
    sets = {"uniform [-1200, 0]": -1200.0 * rng.random(N_BULK),
            "edge list": EXP_EDGES,
            "reduction boundaries": _exp_boundaries(),
            "subnormal results [-745.2, -708.3]": np.linspace(-745.2, -708.3, 1 << 19)}
    for what, x in sets.items():
        outs = {}
        for name in EXPS:
            outs[name], ref = probe(name, x)
            _assert_bits(outs[name], ref, f"{what}: fm::{name} against the in-kernel ::exp", x)
        common = x >= -1100.0
        for name in EXPS[1:]:
            _assert_bits(outs[name][common], outs["exp_neg"][common],
                         f"{what}: fm::{name} against fm::exp_neg on [-1100, 0]", x[common])
        assert (outs["exp_neg"] >= 0).all() and (outs["exp_neg"] <= 1).all()
        assert (outs["exp_neg"][x < -745.2] == 0).all()


def test_exp_neg_forms_are_within_one_ulp_of_exp(probe):
    rng = np.random.default_rng(107)
    x = np.concatenate([-708.0 * rng.random(1536), rng.uniform(-745.2, -708.0, 512),
                        rng.choice(_exp_boundaries(), 1024, replace=False),
                        -np.ldexp(1.0 + rng.random(1024), rng.integers(-60, 1, 1024).astype(np.int32))])
    assert x.size == N_EXACT
    exact = [M.dec_exp(float(v)) for v in x]
    for name in EXPS:
        got, _ = probe(name, x)
        errs = np.array([M.dec_ulp_err(float(g), e) for g, e in zip(got, exact)])
        i = int(np.argmax(errs))
        print(f"{name}: worst error {errs[i]:.4f} ulp at x = {x[i]!r} over {x.size} points "
              f"({(errs[x < -708.4]).max():.4f} in the subnormal range)")
        assert errs.max() <= 1.0, f"fm::{name}({x[i]!r}) is {errs[i]} ulp from exp"


def test_exp_neg_forms_documented_edges(probe):
    x = np.array([np.nan, -np.inf, -1100.0000000000002, -1101.0, -1e9, -0.0, 0.0])
    neg, _ = probe("exp_neg", x)
    nf, _ = probe("exp_neg_nf", x)
    unc, _ = probe("exp_neg_unclamped", x)
    assert np.isnan(neg[0]) and np.isnan(unc[0])          # NaN passes through
    assert M.same_bits(nf[0], 0.0)                          # maxNum(NaN, -1100): exp(-1100) = +0
    assert M.same_bits(neg[1], 0.0) and M.same_bits(nf[1], 0.0)
    assert np.isnan(unc[1])                                 # -inf unclamped: a zero temperature
    assert M.same_bits(unc[2:5], 0.0).all() and M.same_bits(neg[2:5], 0.0).all()
    assert M.same_bits(nf[2:5], 0.0).all()
    for out in (neg, nf, unc):
        assert M.same_bits(out[5:], 1.0).all()


# ------------------------------------------------------------------ Planck forms
def _planck_points(rng, n, x_lo, x_hi):
    """(c1, hcl, iT, x): x = fl(hcl iT) log-uniform in [x_lo, x_hi], c1 and hcl of wavelengths
    log-uniform in [0.3, 500] um."""
    c1, hcl = _planck_c1(rng, n)
    iT = 10 ** rng.uniform(math.log10(x_lo), math.log10(x_hi), n) / hcl
    x = hcl * iT                 # the kernel's single multiply
    keep = (x >= x_lo) & (x <= x_hi)
    return c1[keep], hcl[keep], iT[keep], x[keep]


def test_planck_is_within_its_operation_count_bound(probe):
    rng = np.random.default_rng(108)
    c1, hcl, iT, x = _planck_points(rng, N_EXACT, 1e-4, 700.0)
    assert x.size > N_EXACT - 8
    got, _ = probe("planck", c1, hcl, iT)
    rel = np.array([M.dec_rel_err(float(g), M.dec_planck(float(a), float(v)))
                    for g, a, v in zip(got, c1, x)])
    ratio = rel / ((4.0 + 1.0 / x) * EPS)
    i = int(np.argmax(ratio))
    print(f"planck: worst relative error / ((4 + 1/x) 2^-52) = {ratio[i]:.3f} at x = {x[i]:.4g}; "
          f"worst (rel - 2^-52 / x) = {((rel - EPS / x) / EPS).max():.3f} 2^-52; "
          f"worst rel at x >= 1: {(rel[x >= 1] / EPS).max():.3f} 2^-52")
    assert ratio.max() <= 1.0, f"planck at x = {x[i]!r}: {rel[i] / EPS:.3f} 2^-52 relative"


def test_planck_edges(probe):
    # e is subnormal on [709.8, 745]: finite and 0 <= B <= 2 c1 exp(-x); exactly 0 above 746
    x = np.concatenate([np.linspace(709.8, 745.0, 353), [746.1, 750.0, 800.0, 1e4, 1e9]])
    for c1v in (38.0, 1.2e15):
        got, _ = probe("planck", np.full(x.size, c1v), np.ones(x.size), x)
        assert np.isfinite(got).all() and (got >= 0).all()
        for g, v in zip(got[:353], x[:353]):
            assert M.D(float(g)) <= M.CTX.multiply(M.D(2 * c1v), M.dec_exp(-float(v))), (c1v, v, g)
        assert M.same_bits(got[353:], 0.0).all()
    for name in ("planck", "planck_em"):
        got, _ = probe(name, np.array([1e5, 1e5]), np.array([1.4e4, 1.4e4]),
                       np.array([np.nan, 1e-3]))
        assert np.isnan(got[0]) and got[1] > 0             # a NaN temperature propagates


def _branch_points():
    """The 8 doubles on each side of exp_em's branch n0 = (rint(-x log2e) == 0), x ~ ln2 / 2: the
    last 8 with fl(x log2e) <= 1/2 and the first 8 above."""
    x = float(M.CTX.divide(M.LN2, M.D(2)))
    while x * LOG2E <= 0.5:
        x = math.nextafter(x, 1.0)
    while x * LOG2E > 0.5:
        x = math.nextafter(x, 0.0)
    lo, hi = [x], [math.nextafter(x, 1.0)]
    for _ in range(7):
        lo.insert(0, math.nextafter(lo[0], 0.0))
        hi.append(math.nextafter(hi[-1], 1.0))
    assert all(v * LOG2E <= 0.5 for v in lo) and all(v * LOG2E > 0.5 for v in hi)
    return np.array(lo + hi)


def test_planck_em_is_uniformly_accurate_down_to_long_wavelengths(probe):
    rng = np.random.default_rng(109)
    c1, hcl, iT, x = _planck_points(rng, N_EXACT, 2.0 ** -40, 700.0)
    assert x.size > N_EXACT - 8
    xb = _branch_points()
    c1 = np.concatenate([c1, np.full(xb.size, 1.19e5)])
    hcl = np.concatenate([hcl, np.ones(xb.size)])
    iT = np.concatenate([iT, xb])
    x = np.concatenate([x, xb])
    got, _ = probe("planck_em", c1, hcl, iT)
    rel = np.array([M.dec_rel_err(float(g), M.dec_planck(float(a), float(v)))
                    for g, a, v in zip(got, c1, x)]) / EPS
    i = int(np.argmax(rel))
    small = x <= 0.5 / LOG2E
    print(f"planck_em: worst relative error {rel[i]:.3f} 2^-52 at x = {x[i]:.4g} "
          f"({rel[small].max():.3f} on the series branch, {rel[~small].max():.3f} above it, "
          f"{rel[-xb.size:].max():.3f} at the branch point)")
    assert rel.max() <= 6.0, f"planck_em at x = {x[i]!r}: {rel[i]:.3f} 2^-52 relative"
    # B falls with x: no step up where the denominator changes form
    b = got[-xb.size:]
    print("planck_em across the branch:", " ".join(f"{v - b[8]:+.3e}" for v in b))
    assert (np.diff(b) <= 0).all(), "planck_em is not monotone across x = ln2 / 2"


# ------------------------------------------------------------------ one shell along a ray
def test_shell_step_weights_are_accurate_non_negative_and_sum_to_one(probe):
    rng = np.random.default_rng(110)
    x = np.concatenate([2.0 ** rng.uniform(-60, 12, N_EXACT - 16), _branch_points()])
    out, _ = probe("shell_step", x)
    ln2h = 0.5 / LOG2E
    worst = {"e": 0.0, "u": 0.0, "v": 0.0, "u_rel": 0.0, "v_rel": 0.0, "sum": 0.0}
    assert (out >= 0).all(), "a negative weight"
    for j, xv in enumerate(x.tolist()):
        exact = M.dec_shell(xv)
        for name, g, ex in zip("euv", out[:, j].tolist(), exact):
            err = float(M.CTX.subtract(M.D(g), ex).copy_abs()) / EPS
            worst[name] = max(worst[name], err)
            assert err <= 4.0, f"shell_step {name} at x = {xv!r}: {err:.3f} 2^-52 absolute"
            if name != "e" and xv <= ln2h:
                r = M.dec_rel_err(g, ex) / EPS
                worst[name + "_rel"] = max(worst[name + "_rel"], r)
                assert r <= 16.0, f"shell_step {name} at x = {xv!r}: {r:.3f} 2^-52 relative"
        s = float(abs(sum(Fraction(g) for g in out[:, j].tolist()) - 1)) / EPS
        worst["sum"] = max(worst["sum"], s)
        assert s <= 4.0, f"e + u + v - 1 = {s:.3f} 2^-52 at x = {xv!r}"
    print("shell_step: worst absolute errors e {e:.3f} u {u:.3f} v {v:.3f} 2^-52; relative on "
          "x <= ln2/2: u {u_rel:.3f} v {v_rel:.3f} 2^-52; |e + u + v - 1| {sum:.3f} 2^-52"
          .format(**worst))


def test_shell_step_limits(probe):
    x = np.array([0.0, 2.0 ** 60, 2.0 ** 70, np.inf])
    out, _ = probe("shell_step", x)
    e, u, v = out
    assert e[0] == 1.0 and u[0] == 0.0 and v[0] == 0.0          # a transparent shell
    assert (e[1:] == 0.0).all() and (u[1:] == 0.0).all() and (v[1:] == 1.0).all()
