"""The hard-case generators and exact references of tests/mathref.py, checked without a GPU
against Fraction and math.isqrt: a generator bug must not pass for a kernel result
(tests/test_gpu_math.py runs the device functions on these cases)."""
import math
from fractions import Fraction

import numpy as np

from tests import mathref as M


def test_div_midpoint_cases_sit_on_midpoints_and_ieee_rounds_them():
    cases = M.div_midpoint_cases(1500, seed=3)
    assert len(cases) >= 2000
    worst = 0.0
    for A, B, N, k in cases:
        assert B & 1 and (1 << 52) <= B < (1 << 53) and 0 < A < (1 << 53)
        assert N & 1 and (1 << 53) <= N < (1 << 54)
        q = Fraction(A, B)
        mid = Fraction(N, 1 << 54)
        # the exact quotient misses the midpoint of two doubles in [1/2, 1) by k / (2 B) ulp
        assert (q - mid) / Fraction(1, 1 << 53) == Fraction(k, 2 * B)
        worst = max(worst, abs(k) / (2 * B))
        want = M.div_midpoint_expected(N, k)
        assert want == M.round_div(float(A), float(B)) == float(A) / float(B)
        assert abs(Fraction(want) - mid) == Fraction(1, 1 << 54)
        assert M.is_faithful(want, q)
        # the neighbour on the other side is faithful but not correct; two away is neither
        other = math.ldexp((N - 1) // 2 if k > 0 else (N + 1) // 2, -53)
        assert M.is_faithful(other, q) and other != want
        assert not M.is_faithful(math.nextafter(other, -1.0 if k > 0 else 2.0), q)
    assert worst < 2.0 ** -51


def test_sqrt_midpoint_cases_sit_on_midpoints_and_ieee_rounds_them():
    for binade in (0, 1):
        cases, scale = M.sqrt_midpoint_cases(binade)
        assert len(cases) >= (200 if binade == 0 else 20), len(cases)
        for x, m, c in cases:
            X = Fraction(x)
            assert X == Fraction(m * (m + 1) - c, 1 << (2 * scale))
            if binade == 0:
                assert 0.25 <= x < 1.0 and (1 << 52) <= m < (1 << 53)
            else:
                assert 1.0 <= x <= 1.21 and (1 << 52) <= m
            # the root lies strictly between the midpoint's neighbours, on c's side of it
            mid = Fraction(2 * m + 1, 1 << (scale + 1))
            lo, hi = Fraction(m, 1 << scale), Fraction(m + 1, 1 << scale)
            assert lo * lo < X < hi * hi
            assert (X < mid * mid) == (c >= 0)
            # within (|c| + 1/4) / (2 m) ulp of it: (mid - d)^2 and (mid + d)^2 bracket x
            d = Fraction(4 * abs(c) + 1, 8 * m) / (1 << scale)
            assert (mid - d) ** 2 <= X <= (mid + d) ** 2
            want = M.sqrt_midpoint_expected(m, c, scale)
            assert want == M.round_sqrt(x) == math.sqrt(x)
            assert M.sqrt_is_faithful(want, x)
            other = math.ldexp(m + 1 if c >= 0 else m, -scale)
            assert M.sqrt_is_faithful(other, x)
            assert not M.sqrt_is_faithful(math.nextafter(other, 2.0 if c >= 0 else 0.0), x)


def test_round_sqrt_and_round_div_agree_with_ieee_on_random_operands():
    rng = np.random.default_rng(11)
    x = np.ldexp(1.0 + rng.random(2000), rng.integers(-767, 1023, 2000))
    for v in x.tolist():
        r = M.round_sqrt(v)
        assert r == math.sqrt(v)
        # correctly rounded: x lies between the squares of the midpoints around r
        h = Fraction(math.ulp(r)) / 2 if r != 2.0 ** (math.frexp(r)[1] - 1) else None
        if h is not None:
            assert (Fraction(r) - h) ** 2 < Fraction(v) < (Fraction(r) + h) ** 2
    a = np.ldexp(1.0 + rng.random(2000), rng.integers(-450, 450, 2000)) * rng.choice([-1, 1], 2000)
    b = np.ldexp(1.0 + rng.random(2000), rng.integers(-450, 450, 2000)) * rng.choice([-1, 1], 2000)
    for p, q in zip(a.tolist(), b.tolist()):
        assert M.round_div(p, q) == p / q
    assert math.copysign(1.0, M.round_div(-0.0, 3.0)) == -1.0
    assert math.copysign(1.0, M.round_div(0.0, 3.0)) == 1.0


def test_ulp_measures():
    one = Fraction(1)
    assert M.ulp_of(one) == Fraction(1, 1 << 52)
    assert M.ulp_of(one - Fraction(1, 1 << 60)) == Fraction(1, 1 << 53)
    assert M.ulp_of(Fraction(3, 1 << 1080)) == Fraction(1, 1 << 1074)
    assert M.ulp_of(Fraction(0)) == Fraction(1, 1 << 1074)
    assert M.ulp_err(1.0 + 2.0 ** -52, one) == 1.0
    assert M.ulp_err(5e-324, Fraction(0)) == 1.0
    assert M.is_faithful(1.0, one + Fraction(1, 1 << 60))
    assert M.is_faithful(1.0 + 2.0 ** -52, one + Fraction(1, 1 << 60))
    assert not M.is_faithful(1.0 - 2.0 ** -53, one + Fraction(1, 1 << 60))
    ok, err = M.rcp_within_one_ulp(1.0 / 3.0, 3.0)
    assert ok and err < 0.5
    ok, err = M.rcp_within_one_ulp(math.nextafter(math.nextafter(1.0 / 3.0, 1.0), 1.0), 3.0)
    assert not ok and 1.5 < err < 2.5
    # decimal side: exp(-745.2) is subnormal, measured in units of 2^-1074
    assert M.dec_ulp_err(5e-324, M.dec_exp(-745.2)) < 1.0
    assert M.dec_ulp_err(math.exp(-1.0), M.dec_exp(-1.0)) <= 0.51
    assert M.dec_ulp_err(1.0, M.dec_exp(0.0)) == 0.0
    assert abs(M.dec_ulp_err(1.0 + 2.0 ** -51, M.dec_exp(0.0)) - 2.0) < 1e-12
    e, u, v = M.dec_shell(2.0 ** -60)
    assert abs(float(v) / 2.0 ** -61 - 1.0) < 1e-15 and abs(float(u) / 2.0 ** -61 - 1.0) < 1e-15
    assert abs(float(e + u + v) - 1.0) == 0.0
    assert M.dec_rel_err(1.0 / math.expm1(0.5), M.dec_planck(1.0, 0.5)) < 4 * M.EPS
