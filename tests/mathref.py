"""Exact references and hard-case generators for the device math tests (tests/test_gpu_math.py;
pinned without a GPU by tests/test_math_hardcases_host.py).  Standard library arithmetic only:
``fractions.Fraction``, Python integers and ``decimal`` at 60 digits; NumPy only carries arrays.

ulp errors are measured against the exact value, in units of the ulp of the exact result (the
spacing of doubles at the exact value's binade; 2^-1074 in the subnormal range)."""
import decimal
import math
from fractions import Fraction

import numpy as np

CTX = decimal.Context(prec=60, Emin=-10 ** 6, Emax=10 ** 6, rounding=decimal.ROUND_HALF_EVEN)
D = decimal.Decimal
LN2 = CTX.ln(D(2))
EPS = 2.0 ** -52


def bits(x):
    """The doubles' bit patterns as int64 (bitwise comparison; every NaN compares by payload)."""
    return np.ascontiguousarray(x, dtype=np.float64).view(np.int64)


def same_bits(got, want):
    """Elementwise: identical bits, or both NaN."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# ------------------------------------------------------------------ exact ulp measures
def _floor_log2(v):
    """floor(log2 |v|) of a non-zero Fraction, exactly."""
    p, q = abs(v.numerator), v.denominator
    e = p.bit_length() - q.bit_length()
    # 2^e <= p / q < 2^(e + 1), up to one step
    if e >= 0:
        if p < (q << e):
            e -= 1
    elif (p << -e) < q:
        e -= 1
    return e


def ulp_of(v):
    """The spacing of doubles at the exact value v (a Fraction), as a Fraction."""
    e = -1022 if v == 0 else max(_floor_log2(v), -1022)
    return Fraction(2) ** (e - 52)


def ulp_err(got, exact):
    """|got - exact| in ulps of the exact value (Fraction); got a finite float."""
    return float(abs(Fraction(got) - exact) / ulp_of(exact))


def is_faithful(got, exact):
    """got is one of the two doubles bracketing the exact value (or equals it)."""
    g = Fraction(got)
    if g == exact:
        return True
    if g < exact:
        return Fraction(math.nextafter(got, math.inf)) > exact
    return Fraction(math.nextafter(got, -math.inf)) < exact


def round_div(a, b):
    """The correctly rounded a / b from exact rational arithmetic (int / int true division of
    Python integers is correctly rounded)."""
    q = Fraction(a) / Fraction(b)
    r = q.numerator / q.denominator
    if r == 0.0 and (math.copysign(1.0, a) * math.copysign(1.0, b)) < 0:
        return -0.0
    return r


def round_sqrt(x):
    """The correctly rounded square root of a positive finite double, by math.isqrt: the root of
    the argument scaled to a 2 x 64-bit-plus integer, rounded to nearest at 53 bits (a double's
    root is never a rounding midpoint: the midpoint's square has more than 53 bits)."""
    m, e = math.frexp(x)
    n = int(m * 2 ** 53)          # x = n 2^(e - 53), n < 2^53
    e -= 53
    if e & 1:
        n <<= 1
        e -= 1
    n <<= 128                     # x = n 2^(e - 128), e even: sqrt = isqrt(n) 2^(e / 2 - 64)
    s = math.isqrt(n)
    exact_sq = s * s == n
    extra = s.bit_length() - 53
    low = s & ((1 << extra) - 1)
    s >>= extra
    half = 1 << (extra - 1)
    if low > half or (low == half and (not exact_sq or s & 1)):
        s += 1
    return math.ldexp(s, e // 2 - 64 + extra)


def sqrt_is_faithful(got, x):
    """pred(got)^2 < x < succ(got)^2 exactly (got > 0)."""
    X = Fraction(x)
    g = Fraction(got)
    if g * g == X:
        return True
    lo = Fraction(math.nextafter(got, 0.0))
    hi = Fraction(math.nextafter(got, math.inf))
    return lo * lo < X < hi * hi


def rcp_within_one_ulp(got, b):
    """|got - 1 / b| <= 1 ulp of the exact 1 / b, and that error as a float."""
    exact = 1 / Fraction(b)
    err = abs(Fraction(got) - exact) / ulp_of(exact)
    return err <= 1, float(err)


# ------------------------------------------------------------------ decimal references
def _dec_ulp(v):
    """The spacing of doubles at the exact positive Decimal v."""
    f = float(v)
    if f < 2.0 ** -1022:
        e = -1022
    else:
        e = math.frexp(f)[1] - 1
        if CTX.power(D(2), e) > v:      # float(v) rounded up into the next binade
            e -= 1
    return CTX.power(D(2), e - 52)


def dec_ulp_err(got, exact):
    """|got - exact| in ulps of the exact positive Decimal value."""
    if exact == 0:
        return float(CTX.divide(D(got).copy_abs(), CTX.power(D(2), -1074)))
    return float(CTX.divide(CTX.subtract(D(got), exact).copy_abs(), _dec_ulp(exact)))


def dec_rel_err(got, exact):
    return float(CTX.divide(CTX.subtract(D(got), exact).copy_abs(), exact.copy_abs()))


def dec_exp(x):
    """exp(x) of a double, correctly rounded at 60 digits."""
    return CTX.exp(D(x))


def dec_planck(c1, x):
    """c1 / expm1(x) for doubles c1 and x > 0."""
    return CTX.divide(D(c1), CTX.subtract(CTX.exp(D(x)), D(1)))


def dec_shell(x):
    """(e, u, v) of one shell at optical depth x > 0: e = exp(-x), v = 1 - (1 - e) / x,
    u = (1 - e) - v."""
    e = CTX.exp(CTX.minus(D(x)))
    em = CTX.subtract(D(1), e)
    v = CTX.subtract(D(1), CTX.divide(em, D(x)))
    return e, CTX.subtract(em, v), v


# ------------------------------------------------------------------ hard cases: division
def div_midpoint_cases(n_b, seed=0):
    """Quotients within about 2^-54 ulp of a rounding midpoint.  For odd 53-bit B and
    k in {+-1, +-3}, N = (-k / B) mod 2^54 is odd; where it lies in [2^53, 2^54),
    A = (B N + k) / 2^54 is an integer below 2^53 and A / B = N / 2^54 + k / (2^54 B): the
    midpoint N / 2^54 of two doubles in [1/2, 1) missed by k / (2 B) ulp.
    Returns (A, B, N, k) as Python integer lists."""
    rng = np.random.default_rng(seed)
    Bs = (rng.integers(1 << 51, 1 << 52, n_b, dtype=np.int64) << 1) | 1
    out = []
    for B in Bs.tolist():
        inv = pow(B, -1, 1 << 54)
        for k in (1, -1, 3, -3):
            N = (-k * inv) % (1 << 54)
            if N & 1 and (1 << 53) <= N < (1 << 54):
                A, rem = divmod(B * N + k, 1 << 54)
                assert rem == 0
                out.append((A, B, N, k))
    return out


def div_midpoint_expected(N, k):
    """The correctly rounded A / B of a case: the neighbour of the midpoint N / 2^54 on k's side."""
    return math.ldexp((N + 1) // 2 if k > 0 else (N - 1) // 2, -53)


# ------------------------------------------------------------------ hard cases: square root
def _lift(c, m, nbits):
    """The root of m (m + 1) = c (mod 2^nbits) congruent to m mod 2, by 2-adic Newton steps (the
    derivative 2 m + 1 is odd, hence invertible)."""
    mod = 1 << nbits
    for _ in range(nbits.bit_length() + 1):
        m = (m - (m * (m + 1) - c) * pow(2 * m + 1, -1, mod)) % mod
    assert (m * (m + 1) - c) % mod == 0
    return m


def sqrt_midpoint_cases(binade):
    """Square roots within (|c| + 1/4) / (2 m) ulp of a rounding midpoint, for even |c| <= 256.
    binade 0: m in [2^52, 2^53) with m (m + 1) = c (mod 2^53); x = (m (m + 1) - c) 2^-106 is a
    double in [1/4, 1) whose root is (m + 1/2) 2^-53 less (c + 1/4) / (2 m + 1) ulp.
    binade 1: the same with modulus 2^52 and m = 2^52 + root <= 1.1 2^52:
    x = (m (m + 1) - c) 2^-104 in [1, 1.21], root near (m + 1/2) 2^-52.
    Returns (x, m, c) with x a float, and the scale s such that the midpoint is (m + 1/2) 2^-s."""
    nbits, scale = (53, 53) if binade == 0 else (52, 52)
    out = []
    for c in range(-256, 257, 2):
        for start in (0, 1):
            m = _lift(c, start, nbits)
            if binade == 0:
                if not (1 << 52) <= m < (1 << 53):
                    continue
            else:
                m += 1 << 52
                if m * 10 > 11 * (1 << 52):
                    continue
            X, rem = divmod(m * (m + 1) - c, 1 << nbits)
            assert rem == 0 and X < (1 << 53)
            x = math.ldexp(X, -scale)
            if binade == 1 and not 1.0 <= x <= 1.21:
                continue
            out.append((x, m, c))
    return out, scale


def sqrt_midpoint_expected(m, c, scale):
    """The correctly rounded root of a case: below the midpoint for c >= 0, above it for c < 0."""
    return math.ldexp(m if c >= 0 else m + 1, -scale)
