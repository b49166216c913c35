"""CPU tests that pin tests/emergent_ref.py, the NumPy restatement the GPU tests of
frei_emergent (K11) are held to, so those do not rest on an unchecked formula — and
frei_amd.gauss_angles, the default quadrature.

Measured (pytest -s prints each figure): v(x) against 40-digit arithmetic 2.0e-15 relative;
e + u + v - 1 at most 1.1e-16; restatement against composite Simpson, 2000 panels per shell,
9.1e-11; isothermal I / B - 1 and flux / (pi B) - 1 at most 5.6e-16."""
import decimal

import numpy as np
import pytest

from tests import emergent_ref as R

EPS = 2.0 ** -52


def _ramp(n_layers, rng, hot=2500.0, cold=900.0):
    return np.linspace(hot, cold, n_layers) + 80.0 * rng.standard_normal(n_layers)


# ------------------------------------------------------------------ v(x) and the step weights
def _xs():
    rng = np.random.default_rng(11)
    x = 10 ** rng.uniform(-12, 3, 2000)
    return np.concatenate([x, [np.nextafter(0.125, 0), 0.125, np.nextafter(0.125, 1)]])


def test_v_matches_40_digit_arithmetic():
    decimal.getcontext().prec = 40
    x = _xs()
    v = R.v_of(x)
    worst = 0.0
    for xi, vi in zip(x, v):
        d = decimal.Decimal(float(xi))
        exact = 1 - (1 - (-d).exp()) / d
        worst = max(worst, abs(float((decimal.Decimal(float(vi)) - exact) / exact)))
    print(f"v(x) against 40 digits: {worst:.3e}")
    assert worst <= 1e-14


def test_v_limits():
    v = R.v_of(np.array([0.0, np.inf]))
    assert v[0] == 0.0 and v[1] == 1.0
    assert np.isnan(R.v_of(np.array([np.nan]))[0])


def test_step_weights_are_a_convex_combination():
    x = np.concatenate([_xs(), [0.0, np.inf]])
    e, u, v = R.weights_of(x)
    assert np.all(e >= 0) and np.all(u >= 0) and np.all(v >= 0)
    worst = float(np.max(np.abs((e + u + v) - 1.0)))
    print(f"e + u + v - 1: {worst:.3e}")
    assert worst <= 4 * EPS


# ------------------------------------------------------------------ independent quadrature
def _simpson_intensity(dtaus, T, lam, mu, panels):
    """The same piecewise-linear source integrated along the ray by composite Simpson, ``panels``
    panels (of two intervals) per shell: I = B_1 exp(-X) + sum over shells of the integral of
    S(s) exp(-(distance to the top)) ds, s the slant optical depth from the shell's bottom."""
    nL, n = dtaus.shape
    B = {l: R.planck(lam, T[l]) for l in range(1, nL)}
    B[nL] = B[nL - 1]
    x = {l: dtaus[l] / mu for l in range(1, nL)}
    above = {nL - 1: np.zeros(n)}
    for l in range(nL - 2, 0, -1):
        above[l] = above[l + 1] + x[l + 1]
    t = np.linspace(0.0, 1.0, 2 * panels + 1)[:, None]        # s / x
    w = np.full(2 * panels + 1, 2.0)
    w[1::2] = 4.0
    w[0] = w[-1] = 1.0
    I = B[1] * np.exp(-(above[1] + x[1]))
    for l in range(1, nL):
        S = B[l] + (B[l + 1] - B[l]) * t
        f = S * np.exp(-(x[l] * (1.0 - t) + above[l]))
        I = I + (w[:, None] * f).sum(axis=0) * x[l] / (6.0 * panels)
    return I


def test_restatement_matches_an_independent_quadrature():
    rng = np.random.default_rng(12)
    n_layers, n_lam = 12, 64
    lam = np.logspace(np.log10(0.5), 1.0, n_lam)
    dt = 10 ** rng.uniform(-4, np.log10(5.0), (n_layers, n_lam))
    dt[0] = np.nan
    T = _ramp(n_layers, rng)
    mu = np.array([0.1, 0.3, 0.7, 1.0])
    inten, _ = R.emergent(dt, T, lam, mu)
    worst = 0.0
    for k in range(mu.size):
        q = _simpson_intensity(dt, T, lam, mu[k], 2000)
        worst = max(worst, float(np.max(np.abs(inten[k] - q) / q)))
    print(f"restatement against Simpson, 2000 panels per shell: {worst:.3e}")
    assert worst <= 1e-9


# ------------------------------------------------------------------ physics of the recurrence
def _random_case(seed, n_layers=30, n_lam=97):
    rng = np.random.default_rng(seed)
    lam = np.logspace(np.log10(0.5), 1.0, n_lam)
    dt = 10 ** rng.uniform(-8, 3, (n_layers, n_lam))
    dt[0] = np.nan
    return rng, lam, dt


def test_isothermal_intensity_is_the_planck_function():
    _, lam, dt = _random_case(13)
    T = np.full(dt.shape[0], 1500.0)
    T[0] = np.nan                                  # never read
    mu = np.array([0.05, 0.2, 0.5, 0.9, 1.0])
    inten, _ = R.emergent(dt, T, lam, mu)
    B = R.planck(lam, 1500.0)
    worst = float(np.max(np.abs(inten / B - 1.0)))
    print(f"isothermal I / B - 1: {worst:.3e}")
    assert worst <= 4e-15


@pytest.mark.parametrize("n", [1, 2, 4, 8, 16])
def test_isothermal_flux_is_pi_b(n):
    import frei_amd
    _, lam, dt = _random_case(14)
    T = np.full(dt.shape[0], 1500.0)
    mu, w = frei_amd.gauss_angles(n)
    _, flux = R.emergent(dt, T, lam, mu, w)
    worst = float(np.max(np.abs(flux / (np.pi * R.planck(lam, 1500.0)) - 1.0)))
    print(f"n = {n}: isothermal flux / (pi B) - 1: {worst:.3e}")
    assert worst <= 4e-15


def test_transparent_and_opaque_limits_are_exact():
    rng, lam, dt = _random_case(15)
    T = _ramp(dt.shape[0], rng)
    mu = np.array([0.25, 0.5, 1.0])
    clear, _ = R.emergent(np.zeros_like(dt), T, lam, mu)
    opaque, _ = R.emergent(np.full_like(dt, 1e6), T, lam, mu)
    for k in range(mu.size):
        assert np.array_equal(clear[k], R.planck(lam, T[1])), "zero dtaus: not B_1"
        assert np.array_equal(opaque[k], R.planck(lam, T[-1])), "opaque: not B_{nL-1}"


def test_limb_darkening_follows_the_temperature_gradient():
    rng, lam, dt = _random_case(16)
    mu = np.array([0.05, 0.1, 0.2, 0.35, 0.5, 0.7, 0.85, 1.0])
    T = np.sort(_ramp(dt.shape[0], rng))[::-1].copy()         # decreasing upwards
    down, _ = R.emergent(dt, T, lam, mu)
    up, _ = R.emergent(dt, T[::-1].copy(), lam, mu)
    slack = 1e-13
    assert np.all(down[1:] >= down[:-1] * (1 - slack)), "cooler above: I must rise with mu"
    assert np.all(up[1:] <= up[:-1] * (1 + slack)), "hotter above: I must fall with mu"
    assert np.any(down[-1] > down[0]) and np.any(up[-1] < up[0])


# ------------------------------------------------------------------ the default quadrature
@pytest.mark.parametrize("n", [1, 2, 3, 4, 8, 16, 64])
def test_gauss_angles(n):
    import frei_amd
    mu, w = frei_amd.gauss_angles(n)
    assert mu.shape == (n,) and w.shape == (n,)
    assert np.all(mu > 0) and np.all(mu < 1) and np.all(np.diff(mu) > 0) and np.all(w > 0)
    s0, s1 = float(np.sum(w)), float(np.sum(w * mu))
    print(f"n = {n}: sum w - 1 = {s0 - 1:.3e}, sum w mu - 1/2 = {s1 - 0.5:.3e}")
    assert abs(s0 - 1.0) <= 2 * EPS
    assert abs(s1 - 0.5) <= 2 * EPS * 0.5


def test_gauss_angles_refuses_no_angle():
    import frei_amd
    with pytest.raises(ValueError):
        frei_amd.gauss_angles(0)
