"""Host tests of the broadening (K13) that need no GPU: the plan of Broadening against the
brute-force plan of tests/broaden_ref.py, norm by the library's operations, the argument checks
of frei_brd_create (all made before a device is touched) and the discretisation errors of the
kernel tables at the spacings the constructors ship."""
import ctypes

import numpy as np
import pytest

from tests import broaden_ref as R

_i32p = ctypes.POINTER(ctypes.c_int32)


def _axis(n, seed=0, lo=1.0, hi=1.2, jitter=0.3):
    """Log-spaced with a seeded relative jitter of up to `jitter` of a step."""
    rng = np.random.default_rng(seed)
    ln = np.linspace(np.log(lo), np.log(hi), n)
    step = ln[1] - ln[0]
    return np.exp(ln + step * rng.uniform(-jitter, jitter, n))


def _step_kms(n, lo=1.0, hi=1.2):
    return R.C_KMS * (np.log(hi) - np.log(lo)) / (n - 1)


def _triangle(h, dv):
    from frei_amd.broaden import BroadeningKernel
    return BroadeningKernel(dv, 1.0 - np.abs(np.arange(-h, h + 1)) / (h + 1.0))


@pytest.mark.parametrize("half_steps", [0.4, 1.0, 1.5, 2.0, 8.2, 50.3, 400.0])
def test_plan_matches_the_brute_force_plan(half_steps):
    from frei_amd.broaden import Broadening
    n = 257
    lam = _axis(n, seed=int(10 * half_steps))
    k = _triangle(4, half_steps * _step_kms(n) / 4)
    b = Broadening(lam, k)
    u, tw = R.axis(lam)
    assert np.array_equal(b.u, u) and np.array_equal(b.tw, tw)
    first, count = R.plan(u, k.values.size, k.dv)
    assert b.first.dtype == np.int32 and b.count.dtype == np.int32
    assert np.array_equal(b.first, first) and np.array_equal(b.count, count)
    H, i = k.half_width, np.arange(n)
    last = b.first + b.count - 1
    assert np.all((b.first <= i) & (i <= last)), "every window holds its own point"
    assert np.all(np.abs(u[b.first] - u) <= H) and np.all(np.abs(u[last] - u) <= H)
    below, above = b.first > 0, last < n - 1
    assert np.all(np.abs(u[b.first[below] - 1] - u[below]) > H)
    assert np.all(np.abs(u[last[above] + 1] - u[above]) > H)
    if half_steps >= 400:
        assert np.all(b.count == n)
    assert np.array_equal(b.norm, R.norm(u, tw, first, count, b.inv_dv, b.tab))


def test_plan_on_an_axis_whose_gaps_equal_the_half_width():
    """u in exact steps of 1/4 km/s and H = 3 steps: |u_j - u_i| = H holds with equality, where
    a search for the rounded u_i -+ H and the subtraction itself can disagree."""
    from frei_amd.broaden import BroadeningKernel, windows
    u = 70000.0 + 0.25 * np.arange(100)
    k = BroadeningKernel(0.25, [0, 1, 2, 3, 2, 1, 0])
    first, count = windows(u, k.half_width)
    rf, rc = R.plan(u, 7, 0.25)
    assert np.array_equal(first, rf) and np.array_equal(count, rc)
    assert count[50] == 7
    u = R.C_KMS * np.log(np.exp(np.linspace(0.0, 0.1, 300)))
    H = 3 * (u[1] - u[0])
    k = BroadeningKernel(H / 3, [0, 1, 2, 3, 2, 1, 0])
    first, count = windows(u, k.half_width)
    rf, rc = R.plan(u, 7, k.dv)
    assert np.array_equal(first, rf) and np.array_equal(count, rc)


def test_plan_of_a_long_axis_is_vectorised():
    """500k points build without a Python loop over the points (a fraction of a second)."""
    from frei_amd.broaden import Broadening, BroadeningKernel
    lam = _axis(500_000, seed=3, lo=1.0, hi=2.0)
    b = Broadening(lam, BroadeningKernel.gaussian(resolving_power=50_000, oversample=4))
    mid = b.count[250_000]
    # 4 standard deviations of c / 50 000 / 2.355 = 2.55 km/s over steps of 0.416 km/s: 24.5
    assert 47 <= mid <= 51 and b.count.min() >= mid // 2
    sel = np.array([0, 1, 7, 250_000, 499_998, 499_999])
    for i in sel:
        inside = np.nonzero(np.abs(b.u - b.u[i]) <= b.kernel.half_width)[0]
        assert (b.first[i], b.count[i]) == (inside[0], inside.size)


# ------------------------------------------------------------------ frei_brd_create's checks
def _create(u, tw, first, count, tab, dv, inv_dv=None):
    from frei_amd import _native as N
    u, tw, tab = N.f64(u), N.f64(tw), N.f64(tab)
    first = np.ascontiguousarray(first, dtype=np.int32)
    count = np.ascontiguousarray(count, dtype=np.int32)
    h = ctypes.c_void_p()
    rc = N.lib().frei_brd_create(ctypes.byref(h), 0, u.size, N.dptr(u), N.dptr(tw),
                                 first.ctypes.data_as(_i32p), count.ctypes.data_as(_i32p),
                                 tab.size, dv, 1.0 / dv if inv_dv is None else inv_dv,
                                 N.dptr(tab))
    assert h.value is None
    return rc, N.lib().frei_last_error().decode()


def _good(n=12):
    u = 1000.0 + np.arange(n, dtype=float)
    tw = np.ones(n)
    tab, dv = np.array([0.0, 1.0, 2.0, 1.0, 0.0]), 0.75       # H = 1.5: a point either side
    first, count = R.plan(u, tab.size, dv)
    return dict(u=u, tw=tw, first=first, count=count, tab=tab, dv=dv)


def test_create_argument_errors_fire_without_a_gpu():
    g = _good()
    u = g["u"].copy()
    u[4] = u[3] - 0.5
    rc, msg = _create(**dict(g, u=u))
    assert rc != 0 and "u[4]" in msg and "ascending" in msg
    u = g["u"].copy()
    u[6] = np.inf
    rc, msg = _create(**dict(g, u=u))
    assert rc != 0 and "u[6]" in msg
    rc, msg = _create(**dict(g, tab=[0.0, 1.0, 1.0, 0.0]))
    assert rc != 0 and "n_tab = 4" in msg and "odd" in msg
    rc, msg = _create(**dict(g, tab=[0.0, 1.0, -2.0, 1.0, 0.0]))
    assert rc != 0 and "tab[2]" in msg
    rc, msg = _create(**dict(g, tab=[0.0, 1.0, np.nan, 1.0, 0.0]))
    assert rc != 0 and "tab[2]" in msg
    for dv in (0.0, -1.0):
        rc, msg = _create(**dict(g, dv=dv, inv_dv=1.0))
        assert rc != 0 and "dv must be > 0" in msg
    first, count = g["first"].copy(), g["count"].copy()
    first[5], count[5] = 6, 1
    rc, msg = _create(**dict(g, first=first, count=count))
    assert rc != 0 and "output 5" in msg and "own point" in msg
    count = g["count"].copy()
    count[7] = 2                                   # leaves out the point above
    rc, msg = _create(**dict(g, count=count))
    assert rc != 0 and "output 7" in msg and "leaves out" in msg
    first, count = g["first"].copy(), g["count"].copy()
    first[3], count[3] = 1, 4                      # takes in a point too far below
    rc, msg = _create(**dict(g, first=first, count=count))
    assert rc != 0 and "output 3" in msg and "farther" in msg
    count = g["count"].copy()
    count[11] = 3
    rc, msg = _create(**dict(g, count=count))
    assert rc != 0 and "output 11" in msg and "leaves the axis" in msg
    rc, msg = _create(**dict(g, tab=np.zeros(5)))
    assert rc != 0 and "norm[0]" in msg


def test_create_refuses_a_window_over_the_cap():
    from frei_amd.broaden import MAX_COUNT
    assert MAX_COUNT >= 1024
    n = MAX_COUNT + 1
    u = 1000.0 + np.arange(n, dtype=float)
    first, count = np.zeros(n, np.int32), np.full(n, n, np.int32)
    rc, msg = _create(u, np.ones(n), first, count, [1.0, 1.0, 1.0], float(n))
    assert rc != 0 and "count[0]" in msg and str(MAX_COUNT) in msg
    # one point fewer passes every check and fails only for want of a device, or succeeds
    n = MAX_COUNT
    first, count = np.zeros(n, np.int32), np.full(n, n, np.int32)
    from frei_amd import _native as N
    h = ctypes.c_void_p()
    u, tw, tab = N.f64(u[:n]), np.ones(n), np.ones(3)
    rc = N.lib().frei_brd_create(ctypes.byref(h), 0, n, N.dptr(u), N.dptr(tw),
                                 first.ctypes.data_as(_i32p), count.ctypes.data_as(_i32p), 3,
                                 float(n), 1.0 / n, N.dptr(tab))
    if rc == 0:
        N.lib().frei_brd_destroy(h)
    else:
        assert "device" in N.lib().frei_last_error().decode()


# ------------------------------------------------------------------ the kernel tables
def test_kernel_constructors_reject_bad_tables():
    from frei_amd.broaden import BroadeningKernel
    for dv, vals in ((0.0, [0, 1, 0]), (1.0, [0, 1]), (1.0, [0, 1, 1, 0]), (1.0, [0, -1, 0]),
                     (1.0, [0, np.nan, 0])):
        with pytest.raises(ValueError):
            BroadeningKernel.from_profile(dv, vals)
    with pytest.raises(ValueError):
        BroadeningKernel.gaussian()
    with pytest.raises(ValueError):
        BroadeningKernel.gaussian(fwhm_kms=3.0, resolving_power=1e5)
    k = BroadeningKernel.gaussian(resolving_power=100_000)
    assert np.isclose(k(0.0) / k(0.5 * R.C_KMS / 100_000), 2.0, rtol=1e-3)


def test_gaussian_and_rotation_integrate_to_one():
    """Discretisation errors of the shipped tables, measured here on the CPU (trapezoid integral
    of the table minus 1): Gaussian cut at 4 standard deviations, 16 samples per standard
    deviation, -6.37e-5 (the mass beyond 4 sigma); rotation on 2 x 512 + 1 samples, epsilon 0.6,
    -1.66e-5 (the square-root edge).  Asserted limits, twice the measured values: 1.27e-4 and
    3.3e-5; without limb darkening (epsilon 0, all of the profile in the square root) the error is
    larger by 1 / (1 - 0.6) (1 - 0.6 / 3) = 2, and so is its limit."""
    from frei_amd.broaden import BroadeningKernel
    g = BroadeningKernel.gaussian(fwhm_kms=3.0)
    r = BroadeningKernel.rotation(5.0)
    print(f"gaussian integral - 1 = {g.integral() - 1.0:.3e}; rotation integral - 1 = "
          f"{r.integral() - 1.0:.3e}")
    assert abs(g.integral() - 1.0) <= 1.27e-4
    assert abs(r.integral() - 1.0) <= 3.3e-5
    assert r.values[0] == 0.0 and r.values[-1] == 0.0 and r.half_width == 5.0
    flat = BroadeningKernel.rotation(5.0, epsilon=0.0)
    assert abs(flat.integral() - 1.0) <= 2 * 3.3e-5


def test_convolution_of_gaussians_is_the_gaussian_of_the_summed_variances():
    """Measured here: max |g1 * g2 - g12| / max g12 = 2.73e-4 at the shipped spacing (16 samples
    per standard deviation, both cut at 4 standard deviations; the cut tails dominate).
    Asserted limit, twice that: 5.5e-4."""
    from frei_amd.broaden import BroadeningKernel
    f1, f2 = 3.0, 4.0
    c = BroadeningKernel.gaussian(fwhm_kms=f1).convolve(BroadeningKernel.gaussian(fwhm_kms=f2))
    g12 = BroadeningKernel.gaussian(fwhm_kms=np.hypot(f1, f2), n_sigma=8.0)
    err = float(np.max(np.abs(c.values - g12(c.velocities))) / g12(0.0))
    print(f"convolution: max |g1 * g2 - g12| / max g12 = {err:.3e}")
    assert c.values.size % 2 == 1 and c.dv == BroadeningKernel.gaussian(fwhm_kms=f1).dv
    assert err <= 5.5e-4


def test_restatement_widens_a_gaussian_line_as_the_variances_add():
    """A Gaussian line of 6 km/s FWHM on a log axis of 0.5 km/s steps, broadened by the
    restatement with the shipped 8 km/s Gaussian table: the second moment of the result is that
    of a 10 km/s line.  Measured here: relative error of the standard deviation -6.9e-4 (the
    table's cut at 4 standard deviations narrows it).  Asserted limit, twice that: 1.4e-3."""
    from frei_amd.broaden import Broadening, BroadeningKernel
    step = 0.5
    n = 801
    lam = np.exp(step / R.C_KMS * np.arange(n))
    b = Broadening(lam, BroadeningKernel.gaussian(fwhm_kms=8.0))
    s1 = 6.0 / 2.3548200450309493
    v = b.u - b.u[n // 2]
    line = np.exp(-0.5 * (v / s1) ** 2)
    out, _ = R.apply(line, b.u, b.tw, b.first, b.count, b.inv_dv, b.tab)
    out = out[0]
    sd = np.sqrt(np.sum(out * v * v) / np.sum(out) - (np.sum(out * v) / np.sum(out)) ** 2)
    want = 10.0 / 2.3548200450309493
    print(f"broadened line: sd / expected - 1 = {sd / want - 1.0:.3e}")
    assert abs(sd / want - 1.0) <= 1.6e-4


def test_bound_is_neither_vacuous_nor_tight():
    """Two CPU orders of the same sum — ascending fused multiply-adds in exact arithmetic
    (fractions) rounded once per step, and math.fsum — differ by a fraction of the bound."""
    import math
    from fractions import Fraction
    from frei_amd.broaden import Broadening
    lam = _axis(65, seed=5)
    k = _triangle(4, 8.2 * _step_kms(65) / 4)
    b = Broadening(lam, k)
    x = 10 ** np.random.default_rng(5).uniform(3, 4, (1, 65))
    ref, bound = R.apply(x, b.u, b.tw, b.first, b.count, b.inv_dv, b.tab)
    nm = b.norm
    worst = 0.0
    for i in range(65):
        w = R.weights(b.u, b.tw, i, b.first[i], b.count[i], b.inv_dv, b.tab)
        seg = x[0, b.first[i]:b.first[i] + b.count[i]]
        acc = 0.0
        for wj, xj in zip(w, seg):
            acc = float(Fraction(float(wj)) * Fraction(float(xj)) + Fraction(acc))   # one fma
        fs = math.fsum(float(wj) * float(xj) for wj, xj in zip(w, seg))
        worst = max(worst, abs(acc / nm[i] - fs / nm[i]) / bound[0, i])
        assert abs(acc / nm[i] - ref[0, i]) <= bound[0, i]
    print(f"ascending fma against fsum: {worst:.3f} of the bound")
    assert 0.0 < worst <= 0.5
