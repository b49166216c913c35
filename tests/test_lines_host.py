"""K17 without a GPU: the restatement (tests/lines_ref.py) against exact values, the area of an
isolated line, LineList, and frei_xsec_create_lines' argument checks through the loaded library.

The Voigt bar is the one the float32 table needs, not a measured one: with every term positive,
a relative error <= 2^-26 per term keeps the fp64 sum within 2^-25 of exact, so the stored value
is within one float32 ulp of the correctly rounded one (the prefactors' few fp64 ulps and the
summation's n 2^-53 fit in that margin).  Measured worst of the restatement: 2.2e-11 against
scipy.special.wofz (the worst over several seeds), 7.4e-12 against the 50-digit fixture.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from frei_amd import _native as N
from frei_amd.constants import AMU
from frei_amd.lines import LineList
from tests import lines_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voigt_case.npz")
K_BAR = 2.0 ** -26


@pytest.fixture(scope="module")
def case():
    return dict(np.load(GOLDEN))


def ulps32(a, b):
    """Distance in float32 steps between two non-negative float32 arrays."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def table_of(case, fn=R.cross_section):
    return fn(case["nu0"], case["S_ref"], case["E_low"], case["gamma_ref"], case["n_exp"],
              float(case["mass_amu"]), float(case["T_ref"]), float(case["cutoff"]),
              case["q_ratio"], case["T_nodes"], case["p_nodes"], case["wl_hi"])


def test_fixture_covers_the_branches(case):
    x, y = case["x"], case["y"]
    assert x.min() == 0.0 and x.max() > 1e4
    assert y.min() < 1.5e-7 and y.max() > 1e3
    br = R.branch(x[:, None, :], y[:, :, None])
    assert set(np.unique(br)) == {0, 1, 2}
    # both sides of |z| = 8 within 0.2 % at small y, and of y = 1e-3 within a factor 1.5
    r = np.sqrt(x[:, None, :] ** 2 + y[:, :, None] ** 2)
    assert ((r > 7.98) & (r < 8.0)).any() and ((r > 8.0) & (r < 8.02)).any()
    assert ((y > 1e-3 / 1.5) & (y < 1e-3)).any() and ((y >= 1e-3) & (y < 1.5e-3)).any()
    # points a hair inside and outside the cutoff
    dnu = np.abs(R.wavenumbers(case["wl_hi"]) - case["nu0"][0])
    c = float(case["cutoff"])
    assert ((dnu <= c) & (dnu > c * (1 - 1e-8))).any() and ((dnu > c) & (dnu < c * (1 + 1e-8))).any()
    assert np.array_equal(dnu <= c, case["inside"])
    v = case["values"]
    assert np.all(v[..., ~case["inside"]] == 0) and v[v != 0].min() >= 2.0 ** -100


def test_restatement_K_against_fixture(case):
    K = R.voigt_K(case["x"][:, None, :], case["y"][:, :, None])
    err = np.abs(K - case["K"]) / case["K"]
    print("worst relative error of K against the fixture:", err.max())
    assert err.max() <= K_BAR


def test_restatement_K_against_wofz():
    special = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(17)
    n = 400000
    x = 10.0 ** rng.uniform(-8, 6, n)
    x[:1000] = 0.0
    y = 10.0 ** rng.uniform(-8, 5, n)
    ref = special.wofz(x + 1j * y).real
    err = np.abs(R.voigt_K(x, y) - ref) / ref
    br = R.branch(x, y)
    for b in (0, 1, 2):
        print("branch", b, "points", int((br == b).sum()), "worst", err[br == b].max())
    assert (br == 1).sum() > 1000 and (br == 2).sum() > 1000
    assert err.max() <= K_BAR


def test_restatement_table_against_fixture(case):
    got = table_of(case)
    want = case["values"].astype(np.float32)
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.all(got[..., ~case["inside"]] == 0.0)
    d = ulps32(got, want)
    print("restatement vs fixture: worst float32 ulps", d.max())
    assert d.max() <= 1


def test_area_of_an_isolated_line():
    """The table of one line integrates to its strength: (mass AMU) * integral(values dnu) = S.

    Bound on |area / S - 1|, derived:
      * truncation.  The profile is f = L * G, a Lorentzian of half-width g = gamma p convolved
        with a unit-area Gaussian of 1/e half-width alpha.  The Lorentzian's mass beyond +-c is
        (2 / pi) atan(g / c) = (2 g / (pi c)) (1 - (g / c)^2 / 3 + ...); the convolution moves
        mass outwards by a relative (3/2) alpha^2 / c^2.  With g > 2.2 alpha the sum stays below
        2 g / (pi c).
      * trapezoid rule, spacing h: |E| <= (h^2 / 8) integral |f''| (Peano kernel (t - a)(b - t) / 2
        <= h^2 / 8).  integral |L''| is the total variation of L' = 4 max |L'| =
        3 sqrt(3) / (2 pi g^2), and convolving with a probability density does not raise it:
        <= (h^2 / 8) * 0.827 / g^2.
      * the jump at the cutoff, from f(c) <= g / (pi c^2) to 0 inside one panel on each side:
        <= 2 h g / (pi c^2).
      * the float32 rounding of each value: <= 2^-24.
    Here T = T_ref and q_ratio = 1, so S = S_ref to a few fp64 ulps; g = 0.05, c = 40,
    alpha = 2.8e-3, h = 1e-3: 7.96e-4 + 4.2e-5 + 2e-8 + 6e-8 = 8.4e-4 <= 1e-3."""
    g, c, h, S, mass, T = 0.05, 40.0, 1e-3, 3e-20, 28.0, 296.0
    nu = 2000.0 + np.arange(-40500, 40501)[::-1] * h
    wl = 1e4 / nu
    tab = R.cross_section([2000.0], [S], [120.0], [g], [0.6], mass, T, c, [1.0], [T], [1.0], wl)
    nu_i = R.wavenumbers(wl)
    hmax = np.abs(np.diff(nu_i)).max()
    _, ia, _ = R.line_parameters([2000.0], [S], [120.0], [g], [0.6], mass, T, [1.0], [T])
    assert g > 2.2 / ia[0, 0]
    bound = (2 * g / (math.pi * c) + hmax ** 2 / 8 * 0.827 / g ** 2 +
             2 * hmax * g / (math.pi * c * c) + 2.0 ** -24)
    assert bound <= 1e-3
    v = tab[0, 0].astype(np.float64)
    area = -np.sum(0.5 * (v[1:] + v[:-1]) * np.diff(nu_i)) * (mass * AMU)
    print("area / S - 1 =", area / S - 1, "bound", bound)
    assert abs(area / S - 1) <= bound
    assert area < S          # what is missing is the truncated wings


PART = (np.array([100.0, 296.0, 1000.0, 3000.0]), np.array([40.0, 110.0, 420.0, 2600.0]))


def test_linelist_sorts_stably():
    nu0 = [2001.0, 1999.0, 2001.0, 1999.0, 2000.0]
    S = [1.0, 2.0, 3.0, 4.0, 5.0]
    ll = LineList(nu0, S, [10, 20, 30, 40, 50], [0.1, 0.2, 0.3, 0.4, 0.5], [0.5] * 5, 28.0,
                  partition=PART)
    assert np.array_equal(ll.nu0, [1999.0, 1999.0, 2000.0, 2001.0, 2001.0])
    assert np.array_equal(ll.S, [2.0, 4.0, 5.0, 1.0, 3.0])
    assert np.array_equal(ll.E_low, [20.0, 40.0, 50.0, 10.0, 30.0])
    assert np.array_equal(ll.gamma, [0.2, 0.4, 0.5, 0.1, 0.3])
    assert len(ll) == 5 and ll.T_ref == 296.0


def test_linelist_q_ratio():
    ll = LineList([2000.0], [1.0], [0.0], [0.1], [0.5], 28.0, partition=PART)
    q = ll.q_ratio([296.0, 1000.0, 648.0, 100.0])
    # ln Q linear in T between 296 K and 1000 K: halfway, Q = sqrt(110 * 420)
    np.testing.assert_allclose(q, [1.0, 110.0 / 420.0, 110.0 / math.sqrt(110.0 * 420.0),
                                   110.0 / 40.0], rtol=1e-14)
    with pytest.raises(ValueError, match=r"temperature\[1\] = 3000.5 K lies outside"):
        ll.q_ratio([500.0, 3000.5])
    with pytest.raises(ValueError, match="outside"):
        ll.q_ratio(99.0)


@pytest.mark.parametrize("kw, match", [
    (dict(nu0=[2000.0, -1.0]), r"nu0\[1\]"),
    (dict(nu0=[2000.0, np.nan]), r"nu0\[1\].*not finite"),
    (dict(S=[1.0, -1e-30]), r"S\[1\].*>= 0"),
    (dict(E_low=[np.inf, 0.0]), r"E_low\[0\].*not finite"),
    (dict(gamma=[0.1, 0.0]), r"gamma\[1\].*> 0"),
    (dict(n_exp=[0.5, np.nan]), r"n_exp\[1\]"),
    (dict(S=[1.0]), "entries like nu0"),
    (dict(mass=0.0), "mass"),
    (dict(T_ref=-1.0), "T_ref"),
    (dict(T_ref=50.0), "T_ref = 50.0 K lies outside"),
    (dict(partition=None), "partition"),
    (dict(partition=([100.0, 100.0], [1.0, 2.0])), "ascending"),
    (dict(partition=([100.0, 400.0], [1.0, 0.0])), r"Q_tab\[1\]"),
    (dict(partition=([100.0, 400.0], [1.0])), "one length"),
])
def test_linelist_validation(kw, match):
    args = dict(nu0=[2000.0, 2001.0], S=[1.0, 1.0], E_low=[0.0, 0.0], gamma=[0.1, 0.1],
                n_exp=[0.5, 0.5], mass=28.0, T_ref=296.0, partition=PART)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        LineList(**args)
    with pytest.raises(ValueError, match="at least one line"):
        LineList([], [], [], [], [], 28.0, partition=PART)


def hitran_record(mol, iso, nu, S, A, g_air, g_self, E, n_air, d_air):
    def fw(v, width, prec):   # Fortran's Fw.d: the leading zero goes when the field is full
        s = f"{v:.{prec}f}"
        return (s.replace("0.", ".", 1) if len(s) > width else s).rjust(width)

    rec = (f"{mol:2d}{iso:1d}{nu:12.6f}{S:10.3e}{A:10.3e}{fw(g_air, 5, 4)}{fw(g_self, 5, 3)}"
           f"{E:10.4f}{fw(n_air, 4, 2)}{fw(d_air, 8, 6)}")
    assert len(rec) == 67
    return rec + " " * 93


def test_from_hitran_par(tmp_path):
    recs = [hitran_record(5, 1, 2147.081134, 4.469e-19, 3.614e+01, 0.0579, 0.063, 3.8450, 0.75,
                          -.002677),
            hitran_record(5, 1, 2143.271080, 2.334e-19, 1.081e+01, 0.0756, 0.085, 0.0000, 0.76,
                          -.002000),
            hitran_record(5, 1, 2150.856008, 6.337e-19, 3.471e+01, 0.0552, 0.060, 11.5350, 0.74,
                          -.002840)]
    path = tmp_path / "05_hit.par"
    path.write_text("\n".join(recs) + "\n")
    ll = LineList.from_hitran_par(str(path), 28.0, PART)
    assert np.array_equal(ll.nu0, [2143.271080, 2147.081134, 2150.856008])
    assert np.array_equal(ll.S, [2.334e-19, 4.469e-19, 6.337e-19])
    assert np.array_equal(ll.E_low, [0.0, 3.8450, 11.5350])
    assert np.array_equal(ll.n_exp, [0.76, 0.75, 0.74])
    np.testing.assert_allclose(ll.gamma, np.array([0.0756, 0.0579, 0.0552]) / 1.01325, rtol=1e-15)
    assert ll.T_ref == 296.0 and ll.mass == 28.0
    path.write_text(recs[0][:100] + "\n")
    with pytest.raises(ValueError, match="record 1 has 100 characters"):
        LineList.from_hitran_par(str(path), 28.0, PART)


def test_create_lines_argument_errors_without_gpu():
    """Every argument error is found before any device call, and names the first index."""
    lib = N.lib()
    good = dict(nu0=np.array([1999.0, 2000.0, 2001.0, 2002.0]), S=np.full(4, 1e-20),
                E=np.full(4, 100.0), g=np.full(4, 0.05), n=np.full(4, 0.5), mass=28.0,
                T_ref=296.0, cutoff=25.0, q=np.array([1.0, 0.5]), T=np.array([296.0, 600.0]),
                p=np.array([1.0]), wl=np.array([4.99, 5.0, 5.01]))

    def call(**kw):
        a = {k: (np.array(v, dtype=np.float64) if isinstance(v, np.ndarray) else v)
             for k, v in {**good, **kw}.items()}
        h = ctypes.c_void_p()
        rc = lib.frei_xsec_create_lines(
            ctypes.byref(h), 0, a["nu0"].size, N.dptr(a["nu0"]), N.dptr(a["S"]), N.dptr(a["E"]),
            N.dptr(a["g"]), N.dptr(a["n"]), a["mass"], a["T_ref"], a["cutoff"], N.dptr(a["q"]),
            a["T"].size, a["p"].size, a["wl"].size, N.dptr(a["T"]), N.dptr(a["p"]),
            N.dptr(a["wl"]), None)
        assert rc != 0 and not h.value
        return lib.frei_last_error().decode()

    assert "nu0[2]" in call(nu0=np.array([1999.0, 2000.0, 1999.5, 2002.0]))
    assert "nondecreasing" in call(nu0=np.array([1999.0, 2000.0, 1999.5, 2002.0]))
    msg = call(E=np.array([100.0, np.nan, 100.0, 100.0]))
    assert "E_low[1]" in msg and "not finite" in msg
    assert "cutoff" in call(cutoff=0.0)
    assert "S_ref[3]" in call(S=np.array([1e-20, 0.0, 1e-20, -1e-20]))
    assert "gamma_ref[0]" in call(g=np.array([0.0, 0.05, 0.05, 0.05]))
    assert "nu0[0]" in call(nu0=np.array([0.0, 2000.0, 2001.0, 2002.0]))
    assert "mass_amu" in call(mass=0.0)
    assert "cutoff" in call(cutoff=float("inf"))
    assert "q_ratio[1]" in call(q=np.array([1.0, 0.0]))
    assert "T_nodes[0]" in call(T=np.array([-5.0, 600.0]))
    assert "p_nodes[0]" in call(p=np.array([0.0]))
    assert "wl_hi[2]" in call(wl=np.array([4.99, 5.0, 5.0]))
    assert "n_exp[2]" in call(n=np.array([0.5, 0.5, np.inf, 0.5]))
    h = ctypes.c_void_p()
    assert lib.frei_xsec_create_lines(ctypes.byref(h), 0, 4, None, None, None, None, None, 28.0,
                                      296.0, 25.0, None, 2, 1, 3, None, None, None, None) != 0
    assert "null" in lib.frei_last_error().decode()
    assert lib.frei_xsec_create_lines(
        ctypes.byref(h), 0, 0, N.dptr(good["nu0"]), N.dptr(good["S"]), N.dptr(good["E"]),
        N.dptr(good["g"]), N.dptr(good["n"]), 28.0, 296.0, 25.0, N.dptr(good["q"]), 2, 1, 3,
        N.dptr(good["T"]), N.dptr(good["p"]), N.dptr(good["wl"]), None) != 0
    assert "n_line" in lib.frei_last_error().decode()
    assert lib.frei_xsec_values(None, 0, 0, 0, 1, None) != 0
