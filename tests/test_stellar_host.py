"""Stellar-spectrum binning, the parts that need no GPU: the public names and the C ABI, the
argument checks of frei_sspec_* (made before any device call), the CPU restatement
(tests/stellar_ref.py) against the reference-made fixture, the expecto seam of
get_binned_phoenix_spectrum, and the F_star form of F_TOA."""
import ctypes
import sys
import types

import numpy as np
import pytest

from tests import stellar_ref as SR


def test_public_names_and_abi():
    import frei_amd as fa
    from frei_amd import _native as N
    for name in ("StellarSpectra", "binned_stellar_spectrum", "get_binned_phoenix_spectrum"):
        assert name in fa.__all__ and hasattr(fa, name)
    lib = N.lib()
    for sym in ("frei_sspec_create", "frei_sspec_bin", "frei_sspec_destroy"):
        assert sym in N.SIGNATURES and hasattr(lib, sym)
    assert lib.frei_version() == 20000


def test_sspec_argument_errors_without_gpu():
    """Every argument error comes before the first device call."""
    from frei_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p()
    wl = np.array([1.0, 2.0, 3.0, 4.0])
    flux = np.ones((2, 4))

    def create(f, n_spec, n_hi, w, out=True):
        return lib.frei_sspec_create(ctypes.byref(h) if out else None, 0, N.dptr(f), n_spec,
                                     n_hi, N.dptr(w))
    bad = np.array([1.0, 2.0, 2.0, 3.0])
    assert create(flux, 2, 4, bad) != 0
    assert b"ascending" in lib.frei_last_error()
    assert create(flux, 0, 4, wl) != 0
    assert b"n_spec" in lib.frei_last_error()
    assert create(flux, 2, 1, wl) != 0
    assert b"n_hi" in lib.frei_last_error()
    for args in ((None, 2, 4, wl), (flux, 2, 4, None)):
        assert create(*args) != 0
        assert b"null" in lib.frei_last_error()
    assert create(flux, 2, 4, wl, out=False) != 0
    assert b"null" in lib.frei_last_error()
    assert not h.value

    edges = np.array([0.5, 1.5, 2.5])
    i64p = ctypes.POINTER(ctypes.c_int64)

    def bin_(e, nb, form):
        return lib.frei_sspec_bin(None, N.dptr(e), nb, form, None, i64p(), None, None)
    assert bin_(np.array([0.5, 2.5, 1.5]), 2, 0) != 0
    assert b"wl_bins" in lib.frei_last_error() and b"ascending" in lib.frei_last_error()
    assert bin_(edges, 0, 0) != 0
    assert b"n_bins" in lib.frei_last_error()
    for form in (-1, 3):
        assert bin_(edges, 2, form) != 0
        assert b"form" in lib.frei_last_error()
    assert bin_(None, 2, 0) != 0
    assert b"null" in lib.frei_last_error()
    assert bin_(edges, 2, 1) != 0            # valid arguments, no library handle
    assert b"null" in lib.frei_last_error()
    assert lib.frei_sspec_destroy(None) == 0


def test_restatement_matches_the_reference_bitwise(golden):
    """tests/stellar_ref.py against the reference's own get_binned_phoenix_spectrum
    (golden/make_stellar_goldens.py): values, NaN pattern, shift and padding."""
    g = golden("stellar_bin.npz")
    wl, flux = g["wl"], g["flux"]
    for name in ("a", "b"):
        wl_bins, lam, ref = g[f"{name}_wl_bins"], g[f"{name}_lam"], g[f"{name}_out"]
        n = SR.counts(wl, wl_bins)
        aligned, _ = SR.bin_aligned(wl, flux, wl_bins)
        assert np.array_equal(np.isnan(aligned), np.broadcast_to(n < 2, aligned.shape))
        got = SR.compact_padded(aligned, n, lam.size)
        assert got.shape == ref.shape
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        assert np.array_equal(got, ref, equal_nan=True)
        assert np.array_equal(got[:, int((n > 0).sum()):], np.zeros((3, int((n == 0).sum()))))
    # the fixture holds what it says: "a" has every bin filled, "b" is shifted and has
    # single-point bins
    assert SR.counts(wl, g["a_wl_bins"]).min() >= 2
    nb = SR.counts(wl, g["b_wl_bins"])
    assert nb[0] == 0 and (nb == 1).any() and (nb >= 2).any()


def test_bin_membership_is_right_closed():
    wl = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    assert list(SR.counts(wl, [1.0, 3.0, 5.0])) == [2, 2]     # 1.0 dropped, 3.0 low bin, 5.0 kept
    assert list(SR.plan(wl, [0.0, 2.5, 9.0])) == [0, 2, 5]


class _Model:
    def __init__(self, wl, flux):
        self.wavelength, self.flux = wl, flux


def test_get_binned_phoenix_spectrum_expecto_seam(monkeypatch):
    """The model comes from spectrum= or from expecto.get_spectrum (a stub module here: no test
    imports the real package); both reach the same binning call.  Without expecto the error
    names spectrum=."""
    import frei_amd.stellar as S
    wl, flux = np.linspace(1.0, 2.0, 50), np.linspace(3.0, 4.0, 50)
    edges, lam = np.array([0.9, 1.5, 2.1]), np.array([1.2, 1.8])
    calls = []

    def fake_binned(wavelength, f, wl_bins, lam_, device=0):
        calls.append((wavelength, f, wl_bins, lam_))
        return "binned"
    monkeypatch.setattr(S, "binned_stellar_spectrum", fake_binned)
    assert S.get_binned_phoenix_spectrum(4000.0, 1e4, edges, lam,
                                         spectrum=_Model(wl, flux)) == "binned"
    assert calls[-1][0] is wl and calls[-1][1] is flux and calls[-1][2] is edges

    asked = []
    stub = types.ModuleType("expecto")

    def get_spectrum(T_eff, log_g=None, cache=True):
        asked.append((T_eff, log_g, cache))
        return _Model(wl, flux)
    stub.get_spectrum = get_spectrum
    monkeypatch.setitem(sys.modules, "expecto", stub)
    assert S.get_binned_phoenix_spectrum(4000.0, 1e4, edges, lam, cache=False) == "binned"
    assert asked == [(4000.0, 4.0, False)]
    assert calls[-1][0] is wl and calls[-1][1] is flux

    monkeypatch.setitem(sys.modules, "expecto", None)
    with pytest.raises(ImportError, match="spectrum="):
        S.get_binned_phoenix_spectrum(4000.0, 1e4, edges, lam)


def test_f_toa_with_the_blackbody_as_f_star_is_bitwise_f_toa():
    import frei_amd as fa
    lam, _, _ = fa.wavelength_grid(0.5, 10, 300)
    for T, a in ((5800.0, 6.450964670116429), (3200.0, 11.3)):
        blackbody = fa.F_TOA(lam, T_star=T, a_rstar=a)
        assert np.array_equal(fa.F_TOA(lam, T_star=T, a_rstar=a,
                                       F_star=np.pi * fa.B_star(T, lam)), blackbody)
    # and F_star really is what goes in
    F = np.linspace(1.0, 2.0, 300)
    assert np.array_equal(fa.F_TOA(lam, f=0.5, a_rstar=2.0, F_star=F),
                          0.5 * 2.0 ** -2 * 1 / (2 * np.pi) * F)


def test_non_finite_stellar_spectrum_is_refused():
    import frei_amd as fa
    lam, _, _ = fa.wavelength_grid(0.5, 10, 300)
    F = np.pi * fa.B_star(5800.0, lam)
    F[[7, 120]] = np.nan, np.inf
    msg = "stellar spectrum does not cover the grid: bins 7, 120 hold fewer than 2 points"
    with pytest.raises(ValueError, match=msg):
        fa.F_TOA(lam, F_star=F)
    with pytest.raises(ValueError, match=msg):
        fa.Planet(a_rstar=6.45, m_bar=4e-24, g=2478.0, T_star=5800.0, alpha=1,
                  stellar_spectrum=F)
    pl = fa.Planet.from_hot_jupiter()
    assert pl.stellar_spectrum is None
    pl.stellar_spectrum = F                  # set after construction: the grid refuses it
    gr = fa.Grid(pl, lam=lam, n_layers=8)
    gr.load_opacities(opacities={})
    with pytest.raises(ValueError, match=msg):
        gr.engine()
    with pytest.raises(ValueError, match="one value per grid wavelength"):
        fa.F_TOA(lam, F_star=np.ones(299))
