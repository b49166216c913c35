"""Transmission spectra without a GPU: the level radii (pure NumPy), the new ABI symbol and the
exported names.  The device side is tests/test_gpu_transit.py."""
import ctypes
import inspect

import numpy as np
import pytest

from tests import transit_ref as R

K_B = 1.380649e-16
G_J, M_BAR, R_J, R_SUN = 2478.6519476149147, 4.0142926168559996e-24, 7.1492e9, 6.957e10


def _pressures(n_layers=30):
    return np.logspace(np.log10(200.0), -6, n_layers)


def test_level_radii_of_an_isothermal_atmosphere():
    """r_{l+1} - r_1 = H ln(p_1 / p_{l+1}), H = k_B T / (m_bar g).  Each of the l additions that
    form r_{l+1} rounds by at most half an ulp of r (2^-21 cm at 7e9 cm) and the height grows by
    1.4e7 cm per level here, so the difference is within 3.4e-14 relative."""
    import frei_amd as fa
    p = _pressures()
    T = np.full(p.size, 1500.0)
    r = fa.level_radii(T, p, G_J, M_BAR, R_J)
    assert r.shape == (p.size,) and r[0] == R_J and np.all(np.diff(r) > 0)
    H = K_B * 1500.0 / (M_BAR * G_J)
    p_lev = np.concatenate([p[1:], [p[-1] * p[-2] / p[-3]]])
    ref = H * np.log(p_lev[0] / p_lev[1:])
    got = r[1:] - r[0]
    err = np.max(np.abs(got - ref) / ref)
    print(f"isothermal radii: {err:.3e}")
    assert err <= 1e-13


def test_level_radii_match_the_restatement():
    import frei_amd as fa
    p = _pressures(17)
    T = np.linspace(2400.0, 900.0, 17) + 50.0 * np.sin(np.arange(17))
    for P_ref in (None, 0.01, p[5], p[1], p[-1] * p[-2] / p[-3]):
        r = fa.level_radii(T, p, 1234.5, M_BAR, R_J, P_ref=P_ref)
        ref = R.radii(T, p, 1234.5, M_BAR, R_J, P_ref)
        assert np.all(np.abs(r - ref) <= 1e-14 * ref), P_ref


def test_level_radii_reference_pressure_at_a_level():
    import frei_amd as fa
    p = _pressures()
    T = np.linspace(2300.0, 1000.0, p.size)
    for l in (1, 2, 11, p.size - 1):                # level l sits at p[l], its radius is r[l - 1]
        r = fa.level_radii(T, p, G_J, M_BAR, R_J, P_ref=p[l])
        assert abs(r[l - 1] - R_J) <= 1e-13 * R_J, l
        assert np.all(np.diff(r) > 0)
    # between two levels the reference radius lies inside that shell
    r = fa.level_radii(T, p, G_J, M_BAR, R_J, P_ref=np.sqrt(p[4] * p[5]))
    assert r[3] < R_J < r[4]


def test_level_radii_reference_pressure_out_of_range():
    import frei_amd as fa
    p = _pressures()
    T = np.full(p.size, 1200.0)
    top = p[-1] * p[-2] / p[-3]
    for bad in (p[0], p[1] * 1.0001, top * 0.9999, 0.0, np.nan):
        with pytest.raises(ValueError):
            fa.level_radii(T, p, G_J, M_BAR, R_J, P_ref=bad)


def test_new_symbol_and_names_are_exported():
    import frei_amd as fa
    from frei_amd import _native as N
    lib = N.lib()
    assert "frei_transit" in N.SIGNATURES and hasattr(lib, "frei_transit")
    assert lib.frei_version() == 20000
    assert "level_radii" in fa.__all__ and callable(fa.level_radii)
    for cls in (fa.Engine, fa.BatchEngine):
        sig = inspect.signature(cls.transit).parameters
        assert list(sig) == ["self", "radii", "R_star", "dtaus", "want_tau"]
        assert sig["dtaus"].default is None and sig["want_tau"].default is False
    sig = inspect.signature(fa.Grid.transmission_spectrum).parameters
    assert list(sig) == ["self", "final_temps", "dtaus", "R_p", "R_star", "P_ref"]
    sig = inspect.signature(fa.BatchResult.transmission).parameters
    assert list(sig) == ["self", "R_p", "R_star", "P_ref"]
    assert fa.BatchRecord._fields == ("spectrum", "final_T", "n_iter", "temp_hist", "T_eff",
                                      "T_milne", "T_planck")


def test_transit_rejects_a_null_context_without_a_device():
    from frei_amd import _native as N
    lib = N.lib()
    buf = np.ones(8)
    assert lib.frei_transit(None, None, N.dptr(buf), 1.0, N.dptr(buf), None) < 0
    assert lib.frei_last_error() != b""


def test_planet_carries_both_radii():
    import frei_amd as fa
    pl = fa.Planet.from_hot_jupiter()
    assert pl.R_p == R_J and pl.R_star == R_SUN
    # the values its g and a / R_star already imply: G M_J / R_J^2 and 0.03 AU / R_sun
    assert abs(1.2668653e23 / pl.R_p ** 2 - pl.g) <= 1e-7 * pl.g
    assert abs(0.03 * 1.495978707e13 / pl.R_star - pl.a_rstar) <= 1e-12 * pl.a_rstar
    bare = fa.Planet(a_rstar=5.0, m_bar=M_BAR, g=1000.0, T_star=5000.0, alpha=1)
    assert bare.R_p is None and bare.R_star is None
    own = fa.Planet(a_rstar=5.0, m_bar=M_BAR, g=1000.0, T_star=5000.0, alpha=1, R_p=6e9,
                    R_star=5e10)
    assert (own.R_p, own.R_star) == (6e9, 5e10)


def test_transmission_without_radii_is_a_value_error():
    """With neither a Planet value nor an argument: ValueError, before any device work."""
    import frei_amd as fa
    bare = fa.Planet(a_rstar=5.0, m_bar=M_BAR, g=1000.0, T_star=5000.0, alpha=1)
    gr = fa.Grid(bare, n_layers=8, n_wl_bins=16)
    with pytest.raises(ValueError, match="R_p"):
        gr.transmission_spectrum(gr.init_temperatures, dtaus=np.ones((8, 16)), R_star=R_SUN)
    with pytest.raises(ValueError, match="R_star"):
        gr.transmission_spectrum(gr.init_temperatures, dtaus=np.ones((8, 16)), R_p=R_J)


def test_restatement_limits():
    """The checker itself: transparent and opaque limits of the definition."""
    p = _pressures(9)
    r = R.radii(np.linspace(2000.0, 1000.0, 9), p, G_J, M_BAR, R_J)
    depth, tau = R.transit(np.zeros((9, 3)), r, R_SUN)
    assert np.all(depth == r[0] * r[0] / (R_SUN * R_SUN)) and np.all(tau == 0)
    depth, tau = R.transit(np.full((9, 3), 1e6), r, R_SUN)
    assert np.all(np.abs(depth * R_SUN ** 2 - r[-2] * r[-1]) <= 1e-13 * r[-2] * r[-1])
    assert tau.shape == (8, 3) and np.all(np.diff(r) > 0)
