"""Host-side tests of the phase curves (K16) that need no GPU: the geometry of
frei_amd.phasecurve, the create-time checks of frei_phs_create (it touches no device), the
staleness of a kept result, and the restatement tests/phase_ref.py itself, pinned against
closed forms and tests/emergent_ref.py."""
import ctypes

import numpy as np
import pytest

from frei_amd.phasecurve import PHASE_TILE, PhaseCurve, lonlat_cells
from tests import emergent_ref as R
from tests import phase_ref as P


# ------------------------------------------------------------------ geometry
def test_cells_tile_the_sphere():
    for n_lon, n_lat in ((8, 4), (16, 8), (5, 3), (1, 1)):
        lon, lat, area = lonlat_cells(n_lon, n_lat)
        assert lon.shape == lat.shape == area.shape == (n_lon * n_lat,)
        assert abs(area.sum() - 4 * np.pi) <= 8 * np.finfo(float).eps * 4 * np.pi
        assert np.all(area > 0) and np.all(np.abs(lon) < np.pi) and np.all(np.abs(lat) < np.pi / 2)
        # latitude-major: a band's cells are consecutive, south to north
        assert np.all(np.diff(lat.reshape(n_lat, n_lon), axis=1) == 0)
        assert np.all(np.diff(lat.reshape(n_lat, n_lon)[:, 0]) > 0)
        assert np.all(np.diff(lon.reshape(n_lat, n_lon), axis=1) > 0)


@pytest.mark.parametrize("n_lon,n_lat", [(8, 4), (16, 8), (32, 16), (64, 32)])
def test_projected_area_of_the_disk(n_lon, n_lat):
    """sum_c area max(mu, 0) is the disk's projected area pi; the equal-angle grid misses it by
    0.0725, 0.0184, 0.00467 and 0.00120 of pi at these four grids: <= 6 / n_lon^2."""
    lon, lat, area = lonlat_cells(n_lon, n_lat)
    phases = np.arange(37) / 37.0 + 0.0137
    pc = PhaseCurve(lon, lat, area, phases)
    total = np.sum(area[None, :] * np.maximum(pc.mu, 0.0), axis=1)
    err = float(np.max(np.abs(total - np.pi)) / np.pi)
    print(f"{n_lon} x {n_lat}: {err:.3e} of pi")
    assert err <= 6.0 / n_lon ** 2
    # coef is area * mu on the visible pairs
    vis = pc.mu > 0
    assert np.array_equal(pc.coef[vis], (area[None, :] * pc.mu)[vis])
    assert np.array_equal(pc.n_visible, vis.sum(axis=1))
    assert np.all(pc.mu <= 1.0)


def test_mid_eclipse_sees_the_day_side_and_mid_transit_the_night_side():
    lon, lat, area = lonlat_cells(16, 8)
    pc = PhaseCurve(lon, lat, area, [0.0, 0.5])
    day = np.abs(lon) < np.pi / 2
    assert np.array_equal(pc.mu[1] > 0, day)
    assert not np.any((pc.mu[0] > 0) & day)
    assert list(pc.n_visible) == [64, 64]
    assert np.array_equal(pc.select, np.arange(128)) and pc.select.dtype == np.int32
    # a pole-on orbit sees one hemisphere at every phase, each cell at mu = |sin lat|
    top = PhaseCurve(lon, lat, area, [0.1, 0.7], inclination=0.0)
    assert np.array_equal(top.mu[0] > 0, lat > 0) and np.array_equal(top.mu[1] > 0, lat > 0)
    assert np.allclose(top.mu[0], np.sin(lat), rtol=0, atol=1e-15)


def test_direct_geometry_passes_through():
    mu = np.array([[0.5, -0.25, 1.0], [0.0, 1e-6, -1.0]])
    coef = np.array([[0.25, np.nan, 2.0], [np.nan, 3.0, np.nan]])
    pc = PhaseCurve(mu=mu, coef=coef, select=[2, 0, 2])
    assert np.array_equal(pc.mu, mu) and np.array_equal(pc.coef, coef, equal_nan=True)
    assert (pc.n_phase, pc.n_cell) == (2, 3) and list(pc.n_visible) == [2, 1]
    assert list(pc.select) == [2, 0, 2] and pc._handle is None
    with pytest.raises(ValueError, match="together"):
        PhaseCurve(mu=mu)
    with pytest.raises(ValueError, match=r"\[n_phase\]\[n_cell\]"):
        PhaseCurve(mu=mu, coef=coef[:1])
    with pytest.raises(ValueError, match="select must have 3 entries"):
        PhaseCurve(mu=mu, coef=coef, select=[0, 1])
    with pytest.raises(ValueError, match="lon, lat, area and phases"):
        PhaseCurve([0.0], [0.0], [1.0])


# ------------------------------------------------------------------ create-time checks
_GOOD = dict(mu=[[0.5, -0.25], [1.0, 0.0]], coef=[[0.25, np.nan], [2.0, np.inf]], select=[0, 1])


@pytest.mark.parametrize("change,message", [
    (dict(select=[0, -1]), r"select\[1\] = -1 must be >= 0"),
    (dict(mu=[[0.5, -0.25], [np.nan, 0.0]]), r"mu\[1\]\[0\] must be finite and <= 1"),
    (dict(mu=[[0.5, -np.inf], [1.0, 0.0]]), r"mu\[0\]\[1\] must be finite and <= 1"),
    (dict(mu=[[0.5, -0.25], [1.0, 1.0000000000000002]]), r"mu\[1\]\[1\] must be finite and <= 1"),
    (dict(mu=[[5e-324, -0.25], [1.0, 0.0]]), r"1 / mu\[0\]\[0\] overflows"),
    (dict(coef=[[0.25, np.nan], [-1e-300, np.inf]]), r"coef\[1\]\[0\] must be finite and >= 0"),
    (dict(coef=[[np.inf, np.nan], [2.0, np.inf]]), r"coef\[0\]\[0\] must be finite and >= 0"),
    (dict(coef=[[np.nan, np.nan], [2.0, np.inf]]), r"coef\[0\]\[0\] must be finite and >= 0"),
])
def test_create_errors_come_before_any_handle(change, message):
    pc = PhaseCurve(**{**_GOOD, **change})
    with pytest.raises(RuntimeError, match=message):
        pc.handle()
    assert pc._handle is None


def test_create_touches_no_device_and_apply_validates_first():
    """A valid geometry exists without a GPU (the plan is uploaded by the first apply): the coef
    of an invisible pair may be anything, and the argument errors of frei_phs_apply that come
    before the context are reached here."""
    from frei_amd import _native as N
    lib = N.lib()

    def err():
        return lib.frei_last_error().decode()
    pc = PhaseCurve(**_GOOD)
    h = pc.handle()
    assert h.value and pc._handle is h
    i32p = ctypes.POINTER(ctypes.c_int32)
    sel = np.zeros(1, dtype=np.int32)
    one = np.ones(1)
    raw = ctypes.c_void_p()
    for n_cell, n_phase, msg in ((0, 1, "n_cell must be >= 1"), (1, 0, "n_phase must be >= 1")):
        assert lib.frei_phs_create(ctypes.byref(raw), 0, n_cell, n_phase, sel.ctypes.data_as(i32p),
                                   N.dptr(one), N.dptr(one)) != 0
        assert msg in err() and not raw.value
    assert lib.frei_phs_create(ctypes.byref(raw), 0, 1, 1, None, N.dptr(one), N.dptr(one)) != 0
    assert "null argument" in err()
    T, out = np.ones(4), np.empty((2, 2))
    assert lib.frei_phs_apply(None, None, None, N.dptr(T), N.dptr(out), 0, 0, None, None) != 0
    assert "null handle" in err()
    assert lib.frei_phs_apply(h, None, None, N.dptr(T), N.dptr(out), 0, 0, None, None) != 0
    assert "null context or null T" in err()
    # a launch-grid overflow is found before the context is looked at: 65535 tiles fit, one more
    # phase does not
    n_big = PHASE_TILE * 65535 + 1
    mu_big = np.full((n_big, 1), -1.0)
    mu_big[-1, 0] = 1.0
    big = PhaseCurve(mu=mu_big, coef=np.ones((n_big, 1)), select=[0])
    assert lib.frei_phs_apply(big.handle(), None, None, N.dptr(T), None, 1, 0, None, None) != 0
    assert "n_phase / 8 exceeds the launch grid (65535 tiles)" in err()
    big.release()
    fits = PhaseCurve(mu=mu_big[1:], coef=np.ones((n_big - 1, 1)), select=[0])
    assert lib.frei_phs_apply(fits.handle(), None, None, N.dptr(T), None, 1, 0, None, None) != 0
    assert "null context or null T" in err()
    fits.release()
    # the consumers' fifth source
    assert lib.frei_ccf_apply_phs(None, None, 2, None, 0, None, None, None, 0, None, None, None,
                                  None, None) != 0
    assert "null phase integrator" in err()
    assert lib.frei_obs_apply_phs(None, None, 2, None, None, 0, None, None, None, None, 0, None,
                                  None, None, None) != 0
    assert "null phase integrator" in err()
    assert lib.frei_brd_apply_phs(None, None, 2, 0, None, 0, None, None) != 0
    assert "null phase integrator" in err()
    pc.release()
    assert pc._handle is None and lib.frei_phs_destroy(None) == 0


# ------------------------------------------------------------------ staleness
def test_phase_spectra_go_stale(monkeypatch):
    """The token of integrate(keep=True) in pure Python: (owner, serial), stale at the owner's
    next integrate or release.  frei_phs_apply is stubbed: the rules are the Python layer's."""
    from frei_amd import _native as N
    from frei_amd._device import kept_suffix
    real = N.lib()

    class Lib:
        def __getattr__(self, name):
            return getattr(real, name)

        @staticmethod
        def frei_phs_apply(*a):
            return 0
    monkeypatch.setattr(N, "_lib", Lib())

    class Eng:
        n_atm, n_layers, n_lam, _ctx = 2, 3, 5, None
    pc = PhaseCurve(**_GOOD)
    T = np.full((2, 3), 1000.0)
    kept = pc.integrate(Eng, T, keep=True)
    assert kept_suffix(kept) == "_phs" and kept.suffix == "_phs"
    assert kept.n_atm == kept.n_phase == 2 and kept.n_lam == 5 and not kept.single
    assert kept.owner is pc and kept.handle() is pc._handle
    again = pc.integrate(Eng, T, keep=True)                # the next integrate
    with pytest.raises(RuntimeError, match="stale PhaseSpectra"):
        kept.handle()
    assert again.handle() is pc._handle
    assert pc.integrate(Eng, T).shape == (2, 5)            # kept or not
    with pytest.raises(RuntimeError, match="stale"):
        again.handle()
    kept = pc.integrate(Eng, T, keep=True)
    pc.release()                                           # the handle is gone
    with pytest.raises(RuntimeError, match="stale"):
        kept.handle()
    with pytest.raises(ValueError, match="T must hold 2 x 3 temperatures"):
        pc.integrate(Eng, T[:1])
    with pytest.raises(ValueError, match="dtaus must have shape"):
        pc.integrate(Eng, T, dtaus=np.ones((2, 3, 4)))
    # a model grid refuses it as nodes
    from frei_amd import ModelGrid
    with pytest.raises(TypeError, match="cannot be a model grid's nodes"):
        ModelGrid([np.array([1.0, 2.0])], np.linspace(1.0, 2.0, 5), spectra=kept)


# ------------------------------------------------------------------ the restatement itself
def _column(n_layers, n_lam, seed):
    rng = np.random.default_rng(seed)
    dt = 10 ** rng.uniform(-3, 1, (n_layers, n_lam))
    dt[0] = np.nan
    T = np.linspace(2200.0, 1000.0, n_layers) + 50.0 * rng.standard_normal(n_layers)
    T[0] = np.nan
    return dt, T


def test_restatement_isothermal_planet():
    """Every ray through an isothermal column leaves with B exactly to rounding (each step is a
    convex combination), so out[p] = B sum_c coef over the visible cells; a phase that sees
    nothing gives exactly 0 and an invisible pair's coef is never read."""
    n_layers, n_lam = 6, 7
    lam = np.logspace(0.0, 1.0, n_lam)
    dt, _ = _column(n_layers, n_lam, 1)
    T = np.full(n_layers, 1500.0)
    mu = np.array([[0.3, 1.0, -0.5, 1e-6], [-1.0, 0.0, -0.2, -1e-9], [0.9, -0.1, 0.2, 0.4]])
    coef = np.array([[0.5, 1.5, np.nan, 2.0], [np.nan, np.nan, np.inf, np.nan],
                     [0.25, np.nan, 0.0, 1.0]])
    out = P.phase_curve(np.array([dt, dt]), np.array([T, T]), lam, [0, 1, 1, 0], mu, coef)
    B = R.planck(lam, 1500.0)
    want = np.array([4.0, 0.0, 1.25])[:, None] * B[None, :]
    assert np.all(out[1] == 0.0)
    assert np.all(np.abs(out - want) <= 1e-13 * np.abs(want))
    assert np.array_equal(P.visible(mu).sum(axis=1), [3, 0, 3])


def test_restatement_reproduces_the_gauss_quadrature_flux():
    """Cells at gauss_angles(4) with coef = 2 pi w mu are emergent_ref's flux: the same terms in
    the same order, the 2 pi inside the coefficients instead of outside the sum."""
    from frei_amd import gauss_angles
    n_layers, n_lam = 9, 11
    lam = np.logspace(-0.3, 1.0, n_lam)
    dt, T = _column(n_layers, n_lam, 2)
    g_mu, g_w = gauss_angles(4)
    _, flux = R.emergent(dt, T, lam, g_mu, g_w)
    out = P.phase_curve(dt[None], T[None], lam, [0, 0, 0, 0], g_mu[None, :],
                        (2 * np.pi * g_w * g_mu)[None, :])
    assert out.shape == (1, n_lam)
    assert np.all(np.abs(out[0] - flux) <= 1e-14 * np.abs(flux))
    # and accumulate() is the same sum over supplied intensities
    inten, _ = R.emergent(dt, T, lam, g_mu)
    acc = P.accumulate(lambda m, x: inten[int(np.argmin(np.abs(g_mu - x)))], [0, 0, 0, 0],
                       g_mu[None, :], (2 * np.pi * g_w * g_mu)[None, :], n_lam)
    assert np.array_equal(acc, out)
