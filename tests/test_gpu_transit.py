"""GPU tests of the transmission spectrum (frei_transit, K9): Engine.transit, BatchEngine.transit,
Grid.transmission_spectrum and BatchResult.transmission against tests/transit_ref.py, the plain
NumPy restatement of the definition (the reference has no counterpart).

Tolerance, derived rather than measured.  Every term of tau and of the area is non-negative, so
any evaluation lies within about n_layers x 2^-53 relative of the sum; -expm1(-tau) does not
amplify a relative error in tau; ocml and glibc expm1 / sqrt differ by a few ulp.  So the device
matches the restatement to rtol 1e-12, elementwise, on depth and on every tau_slant row.
Measured on MI355X (each test prints its maximum, pytest -s): 0 on depth and on tau_slant in
every case below, the device's sums being the restatement's operations in the restatement's
order and the two expm1 agreeing on these inputs; 2.3e-16 on the opaque limit's area."""
import functools

import numpy as np
import pytest

from tests import transit_ref as R

pytestmark = pytest.mark.gpu

M_BAR = 4.0142926168559996e-24
R_J, R_SUN = 7.1492e9, 6.957e10
RTOL = 1e-12


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _grid(fa, n_layers, n_lam):
    lam = np.logspace(np.log10(0.5), 1.0, n_lam)
    p = np.logspace(np.log10(200.0), -6, n_layers)
    tabs = {"1H2-16O": fa.OpacityTable(np.ones((n_layers, 2, n_lam)), p, [1000.0, 2000.0])}
    return lam, p, tabs


@functools.lru_cache(maxsize=None)
def _case(n_layers, n_lam, n_atm=1, seed=0):
    """Seeded inputs and the restatement's answer, computed once per shape: dtaus log-uniform in
    [1e-8, 1e3] (row 0 NaN: it is never read), radii from level_radii with a non-isothermal T
    and a different g per atmosphere."""
    import frei_amd as fa
    rng = np.random.default_rng(1000 * n_layers + n_lam + seed)
    p = np.logspace(np.log10(200.0), -6, n_layers)
    dt = 10 ** rng.uniform(-8, 3, (n_atm, n_layers, n_lam))
    dt[:, 0] = np.nan
    T = np.array([np.linspace(2500.0 - 300 * m, 900.0 + 100 * m, n_layers) +
                  80.0 * rng.standard_normal(n_layers) for m in range(n_atm)])
    g = np.array([900.0, 2478.6519476149147, 5200.0, 1700.0][:n_atm])
    radii = np.array([fa.level_radii(T[m], p, g[m], M_BAR, R_J) for m in range(n_atm)])
    ref = [R.transit(dt[m], radii[m], R_SUN) for m in range(n_atm)]
    for a in (dt, radii):
        a.setflags(write=False)
    return dt, radii, ref


def _err(x, ref):
    return float(np.max(np.abs(np.asarray(x) - ref) / np.abs(ref)))


# ------------------------------------------------------------------ 1: restatement parity
@pytest.mark.parametrize("n_layers,n_lam", [(4, 2), (7, 257), (30, 1000), (61, 513)])
def test_transit_matches_the_restatement(fa, n_layers, n_lam):
    """(4, 2): the minimum n_layers and the smallest launch a context admits, two lanes (the
    feature's specification names (4, 1), but no context holds fewer than two wavelengths: frei_ctx_create
    refuses n_lam = 1, which tests/test_abi.py pins and test_one_wavelength_context_is_refused
    below restates; a block with one active lane is the last block of (7, 257)); (7, 257): a
    partial last block of one lane, an odd shell count inside one level tile; (30, 1000): four
    blocks, the last partial, 29 shells = one whole level tile and a partial one; (61, 513):
    60 shells, three blocks, the last of one lane."""
    dt, radii, ref = _case(n_layers, n_lam)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    eng = fa.Engine(lam, p, tabs)
    try:
        depth, tau = eng.transit(radii[0], R_SUN, dtaus=dt[0], want_tau=True)
        plain = eng.transit(radii[0], R_SUN, dtaus=dt[0])
        again = eng.transit(radii[0], R_SUN, dtaus=dt[0])
    finally:
        eng.close()
    rd, rt = ref[0]
    assert depth.shape == (n_lam,) and tau.shape == (n_layers - 1, n_lam)
    e_d, e_t = _err(depth, rd), max(_err(tau[k], rt[k]) for k in range(n_layers - 1))
    print(f"({n_layers}, {n_lam}): depth {e_d:.3e}  tau_slant {e_t:.3e}")
    assert np.all(np.abs(depth - rd) <= RTOL * np.abs(rd)), e_d
    for k in range(n_layers - 1):
        assert np.all(np.abs(tau[k] - rt[k]) <= RTOL * np.abs(rt[k])), (k, e_t)
    assert np.array_equal(plain, depth), "depth differs with and without tau_slant"
    assert np.array_equal(again, depth), "depth differs between two calls"
    # the geometry: above the opaque base, below the top of the atmosphere
    r = radii[0]
    assert np.all(depth >= (r[0] / R_SUN) ** 2) and np.all(depth < (r[-1] / R_SUN) ** 2)


def test_one_wavelength_context_is_refused(fa):
    """Why the smallest parity case has two wavelengths."""
    lam, p, tabs = _grid(fa, 4, 2)
    with pytest.raises(RuntimeError, match="n_lam must be >= 2"):
        fa.Engine(lam, p, tabs, lam_slice=(0, 1))


# ------------------------------------------------------------------ 2: exact limits
def test_transit_limits(fa):
    n_layers, n_lam = 30, 257
    dt, radii, _ = _case(n_layers, n_lam)
    r = radii[0]
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    eng = fa.Engine(lam, p, tabs)
    try:
        clear, tau0 = eng.transit(r, R_SUN, dtaus=np.zeros((n_layers, n_lam)), want_tau=True)
        opaque = eng.transit(r, R_SUN, dtaus=np.full((n_layers, n_lam), 1e6))
        d1 = eng.transit(r, R_SUN, dtaus=dt[0])
        d10 = eng.transit(r, R_SUN, dtaus=dt[0] * 10.0)
    finally:
        eng.close()
    assert np.all(tau0 == 0.0)
    assert np.all(clear == r[0] * r[0] / (R_SUN * R_SUN)), "a transparent atmosphere"
    area = opaque * (R_SUN * R_SUN)            # the sum telescopes to r_{nL-1} r_nL
    e = _err(area, r[-2] * r[-1])
    print(f"opaque limit {e:.3e}")
    assert e <= 1e-13
    assert np.all(d10 >= d1), "more optical depth lowered the transit depth"


# ------------------------------------------------------------------ 3: batched against single
def test_batched_transit_is_bitwise_the_single_call(fa):
    n_layers, n_lam, n_atm = 30, 700, 3
    dt, radii, ref = _case(n_layers, n_lam, n_atm, seed=5)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    beng = fa.BatchEngine(lam, p, tabs, g=np.array([900.0, 2478.65, 5200.0]))
    try:
        bd, bt = beng.transit(radii, R_SUN, dtaus=dt, want_tau=True)
        ms = beng.post_timing()
    finally:
        beng.close()
    assert bd.shape == (n_atm, n_lam) and bt.shape == (n_atm, n_layers - 1, n_lam)
    assert ms > 0.0, "frei_post_timing does not cover the transit kernel"
    eng = fa.Engine(lam, p, tabs)
    try:
        for m in range(n_atm):
            d, t = eng.transit(radii[m], R_SUN, dtaus=dt[m], want_tau=True)
            assert np.array_equal(bd[m], d), f"atmosphere {m}: depth not bitwise"
            assert np.array_equal(bt[m], t), f"atmosphere {m}: tau_slant not bitwise"
            assert np.all(np.abs(d - ref[m][0]) <= RTOL * ref[m][0]), m
    finally:
        eng.close()
    assert not np.array_equal(bd[0], bd[1])


# ------------------------------------------------------------------ 4: kept dtaus
def _example_grids(fa, n):
    lam, _, _ = fa.wavelength_grid(0.5, 10, 500)
    grids, op = [], None
    for T_ref, g in [(2300, 2478.6519476149147), (1400, 1500.0), (2000, 4000.0)][:n]:
        pl = fa.Planet.from_hot_jupiter()
        pl.g = g
        gr = fa.Grid(pl, lam=lam, n_layers=30, T_ref=T_ref)
        if op is None:
            op = fa.load_example_opacity(gr)
        gr.load_opacities(opacities=op)
        grids.append(gr)
    return grids


def test_transmission_spectrum_from_the_kept_dtaus(fa):
    """The C1 example opacity at 30 x 500: after emission_spectrum the device copy of the dtaus
    gives bitwise what the returned host array gives, and both match the restatement."""
    gr, = _example_grids(fa, 1)
    pl = gr.planet
    try:
        with pytest.raises(RuntimeError, match="no device dtaus"):
            gr.transmission_spectrum(gr.init_temperatures)
        spec, T, _, dtaus = gr.emission_spectrum(n_timesteps=1)
        kept = gr.transmission_spectrum(T)
        given = gr.transmission_spectrum(T, dtaus=dtaus.copy())
        shifted = gr.transmission_spectrum(T, P_ref=1e-3)
        own = gr.transmission_spectrum(T, R_p=0.9 * R_J, R_star=0.8 * R_SUN)
    finally:
        gr._close_engine()
    assert isinstance(kept, fa.Spectrum) and kept.flux.shape == (500,)
    assert np.array_equal(kept.wavelength, gr.lam)
    assert np.array_equal(kept.flux, given.flux), "device dtaus and host dtaus differ"
    r = R.radii(T, gr.pressures, pl.g, pl.m_bar, R_J)
    ref, _ = R.transit(dtaus, r, R_SUN)
    e = _err(kept.flux, ref)
    print(f"grid transmission spectrum {e:.3e}; depth {kept.flux.min():.5f} .. "
          f"{kept.flux.max():.5f}")
    assert np.all(np.abs(kept.flux - ref) <= RTOL * ref), e
    ref, _ = R.transit(dtaus, R.radii(T, gr.pressures, pl.g, pl.m_bar, R_J, 1e-3), R_SUN)
    assert np.all(np.abs(shifted.flux - ref) <= RTOL * ref)
    assert np.all(shifted.flux < kept.flux), "R_p at 1 mbar puts level 1 deeper"
    ref, _ = R.transit(dtaus, R.radii(T, gr.pressures, pl.g, pl.m_bar, 0.9 * R_J), 0.8 * R_SUN)
    assert np.all(np.abs(own.flux - ref) <= RTOL * ref)


def test_batch_result_transmission_over_three_grids(fa):
    grids = _example_grids(fa, 3)
    with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
        depth = res.transmission()
        dts = [res.dtaus(m) for m in range(3)]
        radii = np.array([fa.level_radii(res[m].final_T, grids[m].pressures, grids[m].planet.g,
                                         grids[m].planet.m_bar, R_J) for m in range(3)])
        given = res.engine.transit(radii, R_SUN, dtaus=np.array(dts))
        scaled = res.transmission(R_star=[R_SUN, 2 * R_SUN, R_SUN])
    assert depth.shape == (3, 500)
    assert np.array_equal(depth, given), "device dtaus and host dtaus differ"
    for m, gr in enumerate(grids):
        r = R.radii(res[m].final_T, gr.pressures, gr.planet.g, gr.planet.m_bar, R_J)
        ref, _ = R.transit(dts[m], r, R_SUN)
        e = _err(depth[m], ref)
        print(f"grid {m}: batched transmission {e:.3e}")
        assert np.all(np.abs(depth[m] - ref) <= RTOL * ref), (m, e)
    assert np.array_equal(scaled[0], depth[0]) and np.array_equal(scaled[2], depth[2])
    assert np.all(np.abs(scaled[1] - depth[1] / 4) <= 4e-16 * depth[1])


# ------------------------------------------------------------------ 5: wavelength slice
def test_transit_on_a_wavelength_slice(fa):
    n_layers, n_lam = 30, 1000
    dt, radii, _ = _case(n_layers, n_lam)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    full = fa.Engine(lam, p, tabs)
    try:
        fd, ft = full.transit(radii[0], R_SUN, dtaus=dt[0], want_tau=True)
    finally:
        full.close()
    part = fa.Engine(lam, p, tabs, lam_slice=(100, 357))
    try:
        pd, pt = part.transit(radii[0], R_SUN, dtaus=dt[0][:, 100:357], want_tau=True)
    finally:
        part.close()
    assert pd.shape == (257,)
    assert np.array_equal(pd, fd[100:357]) and np.array_equal(pt, ft[:, 100:357])


# ------------------------------------------------------------------ 6: errors, not faults
def test_transit_errors(fa):
    n_layers, n_lam = 7, 257
    dt, radii, _ = _case(n_layers, n_lam)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    eng = fa.Engine(lam, p, tabs)
    try:
        with pytest.raises(RuntimeError, match="no device dtaus"):
            eng.transit(radii[0], R_SUN)
        bad = radii[0].copy()
        bad[3] = bad[2]
        with pytest.raises(RuntimeError, match="ascending"):
            eng.transit(bad, R_SUN, dtaus=dt[0])
        with pytest.raises(RuntimeError, match="ascending"):
            eng.transit(radii[0][::-1].copy(), R_SUN, dtaus=dt[0])
        for rs in (0.0, -R_SUN, np.nan):
            with pytest.raises(RuntimeError, match="r_star"):
                eng.transit(radii[0], rs, dtaus=dt[0])
        with pytest.raises(ValueError, match="radii"):
            eng.transit(radii[0][:-1], R_SUN, dtaus=dt[0])
        with pytest.raises(ValueError, match="dtaus"):
            eng.transit(radii[0], R_SUN, dtaus=dt[0][:, :-1])
        ok = eng.transit(radii[0], R_SUN, dtaus=dt[0])        # the context stays usable
        assert np.all(np.isfinite(ok))
    finally:
        eng.close()
    beng = fa.BatchEngine(lam, p, tabs, g=np.array([1000.0, 2000.0]))
    try:
        with pytest.raises(RuntimeError, match="no device dtaus"):
            beng.transit(np.array([radii[0], radii[0]]), R_SUN)
    finally:
        beng.close()


def test_nan_stays_in_its_column(fa):
    n_layers, n_lam = 7, 257
    dt, radii, ref = _case(n_layers, n_lam)
    d = dt[0].copy()
    d[3, 5], d[2, 200] = np.nan, np.inf
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    eng = fa.Engine(lam, p, tabs)
    try:
        depth = eng.transit(radii[0], R_SUN, dtaus=d)
    finally:
        eng.close()
    assert np.isnan(depth[5]) and np.isfinite(depth[200])
    keep = np.ones(n_lam, dtype=bool)
    keep[[5, 200]] = False
    assert np.all(np.abs(depth[keep] - ref[0][0][keep]) <= RTOL * ref[0][0][keep])
