"""GPU tests of the phase curves (frei_phs_apply, K16): PhaseCurve.integrate,
BatchEngine.phase_curve and BatchResult.phase_curve against tests/phase_ref.py, the plain NumPy
restatement of the definition (the reference has no counterpart; tests/test_phasecurve_host.py
pins the restatement itself), and bit for bit against the intensities of the existing
frei_emergent.

Tolerance, derived rather than measured: rtol 1e-12 against the restatement, K11's bound (every
step of the recurrence is a convex combination of non-negative terms; the Planck exponent's few
ulp between ocml and glibc become about 1e-14); the sum over the cells adds at most n_cell ulp of
non-negative terms, far inside it.

Inputs are K11's recipe: dtaus log-uniform in [1e-8, 1e3] with row 0 NaN, noisy temperature ramps
with T[0] NaN, mu and coef passed directly.  Every plan holds, as far as its shape admits (the
minimum, one cell at one phase, is the single pair at mu = 1): a cell invisible at every phase, a
cell visible at some phases of its tile only, a phase that sees no cell (asserted == 0.0),
mu = 1 exactly, mu = 1e-6, cells sharing an atmosphere, and NaN as the coef of every invisible
pair (it is never read).

Measured maxima on MI355X (relative, against the restatement; pytest -s prints each):
(4, 2, 1, 1, 1) 2.0e-16, (7, 257, 3, 5, 9) 9.8e-16, (30, 1000, 4, 16, 8) 8.6e-16,
(61, 513, 2, 33, 17) 7.3e-16; isothermal 5.9e-16; Gauss-angle plan against the emergent flux
3.2e-16; three grids end to end 7.9e-16.  Every bitwise comparison held."""
import functools

import numpy as np
import pytest

from tests import emergent_ref as R
from tests import phase_ref as P
from tests.interp_ref import same_bits

pytestmark = pytest.mark.gpu

RTOL = 1e-12
SHAPES = [(4, 2, 1, 1, 1), (7, 257, 3, 5, 9), (30, 1000, 4, 16, 8), (61, 513, 2, 33, 17)]


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _lam(n_lam):
    return np.logspace(np.log10(0.5), 1.0, n_lam)


def _grid(fa, n_layers, lam):
    p = np.logspace(np.log10(200.0), -6, n_layers)
    tabs = {"1H2-16O": fa.OpacityTable(np.ones((n_layers, 2, lam.size)), p, [1000.0, 2000.0])}
    return p, tabs


def _batch(fa, n_layers, lam, n_atm):
    p, tabs = _grid(fa, n_layers, lam)
    return fa.BatchEngine(lam, p, tabs, g=np.linspace(900.0, 5200.0, n_atm))


def _columns(n_layers, n_lam, n_atm, seed=0):
    rng = np.random.default_rng(1000 * n_layers + n_lam + 7 * n_atm + seed)
    dt = 10 ** rng.uniform(-8, 3, (n_atm, n_layers, n_lam))
    dt[:, 0] = np.nan
    T = np.array([np.linspace(2500.0 - 300 * m, 900.0 + 100 * m, n_layers) +
                  80.0 * rng.standard_normal(n_layers) for m in range(n_atm)])
    T[:, 0] = np.nan
    return dt, T


def _plan(n_atm, n_cell, n_phase, seed=0):
    """(select, mu, coef): about half the pairs visible, with the special entries of the module
    docstring wherever the shape has room for them."""
    rng = np.random.default_rng(77 + 13 * n_cell + n_phase + seed)
    mu = rng.uniform(-1.0, 1.0, (n_phase, n_cell))
    mu[0, 0] = 1.0                                    # mu = 1 exactly
    if n_phase >= 3:                                  # cell 0: phases 0 and 2 of tile 0 only
        mu[1:, 0] = -np.abs(mu[1:, 0]) - 1e-3
        mu[2, 0] = 0.75
    if n_cell >= 3:
        mu[0, 1] = 1e-6                               # a grazing ray
        mu[:, n_cell - 1] = -0.3                      # a cell no phase sees
        mu[0, 2] = 0.0                                # mu = 0 is invisible
    if n_phase >= 2:
        mu[n_phase - 1, :] = -np.abs(mu[n_phase - 1, :]) - 1e-3    # a phase that sees nothing
    coef = np.where(mu > 0, rng.uniform(0.0, 2.0, mu.shape), np.nan)
    if n_cell >= 3:
        coef[0, 1] = 0.0                              # a zero weight still takes part
    select = ((np.arange(n_cell) * 7 + 1) % n_atm).astype(np.int32)
    return select, mu, coef


@functools.lru_cache(maxsize=None)
def _case(n_layers, n_lam, n_atm, n_cell, n_phase):
    """Seeded inputs and the restatement's answer, computed once per shape and left unchanged."""
    dt, T = _columns(n_layers, n_lam, n_atm)
    select, mu, coef = _plan(n_atm, n_cell, n_phase)
    ref = P.phase_curve(dt, T, _lam(n_lam), select, mu, coef)
    for a in (dt, T, select, mu, coef, ref):
        a.setflags(write=False)
    return dt, T, select, mu, coef, ref


def _err(x, ref):
    ok = ref != 0
    return float(np.max(np.abs(np.asarray(x)[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0


def _close(x, ref, rtol=RTOL):
    return bool(np.all(np.abs(np.asarray(x) - ref) <= rtol * np.abs(ref)))


# ------------------------------------------------------------------ 1: parity, bits of K11
@pytest.mark.parametrize("shape", SHAPES)
def test_phase_curve_matches_the_restatement_and_the_emergent_bits(fa, shape):
    """(4, 2, 1, 1, 1): the minimum; (7, 257, 3, 5, 9): a last block of one lane, a full tile of
    phases plus one; (30, 1000, 4, 16, 8): four blocks, one full tile; (61, 513, 2, 33, 17): two
    tiles plus one phase, 33 cells on 2 atmospheres."""
    n_layers, n_lam, n_atm, n_cell, n_phase = shape
    dt, T, select, mu, coef, ref = _case(*shape)
    lam = _lam(n_lam)
    pc = fa.PhaseCurve(mu=mu, coef=coef, select=select)
    eng = _batch(fa, n_layers, lam, n_atm)
    cache = {}

    def intensity_of(m, x):
        if (m, x) not in cache:
            cache[(m, x)] = eng.emergent(T, mu=[x], dtaus=dt)[m][0]
        return cache[(m, x)]
    try:
        out = pc.integrate(eng, T, dtaus=dt)
        again = eng.phase_curve(pc, T, dtaus=dt)
        hand = P.accumulate(intensity_of, select, mu, coef, n_lam)
    finally:
        eng.close()
        pc.release()
    assert out.shape == (n_phase, n_lam) and pc.form_used == 1
    err = _err(out, ref)
    print(f"{shape}: against the restatement {err:.3e}; {int(pc.n_visible.sum())} visible pairs, "
          f"{len(cache)} distinct rays")
    assert _close(out, ref), err
    assert np.all(np.isfinite(out))
    assert same_bits(out, again), "two calls differ"
    assert same_bits(out, hand), "not the bits of frei_emergent's intensities summed in order"
    for p in np.flatnonzero(pc.n_visible == 0):
        assert np.all(out[p] == 0.0) and not np.any(np.signbit(out[p]))
    if n_phase >= 2:
        assert pc.n_visible[-1] == 0 and np.any(pc.n_visible > 0)
    if n_cell >= 3:
        assert not np.any(mu[:, -1] > 0) and mu[0, 1] == 1e-6 and len(set(select)) < n_cell
    assert mu[0, 0] == 1.0


# ------------------------------------------------------------------ 2: bitwise invariances
def test_outputs_do_not_depend_on_the_rest_of_the_plan(fa):
    shape = (7, 257, 3, 5, 9)
    n_layers, n_lam, n_atm, n_cell, n_phase = shape
    dt, T, select, mu, coef, _ = _case(*shape)
    lam = _lam(n_lam)
    rng = np.random.default_rng(5)
    made = []

    def run(eng, mu, coef, select, T=T, dt=dt):
        pc = fa.PhaseCurve(mu=mu, coef=coef, select=select)
        made.append(pc)
        return pc.integrate(eng, T, dtaus=dt)
    eng = _batch(fa, n_layers, lam, n_atm)
    try:
        full = run(eng, mu, coef, select)
        # a phase alone
        for p in range(n_phase):
            assert same_bits(run(eng, mu[p:p + 1], coef[p:p + 1], select)[0], full[p]), p
        # phases permuted (they change tiles and tile positions)
        perm = rng.permutation(n_phase)
        assert same_bits(run(eng, mu[perm], coef[perm], select), full[perm])
        # phases added: eleven more in front and behind
        s2, mu2, coef2 = _plan(n_atm, n_cell, 11, seed=1)
        more = run(eng, np.vstack([mu2[:4], mu, mu2[4:]]), np.vstack([coef2[:4], coef, coef2[4:]]),
                   select)
        assert same_bits(more[4:4 + n_phase], full)
        # cells invisible at every phase added in front, in between and behind
        pos = [0, 0, 2, 5]
        mu_i = np.insert(mu, pos, -0.5, axis=1)
        coef_i = np.insert(coef, pos, np.nan, axis=1)
        sel_i = np.insert(select, pos, [2, 0, 1, 2])
        assert same_bits(run(eng, mu_i, coef_i, sel_i), full)
        # cells visible at other phases only: the rows of the phases that do not see them
        mu_v = np.insert(mu, [1], -0.5, axis=1)
        coef_v = np.insert(coef, [1], 0.5, axis=1)
        mu_v[3, 1] = 0.4
        sel_v = np.insert(select, [1], 2)
        got = run(eng, mu_v, coef_v, sel_v)
        keep = np.arange(n_phase) != 3
        assert same_bits(got[keep], full[keep]) and not same_bits(got[3], full[3])
    finally:
        eng.close()
    # two cells on one row against the same data in two rows
    shared = np.zeros(n_cell, dtype=np.int32)
    apart = np.arange(n_cell, dtype=np.int32)
    e1 = _batch(fa, n_layers, lam, 1)
    e5 = _batch(fa, n_layers, lam, n_cell)
    single = fa.Engine(lam, *_grid(fa, n_layers, lam))
    try:
        one = run(e1, mu, coef, shared, T=T[:1], dt=dt[:1])
        five = run(e5, mu, coef, apart, T=np.repeat(T[:1], n_cell, axis=0),
                   dt=np.repeat(dt[:1], n_cell, axis=0))
        assert same_bits(one, five)
        # a single Engine against the one-atmosphere batch
        assert same_bits(run(single, mu, coef, shared, T=T[0], dt=dt[0]), one)
    finally:
        for e in (e1, e5, single):
            e.close()
        for pc in made:
            pc.release()


# ------------------------------------------------------------------ 3: NaN containment
def test_nan_and_inf_reach_exactly_the_phases_that_see_their_atmosphere(fa):
    shape = (7, 257, 3, 5, 9)
    n_layers, n_lam, n_atm, n_cell, n_phase = shape
    dt, T, select, mu, coef, _ = _case(*shape)
    bad = dt.copy()
    bad[1, 3, 5], bad[2, 2, 200], bad[0, 6, 256] = np.nan, np.inf, np.nan
    lam = _lam(n_lam)
    pc = fa.PhaseCurve(mu=mu, coef=coef, select=select)
    eng = _batch(fa, n_layers, lam, n_atm)
    try:
        clean = pc.integrate(eng, T, dtaus=dt)
        out = pc.integrate(eng, T, dtaus=bad)
    finally:
        eng.close()
        pc.release()
    sees = np.array([[np.any((mu[p] > 0) & (select == m)) for m in range(n_atm)]
                     for p in range(n_phase)])
    want_nan = np.zeros((n_phase, n_lam), dtype=bool)
    want_nan[:, 5] = sees[:, 1]
    want_nan[:, 256] = sees[:, 0]
    assert sees[:, 1].any() and not sees[:, 1].all()
    assert np.array_equal(np.isnan(out), want_nan)
    # an infinite optical depth is a value (the shell is opaque): finite, in its column alone
    changed = ~same_bits_each(out, clean) & ~want_nan
    assert not np.any(changed[:, np.arange(n_lam) != 200])
    assert not np.any(changed[~sees[:, 2], 200])
    assert np.all(np.isfinite(out[:, 200][~want_nan[:, 200]]))


def same_bits_each(a, b):
    """Elementwise: the same bits, or both NaN."""
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


# ------------------------------------------------------------------ 4: closed forms
def test_isothermal_planet_and_the_gauss_angle_plan(fa):
    n_layers, n_lam, n_atm = 30, 257, 2
    dt, T = _columns(n_layers, n_lam, n_atm, seed=3)
    select, mu, coef = _plan(n_atm, 6, 5, seed=3)
    lam = _lam(n_lam)
    iso = np.full((n_atm, n_layers), 1500.0)
    g_mu, g_w = fa.gauss_angles(4)
    pc = fa.PhaseCurve(mu=mu, coef=coef, select=select)
    quad = fa.PhaseCurve(mu=np.vstack([g_mu, -g_mu]),
                         coef=np.vstack([2 * np.pi * g_w * g_mu, g_w]), select=[1, 1, 1, 1])
    eng = _batch(fa, n_layers, lam, n_atm)
    try:
        out = pc.integrate(eng, iso, dtaus=dt)
        flux = eng.emergent(T, dtaus=dt)[1]
        got = quad.integrate(eng, T, dtaus=dt)
    finally:
        eng.close()
        pc.release()
        quad.release()
    want = np.where(mu > 0, coef, 0.0).sum(axis=1)[:, None] * R.planck(lam, 1500.0)[None, :]
    e_iso, e_q = _err(out, want), _err(got[0], flux)
    print(f"isothermal against planck x sum coef {e_iso:.3e}; gauss-angle plan against the "
          f"emergent flux {e_q:.3e}")
    assert _close(out, want), e_iso
    assert _close(got[0], flux, 1e-13), e_q
    assert np.all(got[1] == 0.0)


# ------------------------------------------------------------------ 5: the kept path
def test_kept_phase_spectra_feed_the_consumers(fa):
    from frei_amd.broaden import BroadeningKernel
    n_layers, n_lam, n_atm, n_cell, n_phase = 7, 70, 3, 5, 9
    lam = np.exp(np.linspace(np.log(1.0), np.log(1.2), n_lam))
    dt, T = _columns(n_layers, n_lam, n_atm, seed=6)
    select, mu, coef = _plan(n_atm, n_cell, n_phase)
    rng = np.random.default_rng(4)
    pc = fa.PhaseCurve(mu=mu, coef=coef, select=select)
    n = lam.size
    delta = fa.Instrument(lam, np.arange(n), np.ones(n, dtype=np.int64), np.ones(n))
    inst = fa.Instrument.top_hat(lam, [1.0, 1.05, 1.1], [1.06, 1.1, 1.2])
    cc = fa.CrossCorrelator(lam, rng.uniform(1.02, 1.18, 40), rng.normal(0.0, 1.0, (3, 40)),
                            np.linspace(-3000.0, 3000.0, 9), weights=rng.uniform(0.5, 1.5, 40))
    b = fa.Broadening(lam, BroadeningKernel(400.0, [0.05, 0.3, 0.6, 0.9, 1.0, 0.9, 0.6, 0.3,
                                                    0.05]))
    scale = rng.uniform(0.5, 2.0, n_phase)
    offset = rng.uniform(-1.0, 1.0, n_phase)
    den = np.abs(rng.normal(1.0, 0.1, (2, n_lam))) + 0.5
    sel = rng.integers(0, 2, n_phase)
    data, sigma = rng.normal(0.0, 1.0, 3), np.array([0.1, 0.2, np.inf])
    eng = _batch(fa, n_layers, lam, n_atm)
    try:
        host = pc.integrate(eng, T, dtaus=dt)
        kept = pc.integrate(eng, T, dtaus=dt, keep=True)
        assert kept.n_phase == kept.n_atm == n_phase and kept.n_lam == n_lam
        assert same_bits(delta.apply(kept), host), "the kept rows are not the downloaded ones"
        # band light curves obs[p][k], per-phase select and scale, chi-square
        got = inst.apply(kept, den=den, select=sel, scale=scale, data=data, sigma=sigma)
        want = inst.apply(host, den=den, select=sel, scale=scale, data=data, sigma=sigma)
        assert got[0].shape == (n_phase, 3)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
        assert same_bits(inst.eclipse(kept, den[0], 7e9, 7e10), inst.eclipse(host, den[0], 7e9,
                                                                            7e10))
        # Broadening.apply, to the host and kept in turn, then the instrument
        broad = b.apply(kept)
        assert same_bits(broad, b.apply(host))
        assert same_bits(inst.apply(b.apply(kept, keep=True)), inst.apply(broad))
        # CrossCorrelator.correlate
        for f in (1, 2):
            res = cc.correlate(kept, den=den, select=sel, scale=scale, offset=offset, form=f)
            hand = cc.correlate(host, den=den, select=sel, scale=scale, offset=offset, form=f)
            for x, y in zip((res.sfg, res.sg, res.sgg), (hand.sfg, hand.sg, hand.sgg)):
                assert same_bits(x, y), f
        # a kept result of another phase count is refused by the library, naming both sides
        from frei_amd import _native as N
        obs = np.empty((4, 3))
        rc = N.lib().frei_obs_apply_phs(inst.handle(), kept.handle(), 4, None, None, 0, None,
                                        None, None, None, 0, N.dptr(obs), None, None, None)
        assert rc != 0 and b"keeps 9 phases, not n_atm = 4" in N.lib().frei_last_error()
        # staleness reaches the consumers; a call that keeps nothing leaves nothing
        pc.integrate(eng, T, dtaus=dt)
        with pytest.raises(RuntimeError, match="stale PhaseSpectra"):
            inst.apply(kept)
        rc = N.lib().frei_obs_apply_phs(inst.handle(), pc.handle(), n_phase, None, None, 0, None,
                                        None, None, None, 0, N.dptr(np.empty((n_phase, 3))), None,
                                        None, None)
        assert rc != 0 and b"holds nothing kept" in N.lib().frei_last_error()
    finally:
        eng.close()
        for o in (pc, delta, inst, cc, b):
            o.release()


# ------------------------------------------------------------------ 6: end to end
def test_batch_result_phase_curve_over_three_grids(fa):
    lam, _, _ = fa.wavelength_grid(0.5, 10, 500)
    grids, op = [], None
    for T_ref, g in [(2300, 2478.6519476149147), (1400, 1500.0), (2000, 4000.0)]:
        pl = fa.Planet.from_hot_jupiter()
        pl.g = g
        gr = fa.Grid(pl, lam=lam, n_layers=30, T_ref=T_ref)
        if op is None:
            op = fa.load_example_opacity(gr)
        gr.load_opacities(opacities=op)
        grids.append(gr)
    # three meridional bands: day side, terminators, night side
    lon, lat, area = fa.lonlat_cells(12, 4)
    band = np.where(np.abs(lon) < np.pi / 4, 0, np.where(np.abs(lon) < 3 * np.pi / 4, 1, 2))
    pc = fa.PhaseCurve(lon, lat, area, np.arange(10) / 10.0 + 0.03, inclination=85.0, select=band)
    try:
        with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
            out = res.phase_curve(pc)
            kept = res.phase_curve(pc, keep=True)
            inst = fa.Instrument.top_hat(lam, [1.0, 3.0], [2.0, 5.0])
            curves = inst.apply(kept)
            inst.release()
            dts = np.array([res.dtaus(m) for m in range(3)])
            Ts = np.array([res[m].final_T for m in range(3)], dtype=float)
            given = res.engine.phase_curve(pc, Ts, dtaus=dts)
    finally:
        pc.release()
    assert out.shape == (10, 500) and curves.shape == (10, 2)
    assert same_bits(out, given), "device dtaus and host dtaus differ"
    ref = P.phase_curve(dts, Ts, np.asarray(lam, dtype=float), band, pc.mu, pc.coef)
    err = _err(out, ref)
    print(f"three grids, 48 cells x 10 phases: against the restatement {err:.3e}")
    assert _close(out, ref), err
    assert np.all(out > 0)


# ------------------------------------------------------------------ 7: apply-time errors
def test_apply_errors_leave_the_handle_usable(fa):
    from frei_amd import _native as N
    shape = (7, 257, 3, 5, 9)
    n_layers, n_lam, n_atm, n_cell, n_phase = shape
    dt, T, select, mu, coef, ref = _case(*shape)
    lam = _lam(n_lam)
    lib = N.lib()
    pc = fa.PhaseCurve(mu=mu, coef=coef, select=select)
    wide = fa.PhaseCurve(mu=mu, coef=coef, select=np.where(select == 2, 3, select))
    eng = _batch(fa, n_layers, lam, n_atm)
    out = np.empty((n_phase, n_lam))

    def apply(h, ctx, d, t, o, keep=0, form=0):
        rc = lib.frei_phs_apply(h, ctx, N.dptr(d), N.dptr(t), N.dptr(o), keep, form, None, None)
        return rc, lib.frei_last_error().decode()
    try:
        h, ctx = pc.handle(), eng._ctx
        good = pc.integrate(eng, T, dtaus=dt)
        for args, msg in (
                ((None, ctx, dt, T, out), "null handle"),
                ((h, None, dt, T, out), "null context or null T"),
                ((h, ctx, dt, None, out), "null context or null T"),
                ((h, ctx, dt, T, None), "out is null and keep is not set"),
                ((h, ctx, dt, T, out, 0, 2), "form must be 0"),
                ((h, ctx, dt, T, out, 0, -1), "form must be 0"),
                ((h, ctx, None, T, out), "no device dtaus")):
            rc, err = apply(*args)
            assert rc != 0 and msg in err, (msg, err)
            assert same_bits(pc.integrate(eng, T, dtaus=dt), good), msg
        rc, err = apply(wide.handle(), ctx, dt, T, out)
        cell = int(np.flatnonzero(select == 2)[0])
        assert rc != 0 and f"select[{cell}] = 3 lies outside [0, n_atm = 3) (cell {cell})" in err
        # ... and the refused handle is good on a context that has the row
        dt4, T4 = _columns(n_layers, n_lam, 4, seed=9)
        eng4 = _batch(fa, n_layers, lam, 4)
        try:
            got4 = wide.integrate(eng4, T4, dtaus=dt4)
        finally:
            eng4.close()
        assert _close(got4, P.phase_curve(dt4, T4, lam, wide.select, mu, coef))
        # a launch-grid overflow: 65536 tiles of phases, one visible pair; refused before any
        # device work, with this context and dtaus, and the next call on them is good
        n_big = 8 * 65535 + 1
        mu_big = np.full((n_big, 1), -1.0)
        mu_big[-1, 0] = 1.0
        big = fa.PhaseCurve(mu=mu_big, coef=np.ones((n_big, 1)), select=[0])
        rc, err = apply(big.handle(), ctx, dt, T, None, keep=1)
        assert rc != 0 and "n_phase / 8 exceeds the launch grid (65535 tiles)" in err, err
        big.release()
        assert same_bits(pc.integrate(eng, T, dtaus=dt), good)
        # one phase fewer fits the grid: the limit is the stated one (nothing is launched here:
        # the context is refused for its missing dtaus, after the grid check)
        fits = fa.PhaseCurve(mu=mu_big[1:], coef=np.ones((n_big - 1, 1)), select=[0])
        rc, err = apply(fits.handle(), ctx, None, T, None, keep=1)
        assert rc != 0 and "no device dtaus" in err, err
        fits.release()
        # a temperature of an atmosphere some visible cell uses
        for v in (np.nan, 0.0, -5.0, np.inf):
            Tb = T.copy()
            Tb[1, 4] = v
            rc, err = apply(h, ctx, dt, Tb, out)
            assert rc != 0 and "T must be finite and positive (atmosphere 1, layer 4)" in err
        assert same_bits(pc.integrate(eng, T, dtaus=dt), good)
        # ... and of one no visible cell uses: not read
        lone = fa.PhaseCurve(mu=mu, coef=coef, select=np.zeros(n_cell, dtype=np.int32))
        Tb = T.copy()
        Tb[1:] = np.nan
        assert same_bits(lone.integrate(eng, Tb, dtaus=dt), lone.integrate(eng, T, dtaus=dt))
        lone.release()
        # a call whose arguments are refused leaves what was kept; an accepted one ends it
        kept = pc.integrate(eng, T, dtaus=dt, keep=True)
        rc, err = apply(h, ctx, None, T, out)
        assert rc != 0 and "no device dtaus" in err
        delta = fa.Instrument(lam, np.arange(n_lam), np.ones(n_lam, dtype=np.int64),
                              np.ones(n_lam))
        assert same_bits(delta.apply(kept), good)
        rc, err = apply(h, ctx, dt, T, out)
        assert rc == 0 and same_bits(out, good)
        with pytest.raises(RuntimeError, match="holds nothing kept"):
            delta.apply(kept)
        delta.release()
        assert same_bits(pc.integrate(eng, T, dtaus=dt), good) and _close(good, ref)
    finally:
        eng.close()
        pc.release()
        wide.release()
