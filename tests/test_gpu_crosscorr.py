"""GPU tests of the Doppler cross-correlation (K12, frei_ccf_apply): CrossCorrelator.correlate,
BatchResult.cross_correlate and Grid.cross_correlate against tests/crosscorr_ref.py, the plain
restatement of the definition (the reference has no counterpart).

Tolerance, derived rather than measured.  Device and restatement form the same g from the same
y, idx and frac (three IEEE operations, not contracted); they differ in the order of the sum and
in whether a product is rounded before it is added, and where den / scale / offset are present
in at most a few roundings of y.  For every output
    |S - S_ref| <= (n_pix + 32) 2^-53 sum_p |c_p| (|y_j| + |y_{j+1}|),
c_p = a[e][p] for S_fg, w[p] for S_g and w[p] (|y_j| + |y_{j+1}|) for S_gg
(crosscorr_ref.bounds).  The terms are signed, so the bound is absolute.  Every parity case
runs with every form of FORMS and with form 0; each test prints its measured maximum of
|S - S_ref| / bound (pytest -s).

Measured on MI355X (maximum |S - S_ref| / bound over S_fg, S_g, S_gg): smallest, exactly the
restatement's numbers; chunk, wave and tile edges 1.0e-2 (VALU form) / 1.3e-2 (MFMA form); injection and
recovery 1.0e-3 / 2.8e-3, with the bound at 1.07e-12 of max |S_fg|; resident eclipse templates
2.5e-3 (a grid on its own against the batch's row 0: the two spectra 5.8e-16 apart).
"""
import functools

import numpy as np
import pytest

from tests import crosscorr_ref as R

pytestmark = pytest.mark.gpu


def _forms():
    from frei_amd.crosscorr import FORMS
    return (*FORMS, 0)


def _chunk():
    from frei_amd.crosscorr import PIXEL_CHUNK
    return PIXEL_CHUNK


def pytest_generate_tests(metafunc):
    if "form" in metafunc.fixturenames:
        metafunc.parametrize("form", _forms())
    if "shape" in metafunc.fixturenames:
        metafunc.parametrize("shape", _edge_shapes(), ids=lambda s: "pix%d-exp%d-vel%d-atm%d" % s)


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _ratio(got, ref, bound):
    """max |S - S_ref| / bound over the three sums (0 / 0 counts as 0)."""
    worst = 0.0
    for g, r, b in zip(got, ref, bound):
        d = np.abs(np.asarray(g) - r)
        with np.errstate(invalid="ignore", divide="ignore"):
            q = np.where(d == 0.0, 0.0, d / b)
        worst = max(worst, float(np.max(q)))
    return worst


def _sums(res):
    return res.sfg, res.sg, res.sgg


# ------------------------------------------------------------------ cases
N_LAM = 257
BASE = dict(n_pix=65, n_exp=3, n_vel=3, n_atm=3)


def _edge_shapes():
    """One case per axis at its edges, the other axes at a small odd value."""
    C = _chunk()
    shapes = []
    for key, values in (("n_pix", (63, 64, 65, C - 1, C, C + 1, 2 * C + 1)),
                        ("n_exp", (1, 15, 16, 17)), ("n_vel", (1, 5, 65)), ("n_atm", (1, 3, 5))):
        for v in values:
            s = dict(BASE, **{key: v})
            s = (s["n_pix"], s["n_exp"], s["n_vel"], s["n_atm"])
            if s not in shapes:
                shapes.append(s)
    return shapes


@functools.lru_cache(maxsize=None)
def _case(n_pix, n_exp, n_vel, n_atm):
    """n_lam = 257 (log-spaced, 1 to 1.2 um); unsorted pixels, two clamped at each end; a
    2-row den library with select = [1, 0, 1, ...]; scale and offset per atmosphere."""
    rng = np.random.default_rng([n_pix, n_exp, n_vel, n_atm])
    lam = np.exp(np.linspace(np.log(1.0), np.log(1.2), N_LAM))
    wl = rng.uniform(1.01, 1.19, n_pix)
    if n_pix >= 8:
        wl[[1, 5]] = 0.99, 0.95
        wl[[2, n_pix - 1]] = 1.21, 1.25
    vel = np.array([30.0]) if n_vel == 1 else np.linspace(-300.0, 300.0, n_vel)
    flux = rng.normal(0.0, 1.0, (n_exp, n_pix))
    w = rng.uniform(0.5, 1.5, n_pix)
    x = 10 ** rng.uniform(3, 4, (n_atm, N_LAM))
    den = 10 ** rng.uniform(5, 6, (2, N_LAM))
    select = (np.arange(n_atm, dtype=np.int32) + 1) % 2
    scale = rng.uniform(0.5, 2.0, n_atm)
    offset = scale * 1e-2 * rng.uniform(0.5, 1.5, n_atm)
    for a in (lam, wl, vel, flux, w, x, den, select, scale, offset):
        a.setflags(write=False)
    return dict(lam=lam, wl=wl, vel=vel, flux=flux, w=w, x=x, den=den, select=select,
                scale=scale, offset=offset)


def _correlator(fa, c, exposures=slice(None), velocities=slice(None)):
    return fa.CrossCorrelator(c["lam"], c["wl"], c["flux"][exposures], c["vel"][velocities],
                              weights=c["w"])


def _kw(c):
    return dict(den=c["den"], select=c["select"], scale=c["scale"], offset=c["offset"])


@functools.lru_cache(maxsize=None)
def _reference(n_pix, n_exp, n_vel, n_atm):
    """(sums, bounds) of the restatement for _case, on the plan the correlator builds (the
    plan itself is held to the restatement bitwise in tests/test_crosscorr_host.py)."""
    from frei_amd.crosscorr import doppler_plan
    c = _case(n_pix, n_exp, n_vel, n_atm)
    idx, frac, _ = doppler_plan(c["lam"], c["wl"], c["vel"])
    y = R.template(c["x"], c["den"], c["select"], c["scale"], c["offset"])
    a = c["w"] * c["flux"]
    return R.sums(y, idx, frac, a, c["w"]), R.bounds(y, idx, a, c["w"])


# ------------------------------------------------------------------ 1: smallest
def test_one_pixel_one_velocity_one_exposure(fa, form):
    """Measured on MI355X: exactly the restatement's numbers (one term per sum)."""
    lam = np.array([1.0, 2.0])
    cc = fa.CrossCorrelator(lam, [1.25], [3.0], [0.0], weights=[0.75])
    try:
        assert cc.idx[0, 0] == 0 and cc.frac[0, 0] == 0.25
        res = cc.correlate(np.array([2.0, 10.0]), form=form)
        batched = cc.correlate(np.array([[2.0, 10.0]]), den=[4.0, 8.0], scale=[3.0],
                               offset=[0.125], form=form)
        used = cc.form_used
    finally:
        cc.release()
    assert used in fa.crosscorr.FORMS and (form == 0 or used == form)
    assert res.sfg.shape == (1, 1) and res.sg.shape == (1,) and res.sgg.shape == (1,)
    assert batched.sfg.shape == (1, 1, 1) and batched.sg.shape == (1, 1)
    ref = R.sums([[2.0, 10.0]], cc.idx, cc.frac, cc.a, cc.weights)
    assert (res.sfg[0, 0], res.sg[0], res.sgg[0]) == (ref[0][0, 0, 0], ref[1][0, 0], ref[2][0, 0])
    assert (res.sfg[0, 0], res.sg[0], res.sgg[0]) == (2.25 * 4.0, 0.75 * 4.0, 0.75 * 16.0)
    y = R.template([[2.0, 10.0]], [[4.0, 8.0]], None, [3.0], [0.125])
    ref = R.sums(y, cc.idx, cc.frac, cc.a, cc.weights)
    assert (batched.sfg[0, 0, 0], batched.sg[0, 0], batched.sgg[0, 0]) == \
        (ref[0][0, 0, 0], ref[1][0, 0], ref[2][0, 0])
    assert (cc.W, cc.S_wf[0], cc.S_wff[0]) == (0.75, 2.25, 6.75)


# ------------------------------------------------------------------ 2: chunk, wave and tile edges
def test_chunk_wave_and_tile_edges(fa, form, shape):
    """Measured on MI355X, maximum |S - S_ref| / bound over the cases: 1.0e-2 on the
    VALU form, 1.3e-2 on the MFMA form, 1.1e-2 with form 0 (the worst case is 65 pixels x 65
    velocities; at 8193 pixels 8.1e-5 / 2.4e-4)."""
    c = _case(*shape)
    ref, bound = _reference(*shape)
    cc = _correlator(fa, c)
    try:
        res = cc.correlate(c["x"], form=form, **_kw(c))
    finally:
        cc.release()
    n_pix, n_exp, n_vel, n_atm = shape
    assert res.sfg.shape == (n_atm, n_exp, n_vel) and res.sg.shape == (n_atm, n_vel)
    if n_pix >= 8:
        assert np.all(cc.n_clamped >= 4), "pixels are clamped at both ends"
    q = _ratio(_sums(res), ref, bound)
    print(f"edges {shape}, form {form}: max |S - S_ref| / bound = {q:.3e}")
    for g, r, b in zip(_sums(res), ref, bound):
        assert np.all(np.abs(g - r) <= b), q


# ------------------------------------------------------------------ 3: injection and recovery
@functools.lru_cache(maxsize=None)
def _injection():
    """Three templates of 120 Gaussian lines each on 4096 log-spaced points (1.0 to 1.1 um);
    700 sorted pixels in 1.02 to 1.08 um; 65 velocities, -64 to 64 km/s; 5 exposures of
    template 1 sampled at +14 km/s, mean-subtracted, with noise."""
    from frei_amd.crosscorr import doppler_plan
    lam = np.exp(np.linspace(np.log(1.0), np.log(1.1), 4096))
    x = []
    for m in range(3):
        rng = np.random.default_rng(100 + m)
        centres = rng.uniform(1.0, 1.1, 120)
        depths = rng.uniform(0.05, 0.6, 120)
        lines = np.zeros(lam.size)
        for c0, d in zip(centres, depths):
            lines += d * np.exp(-0.5 * ((lam - c0) / 2.5e-5) ** 2)
        x.append(1e-3 * (1 + 0.1 * m) * (1.0 - lines))
    x = np.array(x)
    rng = np.random.default_rng(11)
    wl = np.sort(rng.uniform(1.02, 1.08, 700))
    vel = np.arange(-64.0, 65.0, 2.0)
    w = rng.uniform(0.5, 1.5, 700)
    idx, frac, n_clamped = doppler_plan(lam, wl, vel)
    assert not n_clamped.any()
    iv = int(np.nonzero(vel == 14.0)[0][0])
    g = x[1][idx[iv]] + frac[iv] * (x[1][idx[iv] + 1] - x[1][idx[iv]])
    flux = np.array([g - g.mean() + rng.normal(0.0, 2e-6, 700) for _ in range(5)])
    a = w * flux
    ref, bound = R.sums(x, idx, frac, a, w), R.bounds(x, idx, a, w)
    for arr in (lam, x, wl, vel, w, flux):
        arr.setflags(write=False)
    return dict(lam=lam, x=x, wl=wl, vel=vel, w=w, flux=flux, iv=iv, ref=ref, bound=bound)


def test_injected_signal_is_recovered(fa, form):
    """Measured on MI355X: max |S - S_ref| / bound 1.0e-3 (VALU form) / 2.8e-3 (MFMA form); the
    bound is 1.07e-12 of max |S_fg|; the summed CCF at (1, +14 km/s) is 4.9989, the other templates'
    maxima 0.584 and 0.385 (the same figures as the restatement's sums give on the CPU)."""
    c = _injection()
    cc = fa.CrossCorrelator(c["lam"], c["wl"], c["flux"], c["vel"], weights=c["w"])
    try:
        res = cc.correlate(c["x"], form=form)
    finally:
        cc.release()
    q = _ratio(_sums(res), c["ref"], c["bound"])
    tight = float(np.max(c["bound"][0]) / np.max(np.abs(c["ref"][0])))
    print(f"injection, form {form}: max |S - S_ref| / bound = {q:.3e}; bound / max |S_fg| = "
          f"{tight:.3e}")
    for g, r, b in zip(_sums(res), c["ref"], c["bound"]):
        assert np.all(np.abs(g - r) <= b), q
    assert tight <= 1e-11, "the bound bites"
    ccf = res.ccf().sum(axis=1)              # [n_atm][n_vel], summed over the exposures
    ll = res.loglike().sum(axis=1)
    print(f"summed CCF at (1, +14 km/s) {ccf[1, c['iv']]:.4f}; the other templates' maxima "
          f"{ccf[0].max():.3f}, {ccf[2].max():.3f}")
    assert np.unravel_index(np.argmax(ccf), ccf.shape) == (1, c["iv"])
    assert np.unravel_index(np.argmax(ll), ll.shape) == (1, c["iv"])
    assert ccf[1, c["iv"]] > 4.9
    assert ccf[0].max() < 0.7 and ccf[2].max() < 0.7


# ------------------------------------------------------------------ 4: independence
def test_outputs_do_not_depend_on_their_neighbours(fa, form):
    C = _chunk()
    c = _case(C + 1, 5, 5, 3)
    kw = _kw(c)
    full, part_e, part_v = _correlator(fa, c), _correlator(fa, c, exposures=[1, 3]), \
        _correlator(fa, c, velocities=slice(None, None, 2))
    try:
        a = full.correlate(c["x"], form=form, **kw)
        b = full.correlate(c["x"], form=form, **kw)
        only = full.correlate(c["x"], form=form, want="sfg", **kw)
        stats = full.correlate(c["x"], form=form, want=("sg", "sgg"), **kw)
        e = part_e.correlate(c["x"], form=form, **kw)
        v = part_v.correlate(c["x"], form=form, **kw)
        rows = [full.correlate(c["x"][m], den=c["den"], select=c["select"][m:m + 1],
                               scale=c["scale"][m:m + 1], offset=c["offset"][m:m + 1], form=form)
                for m in range(3)]
    finally:
        full.release(), part_e.release(), part_v.release()
    for x, y in zip(_sums(a), _sums(b)):
        assert np.array_equal(x, y), "two identical calls differ"
    assert only.sg is None and only.sgg is None and stats.sfg is None
    assert np.array_equal(only.sfg, a.sfg), "sfg differs when it is the only sum asked for"
    assert np.array_equal(stats.sg, a.sg) and np.array_equal(stats.sgg, a.sgg)
    assert e.sfg.shape == (3, 2, 5) and np.array_equal(e.sfg, a.sfg[:, [1, 3]])
    assert np.array_equal(e.sg, a.sg) and np.array_equal(e.sgg, a.sgg)
    assert v.sfg.shape == (3, 5, 3) and np.array_equal(v.sfg, a.sfg[:, :, ::2])
    assert np.array_equal(v.sg, a.sg[:, ::2]) and np.array_equal(v.sgg, a.sgg[:, ::2])
    for m, row in enumerate(rows):
        assert row.sfg.shape == (5, 5)
        for x, y in zip(_sums(row), _sums(a)):
            assert np.array_equal(x, y[m]), f"atmosphere {m}: not bitwise the single-row call"


# ------------------------------------------------------------------ 5: NaN
def test_nan_stays_in_the_outputs_that_touch_it(fa, form):
    shape = (65, 3, 5, 3)
    c = _case(*shape)
    cc = _correlator(fa, c)
    # the first native point that some velocities touch and others do not
    j0 = next(j for j in range(1, N_LAM) if 0 < np.count_nonzero(
        np.any((cc.idx == j) | (cc.idx == j - 1), axis=1)) < 5)
    bad = c["x"].copy()
    bad[1, j0] = np.nan
    try:
        clean = cc.correlate(c["x"], form=form, **_kw(c))
        res = cc.correlate(bad, form=form, **_kw(c))
    finally:
        cc.release()
    touches = np.any((cc.idx == j0) | (cc.idx == j0 - 1), axis=1)       # [n_vel]
    assert touches.any() and not touches.all(), "the case must separate the velocities"
    hit = np.zeros((3, 5), dtype=bool)
    hit[1] = touches
    hit_fg = np.repeat(hit[:, None, :], 3, axis=1)
    assert np.array_equal(np.isnan(res.sfg), hit_fg), "NaN must reach exactly the touching sums"
    assert np.array_equal(np.isnan(res.sg), hit) and np.array_equal(np.isnan(res.sgg), hit)
    assert np.array_equal(res.sfg[~hit_fg], clean.sfg[~hit_fg])
    assert np.array_equal(res.sg[~hit], clean.sg[~hit])
    assert np.array_equal(res.sgg[~hit], clean.sgg[~hit])
    y = R.template(bad, c["den"], c["select"], c["scale"], c["offset"])
    ref = R.sums(y, cc.idx, cc.frac, cc.a, c["w"])
    assert np.array_equal(np.isnan(ref[0]), hit_fg)
    assert np.array_equal(np.isnan(ref[1]), hit) and np.array_equal(np.isnan(ref[2]), hit)


def test_zero_fraction_still_touches_a_nan(fa, form):
    """A pixel exactly on a native point (t = 0) multiplies its upper neighbour by 0: a NaN
    there still reaches the sum."""
    lam = np.array([1.0, 1.5, 2.0, 2.5])
    cc = fa.CrossCorrelator(lam, [1.5, 2.2], [[1.0, 2.0]], [0.0])
    try:
        assert (cc.idx[0, 0], cc.frac[0, 0]) == (1, 0.0)
        hi = cc.correlate(np.array([1.0, 2.0, np.nan, 4.0]), form=form)
        lo = cc.correlate(np.array([np.nan, 2.0, 3.0, 4.0]), form=form)
    finally:
        cc.release()
    assert np.isnan(hi.sfg).all() and np.isnan(hi.sg).all() and np.isnan(hi.sgg).all()
    assert np.isfinite(lo.sfg).all() and np.isfinite(lo.sg).all() and np.isfinite(lo.sgg).all()


# ------------------------------------------------------------------ 6: resident spectra
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


def test_batch_result_correlates_the_resident_spectra(fa):
    """Measured on MI355X: eclipse templates 2.5e-3 of the bound; the single grid's spectrum 5.8e-16
    from the batch's row 0."""
    grids = _example_grids(fa, 3)
    lam = np.asarray(grids[0].lam, dtype=float)
    rng = np.random.default_rng(6)
    wl = rng.uniform(1.0, 4.0, 300)
    vel = np.linspace(-4000.0, 4000.0, 9)
    flux = rng.normal(0.0, 1.0, (3, 300))
    w = rng.uniform(0.5, 1.5, 300)
    cc = fa.CrossCorrelator(lam, wl, flux, vel, weights=w)
    pl = grids[0].planet
    ratio2 = (pl.R_p / pl.R_star) * (pl.R_p / pl.R_star)
    star = np.pi * fa.B_star(pl.T_star, lam)
    try:
        with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
            spectra = np.array([r.spectrum.flux for r in res])
            resident = res.cross_correlate(cc, kind="flux")
            host = cc.correlate(spectra)
            ecl = res.cross_correlate(cc, kind="eclipse")
            depth = res.transmission()
            tr = res.cross_correlate(cc, kind="transit")
            tr_host = cc.correlate(-depth)
            shifted = res.cross_correlate(cc, kind="eclipse", offset=[1e-4, 2e-4, 3e-4])
        spec, T, _, _ = grids[0].emission_spectrum(n_timesteps=1)
        single = grids[0].cross_correlate(cc, spec, kind="eclipse")
    finally:
        grids[0]._close_engine()
        cc.release()
    assert resident.sfg.shape == (3, 3, 9)
    for x, y in zip(_sums(resident), _sums(host)):
        assert np.array_equal(x, y), "resident and uploaded spectra"
    for x, y in zip(_sums(tr), _sums(tr_host)):
        assert np.array_equal(x, y), "transit templates are minus the transit depth"
    y = R.template(spectra, [star], None, [ratio2] * 3)
    ref, bound = R.sums(y, cc.idx, cc.frac, cc.a, w), R.bounds(y, cc.idx, cc.a, w)
    q = _ratio(_sums(ecl), ref, bound)
    print(f"eclipse templates: max |S - S_ref| / bound = {q:.3e}")
    for g, r, b in zip(_sums(ecl), ref, bound):
        assert np.all(np.abs(g - r) <= b), q
    y = R.template(spectra, [star], None, [ratio2] * 3, [1e-4, 2e-4, 3e-4])
    ref_s, bound_s = R.sums(y, cc.idx, cc.frac, cc.a, w), R.bounds(y, cc.idx, cc.a, w)
    for g, r, b in zip(_sums(shifted), ref_s, bound_s):
        assert np.all(np.abs(g - r) <= b)
    # one grid on its own against the batch's row 0: the sums are linear (S_gg quadratic) in y,
    # so spectra dx apart (relative, elementwise) move a sum by at most dx (S_gg: 2 dx + dx^2)
    # times sum_p |c_p| (|y_j| + |y_{j+1}|) = bound / eps; each side is within the bound
    dx = float(np.max(np.abs(np.asarray(spec.flux) - spectra[0]) / np.abs(spectra[0])))
    eps = (300 + 32) * 2.0 ** -53
    print(f"single grid against the batch's row 0: spectra {dx:.3e} apart")
    assert single.sfg.shape == (3, 9) and single.sg.shape == (9,)
    for g, r, b in zip(_sums(single), _sums(ecl), bound):
        assert np.all(np.abs(g - r[0]) <= 2 * b[0] + (2 * dx + dx * dx) * b[0] / eps)


# ------------------------------------------------------------------ 7: errors, not faults
def test_errors_leave_the_handle_usable(fa):
    c = _case(65, 3, 5, 3)
    kw = _kw(c)
    p = np.logspace(np.log10(200.0), -6, 5)

    def engine(n_lam, **ekw):
        lam = np.exp(np.linspace(np.log(1.0), np.log(1.2), n_lam))
        tabs = {"1H2-16O": fa.OpacityTable(np.ones((5, 2, n_lam)), p, [1000.0, 2000.0])}
        return fa.Engine(lam, p, tabs, **ekw)
    cc = _correlator(fa, c)
    try:
        good = cc.correlate(c["x"], **kw)

        def still_good():
            again = cc.correlate(c["x"], **kw)
            for x, y in zip(_sums(again), _sums(good)):
                assert np.array_equal(x, y)
        for sel in ([1, 2, 0], [0, -1, 0]):
            with pytest.raises(RuntimeError, match="select"):
                cc.correlate(c["x"], **dict(kw, select=sel))
            still_good()
        with pytest.raises(ValueError, match="n_lam"):
            cc.correlate(c["x"][:, :-1])
        still_good()
        with pytest.raises(RuntimeError, match="all null"):
            cc.correlate(c["x"], want=(), **kw)
        still_good()
        with pytest.raises(RuntimeError, match="form"):
            cc.correlate(c["x"], form=max(fa.crosscorr.FORMS) + 1, **kw)
        still_good()
        wide = engine(300)
        try:
            with pytest.raises(RuntimeError, match="n_lam"):
                cc.correlate(None, engine=wide)
        finally:
            wide.close()
        still_good()
        part = engine(1000, lam_slice=(100, 357))
        try:
            with pytest.raises(ValueError, match="slice"):
                cc.correlate(None, engine=part)
        finally:
            part.close()
        still_good()
        # a context of the right shape: its emergent row, in place
        eng = engine(N_LAM)
        try:
            up = np.random.default_rng(8).uniform(1.0, 2.0, (5, N_LAM))
            eng.set_fluxes(up=up)
            resident = cc.correlate(None, engine=eng)
            assert resident.sfg.shape == (3, 5)
            for x, y in zip(_sums(resident), _sums(cc.correlate(up[-1]))):
                assert np.array_equal(x, y)
            with pytest.raises(RuntimeError, match="atmospheres"):
                from frei_amd import _native as N
                sg = np.empty((2, 5))
                N.check(N.lib().frei_ccf_apply(cc.handle(), eng._ctx, None, 2, None, 0, None,
                                               None, None, 0, None, N.dptr(sg), None, None,
                                               None))
        finally:
            eng.close()
        still_good()
        assert cc.timing()[1] >= 10 and cc.timing()[0] > 0.0
    finally:
        cc.release()
