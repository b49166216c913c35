"""GPU tests of the broadening (K13, frei_brd_apply): Broadening.apply, the resident chain into
CrossCorrelator.correlate and Instrument.apply, and BatchResult.cross_correlate / observe with
``broadening=``, against tests/broaden_ref.py, the plain restatement of the definition (the
reference has no counterpart).

Tolerance, derived rather than measured.  Device and restatement use the same weights bitwise
(the same IEEE operations, not contracted).  They differ in the order of the sum, in whether a
product is rounded before it is added, in the rounding of norm and in the final division, so for
every output
    |out - ref| <= (2 count_i + 8) 2^-53 sum_j |w_ij x_mj| / norm_i
(broaden_ref.apply returns it beside its values).  Two CPU orders of the same sum, ascending
fused multiply-adds against math.fsum, come to 0.10 of it (tests/test_broaden_host.py), so it is
neither vacuous nor tight.  Every parity case runs with every form of FORMS and with form 0;
each test prints its measured maximum of |out - ref| / bound (pytest -s).

Measured on MI355X (maximum |out - ref| / bound): smallest, exactly the restatement's numbers;
shape edges 0.267 in either form (the two forms returned the same bits in every case run here,
which the definition does not promise); resident spectra 0.158; the 8-point broadening of the last
test 0.065.  There the CCF at the injected velocity is 0.584 to 0.595 for the sharp template and
0.936 to 0.944 for the device-broadened one, the figures the restatements give on the CPU.
"""
import functools

import numpy as np
import pytest

from tests import broaden_ref as R
from tests import crosscorr_ref as CR

pytestmark = pytest.mark.gpu

FORMS_AND_AUTO = (1, 2, 0)


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _axis(n, seed, lo=1.0, hi=1.2, jitter=0.3):
    """Log-spaced lo to hi um with a seeded relative jitter of up to 0.3 of a step: the
    windows are asymmetric."""
    rng = np.random.default_rng(seed)
    ln = np.linspace(np.log(lo), np.log(hi), n)
    return np.exp(ln + (ln[1] - ln[0]) * rng.uniform(-jitter, jitter, n))


def _step_kms(n, lo=1.0, hi=1.2):
    return R.C_KMS * (np.log(hi) - np.log(lo)) / (n - 1)


def _table(half_width_kms, h=6):
    """A bell on a pedestal, 2 h + 1 samples (the pedestal keeps the end taps' weights from
    vanishing)."""
    from frei_amd.broaden import BroadeningKernel
    k = np.arange(-h, h + 1)
    return BroadeningKernel(half_width_kms / h, np.exp(-0.5 * (k / (0.5 * h)) ** 2) + 0.05)


@functools.lru_cache(maxsize=None)
def _case(n_lam, n_atm, half_steps):
    """Axis, kernel, spectra x = 10**uniform(3, 4) and the restatement's (out, bound); the table's
    half-width is `half_steps` mean steps of the axis."""
    from frei_amd.broaden import Broadening
    lam = _axis(n_lam, seed=n_lam)
    kern = _table(half_steps * _step_kms(n_lam))
    b = Broadening(lam, kern)
    x = 10 ** np.random.default_rng([n_lam, n_atm]).uniform(3, 4, (n_atm, n_lam))
    ref, bound = R.apply(x, b.u, b.tw, b.first, b.count, b.inv_dv, b.tab)
    for a in (lam, x, ref, bound):
        a.setflags(write=False)
    return dict(lam=lam, kern=kern, x=x, ref=ref, bound=bound, first=b.first.copy(),
                count=b.count.copy())


def _ratio(got, ref, bound):
    d = np.abs(np.asarray(got) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(d == 0.0, 0.0, d / bound)))


def _automatic(n_atm, count):
    """The form that form 0 takes."""
    from frei_amd.broaden import automatic_form
    return automatic_form(n_atm, count.mean())


# half-widths in steps and the interior counts they give on the jittered axis
HALF = {1: 0.35, 3: 1.3, 4: 1.75, 5: 2.3, 17: 8.3, 101: 50.3}


def _edge_cases():
    cases = [(n, 3, HALF[5]) for n in (15, 16, 17, 33, 257)]
    cases += [(33, a, HALF[5]) for a in (1, 3, 4, 5, 8, 9, 15, 16, 17, 33)]
    cases += [(257, 3, HALF[c]) for c in (1, 3, 4, 5, 17, 101)]
    # form 0's thresholds: 1 against 2 atmospheres on wide windows (91 points on average), 4
    # against 5 on middling ones (40), narrow ones (17)
    cases += [(257, 1, HALF[101]), (257, 2, HALF[101]), (257, 4, 22.3), (257, 5, 22.3),
              (257, 5, HALF[17]), (257, 17, HALF[17])]
    cases += [(40, 3, 60.0)]                      # every window is the whole axis
    out = []
    for c in cases:
        if c not in out:
            out.append(c)
    return out


# ------------------------------------------------------------------ 1: smallest
@pytest.mark.parametrize("form", FORMS_AND_AUTO)
def test_two_points_one_tap(fa, form):
    """Measured on MI355X: exactly the restatement's numbers, all forms."""
    lam = np.array([1.0, 1.0001])
    step = R.C_KMS * np.log(1.0001)
    kern = fa.BroadeningKernel(0.25 * step, [0.5, 1.0, 0.5])
    b = fa.Broadening(lam, kern)
    assert np.array_equal(b.count, [1, 1]) and np.array_equal(b.first, [0, 1])
    x = 10 ** np.random.default_rng(2).uniform(3, 4, 2)
    ref, bound = R.apply(x, b.u, b.tw, b.first, b.count, b.inv_dv, b.tab)
    try:
        out = b.apply(x, form=form)
        assert np.array_equal(b.device_norm(), b.norm)
    finally:
        b.release()
    w = b.tw * 1.0
    assert np.array_equal(ref[0], (w * x) / w)
    print(f"two points, form {form}: max |out - ref| / bound = {_ratio(out, ref[0], bound[0]):.3e}")
    assert out.shape == (2,) and np.all(np.abs(out - ref[0]) <= bound[0])
    assert b.form_used == (form or 1)


# ------------------------------------------------------------------ 2: shape edges
@pytest.mark.parametrize("form", FORMS_AND_AUTO)
@pytest.mark.parametrize("shape", _edge_cases(), ids=lambda s: "lam%d-atm%d-half%g" % s)
def test_shape_edges(fa, form, shape):
    """Measured on MI355X: max |out - ref| / bound 0.267 over all cases, VALU and MFMA form alike
    (0 where every window is one point; 0.045 at 101 points, 0.058 on the whole-axis windows)."""
    n_lam, n_atm, half = shape
    c = _case(*shape)
    mid = int(c["count"][n_lam // 2])
    want = {v: k for k, v in HALF.items()}.get(half)
    if want is not None and n_lam == 257:
        assert abs(mid - want) <= 1 and np.any(c["count"] == want)
        assert want != 1 or np.all(c["count"] == 1)
    if half == 60.0:
        assert np.all(c["count"] == n_lam)
    b = fa.Broadening(c["lam"], c["kern"])
    try:
        out = b.apply(c["x"], form=form)
        assert np.array_equal(b.device_norm(), b.norm), "norm: host operations, bitwise"
    finally:
        b.release()
    q = _ratio(out, c["ref"], c["bound"])
    print(f"{shape}, form {form} (ran {b.form_used}), interior count {mid}: "
          f"max |out - ref| / bound = {q:.3e}")
    assert b.form_used == (form or _automatic(n_atm, c["count"]))
    assert out.shape == (n_atm, n_lam)
    assert np.all(np.abs(out - c["ref"]) <= c["bound"]), q


# ------------------------------------------------------------------ 3: bitwise properties
@pytest.mark.parametrize("form", (1, 2))
def test_calls_and_rows_are_bitwise_reproducible(fa, form):
    shape = (257, 17, HALF[17])
    c = _case(*shape)
    b = fa.Broadening(c["lam"], c["kern"])
    try:
        a1 = b.apply(c["x"], form=form)
        a2 = b.apply(c["x"], form=form)
        rows = [b.apply(c["x"][m], form=form) for m in (0, 5, 16)]
        other = b.apply(c["x"], form=3 - form)
    finally:
        b.release()
    assert np.array_equal(a1, a2), "two identical calls differ"
    for m, row in zip((0, 5, 16), rows):
        assert row.shape == (257,)
        assert np.array_equal(row, a1[m]), f"row {m}: not bitwise the single-row call"
    q = _ratio(a1, other, c["bound"])
    print(f"form {form} against form {3 - form}: max |difference| / bound = {q:.3e}")
    assert np.all(np.abs(a1 - other) <= c["bound"]), q


def test_errors_leave_the_handle_usable(fa):
    """A refused call — by the library's argument checks or by its check of a resident source —
    leaves handle and device as they were: the next apply gives the first one's bits."""
    c = _case(257, 2, HALF[17])
    p = np.logspace(np.log10(200.0), -6, 5)
    b = fa.Broadening(c["lam"], c["kern"])
    try:
        good = b.apply(c["x"])
        with pytest.raises(RuntimeError, match="form"):
            b.apply(c["x"], form=max(fa.broaden.FORMS) + 1)
        assert np.array_equal(b.apply(c["x"]), good)
        lam = np.linspace(1.0, 2.0, 300)
        tabs = {"1H2-16O": fa.OpacityTable(np.ones((5, 2, 300)), p, [1000.0, 2000.0])}
        wide = fa.Engine(lam, p, tabs)
        try:
            with pytest.raises(RuntimeError, match="n_lam = 300 is not the broadener's 257"):
                b.apply(None, engine=wide)
        finally:
            wide.close()
        assert np.array_equal(b.apply(c["x"]), good)
        kept = b.apply(c["x"], keep=True)
        with pytest.raises(RuntimeError, match="form"):
            b.apply(c["x"], form=-1)
        with pytest.raises(RuntimeError, match="stale"):
            kept.handle()
        assert np.array_equal(b.apply(c["x"]), good)
    finally:
        b.release()


def test_constant_spectrum_comes_back_exactly_in_form_1(fa):
    """With x = 1 the numerator's fma(w, 1, acc) is norm's acc + w, term by term; a power of two
    scales every partial sum exactly.  (Any other constant rounds w x and norm differently and is
    within the bound, not exact.)"""
    c = _case(257, 3, HALF[17])
    b = fa.Broadening(c["lam"], c["kern"])
    try:
        for const in (1.0, 4096.0, 2.0 ** -20):
            out = b.apply(np.full((3, 257), const), form=1)
            assert np.all(out == const), const
    finally:
        b.release()


# ------------------------------------------------------------------ 4: NaN
@pytest.mark.parametrize("form", (1, 2))
def test_nan_reaches_the_outputs_that_cover_it(fa, form):
    shape = (257, 3, HALF[5])
    c = _case(*shape)
    j0 = 97            # covered by outputs of two tiles (80 .. 95 and 96 .. 111)
    bad = c["x"].copy()
    bad[1, j0] = np.nan
    b = fa.Broadening(c["lam"], c["kern"])
    try:
        clean = b.apply(c["x"], form=form)
        out = b.apply(bad, form=form)
    finally:
        b.release()
    covering = R.covers(c["first"], c["count"], j0)
    jlo, jhi = R.tile_spans(c["first"], c["count"])
    in_span = (jlo <= j0) & (j0 < jhi)
    assert covering.sum() == 5 and in_span.sum() == 32
    assert np.all(in_span[covering])
    nan = np.isnan(out)
    assert np.all(nan[1, covering]), "the covering outputs are NaN"
    if form == 1:
        assert np.array_equal(nan[1], covering), "exactly the covering outputs"
        assert np.array_equal(out[1, ~covering], clean[1, ~covering])
    else:
        assert not np.any(nan[1, ~in_span]), "NaN beyond the tiles whose span holds the point"
        assert np.array_equal(out[1, ~in_span], clean[1, ~in_span])
        assert np.all(nan[1, in_span]), "0 * NaN enters the product within such a tile"
    assert np.array_equal(out[[0, 2]], clean[[0, 2]]), "the other rows are bitwise unchanged"
    ref, _ = R.apply(bad, *_plan_args(c))
    assert np.array_equal(np.isnan(ref[1]), covering) and not np.isnan(ref[[0, 2]]).any()


def _plan_args(c):
    from frei_amd.broaden import Broadening
    b = Broadening(c["lam"], c["kern"])
    return b.u, b.tw, b.first, b.count, b.inv_dv, b.tab


# ------------------------------------------------------------------ 5: resident chain
def test_kept_result_feeds_correlator_and_instrument_bitwise(fa):
    from frei_amd.crosscorr import FORMS
    n = 257
    c = _case(n, 5, HALF[5])
    rng = np.random.default_rng(9)
    wl = rng.uniform(1.01, 1.19, 65)
    cc = fa.CrossCorrelator(c["lam"], wl, rng.normal(0.0, 1.0, (3, 65)),
                            np.linspace(-300.0, 300.0, 5), weights=rng.uniform(0.5, 1.5, 65))
    inst = fa.Instrument.gaussian(c["lam"], centres=np.linspace(1.02, 1.18, 9),
                                  resolving_power=300.0)
    den = 10 ** rng.uniform(5, 6, (2, n))
    kw = dict(den=den, select=np.arange(5, dtype=np.int32) % 2, scale=rng.uniform(0.5, 2.0, 5))
    b = fa.Broadening(c["lam"], c["kern"])
    other = fa.Broadening(_axis(100, seed=1), _table(HALF[5] * _step_kms(100)))
    try:
        host = b.apply(c["x"], form=2)
        for f in FORMS:
            tok = b.apply(c["x"], form=2, keep=True)
            assert isinstance(tok, fa.BroadenedSpectra) and tok.n_atm == 5
            res = cc.correlate(tok, form=f, offset=0.01, **kw)
            ref = cc.correlate(host, form=f, offset=0.01, **kw)
            assert res.sfg.shape == (5, 3, 5)
            for x, y in zip((res.sfg, res.sg, res.sgg), (ref.sfg, ref.sg, ref.sgg)):
                assert np.array_equal(x, y), f"correlator form {f}: kept against host copy"
            plain = cc.correlate(tok, form=f)              # no pre-pass: read where it lies
            for x, y in zip((plain.sfg, plain.sg), (cc.correlate(host, form=f).sfg,
                                                    cc.correlate(host, form=f).sg)):
                assert np.array_equal(x, y)
        tok = b.apply(c["x"], form=2, keep=True)
        for f in (1, 2):
            assert np.array_equal(inst.apply(tok, form=f, **kw), inst.apply(host, form=f, **kw))
        one = b.apply(c["x"][2], form=1, keep=True)
        assert np.array_equal(cc.correlate(one).sfg,
                              cc.correlate(b.apply(c["x"][2], form=1)).sfg)
        # stale: the next apply (kept or not) ends a token
        tok = b.apply(c["x"], keep=True)
        b.apply(c["x"][0])
        with pytest.raises(RuntimeError, match="stale"):
            cc.correlate(tok)
        with pytest.raises(RuntimeError, match="stale"):
            inst.apply(tok)
        # another axis: the library's message
        short = other.apply(np.ones((5, 100)), keep=True)
        with pytest.raises(RuntimeError, match="n_lam = 100 is not the correlator's 257"):
            cc.correlate(short)
        with pytest.raises(RuntimeError, match="n_lam = 100 is not the instrument's 257"):
            inst.apply(short)
        # nothing kept, and another atmosphere count: refused by the library
        from frei_amd import _native as N
        sg = np.empty((5, 5))
        b.apply(c["x"])
        args = (None, 0, None, None, None, 0, None, N.dptr(sg), None, None, None)
        with pytest.raises(RuntimeError, match="nothing kept"):
            N.check(N.lib().frei_ccf_apply_brd(cc.handle(), b.handle(), 5, *args))
        b.apply(c["x"][:3], keep=True)
        with pytest.raises(RuntimeError, match="keeps 3 atmospheres"):
            N.check(N.lib().frei_ccf_apply_brd(cc.handle(), b.handle(), 5, *args))
        assert b.timing()[1] >= 8 and b.timing()[0] > 0.0
    finally:
        b.release(), other.release(), cc.release(), inst.release()


# ------------------------------------------------------------------ 6: context source
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


def test_resident_spectra_are_broadened_in_place(fa):
    """Measured on MI355X: max |out - ref| / bound 0.158 on the three example atmospheres."""
    from frei_amd.observe import eclipse_scale, star_library
    grids = _example_grids(fa, 3)
    lam = np.asarray(grids[0].lam, dtype=float)
    rng = np.random.default_rng(6)
    wl = rng.uniform(1.0, 4.0, 300)
    cc = fa.CrossCorrelator(lam, wl, rng.normal(0.0, 1.0, (3, 300)),
                            np.linspace(-4000.0, 4000.0, 9), weights=rng.uniform(0.5, 1.5, 300))
    inst = fa.Instrument.gaussian(lam, centres=np.linspace(1.2, 4.5, 12), resolving_power=40.0)
    b = fa.Broadening(lam, fa.BroadeningKernel.gaussian(resolving_power=40.0))
    assert 8 <= b.count[250] <= 40
    p = np.logspace(np.log10(200.0), -6, 5)
    tabs = {"1H2-16O": fa.OpacityTable(np.ones((5, 2, 1000)), p, [1000.0, 2000.0])}
    lam_long = np.exp(np.linspace(np.log(1.0), np.log(1.2), 1000))
    try:
        with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
            spectra = np.array([r.spectrum.flux for r in res])
            for form in FORMS_AND_AUTO:
                resident = b.apply(engine=res.engine, form=form)
                assert np.array_equal(resident, b.apply(spectra, form=form)), form
            assert b.form_used == 1
            broad = b.apply(spectra)
            planets = res.planets
            lib, select = star_library(planets, lam)
            scale = eclipse_scale(planets, None, None)
            ecl = res.cross_correlate(cc, kind="eclipse", broadening=b)
            hand = cc.correlate(broad, den=lib, select=select, scale=scale)
            flux = res.cross_correlate(cc, kind="flux", broadening=b, offset=[1.0, 2.0, 3.0])
            flux_hand = cc.correlate(broad, offset=[1.0, 2.0, 3.0])
            depth = res.transmission()
            tr = res.cross_correlate(cc, kind="transit", broadening=b)
            tr_hand = cc.correlate(b.apply(-depth))
            obs = res.observe(inst, kind="eclipse", broadening=b)
            obs_hand = inst.apply(broad, den=lib, select=select, scale=scale)
            obs_tr = res.observe(inst, kind="transit", broadening=b)
            obs_tr_hand = inst.apply(b.apply(depth), num=lib, den=lib, select=select)
        spec, _, _, _ = grids[0].emission_spectrum(n_timesteps=1)
        single = grids[0].cross_correlate(cc, spec, kind="eclipse", broadening=b)
        single_hand = cc.correlate(b.apply(np.asarray(spec.flux, dtype=float)), den=lib[:1],
                                   scale=scale[:1])
        part = fa.Engine(lam_long, p, tabs, lam_slice=(100, 357))
        try:
            with pytest.raises(ValueError, match="slice"):
                b.apply(engine=part)
        finally:
            part.close()
        whole = fa.Engine(lam_long, p, tabs)
        try:
            with pytest.raises(RuntimeError, match="n_lam = 1000 is not the broadener's 500"):
                b.apply(engine=whole)
        finally:
            whole.close()
    finally:
        grids[0]._close_engine()
        cc.release(), inst.release(), b.release()
    ref, bound = R.apply(spectra, b.u, b.tw, b.first, b.count, b.inv_dv, b.tab)
    q = _ratio(broad, ref, bound)
    print(f"resident spectra: max |out - ref| / bound = {q:.3e}")
    assert np.all(np.abs(broad - ref) <= bound)
    for name, got, want in (("eclipse", ecl, hand), ("flux", flux, flux_hand),
                            ("transit", tr, tr_hand), ("single grid", single, single_hand)):
        for x, y in zip((got.sfg, got.sg, got.sgg), (want.sfg, want.sg, want.sgg)):
            assert np.array_equal(x, y), f"{name}: broadening= against the hand-made chain"
    assert np.array_equal(obs, obs_hand) and np.array_equal(obs_tr, obs_tr_hand)


# ------------------------------------------------------------------ 7: the point of the feature
N_POINT, V_INJECTED, NOISE = 2049, 60.0, 0.01


@functools.lru_cache(maxsize=None)
def _point_case():
    """2049 jittered points (1 to 1.2 um), 513 pixels, 3 exposures, 41 velocities (-400 to 400
    km/s in steps of 20).  The sharp template is a continuum with 90 lines about a point wide;
    the data are that template broadened by the restatement with a Gaussian of 8 points FWHM,
    sampled at +60 km/s, mean-subtracted, with seeded noise."""
    from frei_amd.broaden import Broadening, BroadeningKernel
    from frei_amd.crosscorr import doppler_plan
    lam = _axis(N_POINT, seed=7)
    rng = np.random.default_rng(70)
    u = R.C_KMS * np.log(lam)
    step = _step_kms(N_POINT)
    sharp = np.ones(N_POINT)
    for c0, d in zip(rng.uniform(u[20], u[-20], 90), rng.uniform(0.05, 0.5, 90)):
        sharp -= d * np.exp(-0.5 * ((u - c0) / (0.6 * step)) ** 2)
    kern = BroadeningKernel.gaussian(fwhm_kms=8.0 * step)
    b = Broadening(lam, kern)
    truth, bound = R.apply(sharp, b.u, b.tw, b.first, b.count, b.inv_dv, b.tab)
    wl = np.sort(rng.uniform(1.02, 1.18, 513))
    vel = np.arange(-400.0, 401.0, 20.0)
    idx, frac, n_clamped = doppler_plan(lam, wl, vel)
    assert not n_clamped.any() and vel.size == 41
    iv = int(np.nonzero(vel == V_INJECTED)[0][0])
    g = truth[0][idx[iv]] + frac[iv] * (truth[0][idx[iv] + 1] - truth[0][idx[iv]])
    flux = np.array([g - g.mean() + rng.normal(0.0, NOISE, 513) for _ in range(3)])
    for a in (lam, sharp, truth, wl, vel, flux):
        a.setflags(write=False)
    return dict(lam=lam, sharp=sharp, kern=kern, truth=truth[0], bound=bound[0], wl=wl, vel=vel,
                flux=flux, iv=iv, idx=idx, frac=frac)


def point_case_on_the_cpu():
    """(ccf, loglike) [2][3][41] of the sharp and the restatement-broadened template, from the
    restatements of both kernels alone: the check that seed and noise give the ordering with
    room to spare."""
    c = _point_case()
    w = np.ones(513)
    y = np.array([c["sharp"], c["truth"]])
    sfg, sg, sgg = CR.sums(y, c["idx"], c["frac"], c["flux"], w)
    W, S_wf, S_wff = CR.host_sums(c["flux"], w)
    return (CR.ccf(sfg, sg, sgg, W, S_wf, S_wff),
            CR.loglike(sfg, sg, sgg, W, S_wf, S_wff, 513))


@pytest.mark.parametrize("form", FORMS_AND_AUTO)
def test_broadened_template_recovers_the_injected_signal(fa, form):
    """On the CPU, with the restatements of both kernels (point_case_on_the_cpu), this seed and
    noise give: CCF at the injected velocity 0.584 to 0.595 for the sharp template, 0.936 to
    0.944 for the broadened one; the broadened template's log-likelihood peaks at the injected
    velocity in every exposure, 32.6 or more above the next velocity (the sharp template's peaks
    one velocity step off).  Measured on MI355X: the same CCF figures in every form; max
    |out - ref| / bound 0.065."""
    c = _point_case()
    cc = fa.CrossCorrelator(c["lam"], c["wl"], c["flux"], c["vel"])
    b = fa.Broadening(c["lam"], c["kern"])
    try:
        sharp = cc.correlate(c["sharp"])
        host = b.apply(c["sharp"], form=form)
        broad = cc.correlate(b.apply(c["sharp"], form=form, keep=True))
    finally:
        cc.release(), b.release()
    q = _ratio(host, c["truth"], c["bound"])
    iv = c["iv"]
    cs, cb = sharp.ccf()[:, iv], broad.ccf()[:, iv]
    ll = broad.loglike().sum(axis=0)
    print(f"8-point broadening, form {form}: max |out - ref| / bound = {q:.3e}; CCF at the "
          f"injected velocity, sharp {cs.min():.3f} .. {cs.max():.3f}, broadened "
          f"{cb.min():.3f} .. {cb.max():.3f}")
    assert np.all(np.abs(host - c["truth"]) <= c["bound"]), q
    assert np.all(cb > cs), "the broadened template correlates better, every exposure"
    assert int(np.argmax(ll)) == iv, "the log-likelihood peaks at the injected velocity"
    assert np.all(np.argmax(broad.loglike(), axis=1) == iv)
