"""GPU tests of the synthetic observations (K10, frei_obs_apply): Instrument.apply,
BatchResult.observe and Grid.observe against tests/observe_ref.py, the plain restatement of the
definition (the reference has no counterpart).

Tolerance, derived rather than measured.  The inputs make every term of N and D non-negative
(w >= 0; x, num, den > 0), so the device and the restatement each lie within (c + 4) 2^-53
relative of the exact sum of a channel of c points (c - 1 additions, two products, slack); the
ratio and the scale add two more roundings each side: |obs - ref| <= (4 c_max + 20) 2^-53 ref,
elementwise, c_max taken from the case (2.2e-12 at 5000 points).  chi^2 is held to the bound the
test forms from the restatement (observe_ref.chi2_bound), with data another atmosphere's
reference row and sigma = 1e-2 data, so the residuals are of order 1 to 100 and the bound bites.
Every parity case runs with form 1, 2 and 0; each test prints its measured maximum (pytest -s).

Measured on MI355X (maximum |obs - ref| / ref, lane form / group form; bound in brackets):
smallest 0 / 0; wave and block edges 0 / 1.1e-15 (1.2e-13); 1250 channels of 4 points 0 / 5.3e-16
(4.0e-15); one channel of 5000 points 0 / 3.9e-15 (2.2e-12); zero weights 0 / 4.4e-16 (2.9e-14):
the lane form is the restatement's operations in the restatement's order.  chi^2 of 2.8e5 to
1.1e6: off by at most 9.3e-10 (bound 9.0e-8 to 3.5e-7).  Resident spectra: eclipse depths 5.6e-16
(2.2e-13), transit depths 6.1e-16; a grid on its own against the batch's row 0 (the two spectra
5.8e-16 apart).
"""
import functools

import numpy as np
import pytest

from tests import observe_ref as R

pytestmark = pytest.mark.gpu

FORMS = (1, 2, 0)


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _err(x, ref):
    return float(np.max(np.abs(np.asarray(x) - ref) / np.abs(ref)))


def _close(x, ref, rtol):
    return np.all(np.abs(np.asarray(x) - ref) <= rtol * np.abs(ref))


def _spectra(rng, n_atm, n_lam):
    """Positive rows that differ by tens of per cent from one atmosphere to the next."""
    base = 10 ** rng.uniform(3, 5, n_lam)
    return np.array([base * (1 + 0.2 * m) * rng.uniform(0.9, 1.1, n_lam) for m in range(n_atm)])


@functools.lru_cache(maxsize=None)
def _edges_case():
    """Case 2: n_lam = 257; channels of 1, 2, 63, 64, 65 and 257 points plus one (80 points)
    overlapping two others, out of wavelength order; 3 atmospheres (a partial tile); libraries
    of 2 rows with select = [1, 0, 1]; a scale per atmosphere."""
    rng = np.random.default_rng(257)
    n_lam = 257
    first = np.array([200, 10, 100, 20, 150, 0, 60])
    count = np.array([1, 2, 63, 64, 65, 257, 80])
    w = rng.uniform(0.1, 1.0, int(count.sum()))
    x = _spectra(rng, 3, n_lam)
    num, den = rng.uniform(0.5, 2.0, (2, n_lam)), 10 ** rng.uniform(5, 7, (2, n_lam))
    select, scale = np.array([1, 0, 1], dtype=np.int32), np.array([0.5, 2.0, 1.25])
    ref = R.apply(first, count, w, x, num, den, select, scale)
    for a in (first, count, w, x, num, den, select, scale, ref):
        a.setflags(write=False)
    return dict(lam=np.linspace(1.0, 2.0, n_lam), first=first, count=count, w=w, x=x, num=num,
                den=den, select=select, scale=scale, ref=ref, rtol=R.rtol_for(257))


@functools.lru_cache(maxsize=None)
def _regimes_case():
    """Case 3: n_lam = 5000, 5 atmospheres (one full tile and a remainder of one); `fine` 1250
    channels of 4 points (num and den), `broad` a single channel of 5000 points (num only)."""
    rng = np.random.default_rng(5000)
    n_lam, n_atm = 5000, 5
    x = _spectra(rng, n_atm, n_lam)
    num, den = rng.uniform(0.5, 2.0, (1, n_lam)), 10 ** rng.uniform(5, 7, (1, n_lam))
    fine = dict(first=np.arange(0, n_lam, 4), count=np.full(1250, 4),
                w=rng.uniform(0.1, 1.0, n_lam))
    fine["ref"] = R.apply(fine["first"], fine["count"], fine["w"], x, num, den)
    broad = dict(first=np.array([0]), count=np.array([n_lam]), w=rng.uniform(0.1, 1.0, n_lam))
    broad["ref"] = R.apply(broad["first"], broad["count"], broad["w"], x, num)
    for a in (x, num, den, *fine.values(), *broad.values()):
        a.setflags(write=False)
    return dict(lam=np.linspace(1.0, 5.0, n_lam), x=x, num=num, den=den, fine=fine, broad=broad)


def _instrument(fa, lam, d):
    return fa.Instrument(lam, d["first"], d["count"], d["w"])


# ------------------------------------------------------------------ 1: smallest
@pytest.mark.parametrize("form", FORMS)
def test_one_point_one_channel_one_atmosphere(fa, form):
    inst = fa.Instrument([1.0], [0], [1], [0.25])
    try:
        obs = inst.apply(np.array([3.5]), form=form)
        scaled = inst.apply(np.array([[3.5]]), num=[2.0], den=[4.0], scale=[3.0], form=form)
    finally:
        inst.release()
    assert obs.shape == (1,) and scaled.shape == (1, 1)
    ref = R.apply([0], [1], [0.25], [3.5])
    ref2 = R.apply([0], [1], [0.25], [3.5], [[2.0]], [[4.0]], None, [3.0])
    print(f"smallest, form {form}: {_err(obs, ref[0]):.3e} {_err(scaled, ref2):.3e}")
    assert _close(obs, ref[0], R.rtol_for(1)) and _close(scaled, ref2, R.rtol_for(1))
    assert obs[0] == 3.5


# ------------------------------------------------------------------ 2: wave and block edges
@pytest.mark.parametrize("form", FORMS)
def test_wave_and_block_edges(fa, form):
    c = _edges_case()
    inst = _instrument(fa, c["lam"], c)
    try:
        obs = inst.apply(c["x"], num=c["num"], den=c["den"], select=c["select"],
                         scale=c["scale"], form=form)
        used = inst.form_used
    finally:
        inst.release()
    assert obs.shape == (3, 7)
    e = _err(obs, c["ref"])
    print(f"edges, form {form} (used {used}): {e:.3e} (bound {c['rtol']:.3e})")
    assert used == (form or 2)          # 76 points per channel on average
    assert _close(obs, c["ref"], c["rtol"]), e


# ------------------------------------------------------------------ 3: both regimes
@pytest.mark.parametrize("form", FORMS)
def test_both_regimes(fa, form):
    c = _regimes_case()
    fine, broad = _instrument(fa, c["lam"], c["fine"]), _instrument(fa, c["lam"], c["broad"])
    try:
        of = fine.apply(c["x"], num=c["num"], den=c["den"], form=form)
        ob = broad.apply(c["x"], num=c["num"], form=form)
        used = fine.form_used, broad.form_used
    finally:
        fine.release(), broad.release()
    assert of.shape == (5, 1250) and ob.shape == (5, 1)
    ef, eb = _err(of, c["fine"]["ref"]), _err(ob, c["broad"]["ref"])
    print(f"regimes, form {form} (used {used}): 1250 x 4 points {ef:.3e} (bound "
          f"{R.rtol_for(4):.3e}), 1 x 5000 points {eb:.3e} (bound {R.rtol_for(5000):.3e})")
    assert used == ((form, form) if form else (1, 2)), "form 0: lanes for 4 points, groups for 5000"
    assert _close(of, c["fine"]["ref"], R.rtol_for(4)), ef
    assert _close(ob, c["broad"]["ref"], R.rtol_for(5000)), eb


# ------------------------------------------------------------------ 4: zero weights, NaN
@pytest.mark.parametrize("form", FORMS)
def test_zero_weights_and_nan_stays_in_its_channels(fa, form):
    rng = np.random.default_rng(4)
    n_lam = 257
    first, count = np.array([0, 40, 120, 44]), np.array([50, 60, 10, 3])
    w = rng.uniform(0.1, 1.0, int(count.sum()))
    w[[3, 17, 45, 49]] = 0.0            # channel 0: zeros inside and at its end (index 45 too)
    w[50 + 20] = 0.0                    # channel 1, index 60
    x = _spectra(rng, 3, n_lam)
    ref = R.apply(first, count, w, x)
    bad = x.copy()
    bad[1, 45] = np.nan                 # covered by channels 0 (weight 0), 1 and 3 of atmosphere 1
    inst = fa.Instrument(np.linspace(1.0, 2.0, n_lam), first, count, w)
    try:
        clean = inst.apply(x, form=form)
        obs = inst.apply(bad, form=form)
    finally:
        inst.release()
    rtol = R.rtol_for(60)
    print(f"zero weights, form {form}: {_err(clean, ref):.3e} (bound {rtol:.3e})")
    assert _close(clean, ref, rtol)
    hit = np.zeros((3, 4), dtype=bool)
    hit[1, [0, 1, 3]] = True
    assert np.array_equal(np.isnan(obs), hit), "NaN must reach exactly the covering channels"
    assert np.array_equal(np.isnan(R.apply(first, count, w, bad)), hit)
    assert np.array_equal(obs[~hit], clean[~hit])


# ------------------------------------------------------------------ 5: reproducibility
@pytest.mark.parametrize("form", FORMS)
def test_results_are_bitwise_reproducible(fa, form):
    c = _edges_case()
    kw = dict(num=c["num"], den=c["den"], form=form)
    data, sigma = c["ref"][0], 1e-2 * c["ref"][0]
    inst = _instrument(fa, c["lam"], c)
    try:
        a = inst.apply(c["x"], select=c["select"], scale=c["scale"], **kw)
        b = inst.apply(c["x"], select=c["select"], scale=c["scale"], **kw)
        with_chi2, chi2 = inst.apply(c["x"], select=c["select"], scale=c["scale"], data=data,
                                     sigma=sigma, **kw)
        rows = [inst.apply(c["x"][m], select=c["select"][m:m + 1], scale=c["scale"][m:m + 1],
                           data=data, sigma=sigma, **kw) for m in range(3)]
    finally:
        inst.release()
    assert np.array_equal(a, b), "two identical calls differ"
    assert np.array_equal(a, with_chi2), "obs differs when chi2 is requested"
    for m, (row, row_chi2) in enumerate(rows):
        assert row.shape == (7,)
        assert np.array_equal(row, a[m]), f"atmosphere {m}: not bitwise the single-row call"
        assert row_chi2 == chi2[m], f"atmosphere {m}: chi2 not bitwise the single-row call"


# ------------------------------------------------------------------ 6: chi^2
def test_chi2_within_its_bound(fa):
    c = _regimes_case()
    d = c["fine"]
    ref, rtol, K = d["ref"], R.rtol_for(4), 1250
    data = ref[2].copy()
    sigma = 1e-2 * data
    ref_chi2 = R.chi2(ref, data, sigma)
    bound = R.chi2_bound(ref, data, sigma, rtol)
    dropped = 7
    s_inf = sigma.copy()
    s_inf[dropped] = np.inf
    keep = np.arange(K) != dropped
    without = dict(first=d["first"][keep], count=d["count"][keep],
                   w=d["w"][np.repeat(keep, 4)])
    ref_wo = R.chi2(ref[:, keep], data[keep], sigma[keep])
    bound_wo = R.chi2_bound(ref[:, keep], data[keep], sigma[keep], rtol)
    inst, inst_wo = _instrument(fa, c["lam"], d), _instrument(fa, c["lam"], without)
    kw = dict(num=c["num"], den=c["den"])
    try:
        obs, chi2 = inst.apply(c["x"], data=data, sigma=sigma, **kw)
        _, own = inst.apply(c["x"], data=obs[1].copy(), sigma=1e-2 * obs[1], **kw)
        _, chi2_inf = inst.apply(c["x"], data=data, sigma=s_inf, **kw)
        _, chi2_wo = inst_wo.apply(c["x"], data=data[keep], sigma=sigma[keep], **kw)
    finally:
        inst.release(), inst_wo.release()
    assert chi2.shape == (5,)
    print("chi2 reference", ref_chi2, "\n|chi2 - ref|", np.abs(chi2 - ref_chi2), "\nbound", bound)
    assert np.all(ref_chi2[[0, 1, 3, 4]] > K), "the residuals are of order 1 to 100"
    assert np.all(np.abs(chi2 - ref_chi2) <= bound)
    assert np.all(bound <= 1e-9 * np.maximum(ref_chi2, 1.0)), "the bound bites"
    assert own[1] == 0.0 and own[0] > 0.0
    # sigma = +inf removes exactly that channel's term
    assert np.all(np.abs(chi2_inf - ref_wo) <= bound_wo)
    assert np.all(np.abs(chi2_wo - ref_wo) <= bound_wo)
    assert np.all(np.abs(chi2_inf - chi2_wo) <= 2 * (K + 4) * 2.0 ** -52 * ref_wo)


# ------------------------------------------------------------------ 7: resident spectra
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


def test_batch_result_observes_the_resident_spectra(fa):
    grids = _example_grids(fa, 3)
    lam = grids[0].lam
    inst = fa.Instrument.top_hat(lam, [0.6, 1.1, 3.0, 4.0, lam[0]], [0.9, 1.7, 4.0, 5.0, lam[-1]])
    first, count, w = inst.first, inst.count, inst.weights
    rtol = R.rtol_for(int(count.max()))
    pl = grids[0].planet
    ratio2 = (pl.R_p / pl.R_star) * (pl.R_p / pl.R_star)
    star = np.pi * fa.B_star(pl.T_star, lam)
    other = star * np.linspace(0.5, 1.5, lam.size)
    try:
        with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
            spectra = np.array([r.spectrum.flux for r in res])
            flux = res.observe(inst, kind="flux")
            host = inst.apply(spectra)
            ecl, chi2 = res.observe(inst, kind="eclipse", data=np.full(5, 1e-3),
                                    sigma=np.full(5, 1e-4))
            res.planets[1].stellar_spectrum = other       # the flux state stays as it is
            routed = res.observe(inst, kind="eclipse")
            res.planets[1].stellar_spectrum = None
            depth = res.transmission()
            tr = res.observe(inst, kind="transit")
            tr_flat = res.observe(inst, kind="transit", depth=depth, weighting="flat")
        spec, T, _, _ = grids[0].emission_spectrum(n_timesteps=1)
        single = grids[0].observe(inst, spec, kind="eclipse")
        from_record = grids[0].observe(inst, fa.Spectrum(spectra[0], lam), kind="eclipse")
    finally:
        grids[0]._close_engine()
        inst.release()
    assert flux.shape == (3, 5) and np.array_equal(flux, host), "resident and uploaded spectra"
    ref = R.apply(first, count, w, spectra, None, [star], None, [ratio2] * 3)
    e = _err(ecl, ref)
    print(f"eclipse depths {ecl[0]}; {e:.3e} (bound {rtol:.3e})")
    assert _close(ecl, ref, rtol), e
    assert np.all(np.abs(chi2 - R.chi2(ref, np.full(5, 1e-3), np.full(5, 1e-4))) <=
                  R.chi2_bound(ref, np.full(5, 1e-3), np.full(5, 1e-4), rtol))
    ref = R.apply(first, count, w, spectra, None, [star, other], [0, 1, 0], [ratio2] * 3)
    assert _close(routed, ref, rtol)
    assert np.array_equal(routed[[0, 2]], ecl[[0, 2]]), "select moved the other atmospheres"
    assert not np.array_equal(routed[1], ecl[1])
    ref = R.apply(first, count, w, depth, [star], [star])
    e = _err(tr, ref)
    print(f"transit depths {tr[0]}; {e:.3e}")
    assert _close(tr, ref, rtol), e
    assert _close(tr_flat, R.apply(first, count, w, depth), rtol)
    # one grid on its own: its restatement, and the batch's row up to the two spectra's distance
    # (obs is a mean of x with non-negative weights: it moves no more than x does, relatively)
    ref = R.apply(first, count, w, spec.flux, None, [star], None, [ratio2])[0]
    assert single.shape == (5,) and _close(single, ref, rtol)
    dx = _err(spec.flux, spectra[0])
    print(f"single grid against the batch's row {_err(single, ecl[0]):.3e} (spectra {dx:.3e})")
    assert _close(single, ecl[0], 2 * rtol + dx)
    assert _close(from_record, ecl[0], 2 * rtol)


# ------------------------------------------------------------------ 8: errors, not faults
def test_errors_leave_the_handle_usable(fa):
    c = _edges_case()
    kw = dict(num=c["num"], den=c["den"], scale=c["scale"])
    data, sigma = c["ref"][0], 1e-2 * c["ref"][0]
    p = np.logspace(np.log10(200.0), -6, 5)

    def engine(n_lam, **ekw):
        lam = np.linspace(1.0, 2.0, n_lam)
        tabs = {"1H2-16O": fa.OpacityTable(np.ones((5, 2, n_lam)), p, [1000.0, 2000.0])}
        return fa.Engine(lam, p, tabs, **ekw)
    inst = _instrument(fa, c["lam"], c)
    try:
        good = inst.apply(c["x"], select=c["select"], **kw)

        def still_good():
            assert np.array_equal(inst.apply(c["x"], select=c["select"], **kw), good)
        for sel in ([1, 2, 0], [0, -1, 0]):
            with pytest.raises(RuntimeError, match="select"):
                inst.apply(c["x"], select=sel, **kw)
            still_good()
        for s in (0.0, -1.0, np.nan):
            bad = sigma.copy()
            bad[3] = s
            with pytest.raises(RuntimeError, match=r"sigma\[3\]"):
                inst.apply(c["x"], select=c["select"], data=data, sigma=bad, **kw)
            still_good()
        with pytest.raises(ValueError, match="n_lam"):
            inst.apply(c["x"][:, :-1])
        with pytest.raises(ValueError, match="data and sigma"):
            inst.apply(c["x"], data=data)
        still_good()
        wide = engine(300)
        try:
            with pytest.raises(RuntimeError, match="n_lam"):
                inst.apply(None, engine=wide)
        finally:
            wide.close()
        still_good()
        part = engine(1000, lam_slice=(100, 357))
        try:
            with pytest.raises(ValueError, match="slice"):
                inst.apply(None, engine=part)
        finally:
            part.close()
        still_good()
        # a context of the right shape: its emergent row, in place
        eng = engine(257)
        try:
            up = np.random.default_rng(8).uniform(1.0, 2.0, (5, 257))
            eng.set_fluxes(up=up)
            resident = inst.apply(None, engine=eng)
            assert resident.shape == (7,)
            assert np.array_equal(resident, inst.apply(up[-1]))
            with pytest.raises(RuntimeError, match="atmospheres"):
                from frei_amd import _native as N
                obs = np.empty((2, 7))
                N.check(N.lib().frei_obs_apply(inst.handle(), eng._ctx, None, 2, None, None, 0,
                                               None, None, None, None, 0, N.dptr(obs), None,
                                               None, None))
        finally:
            eng.close()
        still_good()
    finally:
        inst.release()
