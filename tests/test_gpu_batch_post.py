"""GPU parity of batched post-processing (§8(f) #3 for batched contexts): a batched run returns
what the reference's per-Grid loop returns — temperature history and dtaus per atmosphere
(core.py:335-338) — and effective_temperature (core.py:386-439) and the contribution function
(plot.py:63-79) of every atmosphere come from one launch over (wavelength block, atmosphere).

Tolerances.  p_milne and cf are bitwise the single-atmosphere kernels' on the same inputs and
within 1e-12 relative of the oracle (ocml vs libm exp / expm1 / pow ulps: tests/test_gpu_post.py's
criterion).  The three wavelength sums have non-negative terms only, so any two summation
orders differ by at most about (tree depth + numpy's 128-element pairwise block) x 2^-53
relative — under 1e-13 at these sizes — and are held to 1e-12.  Quantities that went through
T-P iterations (history, dtaus) follow tests/test_gpu_batch.py's rule for final_T:
max(1e-10, 2 x the oracle's own one-ulp floor from perturbed_exp())."""
import numpy as np
import pytest

from oracle import frei_oracle as O
from tests.parity import perturbed_exp, rel

pytestmark = pytest.mark.gpu

M_BAR = 4.0142926168559996e-24
NAMES = ["1H2-16O", "12C-16O", "Na"]


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _setup(fa, n_atm, n_lam, n_layers, names, seed):
    """tests/test_gpu_batch.py::_setup (copied: test files do not import each other)."""
    rng = np.random.default_rng(seed)
    lam, _, _ = O.wavelength_grid(0.5, 10, n_lam)
    p = O.pressure_grid(n_layers, -6, np.log10(200))
    Tn = np.linspace(400.0, 4000.0, 12)
    tabs_o, tabs_f = {}, {}
    for n in names:
        base = 10 ** rng.uniform(-3, 1.5, lam.size)
        fp, fT = (p / 1.0) ** 0.1, (Tn / 1000.0) ** 0.5
        tabs_o[n] = O.Table(O.separable_table(base, fp, fT), p, Tn)
        tabs_f[n] = fa.SeparableTable(base, fp, fT, p, Tn)
    T_ref = rng.uniform(1100, 2500, n_atm)
    g = rng.uniform(800.0, 6000.0, n_atm)
    mh = rng.uniform(-0.5, 1.0, n_atm)
    mmr0 = O.mock_mmr(names, M_BAR)
    mmr = np.array([(mmr0 * 10 ** m)[:, None] * np.ones(n_layers) for m in mh])
    T0 = np.array([O.temperature_grid(p, t, 0.1, 0.1) for t in T_ref])
    return lam, p, tabs_o, tabs_f, g, mmr, T0


def _close(x, ref, tol=1e-12):
    return np.all(np.abs(np.asarray(x) - ref) <= tol * np.abs(ref))


def _assert_cf(cf, ref, what):
    ok = ref != 0
    assert _close(cf[ok], ref[ok]), f"{what}: cf {rel(cf[ok], ref[ok]):.3e}"
    assert np.all(np.abs(cf[~ok]) <= 1e-300), f"{what}: cf where the oracle is zero"


# ------------------------------------------------------------------ G1: the kernel, host-fed
@pytest.mark.parametrize("n_atm,n_layers,n_lam", [(3, 12, 700), (2, 4, 130)])
def test_post_kernel_on_host_fed_rows(fa, n_atm, n_layers, n_lam):
    """Random unsorted transmissions (numpy's guess / linear-probe / bisection search branches at
    12 layers, the len <= 4 linear branch at 4, exact hits of 2/3), random spectra and a
    different T for every atmosphere: 700 wavelengths are two full blocks and a partial one with
    a partial wave, 130 a single partial block."""
    rng = np.random.default_rng(3)
    lam, _, _ = O.wavelength_grid(0.5, 10, n_lam)
    p = np.logspace(2, -6, n_layers)
    dt = rng.uniform(0.0, 2.0, (n_atm, n_layers, n_lam))
    dt[:, 3 if n_layers > 4 else 1, ::97] = -np.log(2 / 3)   # transmission hits 2/3
    spectra = rng.uniform(1e10, 1e13, (n_atm, n_lam))
    T = rng.uniform(500.0, 3000.0, (n_atm, n_layers))
    tabs = {"1H2-16O": fa.OpacityTable(np.ones((n_layers, 2, n_lam)), p, [1000.0, 2000.0])}
    eng = fa.BatchEngine(lam, p, tabs, g=np.full(n_atm, 1000.0))
    try:
        out = eng.post(dt, spectra, T, want_p_milne=True, want_cf=True)
        again = eng.post(dt, spectra, T)
        no_cf = eng.post(dt, spectra, T, want_p_milne=True)
    finally:
        eng.close()
    single = fa.Engine(lam, p, tabs)
    try:
        pm1 = [single.milne_pressure(p, dt[m]) for m in range(n_atm)]
        cf1 = [single.contribution(p, T[m], dt[m]) for m in range(n_atm)]
    finally:
        single.close()
    assert np.array_equal(out["sums"], again["sums"]), "sums differ between two calls"
    assert np.array_equal(out["sums"], no_cf["sums"]), "sums differ with and without cf"
    assert np.array_equal(out["p_milne"], no_cf["p_milne"])
    assert set(again) == {"T_milne", "T_planck", "T_eff", "sums"}
    lam_cm = lam * 1e-4
    for m in range(n_atm):
        what = f"atmosphere {m}"
        assert np.array_equal(out["p_milne"][m], pm1[m]), f"{what}: p_milne not bitwise"
        ref_pm = O.milne_pressures(dt[m], p)
        assert _close(out["p_milne"][m], ref_pm), f"{what}: p_milne vs oracle"
        assert np.array_equal(out["cf"][m], cf1[m]), f"{what}: cf not bitwise"
        _assert_cf(out["cf"][m], O.contribution_function(lam, p, T[m], dt[m]), what)
        # the reductions, on the device's own p_milne (held to the oracle above) so that only
        # the summation order differs
        A, B, C = out["sums"][m]
        w = spectra[m] * lam_cm
        ref_pbar = np.average(out["p_milne"][m], weights=w)
        ref_C = np.sum(np.diff(lam_cm) * (spectra[m][1:] + spectra[m][:-1]) / 2.0)
        print(f"{what}: A/B {abs(A / B - ref_pbar) / ref_pbar:.3e}  C {abs(C - ref_C) / ref_C:.3e}")
        assert abs(A / B - ref_pbar) <= 1e-12 * ref_pbar, what
        assert abs(C - ref_C) <= 1e-12 * ref_C, what
        # and the host's scalar finish against the oracle's whole effective_temperature
        ref_te = O.effective_temperature(lam, p, spectra[m], dt[m], T[m])
        assert abs(out["T_planck"][m] - O.effective_temperature_planck(lam, spectra[m])) <= \
            1e-12 * out["T_planck"][m]
        print(f"{what}: T_eff {abs(out['T_eff'][m] - ref_te) / ref_te:.3e}")
        assert abs(out["T_eff"][m] - ref_te) <= 1e-12 * ref_te, what


# ------------------------------------------------------------------ G2: end to end
@pytest.fixture(scope="module")
def five(fa):
    """Five atmospheres, 40 iterations without early convergence, run once with history and
    kept dtaus; the oracle's runs (plain and one ulp off) beside it."""
    lam, p, tabs_o, tabs_f, g, mmr, T0 = _setup(fa, 5, 2048, 30, NAMES, 17)
    Ft = O.F_TOA(lam)
    eng = fa.BatchEngine(lam, p, tabs_f, g=g, mmr=mmr, F_toa=Ft)
    try:
        out = eng.run(T0, n_timesteps=40, n_zero_crossings=2, convergence_dT=3.0, alpha=1.0,
                      want_hist=True, keep_dtaus=True)
        dtaus = [eng.get_dtaus(m) for m in range(5)]
        post = eng.post(want_p_milne=True, want_cf=True)
    finally:
        eng.close()

    def oracle(m):
        return O.emission_spectrum(tabs_o, T0[m], p, lam, Ft, g[m], M_BAR, 1, n_timesteps=40,
                                   n_zero_crossings=2, convergence_dT=3.0, mmr=mmr[m])
    ref, pert = [], []
    for m in range(5):
        ref.append(oracle(m))
        with perturbed_exp():
            pert.append(oracle(m))
    return dict(lam=lam, p=p, out=out, dtaus=dtaus, post=post, ref=ref, pert=pert)


@pytest.mark.parametrize("m", range(5))
def test_batched_history_and_dtaus_match_oracle(five, m):
    out, (osp, oT, oth, odt, _, _, it), (_, pT, pth, _, _, _, _) = \
        five["out"], five["ref"][m], five["pert"][m]
    assert it == 40 and out["n_iter"][m] == 40
    th = out["temp_hist"][m]
    assert th.shape == (30, 80)
    h_floor, T_floor = rel(pth, oth), rel(pT, oT)
    e_h = rel(th, oth)
    print(f"atmosphere {m}: history {e_h:.3e} (floor {h_floor:.3e})")
    assert e_h <= max(1e-10, 2 * h_floor)
    dt = five["dtaus"][m]
    assert dt.shape == odt.shape and np.all(dt[0] == 1.0), "row 0 is the ones placeholder"
    e_d = rel(dt[1:], odt[1:])
    print(f"atmosphere {m}: dtaus {e_d:.3e} (T floor {T_floor:.3e})")
    assert e_d <= max(1e-10, 2 * T_floor)


@pytest.mark.parametrize("m", range(5))
def test_post_on_device_state_matches_oracle_on_returned_arrays(five, m):
    """post() with every input NULL (kept dtaus, F_up top rows, device T) against the oracle
    applied to the arrays the same run returned: self-consistent inputs, 1e-12, no floor."""
    lam, p, out, post = five["lam"], five["p"], five["out"], five["post"]
    dt, sp, T = five["dtaus"][m], out["spectra"][m], out["final_T"][m]
    assert _close(post["p_milne"][m], O.milne_pressures(dt, p)), "p_milne"
    _assert_cf(post["cf"][m], O.contribution_function(lam, p, T, dt), f"atmosphere {m}")
    ref = dict(T_eff=O.effective_temperature(lam, p, sp, dt, T),
               T_milne=O.effective_temperature_milne(lam, p, sp, dt, T),
               T_planck=O.effective_temperature_planck(lam, sp))
    for k, r in ref.items():
        e = abs(post[k][m] - r) / r
        print(f"atmosphere {m}: {k} {e:.3e}")
        assert e <= 1e-12, (k, e)


# ------------------------------------------------------------------ G3: grid level
def _three_grids(fa):
    lam, _, _ = O.wavelength_grid(0.5, 10, 1024)
    grids, op = [], None
    for T_ref, g, T_star, a_r in [(1400, 1500.0, 5800.0, 6.450964670116429),
                                  (2000, 2478.6519476149147, 4500.0, 5.0),
                                  (2400, 4000.0, 6500.0, 8.0)]:
        pl = fa.Planet.from_hot_jupiter()
        pl.g = g
        pl.T_star = T_star
        pl.a_rstar = a_r
        gr = fa.Grid(pl, lam=lam, n_layers=20, T_ref=T_ref)
        if op is None:
            op = fa.load_example_opacity(gr, scale_factor=2)
        gr.load_opacities(opacities=op)
        grids.append(gr)
    return lam, grids, op


def test_batched_emission_spectra_with_post_over_grids(fa):
    """The three grids of test_batched_emission_spectra_over_grids with post=True.
    convergence_dT = 20.0: with the package's own setup the oracle converges after 5, 2 and 1
    iterations (the same under perturbed_exp()); at 25.0 the counts were 4, 1, 1, not pairwise
    different, so the threshold was moved (18.0 gives 5, 3, 1; 15.0 gives 7, 4, 1)."""
    lam, grids, op = _three_grids(fa)
    dT = 20.0
    tabs_o = {"1H2-16O": O.Table(op["1H2-16O"].values, op["1H2-16O"].pressure,
                                 op["1H2-16O"].temperature)}
    keys = ("T_eff", "T_milne", "T_planck")

    def oracle(gr):
        pl = gr.planet
        Ft = O.F_TOA(lam, T_star=pl.T_star, a_rstar=pl.a_rstar)
        sp, T, th, dt, _, _, it = O.emission_spectrum(
            tabs_o, gr.init_temperatures, gr.pressures, lam, Ft, pl.g, pl.m_bar, pl.alpha,
            n_timesteps=30, convergence_dT=dT)
        return it, dict(T_eff=O.effective_temperature(lam, gr.pressures, sp, dt, T),
                        T_milne=O.effective_temperature_milne(lam, gr.pressures, sp, dt, T),
                        T_planck=O.effective_temperature_planck(lam, sp))
    its, refs, floors = [], [], []
    for gr in grids:
        it, te = oracle(gr)
        with perturbed_exp():
            pit, pte = oracle(gr)
        assert pit == it
        its.append(it)
        refs.append(te)
        floors.append({k: abs(pte[k] - te[k]) / te[k] for k in keys})
    assert len(set(its)) == 3, its
    with fa.batched_emission_spectra(grids, n_timesteps=30, convergence_dT=dT, post=True) as res:
        assert isinstance(res, fa.BatchResult) and len(res) == 3
        dts = [res.dtaus(m) for m in range(3)]
        cf1 = res.contribution(1)
    for m, (gr, rec) in enumerate(zip(grids, res)):
        assert isinstance(rec, fa.BatchRecord)
        assert rec.n_iter == its[m], (m, rec.n_iter, its)
        assert rec.temp_hist.shape == (20, 2 * rec.n_iter)
        # the oracle applied to the batched outputs
        own = dict(T_eff=O.effective_temperature(lam, gr.pressures, rec.spectrum.flux, dts[m],
                                                 rec.final_T),
                   T_milne=O.effective_temperature_milne(lam, gr.pressures, rec.spectrum.flux,
                                                         dts[m], rec.final_T),
                   T_planck=O.effective_temperature_planck(lam, rec.spectrum.flux))
        # each grid's own emission_spectrum + effective_temperature
        spec, T, th, dt = gr.emission_spectrum(n_timesteps=30, convergence_dT=dT)
        single = dict(T_eff=fa.effective_temperature(gr, spec, dt, T),
                      T_milne=fa.effective_temperature_milne(gr, spec, dt, T),
                      T_planck=fa.effective_temperature_planck(gr, spec))
        gr._close_engine()
        assert th.shape == rec.temp_hist.shape
        for k in keys:
            v = getattr(rec, k)
            e_own, e_single = abs(v - own[k]) / own[k], abs(v - single[k]) / single[k]
            print(f"grid {m}: {k} vs oracle on own outputs {e_own:.3e}, vs single grid "
                  f"{e_single:.3e} (floor {floors[m][k]:.3e})")
            assert e_own <= 1e-12, (m, k, e_own)
            assert e_single <= max(1e-10, 2 * floors[m][k]), (m, k, e_single)
    _assert_cf(cf1, O.contribution_function(lam, grids[1].pressures, res[1].final_T, dts[1]),
               "grid 1")
    plain = fa.batched_emission_spectra(grids, n_timesteps=30, convergence_dT=dT, post=False)
    assert all(type(r) is tuple and len(r) == 3 for r in plain)
    for (sp, T, it), rec in zip(plain, res):
        assert it == rec.n_iter and np.array_equal(T, rec.final_T)
        assert np.array_equal(sp.flux, rec.spectrum.flux)


# ------------------------------------------------------------------ G4: errors, not faults
def test_post_without_kept_dtaus_is_an_error(fa):
    lam, p, tabs_o, tabs_f, g, mmr, T0 = _setup(fa, 2, 300, 8, NAMES, 5)
    eng = fa.BatchEngine(lam, p, tabs_f, g=g, mmr=mmr)
    try:
        with pytest.raises(RuntimeError, match="no device dtaus"):
            eng.post()
        with pytest.raises(RuntimeError, match="no device dtaus"):
            eng.get_dtaus(0)
        plain = eng.run(T0, n_timesteps=2)
        assert set(plain) == {"spectra", "final_T", "n_iter"}
        with pytest.raises(RuntimeError, match="no device dtaus"):
            eng.post()
        kept = eng.run(T0, n_timesteps=2, keep_dtaus=True)
        assert set(kept) == {"spectra", "final_T", "n_iter"}
        assert np.array_equal(kept["spectra"], plain["spectra"])
        assert np.array_equal(kept["final_T"], plain["final_T"])
        te = eng.post()["T_eff"]
        assert te.shape == (2,) and np.all(np.isfinite(te))
        eng.run(T0, n_timesteps=2)                      # a plain run: the kept dtaus are stale
        with pytest.raises(RuntimeError, match="no device dtaus"):
            eng.post()
        with pytest.raises(RuntimeError, match="no device dtaus"):
            eng.get_dtaus(1)
        eng.run(T0, n_timesteps=2, keep_dtaus=True)
        with pytest.raises(RuntimeError, match="range"):
            eng.get_dtaus(2)
        with pytest.raises(ValueError, match="shape"):
            eng.post(dtaus=np.zeros((2, 8, 299)))
    finally:
        eng.close()


def test_post_batch_on_a_single_context_points_to_the_single_calls(fa):
    from frei_amd import _native as N
    n, nL = 130, 6
    lam, _, _ = O.wavelength_grid(0.5, 10, n)
    p = np.logspace(2, -6, nL)
    tabs = {"1H2-16O": fa.OpacityTable(np.ones((nL, 2, n)), p, [1000.0, 2000.0])}
    eng = fa.Engine(lam, p, tabs)
    try:
        dt, sp, T = np.ones((1, nL, n)), np.ones((1, n)), np.full((1, nL), 1000.0)
        sums = np.zeros((1, 3))
        rc = N.lib().frei_post_batch(eng._ctx, N.dptr(dt), N.dptr(sp), N.dptr(T), N.dptr(p),
                                     N.dptr(lam * 1e-4), None, None, 1.0, N.dptr(sums), None,
                                     None)
        assert rc < 0
        with pytest.raises(RuntimeError, match="frei_milne_pressure / frei_contribution"):
            N.check(rc)
    finally:
        eng.close()


def test_batch_context_of_one_atmosphere(fa):
    """frei_ctx_create_batch with n_atm = 1: the same run, kept dtaus and post()."""
    lam, p, tabs_o, tabs_f, g, mmr, T0 = _setup(fa, 1, 300, 8, NAMES, 7)
    eng = fa.BatchEngine(lam, p, tabs_f, g=g, mmr=mmr)
    try:
        out = eng.run(T0, n_timesteps=3, want_hist=True, keep_dtaus=True)
        dt = eng.get_dtaus(0)
        post = eng.post(want_p_milne=True)
    finally:
        eng.close()
    assert out["temp_hist"][0].shape == (8, 2 * out["n_iter"][0])
    assert np.all(dt[0] == 1.0)
    ref = O.effective_temperature(lam, p, out["spectra"][0], dt, out["final_T"][0])
    assert abs(post["T_eff"][0] - ref) <= 1e-12 * ref
    assert _close(post["p_milne"][0], O.milne_pressures(dt, p))
