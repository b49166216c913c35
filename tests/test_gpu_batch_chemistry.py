"""Batched contexts with temperature-dependent chemistry tables (frei_set_chemistry_batch):
every atmosphere interpolates its own table at its own layer temperatures every sweep, the
species sum stays in the sweep (no contracted table), and the sweep runs either over (wavelength
block, atmosphere) with the one-lane per-species kernel (``atm_tile`` 1) or atmosphere-tiled
(2 or 4 atmospheres per block, table rows loaded once for neighbours in the same T bracket).

Fixture: five atmospheres, three species on strong separable tables, 700 wavelengths (two full
256-blocks and one of 188 lanes), 20 layers, two chemistry tables.  Atmospheres 0 and 1 share
every T bracket, atmosphere 2 differs from them on one layer, 3 and 4 share: a tile of 2 or 4
sees reuse, reload and a remainder tile.  Each atmosphere is checked against the oracle's
emission_spectrum with its ChemistryTable (1e-10 outright; the oracle's own one-ulp floor here
is <= 1.8e-14 for fluxes and <= 5e-16 for T) and against single-atmosphere engines, bit for bit.

Oracle iteration counts of the convergence run (n_timesteps=30, n_zero_crossings=2,
convergence_dT=10.0): 13, 14, 13, 13, 12, unchanged with exp perturbed by one ulp."""
import ctypes

import numpy as np
import pytest

from oracle import frei_oracle as O
from tests.parity import assert_grid_parity, grid_floor, perturbed_exp, rel

pytestmark = pytest.mark.gpu

M_BAR = 4.0142926168559996e-24
NAMES = ["1H2-16O", "12C-16O", "12C-1H4"]
T_REF = [1500.0, 1500.0, 1540.0, 2100.0, 2100.0]
G = np.array([1200.0, 2478.65, 4000.0, 900.0, 3000.0])
ATM_TAB = [0, 1, 0, 1, 1]
TILES = [1, 2, 4]


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _chem_values(names, T_lo=300.0, T_hi=4000.0, n_T=14, n_p=9):
    """tests/test_gpu_parity.py::_chem_table (copied: test files do not import each other)."""
    T = np.linspace(T_lo, T_hi, n_T)
    p = np.logspace(-7, 3, n_p)
    x = np.tanh((T[:, None] - 1500.0) / 400.0) + 0.05 * np.log10(p)[None, :]
    base = O.mock_mmr(names, M_BAR)
    vals = []
    for s, n in enumerate(names):
        sign = -1.0 if s % 2 == 0 else 1.0
        vals.append(base[s] * 10 ** (0.8 * sign * x))
    return np.array(vals), T, p


def _tables(fa, rng, names, lam, p, Tn):
    tabs_o, tabs_f = {}, {}
    for n in names:
        base = 10 ** rng.uniform(0, 4.5, lam.size)
        fp, fT = (p / 1.0) ** 0.1, (Tn / 1000.0) ** 0.5
        tabs_o[n] = O.Table(O.separable_table(base, fp, fT, 10.0, 1e3), p, Tn)
        tabs_f[n] = fa.SeparableTable(base, fp, fT, p, Tn, lo=10.0, hi=1e3)
    return tabs_o, tabs_f


def _chem_pair(fa, names):
    """Two chemistry tables on shared nodes, at +0.0 and +0.5 dex: (engine's, oracle's)."""
    vals, cT, cp = _chem_values(names)
    f, o = [], []
    for dex in (0.0, 0.5):
        v = vals * 10 ** dex
        f.append(fa.ChemistryTable({n: v[s] for s, n in enumerate(names)}, cT, cp))
        o.append(O.ChemistryTable(v, cT, cp))
    return f, o


@pytest.fixture(scope="module")
def fx(fa):
    rng = np.random.default_rng(30)
    lam, _, _ = O.wavelength_grid(0.5, 10, 700)
    p = O.pressure_grid(20, -6, np.log10(200))
    Tn = np.linspace(400.0, 5000.0, 12)
    tabs_o, tabs_f = _tables(fa, rng, NAMES, lam, p, Tn)
    chem_f, chem_o = _chem_pair(fa, NAMES)
    T0 = np.array([O.temperature_grid(p, t, 0.1, 0.1) for t in T_REF])
    # the brackets the fixture is built for (the tile sees reuse, one reload, a remainder)
    br = np.array([np.searchsorted(Tn, T0[m], side="right") for m in range(5)])
    assert np.array_equal(br[0], br[1]) and np.array_equal(br[3], br[4])
    assert np.count_nonzero(br[2] != br[0]) == 1
    return dict(lam=lam, p=p, Tn=Tn, tabs_o=tabs_o, tabs_f=tabs_f, chem_f=chem_f, chem_o=chem_o,
                T0=T0, Ft=O.F_TOA(lam), cache={})


def _oracle(fx, key, m, **kw):
    """Oracle run of atmosphere m (computed once per module and shared)."""
    k = (key, m)
    if k not in fx["cache"]:
        fx["cache"][k] = O.emission_spectrum(
            fx["tabs_o"], fx["T0"][m], fx["p"], fx["lam"], fx["Ft"], G[m], M_BAR, 1,
            mmr=fx["chem_o"][ATM_TAB[m]], **kw)
    return fx["cache"][k]


def _batch(fa, fx, tile, monkeypatch):
    monkeypatch.setenv("FREI_ATM_TILE", str(tile))
    return fa.BatchEngine(fx["lam"], fx["p"], fx["tabs_f"], g=G,
                          mmr=[fx["chem_f"][k] for k in ATM_TAB], F_toa=fx["Ft"])


@pytest.mark.parametrize("tile", TILES)
def test_fixed_work_matches_oracle_per_atmosphere(fa, fx, monkeypatch, tile):
    """G1: four fixed iterations, every atmosphere against the oracle at 1e-10 outright."""
    kw = dict(n_timesteps=4, n_zero_crossings=10 ** 6, convergence_dT=-1.0)
    eng = _batch(fa, fx, tile, monkeypatch)
    try:
        path = eng.path()
        assert not path["contracted"] and path["atm_tile"] == tile, path
        out = eng.run(fx["T0"], alpha=1.0, **kw)
        ups, downs = eng.get_fluxes()
    finally:
        eng.close()
    for m in range(5):
        osp, oT, oth, odt, ou, od, it = _oracle(fx, "fixed", m, **kw)
        if ("floor", m) not in fx["cache"]:
            with perturbed_exp():
                psp, pT, _, _, pu, pd, _ = O.emission_spectrum(
                    fx["tabs_o"], fx["T0"][m], fx["p"], fx["lam"], fx["Ft"], G[m], M_BAR, 1,
                    mmr=fx["chem_o"][ATM_TAB[m]], **kw)
            fx["cache"][("floor", m)] = (max(grid_floor(osp, ou, od, psp, pu, pd)), rel(pT, oT))
        f_floor, T_floor = fx["cache"][("floor", m)]
        print(f"atmosphere {m}: oracle one-ulp floor fluxes {f_floor:.2e} T {T_floor:.2e}")
        assert f_floor < 1e-12 and T_floor < 1e-12
        e = assert_grid_parity(out["spectra"][m], osp, ups[m], ou, downs[m], od,
                               f"chemistry batch, tile {tile}, atmosphere {m} (outright)",
                               T=out["final_T"][m], ref_T=oT)
        print({k: v for k, v in e.items() if k.endswith(("wise", "norm"))})
        assert e["within_1e-10"], e
        # the chemistry is live: the mixing ratios moved between T0 and the final T
        ch = fx["chem_o"][ATM_TAB[m]]
        a = np.array([ch(fx["T0"][m][i], fx["p"][i]) for i in range(20)])
        b = np.array([ch(oT[i], fx["p"][i]) for i in range(20)])
        assert rel(b, a) > 1e-3


@pytest.mark.parametrize("tile", TILES)
def test_convergence_inside_a_tile(fa, fx, monkeypatch, tile):
    """G2: atmospheres of one tile stop at different iterations (oracle: 13, 14, 13, 13, 12);
    counts, T, spectrum, history, kept dtaus and post() of every atmosphere."""
    kw = dict(n_timesteps=30, n_zero_crossings=2, convergence_dT=10.0)
    eng = _batch(fa, fx, tile, monkeypatch)
    try:
        assert eng.path()["atm_tile"] == tile
        out = eng.run(fx["T0"], alpha=1.0, want_hist=True, keep_dtaus=True, **kw)
        dt = np.array([eng.get_dtaus(m) for m in range(5)])
        post = eng.post()
        again = eng.post(dtaus=dt, spectra=out["spectra"], T=out["final_T"])
    finally:
        eng.close()
    ora = [_oracle(fx, "conv", m, **kw) for m in range(5)]
    counts = [o[6] for o in ora]
    print("iterations", list(out["n_iter"]), "oracle", counts)
    assert counts == [13, 14, 13, 13, 12]
    assert list(out["n_iter"]) == counts
    for m in range(5):
        osp, oT, oth, odt, ou, od, it = ora[m]
        errs = (rel(out["final_T"][m], oT), rel(out["spectra"][m], osp),
                rel(out["temp_hist"][m], oth), rel(dt[m][1:], odt[1:]))
        print(f"atmosphere {m}: T {errs[0]:.2e} spectrum {errs[1]:.2e} history {errs[2]:.2e} "
              f"dtaus {errs[3]:.2e}")
        assert out["temp_hist"][m].shape == oth.shape
        assert max(errs) <= 1e-10, (m, errs)
        assert np.all(dt[m][0] == 1.0)
    assert np.all(np.isfinite(post["T_eff"])) and np.all(post["T_eff"] > 0)
    assert np.array_equal(post["T_eff"], again["T_eff"])


def _iterate(eng, T0, n):
    eng.state_init(T0)
    eng.iterate(n)
    eng.synchronize()
    up, down = eng.get_fluxes()
    return eng.get_temperatures(), up, down


@pytest.mark.parametrize("tile", TILES)
def test_bitwise_against_single_contexts(fa, fx, monkeypatch, tile):
    """G3: three fixed-work iterations; each atmosphere's T and fluxes are bit for bit those
    of a single-atmosphere engine with that atmosphere's table and gravity."""
    if "single" not in fx["cache"]:
        ref = []
        for m in range(5):
            single = fa.Engine(fx["lam"], fx["p"], fx["tabs_f"], g=G[m],
                               mmr=fx["chem_f"][ATM_TAB[m]], F_toa=fx["Ft"])
            try:
                assert not single.path()["contracted"]
                ref.append(_iterate(single, fx["T0"][m], 3))
            finally:
                single.close()
        fx["cache"]["single"] = ref
    eng = _batch(fa, fx, tile, monkeypatch)
    try:
        assert eng.path()["atm_tile"] == tile
        T, up, down = _iterate(eng, fx["T0"], 3)
    finally:
        eng.close()
    for m, (Ts, su, sd) in enumerate(fx["cache"]["single"]):
        assert np.array_equal(T[m], Ts), f"atmosphere {m}: T {rel(T[m], Ts):.3e}"
        assert np.array_equal(up[m], su), f"atmosphere {m}: F_up"
        assert np.array_equal(down[m], sd), f"atmosphere {m}: F_down"


def test_eight_species_tiles_match_one_atmosphere_per_block(fa, monkeypatch):
    """G4: the widest instantiation (S = 8), a 44-lane remainder block, 3 atmospheres (tile 2:
    one full tile and a remainder; tile 4: one partial tile): bitwise the tile-1 run."""
    from frei_amd.workloads import C3_SPECIES
    names = list(C3_SPECIES)
    assert len(names) == 8
    rng = np.random.default_rng(31)
    lam, _, _ = O.wavelength_grid(0.5, 10, 300)
    p = O.pressure_grid(8, -6, np.log10(200))
    Tn = np.linspace(400.0, 5000.0, 12)
    _, tabs_f = _tables(fa, rng, names, lam, p, Tn)
    chem_f, _ = _chem_pair(fa, names)
    g = np.array([1200.0, 2478.65, 4000.0])
    T0 = np.array([O.temperature_grid(p, t, 0.1, 0.1) for t in (1500.0, 1500.0, 2100.0)])
    out = {}
    for tile in TILES:
        monkeypatch.setenv("FREI_ATM_TILE", str(tile))
        eng = fa.BatchEngine(lam, p, tabs_f, g=g, mmr=[chem_f[0], chem_f[1], chem_f[1]])
        try:
            path = eng.path()
            assert not path["contracted"] and path["atm_tile"] == tile, path
            out[tile] = _iterate(eng, T0, 3)
        finally:
            eng.close()
    assert np.all(np.isfinite(out[1][0])) and np.all(out[1][1][:, -1] > 0)
    for tile in (2, 4):
        for a, b, what in zip(out[tile], out[1], ("T", "F_up", "F_down")):
            assert np.array_equal(a, b), f"tile {tile}: {what}"


def test_automatic_tile_width_follows_the_launch_size(fa, monkeypatch):
    """Without FREI_ATM_TILE the widest tile that leaves the launch one resident round of blocks
    (four per CU; 256 CUs on the MI355X): 64 wavelength blocks x 64 atmospheres -> 4, x 32 -> 2,
    x 8 -> 1; the automatic run is bitwise the tile-1 run."""
    monkeypatch.delenv("FREI_ATM_TILE", raising=False)
    names = NAMES[:2]
    rng = np.random.default_rng(32)
    lam, _, _ = O.wavelength_grid(0.5, 10, 64 * 256)
    p = O.pressure_grid(6, -6, np.log10(200))
    Tn = np.linspace(400.0, 5000.0, 12)
    _, tabs_f = _tables(fa, rng, names, lam, p, Tn)
    chem_f, _ = _chem_pair(fa, names)
    out = {}
    for n_atm, want in ((64, 4), (32, 2), (8, 1)):
        g = np.linspace(900.0, 4000.0, n_atm)
        T0 = np.array([O.temperature_grid(p, t, 0.1, 0.1)
                       for t in np.repeat(np.linspace(1300.0, 2300.0, n_atm // 4), 4)])
        for tile in (None, 1) if n_atm == 64 else (None,):
            if tile:
                monkeypatch.setenv("FREI_ATM_TILE", str(tile))
            eng = fa.BatchEngine(lam, p, tabs_f, g=g, mmr=[chem_f[m % 2] for m in range(n_atm)])
            try:
                assert eng.path()["atm_tile"] == (tile or want), (n_atm, eng.path())
                if n_atm == 64:
                    out[tile] = _iterate(eng, T0, 2)
            finally:
                eng.close()
            monkeypatch.delenv("FREI_ATM_TILE", raising=False)
    for a, b, what in zip(out[None], out[1], ("T", "F_up", "F_down")):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b), what


def test_one_atmosphere_batch_context_equals_the_single_context(fa, fx):
    """G5: frei_ctx_create_batch with n_atm = 1 and a chemistry table (the second of two)."""
    m = 1
    eng = fa.BatchEngine(fx["lam"], fx["p"], fx["tabs_f"], g=[G[m]], F_toa=fx["Ft"])
    try:
        eng.set_chemistry(fx["chem_f"], [1])
        assert not eng.path()["contracted"]
        Tb, ub, db = _iterate(eng, fx["T0"][m:m + 1], 3)
    finally:
        eng.close()
    single = fa.Engine(fx["lam"], fx["p"], fx["tabs_f"], g=G[m], mmr=fx["chem_f"][1],
                       F_toa=fx["Ft"])
    try:
        Ts, su, sd = _iterate(single, fx["T0"][m], 3)
    finally:
        single.close()
    assert np.array_equal(Tb[0], Ts)
    assert np.array_equal(ub[0], su) and np.array_equal(db[0], sd)


def test_chemistry_switched_off_returns_to_the_contracted_path(fa, fx):
    """G6: frei_set_chemistry_batch(values=NULL) — the run is then bitwise that of a fresh
    fixed-mmr BatchEngine."""
    kw = dict(n_timesteps=3, n_zero_crossings=10 ** 6, convergence_dT=-1.0)
    eng = fa.BatchEngine(fx["lam"], fx["p"], fx["tabs_f"], g=G,
                         mmr=[fx["chem_f"][k] for k in ATM_TAB], F_toa=fx["Ft"])
    try:
        assert not eng.path()["contracted"]
        chem = eng.run(fx["T0"], **kw)
        eng.set_chemistry(None)
        path = eng.path()
        assert path["contracted"] and path["atm_tile"] == 0, path
        off = eng.run(fx["T0"], **kw)
    finally:
        eng.close()
    fresh_eng = fa.BatchEngine(fx["lam"], fx["p"], fx["tabs_f"], g=G, F_toa=fx["Ft"])
    try:
        fresh = fresh_eng.run(fx["T0"], **kw)
    finally:
        fresh_eng.close()
    assert np.array_equal(off["final_T"], fresh["final_T"])
    assert np.array_equal(off["spectra"], fresh["spectra"])
    assert not np.array_equal(chem["final_T"], fresh["final_T"])


def test_batched_emission_spectra_over_grids_with_chemistry_tables(fa):
    """G7: three Grids (different T_ref, g, star and orbit), two sharing one ChemistryTable, as
    one batched run with post=True, against each Grid's own emission_spectrum and the oracle."""
    lam, _, _ = O.wavelength_grid(0.5, 10, 1024)
    grids, op = [], None
    names = None
    tabs = {}
    for k, (T_ref, g, T_star, a_r) in enumerate([(1400, 1500.0, 5800.0, 6.450964670116429),
                                                 (2000, 2478.6519476149147, 4500.0, 5.0),
                                                 (2400, 4000.0, 6500.0, 8.0)]):
        pl = fa.Planet.from_hot_jupiter()
        pl.g = g
        pl.T_star = T_star
        pl.a_rstar = a_r
        gr = fa.Grid(pl, lam=lam, n_layers=20, T_ref=T_ref)
        if op is None:
            op = fa.load_example_opacity(gr, scale_factor=2)
            names = list(op)
            vals, cT, cp = _chem_values(names)
            for dex in (0.0, 0.5):
                v = vals * 10 ** dex
                tabs[dex] = (fa.ChemistryTable({n: v[s] for s, n in enumerate(names)}, cT, cp),
                             O.ChemistryTable(v, cT, cp))
        gr.load_opacities(opacities=op, mmr=tabs[0.0 if k != 1 else 0.5][0])
        grids.append(gr)
    tabs_o = {n: O.Table(op[n].values, op[n].pressure, op[n].temperature) for n in names}
    with fa.batched_emission_spectra(grids, n_timesteps=30, post=True) as res:
        assert not res.engine.path()["contracted"]
        assert res.engine.chemistry[1].tolist() == [0, 1, 0]
        recs = list(res)
    for k, (gr, rec) in enumerate(zip(grids, recs)):
        s1, T1, th1, _ = gr.emission_spectrum(n_timesteps=30)
        gr._close_engine()
        assert rec.n_iter == th1.shape[1] // 2
        assert np.isfinite(rec.T_eff) and rec.T_eff > 0
        pl = gr.planet
        Ft = O.F_TOA(lam, T_star=pl.T_star, a_rstar=pl.a_rstar)
        ch = tabs[0.0 if k != 1 else 0.5][1]

        def run():
            return O.emission_spectrum(tabs_o, gr.init_temperatures, gr.pressures, lam, Ft, pl.g,
                                       pl.m_bar, pl.alpha, n_timesteps=30, mmr=ch)
        osp, oT, *_ = run()
        with perturbed_exp():
            psp, pT, *_ = run()
        fT, fS = rel(pT, oT), rel(psp, osp)
        for t, sp_ in ((rec.final_T, rec.spectrum.flux), (T1, s1.flux)):
            print(f"grid {k}: T {rel(t, oT):.2e} (floor {fT:.2e}) spectrum {rel(sp_, osp):.2e} "
                  f"(floor {fS:.2e})")
            assert rel(t, oT) <= max(1e-10, 2 * fT), (rel(t, oT), fT)
            assert rel(sp_, osp) <= max(1e-10, 2 * fS), (rel(sp_, osp), fS)


def test_c_abi_refusals(fa, fx):
    """G8: frei_set_chemistry_batch names what it refuses."""
    from frei_amd import _native as N
    lib = N.lib()
    vals, cT, cp = _chem_values(NAMES)
    v = N.f64(np.array([vals, vals]))
    cp_cgs = N.f64(cp * 1e6)
    cT = N.f64(cT)
    i32 = ctypes.POINTER(ctypes.c_int32)

    def call(ctx, n_tab, atm, T=cT, p=cp_cgs):
        atm = np.asarray(atm, dtype=np.int32)
        rc = lib.frei_set_chemistry_batch(ctx, N.dptr(v), n_tab, atm.ctypes.data_as(i32),
                                          N.dptr(T), T.size, N.dptr(p), p.size)
        return rc, lib.frei_last_error().decode()

    single = fa.Engine(fx["lam"], fx["p"], fx["tabs_f"], g=G[0], F_toa=fx["Ft"])
    try:
        rc, msg = call(single._ctx, 1, [0])
        assert rc < 0 and "frei_ctx_create_batch" in msg and "frei_set_chemistry" in msg, msg
    finally:
        single.close()
    eng = fa.BatchEngine(fx["lam"], fx["p"], fx["tabs_f"], g=G[:3], F_toa=fx["Ft"])
    try:
        rc, msg = call(eng._ctx, 0, [0, 0, 0])
        assert rc < 0 and "n_tab must be >= 1" in msg, msg
        for bad in ([0, 2, 0], [0, 0, -1]):
            rc, msg = call(eng._ctx, 2, bad)
            assert rc < 0 and "outside [0, n_tab)" in msg, msg
        rc, msg = call(eng._ctx, 2, [0, 1, 0], T=N.f64(cT[::-1]))
        assert rc < 0 and "T nodes must ascend" in msg, msg
        rc, msg = call(eng._ctx, 2, [0, 1, 0], p=N.f64(cp_cgs[::-1]))
        assert rc < 0 and "p nodes must be positive and ascend" in msg, msg
        # every refusal left the context on its fixed mixing ratios; a valid call then takes
        assert eng.path()["contracted"]
        rc, msg = call(eng._ctx, 2, [0, 1, 0])
        assert rc == 0, msg
        assert not eng.path()["contracted"]
        # frei_set_chemistry still refuses a batched context
        rc = lib.frei_set_chemistry(eng._ctx, N.dptr(v), N.dptr(cT), cT.size, N.dptr(cp_cgs),
                                    cp_cgs.size)
        assert rc < 0 and b"batched" in lib.frei_last_error()
    finally:
        eng.close()
