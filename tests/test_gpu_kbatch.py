"""K20 on the GPU: batches of correlated-k atmospheres, one composition each.  The batch's
per-atmosphere tables are K19's mixtures bit for bit (frei_set_table_kmix_batch writes them
through a row list), set_mix re-mixes some of them in place, the T-P loop on them is held to the
oracle per atmosphere as tests/test_gpu_batch.py holds the batched engine, the single-atmosphere
path and the batch agree under the same criterion, the post-processing of a KBatchResult is the
collapse of the per-column calls, Milne on k-columns reduces to the reference's formula when k
does not depend on g, and every C-level argument error is refused with its text.
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import frei_amd as fa
from frei_amd import _native as N
from frei_amd import constants as K
from frei_amd.binning import CrossSection, KLibrary
from frei_amd.core import collapse_columns
from frei_amd.engine import planck_prefactor, quadrature_weights
from frei_amd.kdist import KGrid, batched_k_spectra, gauss_g
from frei_amd.opacity import sigma_scattering
from frei_amd.transit import level_radii
from oracle import frei_oracle as O
from tests import kdist_ref as R
from tests import kmix_ref as M
from tests.parity import (EPS, assert_flux_parity, assert_grid_parity, grid_floor,
                          perturbed_exp, rel)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M_BAR = K.M_BAR_HOT_JUPITER


def same_bits(a, b):
    return (np.array_equal(a, b, equal_nan=True) and
            np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b)))


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------ the small case
T3 = np.array([2000.0, 1000.0, 1500.0])          # unsorted: the engine stores them ascending
P6 = np.logspace(1, -4, 6)                       # bar, the library's pressure nodes
USED = [0, 2, 3, 5]                              # the nodes the 4 layers sit on
WL5 = np.linspace(1.0, 3.0, 6)


def small_case(n_g):
    """Library (n_src 3, n_p 6, n_T 3, n_bins 5, n_g) of random lognormal k-tables and five
    compositions (n_comp, n_src, n_T, n_p), atmosphere 2 without species 1."""
    rng = np.random.default_rng(200 + n_g)
    Ks = np.sort(rng.lognormal(0.0, 2.0, (3, 6, 3, 5, n_g)), axis=-1)
    g, w = gauss_g(n_g)
    lib = KLibrary({f"s{k}": t for k, t in enumerate(Ks)}, WL5, g, w, T3, P6)
    x = rng.uniform(1e-3, 1e-1, (5, 3, 3, 6))
    x[2, 1] = 0.0
    lam = np.repeat((WL5[:-1] + WL5[1:]) / 2, n_g)
    qw = np.outer(np.diff(WL5) * K.UM, w).ravel()
    return dict(Ks=Ks, lib=lib, x=x, lam=lam, qw=qw, p=P6[USED], w=w, n_g=n_g,
                g=np.array([K.G_JUPITER, 900.0, 2500.0, 4000.0, 1500.0]),
                T0=np.linspace(1700.0, 1100.0, 4))


def small_engine(c, x=None, atm=slice(None)):
    x = c["x"] if x is None else x
    return fa.BatchEngine(c["lam"], c["p"], {"mix": c["lib"].tables(x[atm])}, c["g"][atm],
                          quad_weights=c["qw"])


def small_digest(n_g):
    """The tables of the five atmospheres and a two-iteration run, as one digest."""
    c = small_case(n_g)
    eng = small_engine(c)
    try:
        tabs = [eng.table(m) for m in range(5)]
        out = eng.run(c["T0"], n_timesteps=2)
    finally:
        eng.close()
    return digest(*tabs, out["spectra"], out["final_T"]), tabs, out


def child_main(n_g):
    print("digest", small_digest(n_g)[0])


def raw_context(lam, qw, p, n_atm, n_species=1, grid=True, batch=True):
    """A context through the C ABI alone -> (lib, ctx)."""
    lib, ctx = N.lib(), ctypes.c_void_p()
    if batch:
        N.check(lib.frei_ctx_create_batch(ctypes.byref(ctx), 0, p.size, lam.size, n_species, n_atm))
    else:
        N.check(lib.frei_ctx_create(ctypes.byref(ctx), 0, p.size, lam.size, n_species))
    if grid:
        lam_cm = lam * K.UM
        N.check(lib.frei_set_grid(
            ctx, N.dptr(N.f64(planck_prefactor(lam_cm))), N.dptr(N.f64(lam_cm * K.K_B)),
            N.dptr(N.f64(sigma_scattering(lam, M_BAR))), N.dptr(N.f64(O.F_TOA(lam))),
            N.dptr(N.f64(quadrature_weights(lam_cm, qw))), N.dptr(N.f64(p * K.BAR)),
            float(K.G_JUPITER), M_BAR))
    return lib, ctx


# ------------------------------------------------------------------------------ 1. the tables
@pytest.mark.parametrize("n_g", [2, 8, 12])
def test_tables_are_k19s_bit_for_bit(n_g, monkeypatch):
    """n_g = 2 the wave form, 8 the forced-wave boundary (the automatic choice is the block
    form; FREI_KMIX_FORM=wave is checked too), 12 the block form."""
    monkeypatch.delenv("FREI_KMIX_FORM", raising=False)
    monkeypatch.delenv("FREI_ALLOC_FILL", raising=False)
    c = small_case(n_g)
    lib, x = c["lib"], c["x"]
    want = lib.mix(x).reshape(5, 6, 3, -1)
    assert np.all(np.isfinite(want)) and not same_bits(want[0], want[1])
    dig, tabs, out = small_digest(n_g)
    unused = [k for k in range(6) if k not in USED]
    for m in range(5):
        assert tabs[m].shape == (6, 3, 5 * n_g)
        assert same_bits(tabs[m][USED], want[m][USED]), m
        assert np.all(tabs[m][unused] == 0) and not np.signbit(tabs[m][unused]).any(), m
    assert np.all(np.isfinite(out["spectra"])) and np.all(out["n_iter"] == 2)
    if n_g == 8:
        monkeypatch.setenv("FREI_KMIX_FORM", "wave")
        eng = small_engine(c)
        assert all(same_bits(eng.table(m), tabs[m]) for m in range(5))
        eng.close()
        monkeypatch.delenv("FREI_KMIX_FORM")
    # one atmosphere: the non-batched route, composition 0 is species 0's table (every row)
    one = small_engine(c, atm=slice(3, 4))
    try:
        assert same_bits(one.table(0), want[3])
        o1 = one.run(c["T0"], n_timesteps=2)
    finally:
        one.close()
    # (the one-species sweep against the batch's: another kernel on a table of the same bits)
    print("n_atm = 1 against row 3 of the batch: T", rel(o1["final_T"][0], out["final_T"][3]))
    assert o1["n_iter"][0] == 2 and rel(o1["final_T"][0], out["final_T"][3]) < 1e-9
    # a column slice that cuts bins 0 and 3, through the C ABI
    lo, hi = n_g - 1, 3 * n_g + 1
    clib, ctx = raw_context(c["lam"][lo:hi], c["qw"][lo:hi], c["p"], 5)
    xc = lib.tables(x).x
    try:
        N.check(clib.frei_set_table_kmix_batch(ctx, lib.handle(), N.dptr(xc), lo))
        part = np.empty((6, 3, hi - lo))
        for m in range(5):
            N.check(clib.frei_get_table_batch(ctx, m, N.dptr(part)))
            assert same_bits(part[USED], want[m][USED][:, :, lo:hi]), m
            assert np.all(part[unused] == 0), m
    finally:
        clib.frei_ctx_destroy(ctx)
    # a fresh process whose every new device buffer is filled with 0xFF gives the same bits
    r = subprocess.run([sys.executable, "-c",
                        f"from tests.test_gpu_kbatch import child_main; child_main({n_g})"],
                       cwd=ROOT, env=dict(os.environ, FREI_ALLOC_FILL="255"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split("digest")[-1].strip() == dig
    # the row list did not change K19: frei_klib_mix and frei_set_table_kmix against the
    # restatement, to K19's bound
    ref, lnmax = M.kmix_ref(c["Ks"], xc[0], c["w"])
    eps = np.array([[[M.step_bound(n_g, v) for v in row] for row in pl] for pl in lnmax])
    bound = ((1.0 + eps) ** 2 - 1.0)[..., None]
    got = lib.mix(x[0])
    assert np.all(np.abs(got / ref - 1.0) <= bound)
    single = fa.BatchEngine(c["lam"], c["p"], {"mix": lib.table(x[0])}, c["g"][:1],
                            mmr=np.ones((1, 1, 4)), quad_weights=c["qw"])
    try:
        tab = np.empty((6, 3, 5 * n_g))
        N.check(N.lib().frei_get_table_batch(single._ctx, 0, N.dptr(tab)))
    finally:
        single.close()
    assert same_bits(tab, got.reshape(6, 3, -1)[:, np.argsort(T3)])     # stored ascending in T
    lib.release()


# ------------------------------------------------------------------------------ 2. set_mix
def test_set_mix_is_in_place():
    c = small_case(12)
    lib, x = c["lib"], c["x"]
    rng = np.random.default_rng(77)
    x_new = x.copy()
    x_new[[1, 3]] = rng.uniform(1e-3, 1e-1, (2, 3, 3, 6))
    eng = small_engine(c)
    fresh = None
    try:
        before = [eng.table(m) for m in range(5)]
        first = eng.run(c["T0"], n_timesteps=3)
        eng.set_mix(x_new[[1, 3]], atm=[1, 3])
        after = [eng.table(m) for m in range(5)]
        want = lib.mix(x_new).reshape(5, 6, 3, -1)
        for m in (1, 3):
            assert same_bits(after[m][USED], want[m][USED]) and not same_bits(after[m], before[m])
        for m in (0, 2, 4):
            assert same_bits(after[m], before[m])
        out = eng.run(c["T0"], n_timesteps=3)
        fresh = small_engine(c, x=x_new)
        ref = fresh.run(c["T0"], n_timesteps=3)
        for k in ("spectra", "final_T", "n_iter"):
            assert same_bits(np.asarray(out[k], float), np.asarray(ref[k], float)), k
        assert not same_bits(out["spectra"][1], first["spectra"][1])
        assert same_bits(out["spectra"][0], first["spectra"][0])
        # all atmospheres at once, and the arguments Python refuses
        eng.set_mix(x)
        assert all(same_bits(eng.table(m), before[m]) for m in range(5))
        with pytest.raises(ValueError, match="2 compositions for 1 atmospheres"):
            eng.set_mix(x[:2], atm=[0])
        with pytest.raises(ValueError, match="atmosphere 5 lies outside"):
            eng.set_mix(x[:1], atm=[5])
    finally:
        eng.close()
        if fresh is not None:
            fresh.close()
        lib.release()


def test_update_of_a_one_atmosphere_context_remixes_species_0():
    """A k-mix context from frei_ctx_create_batch with n_atm = 1 sweeps species 0's table:
    frei_kmix_batch_update re-mixes that table in place, frei_get_table_batch returns the
    library's mix of the new composition bit for bit in the library's node order (T3, unsorted),
    and a run on it is finite.  4 layers, 13 bins x n_g 5 = 65 columns (one past the 64-element
    row pitch), 3 x 3 nodes."""
    rng = np.random.default_rng(165)
    n_g, bins = 5, np.linspace(1.0, 3.0, 14)
    P3 = np.array([10.0, 1e-1, 1e-3])
    g, w = gauss_g(n_g)
    Ks = np.sort(rng.lognormal(0.0, 2.0, (2, 3, 3, 13, n_g)), axis=-1)
    klib = KLibrary({"a": Ks[0], "b": Ks[1]}, bins, g, w, T3, P3)
    lam = np.repeat((bins[:-1] + bins[1:]) / 2, n_g)
    qw = np.outer(np.diff(bins) * K.UM, w).ravel()
    p = np.array([10.0, 1.0, 1e-1, 1e-3])
    x = rng.uniform(1e-3, 1e-1, (2, 2, 3, 3))                   # (n_comp, n_src, n_T, n_p)
    xc = klib.tables(x).x
    want = klib.mix(x).reshape(2, 3, 3, -1)
    assert lam.size == 65 and not same_bits(want[0], want[1])
    lib, ctx = raw_context(lam, qw, p, 1)
    try:
        tab = np.empty((3, 3, 65))
        N.check(lib.frei_set_table_kmix_batch(ctx, klib.handle(), N.dptr(N.f64(xc[:1])), 0))
        N.check(lib.frei_get_table_batch(ctx, 0, N.dptr(tab)))
        assert same_bits(tab, want[0])
        N.check(lib.frei_kmix_batch_update(ctx, 0, 1, N.dptr(N.f64(xc[1:]))))
        N.check(lib.frei_get_table_batch(ctx, 0, N.dptr(tab)))
        assert same_bits(tab, want[1])
        n_iter = (ctypes.c_int * 1)()
        Tf, sp = np.empty((1, 4)), np.empty((1, 65))
        T0 = N.f64(np.linspace(1700.0, 1100.0, 4)[None])
        N.check(lib.frei_run_batch(ctx, N.dptr(T0), 2, 2, 3.0, 1.0, n_iter, N.dptr(Tf), N.dptr(sp)))
        assert np.all(np.isfinite(sp)) and np.all(np.isfinite(Tf)) and n_iter[0] >= 1
    finally:
        lib.frei_ctx_destroy(ctx)
        klib.release()


# ------------------------------------------------------------------------------ 3. the oracle
COMPS =[(0.6, 0.4), (0.2, 0.8), (1.0, 0.0), (3e-3, 0.5), (0.05, 0.01)]
GRAVITIES = [K.G_JUPITER, 900.0, 2500.0, 4000.0, 1500.0]
N_STEPS = 6


def oracle_run(table, p, T_nodes, lam, qw, g, T0):
    """The oracle's emission_spectrum on one k-table (n_p, n_T, n_col), the bolometric sums the
    dot product with the column weights, and its own one-ulp-of-exp floors."""
    tabs = {"mix": O.Table(table, p, T_nodes)}
    Ft = O.F_TOA(lam)
    mmr = np.ones((1, p.size))

    def bol(*rows):
        return tuple(float(np.dot(r, qw)) for r in rows)

    def run(err=None):
        return O.emission_spectrum(tabs, T0, p, lam, Ft, g, M_BAR, 1, n_timesteps=N_STEPS,
                                   n_zero_crossings=2, convergence_dT=3.0, mmr=mmr, err=err,
                                   bol_fn=bol)
    cond = dict(up=np.zeros((p.size, lam.size)), down=np.zeros((p.size, lam.size)), delta=1.0)
    sp, T, th, dt, up, down, it = run(cond)
    with perturbed_exp():
        psp, pT, _, pdt, pu, pd, _ = run()
    return dict(spec=sp, T=T, dtaus=dt, up=up, down=down, it=it, cond=cond["up"][-1],
                T_floor=rel(pT, T), floor=grid_floor(sp, up, down, psp, pu, pd),
                dt_floor=rel(pdt[1:], dt[1:]))


def hold_to_oracle(o, spectra, T, n_iter, up, down, what):
    """The assertions of tests/test_gpu_batch.py for one atmosphere."""
    assert n_iter == o["it"], f"{what}: iterations"
    relT = rel(T, o["T"])
    print(f"{what}: T {relT:.3e} (floor {o['T_floor']:.3e}), spectrum "
          f"{rel(spectra, o['spec']):.3e} (floor {o['floor'][0]:.3e})")
    assert relT <= max(1e-10, 2 * o["T_floor"]), f"{what}: T {relT:.3e}"
    assert_flux_parity(spectra, o["spec"], o["cond"], max(EPS, relT), f"{what} spectrum")
    assert_grid_parity(spectra, o["spec"], up, o["up"], down, o["down"], what, o["floor"], T=T,
                       ref_T=o["T"], T_floor=o["T_floor"])


@pytest.fixture(scope="module")
def forest():
    """The two-species forest at n_g = 8 (64 columns x 12 layers): the library, five KGrids on
    it (compositions COMPS, gravities GRAVITIES), their batch, and the oracle per atmosphere."""
    case = M.forest_pair()
    g, w = gauss_g(8)
    Ks = M.species_tables(case, g)
    lib = KLibrary({"one": Ks[0], "two": Ks[1]}, case["wl_bins"], g, w, case["T_nodes"],
                   case["p"])
    grids = []
    for comp, grav in zip(COMPS, GRAVITIES):
        pl = fa.Planet.from_hot_jupiter()
        pl.g = grav
        gr = KGrid(pl, case["wl_bins"], g=g, weights=w, pressures=case["p"],
                   init_temperatures=case["T"])
        gr.load_opacities(klibrary=lib, mix=np.array(comp)[:, None, None])
        grids.append(gr)
    res = batched_k_spectra(grids, n_timesteps=N_STEPS, convergence_dT=3, post=True)
    g0 = grids[0]
    oracle = []
    for comp, grav in zip(COMPS, GRAVITIES):
        want, _ = M.kmix_ref(Ks, np.array(comp)[:, None, None], w)
        oracle.append(oracle_run(want.reshape(want.shape[:2] + (-1,)), case["p"],
                                 case["T_nodes"], g0.col_lam, g0.col_weights, grav, case["T"]))
    yield dict(case=case, lib=lib, grids=grids, res=res, oracle=oracle, Ks=Ks)
    res.close()
    for gr in grids:
        gr._close_engine()
    lib.release()


def test_forest_batch_matches_oracle_per_atmosphere(forest):
    res, eng = forest["res"], forest["res"].engine
    assert eng.kmix is not None and eng.path()["contracted"]
    cols = eng._last_spectra
    ups, downs = eng.get_fluxes()
    assert same_bits(cols, ups[:, -1])
    for m, o in enumerate(forest["oracle"]):
        assert o["it"] == N_STEPS and 913.0 <= o["T"].min() and o["T"].max() <= 1798.0
        assert o["T_floor"] <= 4.5e-14 and o["floor"][0] <= 3.8e-12
        hold_to_oracle(o, cols[m], res[m].final_T, res[m].n_iter, ups[m], downs[m],
                       f"forest atmosphere {m}")
        assert same_bits(res[m].spectrum.flux, forest["grids"][0].collapse(cols[m]))


def test_block_crossing_shape_matches_oracle():
    """24 bins x n_g = 12 = 288 columns: a second 256-column block and 32 columns of padding up
    to the pitch; random sorted lognormal k-tables, the forest's layers, 3 atmospheres."""
    case = R.forest_case()
    rng = np.random.default_rng(53)
    n_g, n_bins = 12, 24
    g, w = gauss_g(n_g)
    p, Tn = case["p"], case["T_nodes"]
    Ks = np.sort(rng.lognormal(0.0, 2.0, (2, p.size, Tn.size, n_bins, n_g)), axis=-1)
    bins = np.linspace(2.5, 3.0, n_bins + 1)
    lib = KLibrary({"a": Ks[0], "b": Ks[1]}, bins, g, w, Tn, p)
    lam = np.repeat((bins[:-1] + bins[1:]) / 2, n_g)
    qw = np.outer(np.diff(bins) * K.UM, w).ravel()
    x = rng.uniform(1e-3, 1e-1, (3, 2, Tn.size, p.size))
    grav = np.array(GRAVITIES[:3])
    eng = fa.BatchEngine(lam, p, {"mix": lib.tables(x)}, grav, F_toa=O.F_TOA(lam),
                         m_bar=M_BAR, quad_weights=qw)
    try:
        out = eng.run(case["T"], n_timesteps=N_STEPS, convergence_dT=3.0)
        ups, downs = eng.get_fluxes()
        tabs = [eng.table(m) for m in range(3)]
    finally:
        eng.close()
    want = lib.mix(x).reshape(3, p.size, Tn.size, -1)
    for m in range(3):
        assert same_bits(tabs[m], want[m])
        ref, _ = M.kmix_ref(Ks, x[m].transpose(0, 2, 1), w)
        o = oracle_run(ref.reshape(ref.shape[:2] + (-1,)), p, Tn, lam, qw, grav[m], case["T"])
        hold_to_oracle(o, out["spectra"][m], out["final_T"][m], out["n_iter"][m], ups[m],
                       downs[m], f"288-column atmosphere {m}")
    lib.release()


# ------------------------------------------------------------------------------ 4. single path
def test_batch_against_the_single_path(forest):
    """KGrid.emission_spectrum per composition (one context per run, frei_set_table_kmix)
    against row m of the batch.  The two sweep different kernels over tables of the same bits, so
    no bit equality is asserted: the criterion is test 3's, with the oracle's floors."""
    res, grids = forest["res"], forest["grids"]
    worst = dict(spec=0.0, T=0.0, dtaus=0.0)
    for m, (gr, o) in enumerate(zip(grids, forest["oracle"])):
        gr.set_mix(np.array(COMPS[m])[:, None, None])
        spec, T, th, dtaus = gr.emission_spectrum(n_timesteps=N_STEPS, convergence_dT=3)
        assert th.shape[1] // 2 == res[m].n_iter
        relT = rel(res[m].final_T, T)
        assert relT <= max(1e-10, 2 * o["T_floor"]), f"atmosphere {m}: T {relT:.3e}"
        assert_flux_parity(res[m].spectrum.flux, spec.flux, gr.collapse(o["cond"]),
                           max(EPS, relT), f"atmosphere {m} collapsed spectrum")
        bd = res.dtaus(m)
        rd = rel(bd[1:], dtaus[1:])
        assert rd <= max(1e-10, 2 * o["dt_floor"]), f"atmosphere {m}: dtaus {rd:.3e}"
        assert np.all(bd[0] == 1.0)
        worst = dict(spec=max(worst["spec"], rel(res[m].spectrum.flux, spec.flux)),
                     T=max(worst["T"], relT), dtaus=max(worst["dtaus"], rd))
        # Milne on the batch's own dtaus, through the single grid: the same bits
        t_m = gr.effective_temperature_milne(res[m].spectrum, bd, res[m].final_T)
        assert t_m == res[m].T_milne, (m, t_m, res[m].T_milne)
        assert res[m].T_planck == fa.effective_temperature_planck(gr, res[m].spectrum)
        assert res[m].T_eff == float(np.mean([res[m].T_milne, res[m].T_planck]))
        assert gr.effective_temperature(res[m].spectrum, bd, res[m].final_T) == res[m].T_eff
        assert 900.0 < res[m].T_milne < 1800.0
        gr._close_engine()
    print("worst batch-vs-single difference:", worst)


def test_shared_premix_route():
    """Route (b): three KGrids on one premixed KTable, different g and init temperatures."""
    case = M.forest_pair()
    xs = {n: CrossSection(case[k], case["T_nodes"], case["p"], case["wl"], n)
          for n, k in (("one", "xsec1"), ("two", "xsec2"))}
    mix = np.array(M.FOREST_MIX)[:, None, None]
    grids = []
    for grav, dT in zip(GRAVITIES[:3], (0.0, 60.0, -40.0)):
        pl = fa.Planet.from_hot_jupiter()
        pl.g = grav
        gr = KGrid(pl, case["wl_bins"], n_g=8, pressures=case["p"],
                   init_temperatures=case["T"] + dT)
        if grids:
            gr.opacities, gr.mmr = grids[0].opacities, grids[0].mmr
        else:
            gr.load_opacities(cross_sections=xs, mix=mix)
        grids.append(gr)
    out = batched_k_spectra(grids, n_timesteps=N_STEPS)
    g0 = grids[0]
    table, _ = R.kdist_ref(case["xsec"], case["T_nodes"], case["p"], case["wl"], case["wl_bins"],
                           g0.g, case["T_nodes"], case["p"])
    for m, gr in enumerate(grids):
        o = oracle_run(table.reshape(table.shape[:2] + (-1,)), case["p"], case["T_nodes"],
                       g0.col_lam, g0.col_weights, gr.planet.g, gr.init_temperatures)
        spec, T, th, _ = gr.emission_spectrum(n_timesteps=N_STEPS)
        gr._close_engine()
        bs, bT, it = out[m]
        assert it == th.shape[1] // 2 == o["it"]
        for what, (s, t) in (("batch", (bs.flux, bT)), ("single", (spec.flux, T))):
            relT = rel(t, o["T"])
            assert relT <= max(1e-10, 2 * o["T_floor"]), f"{what} {m}: T {relT:.3e}"
            assert_flux_parity(s, g0.collapse(o["spec"]), g0.collapse(o["cond"]),
                               max(EPS, relT), f"{what} {m} collapsed spectrum")
        print(f"premix atmosphere {m}: batch vs single T {rel(bT, T):.3e}, spectrum "
              f"{rel(bs.flux, spec.flux):.3e}")


# ------------------------------------------------------------------------------ 5. post
def apply_ref(inst, x):
    off = np.concatenate([[0], np.cumsum(inst.count)])
    return np.array([np.sum(inst.weights[off[k]:off[k + 1]] * x[a:a + n]) /
                     np.sum(inst.weights[off[k]:off[k + 1]])
                     for k, (a, n) in enumerate(zip(inst.first, inst.count))])


def test_post_processing_of_a_kbatch_result(forest):
    res, eng, g0 = forest["res"], forest["res"].engine, forest["grids"][0]
    lam, A = g0.lam, len(res)
    T = np.array([r.final_T for r in res])
    pl = g0.planet
    radii = np.array([level_radii(T[m], eng.p_bar, float(eng.g[m]), eng.m_bar, pl.R_p, None)
                      for m in range(A)])
    depth = res.transmission()
    assert depth.shape == (A, lam.size)
    assert same_bits(depth, g0.collapse(eng.transit(radii, pl.R_star)))
    flux, inten = res.emergent(want_intensity=True)
    f_col, i_col = eng.emergent(T, want_intensity=True)
    assert same_bits(flux, g0.collapse(f_col)) and same_bits(inten, i_col)
    assert same_bits(res.emergent(), flux) and inten.shape[-1] == g0.col_lam.size
    assert res.contribution(1).shape == res.dtaus(1).shape == (eng.n_layers, g0.col_lam.size)
    # observe on the columns against the NumPy restatement on the downloaded columns
    inst = fa.Instrument.top_hat(lam, [2.5, 2.6, 2.8], [2.72, 2.9, 3.0])
    cols_inst = inst.for_columns(g0.n_g, g0.weights)
    cols = eng._last_spectra
    want = np.array([apply_ref(cols_inst, cols[m]) for m in range(A)])
    obs = res.observe(inst, kind="flux")
    assert obs.shape == (A, 3) and rel(obs, want) <= 1e-13
    band = np.array([apply_ref(inst, res[m].spectrum.flux) for m in range(A)])
    assert rel(obs, band) <= 1e-12          # the band value of the collapsed spectrum
    # (data of the other sign: obs - data cancels nothing, so chi2 inherits obs' bound)
    data, sigma = -want[0], np.abs(want[0])
    obs2, chi2 = res.observe(inst, kind="flux", data=data, sigma=sigma)
    assert same_bits(obs2, obs)
    assert rel(chi2, np.sum(((want - data) / sigma) ** 2, axis=1)) <= 1e-13
    ecl = res.observe(inst)                  # eclipse depths: positive and small
    assert ecl.shape == (A, 3) and np.all((ecl > 0) & (ecl < 1))
    # a 1-axis model grid interpolates the collapsed spectra
    mg = res.model_grid([np.arange(float(A))])
    got = mg.interpolate(np.array([[1.5], [3.0]]))
    s = np.array([r.spectrum.flux for r in res])
    assert rel(got[0], 0.5 * s[1] + 0.5 * s[2]) <= 1e-13 and rel(got[1], s[3]) <= 1e-15
    with pytest.raises(ValueError, match="no line positions"):
        res.cross_correlate(None)
    # set_mix + rerun on the same context: atmosphere 0 takes atmosphere 1's composition
    ctx = eng._ctx.value
    old = [(r.spectrum.flux.copy(), r.final_T.copy()) for r in res]
    res.set_mix(np.array(COMPS[1])[None, :, None, None], atm=[0])
    res.rerun()
    assert eng._ctx.value == ctx
    assert same_bits(res[1].spectrum.flux, old[1][0]) and same_bits(res[1].final_T, old[1][1])
    assert not same_bits(res[0].spectrum.flux, old[0][0])
    res.set_mix(np.array(COMPS[0])[None, :, None, None], atm=[0])
    res.rerun()
    assert same_bits(res[0].spectrum.flux, old[0][0]) and same_bits(res[0].final_T, old[0][1])


# ------------------------------------------------------------------------------ 6. Milne
def test_milne_with_k_constant_in_g():
    rng = np.random.default_rng(91)
    n_g, nL = 8, 10
    g, w = gauss_g(n_g)
    bins = np.linspace(1.0, 4.0, 13)
    p = np.logspace(1, -5, nL)
    Tn = np.array([800.0, 2400.0])
    k = rng.lognormal(0.0, 1.0, (nL, 2, 12))
    pl = fa.Planet.from_hot_jupiter()
    kg = KGrid(pl, bins, g=g, weights=w, pressures=p)
    kg.load_opacities(ktables={"x": np.repeat(k[..., None], n_g, axis=-1)}, mix=np.ones((1, 1, 1)),
                      temperatures=Tn, overlap="random")
    gr = fa.Grid(pl, lam=kg.lam, pressures=p)
    gr.load_opacities(opacities={"x": fa.OpacityTable(k, p, Tn, kg.lam)}, mmr=np.ones((1, nL)))
    d_bin = np.vstack([np.ones(12), rng.lognormal(-1.0, 1.5, (nL - 1, 12))])
    dtaus = np.repeat(d_bin, n_g, axis=1)
    T = np.linspace(2000.0, 900.0, nL)
    spec = fa.Spectrum(rng.lognormal(10.0, 1.0, 12), kg.lam)
    got = kg.effective_temperature_milne(spec, dtaus, T)
    want = fa.effective_temperature_milne(gr, spec, np.ascontiguousarray(dtaus[:, ::n_g]), T)
    assert T.min() < got < T.max() and abs(got / want - 1.0) <= 1e-12
    assert kg.effective_temperature(spec, dtaus, T) == float(
        np.mean([got, fa.effective_temperature_planck(kg, spec)]))
    kg._close_engine()
    gr._close_engine()
    kg.klibrary.release()


# ------------------------------------------------------------------------------ 7. C errors
def test_c_level_argument_errors():
    c = small_case(4)
    klib, x = c["lib"], c["lib"].tables(c["x"]).x
    h = klib.handle()
    lam, qw, p = c["lam"], c["qw"], c["p"]
    lib, ctx = raw_context(lam, qw, p, 5)
    made = [ctx]

    def fails(rc, msg):
        err = lib.frei_last_error().decode()
        assert rc != 0 and msg in err, err

    tab = np.empty((6, 3, lam.size))
    fails(lib.frei_set_table_kmix_batch(None, h, N.dptr(x), 0), "null argument")
    fails(lib.frei_set_table_kmix_batch(ctx, None, N.dptr(x), 0), "null argument")
    fails(lib.frei_set_table_kmix_batch(ctx, h, None, 0), "null argument")
    fails(lib.frei_kmix_batch_update(None, 0, 1, N.dptr(x)), "null argument")
    fails(lib.frei_kmix_batch_update(ctx, 0, 1, None), "null argument")
    fails(lib.frei_get_table_batch(None, 0, N.dptr(tab)), "null argument")
    fails(lib.frei_get_table_batch(ctx, 0, None), "null argument")
    _, plain = raw_context(lam, qw, p, 1, batch=False)
    made.append(plain)
    fails(lib.frei_set_table_kmix_batch(plain, h, N.dptr(x), 0), "frei_ctx_create_batch")
    fails(lib.frei_get_table_batch(plain, 0, N.dptr(tab)), "frei_ctx_create_batch")
    _, two = raw_context(lam, qw, p, 5, n_species=2)
    made.append(two)
    fails(lib.frei_set_table_kmix_batch(two, h, N.dptr(x), 0), "n_species = 1")
    _, bare = raw_context(lam, qw, p, 5, grid=False)
    made.append(bare)
    fails(lib.frei_set_table_kmix_batch(bare, h, N.dptr(x), 0), "frei_set_grid")
    fails(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(x), 1),
          f"columns [1, {lam.size + 1}) lie outside the {lam.size}")
    fails(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(x), -1), "columns [-1,")
    bad = x.copy()
    bad[3, 1, 2, 0] = -0.25
    fails(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(bad), 0), "x[3][1][2][0] = -0.25")
    bad[2, 0, 1, 1] = np.inf                                    # the first offender is named
    fails(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(bad), 0), "x[2][0][1][1]")
    fails(lib.frei_kmix_batch_update(ctx, 0, 1, N.dptr(x)), "holds no k-mix batch")
    # a library with an unset slot
    g4, w4 = gauss_g(4)
    empty = ctypes.c_void_p()
    N.check(lib.frei_klib_create(ctypes.byref(empty), 0, 3, 6, 3, 5, 4, N.dptr(N.f64(WL5)),
                                 N.dptr(N.f64(g4)), N.dptr(N.f64(w4)), N.dptr(N.f64(P6)),
                                 N.dptr(N.f64(T3))))
    N.check(lib.frei_klib_set(empty, 0, N.dptr(N.f64(c["Ks"][0]))))
    fails(lib.frei_set_table_kmix_batch(ctx, empty, N.dptr(x), 0), "slot 1 holds no table")
    assert lib.frei_klib_destroy(empty) == 0
    if N.device_count() > 1:
        other = KLibrary({f"s{k}": t for k, t in enumerate(c["Ks"])}, WL5, g4, w4, T3, P6, device=1)
        fails(lib.frei_set_table_kmix_batch(ctx, other.handle(), N.dptr(x), 0),
              "the library lives on device 1, the context on device 0")
        other.release()
    # a chemistry batch refuses the k-mix, and the reverse
    Tc, pc = N.f64([500.0, 3000.0]), N.f64(np.array([1e-6, 1e2]) * K.BAR)
    chem = N.f64(np.full((1, 1, 2, 2), 0.5))
    atm = np.zeros(5, dtype=np.int32)
    atm_p = atm.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    N.check(lib.frei_set_chemistry_batch(ctx, N.dptr(chem), 1, atm_p, N.dptr(Tc), 2, N.dptr(pc), 2))
    fails(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(x), 0), "chemistry tables")
    N.check(lib.frei_set_chemistry_batch(ctx, None, 0, None, None, 0, None, 0))
    # now it works, and the context refuses what does not fit a k-mix batch
    N.check(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(x), 0))
    fails(lib.frei_set_chemistry_batch(ctx, N.dptr(chem), 1, atm_p, N.dptr(Tc), 2, N.dptr(pc), 2),
          "k-mix batch")
    mmr = N.f64(np.ones((5, 1, 4)))
    assert lib.frei_set_mmr(ctx, N.dptr(mmr)) == 0
    mmr[2, 0, 3] = 0.5
    fails(lib.frei_set_mmr(ctx, N.dptr(mmr)), "the compositions hold the mixing ratios")
    assert "mmr[11] = 0.5" in lib.frei_last_error().decode()
    for lo, n in ((-1, 1), (0, 0), (4, 2), (5, 1)):
        fails(lib.frei_kmix_batch_update(ctx, lo, n, N.dptr(x)),
              f"atmospheres [{lo}, {lo + n}) lie outside [0, n_atm = 5)")
    fails(lib.frei_kmix_batch_update(ctx, 1, 4, N.dptr(bad)), "x[2][0][1][1]")
    fails(lib.frei_get_table_batch(ctx, 5, N.dptr(tab)), "atmosphere 5 lies outside [0, n_atm = 5)")
    fails(lib.frei_get_table_batch(ctx, -1, N.dptr(tab)), "atmosphere -1")
    # a NaN in a row that a layer uses names the atmosphere; the context then goes on working
    nan_lib = KLibrary({f"s{k}": t.copy() for k, t in enumerate(c["Ks"])}, WL5, g4, w4, T3, P6)
    nan_lib.sources["s1"][USED[1], 0, 2, 1] = -1.0          # a negative k: NaN after the fold
    _, nctx = raw_context(lam, qw, p, 5)
    made.append(nctx)
    zero = x.copy()
    zero[:, 0] = 0.0                    # without species 0 the negative value is the smallest pair
    fails(lib.frei_set_table_kmix_batch(nctx, nan_lib.handle(), N.dptr(zero), 0),
          "the mixed table of atmosphere 0 holds a NaN")
    nan_lib.release()
    # context and library both go on working after all of this
    want = klib.mix(c["x"]).reshape(5, 6, 3, -1)
    N.check(lib.frei_kmix_batch_update(ctx, 1, 2, N.dptr(N.f64(x[3:5]))))
    N.check(lib.frei_get_table_batch(ctx, 2, N.dptr(tab)))
    assert same_bits(tab[USED], want[4][USED])
    N.check(lib.frei_get_table_batch(ctx, 0, N.dptr(tab)))
    assert same_bits(tab[USED], want[0][USED])
    T0 = N.f64(np.broadcast_to(c["T0"], (5, 4)))
    n_iter = (ctypes.c_int * 5)()
    Tf, sp = np.empty((5, 4)), np.empty((5, lam.size))
    N.check(lib.frei_run_batch(ctx, N.dptr(T0), 2, 2, 3.0, 1.0, n_iter, N.dptr(Tf), N.dptr(sp)))
    assert np.all(np.isfinite(sp)) and list(n_iter) == [2] * 5
    for cx in made:
        assert lib.frei_ctx_destroy(cx) == 0
    klib.release()
