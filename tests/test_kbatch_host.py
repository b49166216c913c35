"""K20 without a GPU: Instrument.for_columns against collapse-then-apply (both restated in
NumPy), the Milne definition on k-columns, and every validation of KLibrary.tables,
KGrid.load_opacities(klibrary=), BatchEngine's k-mix arguments, batched_k_spectra and
KBatchResult that is raised before any device use (tests/test_gpu_kbatch.py holds the device).
"""
import numpy as np
import pytest

import frei_amd as fa
from frei_amd import constants as K
from frei_amd.batch import BatchRecord, check_kmix
from frei_amd.binning import KLibrary, MixedKTables
from frei_amd.core import collapse_columns, milne_on_columns
from frei_amd.kdist import KBatchResult, KGrid, batched_k_spectra, gauss_g

WL3 = np.array([1.0, 1.5, 2.5, 3.0])


def apply_ref(first, count, weights, x, num=None, den=None):
    """frei_obs_apply restated: obs[k] = sum_t w x num / sum_t w den over channel k's points."""
    off = np.concatenate([[0], np.cumsum(count)])
    out = np.empty(len(first))
    for k, (a, n) in enumerate(zip(first, count)):
        w = weights[off[k]:off[k + 1]]
        sl = slice(a, a + n)
        top = w * x[sl] * (1.0 if num is None else num[sl])
        bot = w * (1.0 if den is None else den[sl])
        out[k] = np.sum(top) / np.sum(bot)
    return out


# ------------------------------------------------------------------------------ for_columns
@pytest.mark.parametrize("n_g", [2, 8, 16])
def test_for_columns_equals_collapse_then_apply(n_g):
    """Random positive columns, overlapping channels in any order, per-wavelength num and den:
    the expanded plan on the columns against the plan on the collapsed spectrum.  Both are sums of
    about n_g * count positive terms in another order: 1e-13 relative."""
    rng = np.random.default_rng(7 + n_g)
    n_bins = 40
    lam = np.sort(rng.uniform(1.0, 5.0, n_bins))
    first = np.array([5, 0, 17, 12])
    count = np.array([20, 9, 23, 1])
    weights = rng.uniform(0.1, 2.0, count.sum())
    inst = fa.Instrument(lam, first, count, weights)
    g, w = gauss_g(n_g)
    cols = inst.for_columns(n_g, w)
    assert inst._handle is None and cols._handle is None          # host plan construction only
    assert np.array_equal(cols.lam, np.repeat(lam, n_g))
    assert np.array_equal(cols.first, first * n_g) and np.array_equal(cols.count, count * n_g)
    assert cols.weights.size == count.sum() * n_g
    x = rng.lognormal(0.0, 1.5, n_bins * n_g)
    num, den = rng.uniform(0.5, 2.0, n_bins), rng.uniform(0.5, 2.0, n_bins)
    for nm, dn in ((None, None), (num, None), (None, den), (num, den)):
        want = apply_ref(first, count, weights, collapse_columns(x, w), nm, dn)
        got = apply_ref(cols.first, cols.count, cols.weights, x,
                        None if nm is None else np.repeat(nm, n_g),
                        None if dn is None else np.repeat(dn, n_g))
        # (the expanded denominator carries sum_q w_q = 1 to n_g roundings)
        rel = np.max(np.abs(got / want - 1.0))
        print(n_g, nm is not None, dn is not None, rel)
        assert rel <= 1e-13


def test_for_columns_is_exact_for_one_point():
    rng = np.random.default_rng(3)
    lam = np.linspace(1.0, 2.0, 12)
    inst = fa.Instrument(lam, [2, 0], [5, 12], rng.uniform(0.1, 1.0, 17))
    cols = inst.for_columns(1, [1.0])
    assert np.array_equal(cols.first, inst.first) and np.array_equal(cols.count, inst.count)
    assert np.array_equal(cols.weights, inst.weights) and np.array_equal(cols.lam, inst.lam)
    x = rng.lognormal(0.0, 1.0, 12)
    assert np.array_equal(apply_ref(cols.first, cols.count, cols.weights, x),
                          apply_ref(inst.first, inst.count, inst.weights, x))
    with pytest.raises(ValueError, match="n_g = 4"):
        inst.for_columns(4, [0.5, 0.5])
    with pytest.raises(ValueError, match="finite and positive"):
        inst.for_columns(2, [0.5, 0.0])


# ------------------------------------------------------------------------------ Milne
def milne_bins_ref(p_milne, flux, lam_um, p, T):
    """The reference's formula (core.py:386-405) on an axis of bins."""
    return np.interp(np.average(p_milne, weights=flux * (lam_um * K.UM)), p[::-1], T[::-1])


def test_milne_on_identical_columns_is_the_formula_on_the_bins():
    """Every g-column of a bin equal: p_b = p (sum_q w_q), and sum_q w_q = 1 to n_g roundings."""
    rng = np.random.default_rng(11)
    n_bins, n_g = 30, 8
    g, w = gauss_g(n_g)
    p = np.logspace(2, -5, 20)
    T = np.linspace(2200.0, 700.0, 20)
    lam = np.linspace(1.0, 5.0, n_bins)
    pm = 10.0 ** rng.uniform(-3, 1, n_bins)
    flux = rng.lognormal(10.0, 1.0, n_bins)
    got = milne_on_columns(np.repeat(pm, n_g), flux, lam, w, p, T)
    want = milne_bins_ref(pm, flux, lam, p, T)
    assert abs(got / want - 1.0) <= 1e-12
    # and the definition itself, on columns that differ, restated with explicit loops
    pmc = 10.0 ** rng.uniform(-3, 1, n_bins * n_g)
    p_b = np.array([sum(w[q] * pmc[b * n_g + q] for q in range(n_g)) for b in range(n_bins)])
    assert milne_on_columns(pmc, flux, lam, w, p, T) == milne_bins_ref(p_b, flux, lam, p, T)


# ------------------------------------------------------------------------------ validation
def _library(n_g=4, n_src=2, p=None, device=0):
    g, w = gauss_g(n_g)
    p = np.logspace(0, -3, 4) if p is None else p
    rng = np.random.default_rng(5)
    tabs = {f"s{k}": np.sort(rng.lognormal(0.0, 1.0, (p.size, 2, 3, n_g)), axis=-1)
            for k in range(n_src)}
    return KLibrary(tabs, WL3, g, w, np.array([1000.0, 2000.0]), p, device)


def _grid(lib, mix=(0.5, 0.5), n_g=4, **kw):
    kw.setdefault("pressures", np.logspace(0, -3, 4))
    grid = KGrid(fa.Planet.from_hot_jupiter(), WL3, n_g=n_g, **kw)
    if lib is not None:
        grid.load_opacities(klibrary=lib, mix=np.array(mix)[:, None, None])
    return grid


def test_tables_validation():
    lib = _library()
    x = np.full((3, 2, 2, 4), 0.5)
    tabs = lib.tables(x)
    assert isinstance(tabs, MixedKTables) and tabs.n_comp == 3 and tabs.x.shape == (3, 2, 4, 2)
    assert tabs.library is lib and np.array_equal(tabs[1].x, tabs.x[1])
    with pytest.raises(ValueError, match="n_comp, n_src, n_T, n_p"):
        lib.tables(x[0])
    with pytest.raises(ValueError, match="does not broadcast"):
        lib.tables(np.ones((3, 3, 2, 4)))
    bad = x.copy()
    bad[2, 1, 0, 3] = -1e-3
    with pytest.raises(ValueError, match=r"x\[2\]\[1\]\[0\]\[3\] = -0.001.*'s1'"):
        lib.tables(bad)
    bad[1, 0, 1, 0] = np.nan
    with pytest.raises(ValueError, match=r"x\[1\]\[0\]\[1\]\[0\]"):
        lib.tables(bad)
    assert lib._handle is None


def test_batch_engine_kmix_arguments():
    lib = _library()
    tabs = lib.tables(np.full((3, 2, 2, 4), 0.5))
    args = dict(n_atm=3, n_lam=12, n_layers=4, device=0)
    assert check_kmix({"mix": tabs}, None, **args) is tabs
    assert check_kmix({"mix": tabs}, np.ones((3, 1, 4)), **args) is tabs
    assert check_kmix({"h2o": np.ones((4, 2, 12))}, None, **args) is None
    with pytest.raises(ValueError, match="3 compositions for n_atm = 2"):
        check_kmix({"mix": tabs}, None, **dict(args, n_atm=2))
    with pytest.raises(ValueError, match="do not add"):
        check_kmix({"mix": tabs, "h2o": np.ones((4, 2, 12))}, None, **args)
    with pytest.raises(ValueError, match="None or all ones"):
        check_kmix({"mix": tabs}, np.full((1, 4), 0.5), **args)
    with pytest.raises(ValueError, match="columns"):
        check_kmix({"mix": tabs}, None, **dict(args, n_lam=11))
    with pytest.raises(ValueError, match="device 0, the engine on device 1"):
        check_kmix({"mix": tabs}, None, **dict(args, device=1))
    with pytest.raises(ValueError, match="do not add"):      # raised before the context exists
        fa.BatchEngine(np.repeat([1.25, 2.0, 2.75], 4), np.logspace(0, -3, 4),
                       {"mix": tabs, "b": tabs}, np.full(3, 1e3))
    assert lib._handle is None


def test_attach_library_validation():
    lib = _library()
    grid = _grid(lib, mix=(0.2, 0.8))
    assert grid.klibrary is lib and list(grid.opacities) == ["mix"]
    assert np.array_equal(grid.mix, np.array([0.2, 0.8])[:, None, None])
    assert np.array_equal(grid.mmr, np.ones((1, 4)))
    grid.set_mix(np.array([0.3, 0.7])[:, None, None])
    assert grid.mix[1, 0, 0] == 0.7
    other = _grid(lib)
    assert other.klibrary is grid.klibrary
    with pytest.raises(ValueError, match="needs mix="):
        _grid(None).load_opacities(klibrary=lib)
    with pytest.raises(ValueError, match="the library's g are not the grid's"):
        _grid(None, n_g=8).load_opacities(klibrary=lib, mix=np.ones((2, 1, 1)))
    with pytest.raises(ValueError, match="layer 1 .* does not sit on a pressure node"):
        _grid(None, pressures=np.array([1.0, 0.2, 0.01, 0.001])).load_opacities(
            klibrary=lib, mix=np.ones((2, 1, 1)))
    with pytest.raises(ValueError, match="device"):
        _grid(None, device=1).load_opacities(klibrary=lib, mix=np.ones((2, 1, 1)))
    with pytest.raises(ValueError, match="neither"):
        _grid(None).load_opacities(klibrary=lib, mix=np.ones((2, 1, 1)), ktables={"a": 1})
    assert lib._handle is None


def test_batched_k_spectra_validation():
    lib = _library()
    a, b = _grid(lib, (0.5, 0.5)), _grid(lib, (0.1, 0.9))
    with pytest.raises(ValueError, match="grid 1 has no opacities"):
        batched_k_spectra([a, _grid(None)])
    with pytest.raises(ValueError, match="grid 1 does not share grid 0's g"):
        batched_k_spectra([a, _grid(_library(n_g=8), n_g=8)])
    with pytest.raises(ValueError, match="grid 1 does not share grid 0's klibrary object"):
        batched_k_spectra([a, _grid(_library())])
    with pytest.raises(ValueError, match="grid 1 does not share grid 0's pressures"):
        p = np.logspace(0, -3, 4) * 2
        batched_k_spectra([a, _grid(_library(p=p), pressures=p)])
    with pytest.raises(ValueError, match="grid 1 is not a KGrid"):
        batched_k_spectra([a, fa.Grid(fa.Planet.from_hot_jupiter(), lam=a.lam, n_layers=4)])
    pl = fa.Planet.from_hot_jupiter()
    pl.alpha = 0.5
    with pytest.raises(ValueError, match="alpha"):
        batched_k_spectra([a, _planet_grid(lib, pl)])
    c = _grid(None)
    c.load_opacities(ktables={"x": np.ones((4, 2, 3, 4))}, mix=np.ones((1, 1, 1)),
                     temperatures=[1000.0, 2000.0], overlap="random")
    c.opacities = {"mix": c.opacities["mix"], "more": c.opacities["mix"]}
    with pytest.raises(ValueError, match="one klibrary object .* or one opacity dict"):
        batched_k_spectra([a, c])
    with pytest.raises(ValueError, match="at least one"):
        batched_k_spectra([])
    assert lib._handle is None and a._engine is None and b._engine is None


def _planet_grid(lib, planet):
    grid = KGrid(planet, WL3, n_g=4, pressures=np.logspace(0, -3, 4))
    grid.load_opacities(klibrary=lib, mix=np.ones((2, 1, 1)))
    return grid


def test_kbatch_result_refusals_need_no_device():
    lam = np.array([1.25, 2.0, 2.75])
    g, w = gauss_g(4)
    rec = BatchRecord(fa.Spectrum(np.ones(3), lam), np.ones(4), 1, None, 0.0, 0.0, 0.0)

    class NoDevice:            # any use of the engine is an AttributeError
        pass
    pl = fa.Planet.from_hot_jupiter()
    res = KBatchResult([rec, rec], NoDevice(), [pl, pl], lam, w)
    inst = fa.Instrument.top_hat(lam, [1.0], [3.0])
    with pytest.raises(ValueError, match="no line positions: cross_correlate"):
        res.cross_correlate(None)
    with pytest.raises(ValueError, match="phase curves on the columns"):
        res.phase_curve(None)
    with pytest.raises(ValueError, match="no line positions: broadening="):
        res.observe(inst, kind="flux", broadening=object())
    with pytest.raises(ValueError, match="no line positions: broadening="):
        res.model_grid([np.array([0.0, 1.0])], broadening=object())
    with pytest.raises(ValueError, match="must be an Instrument on lam"):
        res.observe(fa.Instrument.top_hat(np.repeat(lam, 4) + np.arange(12) * 1e-9, [1.0], [3.0]),
                    kind="flux")
    with pytest.raises(ValueError, match="no run to repeat"):
        res.rerun()
    assert inst._handle is None
    assert np.array_equal(res.collapse(np.ones((2, 12))), collapse_columns(np.ones((2, 12)), w))


def test_old_entry_points_still_refuse_kgrids():
    grid = _grid(None)
    with pytest.raises(NotImplementedError, match="KGrid.effective_temperature_milne"):
        fa.effective_temperature_milne(grid, None, None, None)
    with pytest.raises(NotImplementedError, match="batched_k_spectra"):
        fa.effective_temperature_milne(grid, None, None, None)
    with pytest.raises(NotImplementedError, match="quad_weights.*batched_k_spectra"):
        fa.batched_emission_spectra([grid, grid])
    for name in ("batched_k_spectra", "KBatchResult", "MixedKTables"):
        assert name in fa.__all__ and hasattr(fa, name)
