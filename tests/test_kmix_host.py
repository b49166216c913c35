"""K19 without a GPU: the NumPy restatement (tests/kmix_ref.py) held to the properties of the
definition in include/frei_hip.h — conservation of the weighted log-mean, monotone output, the
one-species and zero-abundance limits, the (v, e) order of ties, where zero, negative and NaN
values land — the two-species line-forest case through the oracle alone, and every argument
error of the Python layer that needs no device (tests/test_gpu_kmix.py holds the device to the
restatement).
"""
from fractions import Fraction
import math

import numpy as np
import pytest

import frei_amd as fa
from frei_amd import constants as K
from frei_amd.binning import CrossSection, KLibrary, MixedKTable, fixed_point_weights
from frei_amd.kdist import KGrid, gauss_g
from tests import kdist_ref as R
from tests import kmix_ref as M

PLANET = dict(T_star=5800.0, a_rstar=K.A_RSTAR_HOT_JUPITER, g=K.G_JUPITER,
              m_bar=K.M_BAR_HOT_JUPITER)
N_G = [1, 2, 8, 12, 16, 64]


def quad(n_g):
    return gauss_g(n_g) if n_g > 1 else (np.array([0.5]), np.array([1.0]))


def test_fixed_point_weights():
    for n_g in N_G:
        w = quad(n_g)[1]
        W = M.fixed_weights(w)
        assert W == [int(x) for x in fixed_point_weights(w)]
        assert min(W) >= 1 and abs(sum(W) - 2 ** 30) <= n_g and sum(W) <= 2 ** 31
        E = M.intervals(W)
        assert E[0] == 0 and E[-1] == sum(W) ** 2 < 2 ** 62
        assert [E[q + 1] - E[q] for q in range(n_g)] == [x * sum(W) for x in W]


@pytest.mark.parametrize("n_g", N_G)
def test_conservation(n_g):
    """Every fold keeps sum_q W_q ln a'[q] / Wt = sum_e u_e ln v_e / Wt^2 to
    (n_g^2 + 4) 2^-52 max(1, max |ln v|); both sides summed exactly (Fractions) from the float64
    logarithms.  Worst measured over these cases: 2.6e-16, against bounds of 1.1e-15 to
    1.3e-11."""
    rng = np.random.default_rng(100 + n_g)
    W = M.fixed_weights(quad(n_g)[1])
    Wt = sum(W)
    a = rng.lognormal(-3.0, 4.0, n_g)               # neither a nor b monotone
    worst = 0.0
    for step in range(3):
        b = rng.lognormal(-3.0, 4.0, n_g) * 10.0 ** rng.uniform(-6, 2)
        out, st = M.fold(a, b, W)
        lhs = sum(Fraction(W[q]) * Fraction(math.log(out[q])) for q in range(n_g)) / Wt
        rhs = sum(Fraction(st["u"][e]) * Fraction(float(st["lnv"][e]))
                  for e in range(n_g * n_g)) / (Wt * Wt)
        err, bound = abs(float(lhs - rhs)), M.step_bound(n_g, M.ln_max(st["v"]))
        print(n_g, step, err, bound)
        assert err <= bound
        worst = max(worst, err)
        a = out
    assert worst < 1e-13


@pytest.mark.parametrize("n_g", N_G)
def test_monotone_output_for_monotone_inputs(n_g):
    rng = np.random.default_rng(200 + n_g)
    W = M.fixed_weights(quad(n_g)[1])
    a = np.sort(rng.lognormal(0.0, 3.0, n_g))
    b = np.sort(rng.lognormal(0.0, 3.0, n_g))
    out, st = M.fold(a, b, W)
    assert np.all(np.diff(out) >= 0) and np.all(np.isfinite(out))
    # a geometric mean over the interval: inside the range of the pairs it overlaps
    for q in range(n_g):
        vs = [st["v"][e] for e, _ in st["parts"][q]]
        assert min(vs) * (1 - 1e-12) <= out[q] <= max(vs) * (1 + 1e-12)
    assert a[0] + b[0] <= out[0] * (1 + 1e-12) and out[-1] <= (a[-1] + b[-1]) * (1 + 1e-12)


@pytest.mark.parametrize("n_g", N_G)
def test_one_species_and_zero_abundance(n_g):
    rng = np.random.default_rng(300 + n_g)
    w = quad(n_g)[1]
    K0 = np.sort(rng.lognormal(0.0, 3.0, (2, 2, 3, n_g)), axis=-1)
    K0[0, 0, 0, : n_g // 2] = K0[0, 0, 0, 0]         # ties stay in their intervals
    K1 = rng.lognormal(0.0, 3.0, (2, 2, 3, n_g))
    x0 = rng.uniform(0.1, 1.0, (1, 2, 2))
    one, _ = M.kmix_ref(K0[None], x0, w)
    assert np.array_equal(one, x0[0][:, :, None, None] * K0)      # no log, no exp
    got, lnmax = M.kmix_ref(np.stack([K0, K1]), np.array([1.0, 0.0])[:, None, None], w)
    bound = np.array([[[M.step_bound(n_g, v) for v in r] for r in pl] for pl in lnmax])
    rel = np.abs(got / K0 - 1.0)
    print(n_g, rel.max(), bound.min())
    assert np.all(rel <= bound[..., None])


def test_ties_follow_the_v_e_order():
    W = M.fixed_weights([0.25, 0.5, 0.25])
    out, st = M.fold([1.0, 1.0, 3.0], [2.0, 2.0, 0.0], W)
    # v = [3, 3, 1, 3, 3, 1, 5, 5, 3]: the 1s first, then the 3s by e, then the 5s
    assert list(st["v"]) == [3, 3, 1, 3, 3, 1, 5, 5, 3]
    assert st["order"] == [2, 5, 0, 1, 3, 4, 8, 6, 7]
    q = 2 ** 28                                         # W = [q, 2q, q], Wt = 4q
    assert W == [q, 2 * q, q] and st["u"] == [q * q * f for f in (1, 2, 1, 2, 4, 2, 1, 2, 1)]
    # cumulative weights 1, 3 | 4 | 6, 8, 12 | 13, 14, 16 (units of q^2): intervals 4, 12, 16
    assert st["parts"][0] == [(2, q * q), (5, 2 * q * q), (0, q * q)]
    assert st["parts"][1] == [(1, 2 * q * q), (3, 2 * q * q), (4, 4 * q * q)]
    assert st["parts"][2] == [(8, q * q), (6, q * q), (7, 2 * q * q)]
    want = [math.exp((3 * math.log(1.0) + math.log(3.0)) / 4), 3.0,
            math.exp((math.log(3.0) + 3 * math.log(5.0)) / 4)]
    assert np.allclose(out, want, rtol=1e-15, atol=0)
    # -0 compares as +0: the order of equal zeros is e's
    _, st = M.fold([0.0, -0.0], [-0.0, 0.0], M.fixed_weights([0.5, 0.5]))
    assert st["order"] == [0, 1, 2, 3]
    # neither input is assumed monotone
    _, st = M.fold([5.0, 1.0], [2.0, 0.5], M.fixed_weights([0.5, 0.5]))
    assert st["order"] == [3, 2, 1, 0]


def test_zero_negative_and_nan_values():
    W = M.fixed_weights([0.25, 0.25, 0.25, 0.25])
    # one zero pair (a[0] + b[0]): 1/16 of the weight, inside interval 0 alone
    out, _ = M.fold([0.0, 1.0, 2.0, 3.0], [0.0, 1.0, 2.0, 3.0], W)
    assert out[0] == 0.0 and np.all(out[1:] > 0) and np.all(np.isfinite(out))
    # negative pairs sort first: a[0] = -5 makes 4 pairs negative, exactly interval 0
    out, _ = M.fold([-5.0, 1.0, 2.0, 3.0], [0.5, 1.0, 1.5, 2.0], W)
    assert np.isnan(out[0]) and np.all(np.isfinite(out[1:]))
    # one negative pair: interval 0 alone
    out, _ = M.fold([-1.0, 1.0, 2.0, 3.0], [0.5, 2.0, 2.5, 3.0], W)
    assert np.isnan(out[0]) and np.all(np.isfinite(out[1:]))
    # NaN sorts last: b[2] = NaN makes 4 pairs NaN, exactly the last interval
    out, st = M.fold([1.0, 2.0, 3.0, 4.0], [0.5, 1.0, np.nan, 2.0], W)
    assert np.all(np.isfinite(out[:3])) and np.isnan(out[3])
    assert [e for e in st["order"][-4:]] == [2, 6, 10, 14]
    # a NaN in a[] from an earlier fold: its 4 pairs, the last interval again
    out, _ = M.fold([np.nan, 2.0, 3.0, 4.0], [0.5, 1.0, 1.5, 2.0], W)
    assert np.all(np.isfinite(out[:3])) and np.isnan(out[3])
    # uneven weights: a NaN pair of weight 0.01 reaches the last interval only
    W = M.fixed_weights([0.1, 0.9])
    out, _ = M.fold([np.nan, 1.0], [1.0, 2.0], W)
    assert np.isfinite(out[0]) and np.isnan(out[1])


# ------------------------------------------------------------------------------ physics
def _worst(x, ref):
    return float(np.max(np.abs(x / ref - 1.0)))


def test_forest_pair_through_the_oracle():
    """Two species' forests mixed 0.6 : 0.4, 16 Gauss points; the worst relative error over the
    8 bins of the band-mean F_up[top] after emit -> absorb -> emit against the native-axis run of
    the true mixture: (a) random overlap of the species' k-tables 3.94e-2, (b) the premixed
    k-table 3.3e-3, (c) the species' k summed at equal g 0.132.  Asserted: (a) < (c) and
    (b) < (c)."""
    case = M.forest_pair()
    n_g = 16
    g, w = gauss_g(n_g)
    ref = R.band_mean(R.oracle_top_flux(R.native_table(case), case["wl"], case, PLANET))
    lam_c = (case["wl_bins"][:-1] + case["wl_bins"][1:]) / 2

    def err(table):
        f = R.oracle_top_flux(table.reshape(table.shape[:2] + (-1,)), np.repeat(lam_c, n_g),
                              case, PLANET)
        return _worst((f.reshape(8, n_g) * w).sum(axis=-1), ref)

    Ks = M.species_tables(case, g)
    x = np.array(M.FOREST_MIX)[:, None, None]
    random_overlap, _ = M.kmix_ref(Ks, x, w)
    premixed, _ = R.kdist_ref(case["xsec"], case["T_nodes"], case["p"], case["wl"],
                              case["wl_bins"], g, case["T_nodes"], case["p"])
    summed = M.FOREST_MIX[0] * Ks[0] + M.FOREST_MIX[1] * Ks[1]
    e_a, e_b, e_c = err(random_overlap), err(premixed), err(summed)
    print("random overlap", e_a, "premixed", e_b, "summed at equal g", e_c)
    assert e_a < e_c
    assert e_b < e_c


# ------------------------------------------------------------------------------ Python layer
WL3 = np.array([1.0, 1.5, 2.5, 3.0])
T2, P2 = np.array([1000.0, 2000.0]), np.array([1e-3, 1.0])


def _tables(n_g=4, names=("a", "b")):
    rng = np.random.default_rng(7)
    return {n: np.sort(rng.lognormal(0.0, 1.0, (2, 2, 3, n_g)), axis=-1) for n in names}


def _lib(n_g=4, **kw):
    g, w = gauss_g(n_g)
    args = dict(tables=_tables(n_g), wl_bins=WL3, g=g, weights=w, temperatures=T2, pressures=P2)
    args.update(kw)
    return KLibrary(**args)


def test_klibrary_layout():
    lib = _lib()
    assert lib.names == ["a", "b"] and lib.n_src == 2 and lib.shape == (2, 2, 3, 4)
    assert lib.resident_bytes == 2 * 48 * 8
    assert np.array_equal(lib.wavelength, np.repeat([1.25, 2.0, 2.75], 4))
    x = np.array([[[0.1, 0.2], [0.3, 0.4]], [[0.5, 0.6], [0.7, 0.8]]])      # (n_src, n_T, n_p)
    xc, batched = lib.composition(x)
    assert not batched and xc.shape == (1, 2, 2, 2) and xc.flags["C_CONTIGUOUS"]
    assert np.array_equal(xc[0], x.transpose(0, 2, 1))                     # [n_src][n_p][n_T]
    xc, batched = lib.composition(np.array([0.25, 0.75])[:, None, None])    # broadcast
    assert not batched and np.array_equal(xc[0, 1], np.full((2, 2), 0.75))
    xc, batched = lib.composition(np.ones((5, 2, 1, 1)))
    assert batched and xc.shape == (5, 2, 2, 2)
    tab = lib.table(x)
    assert isinstance(tab, MixedKTable) and tab.shape == (2, 2, 12) and tab.n_bins == 3
    assert tab.dims == ("pressure", "temperature", "wavelength")
    assert np.array_equal(tab.pressure, P2) and np.array_equal(tab.temperature, T2)
    assert np.array_equal(tab.wavelength, lib.wavelength) and tab.x.shape == (2, 2, 2)
    assert fa.KLibrary is KLibrary and fa.MixedKTable is MixedKTable


def test_klibrary_argument_errors():
    g, w = gauss_g(4)
    with pytest.raises(ValueError, match="tables="):
        _lib(tables={})
    with pytest.raises(ValueError, match="wl_bins"):
        _lib(wl_bins=[1.0, 2.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="one length"):
        _lib(weights=w[:3])
    with pytest.raises(ValueError, match=r"n_g = 65"):
        _lib(g=np.linspace(0.01, 0.99, 65), weights=np.full(65, 1 / 65))
    with pytest.raises(ValueError, match=r"g\[2\]"):
        _lib(g=[0.1, 0.5, 0.4, 0.9])
    with pytest.raises(ValueError, match=r"g\[3\]"):
        _lib(g=[0.1, 0.2, 0.3, 1.0])
    with pytest.raises(ValueError, match=r"g\[0\]"):
        _lib(g=[np.nan, 0.2, 0.3, 0.4])
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        _lib(weights=[0.5, -0.1, 0.3, 0.3])
    with pytest.raises(ValueError, match=r"weights\[2\]"):
        _lib(weights=[0.5, 0.2, np.inf, 0.3])
    with pytest.raises(ValueError, match=r"weights\[3\].*2\^-30"):
        _lib(weights=[0.5, 0.3, 0.2, 1e-10])
    with pytest.raises(ValueError, match=r"weights\[2\] sum to more than 2"):
        _lib(weights=[0.9, 0.9, 0.9, 0.1])
    with pytest.raises(ValueError, match=r"table 'b' has shape \(2, 2, 3, 5\)"):
        _lib(tables={"a": _tables()["a"], "b": np.ones((2, 2, 3, 5))})
    lib = _lib()
    with pytest.raises(ValueError, match="does not broadcast"):
        lib.mix(np.ones((3, 2, 2)))
    with pytest.raises(ValueError, match="5 axes"):
        lib.mix(np.ones((1, 1, 2, 2, 2)))
    x = np.ones((2, 2, 2))
    x[1, 0, 1] = -1e-3
    with pytest.raises(ValueError, match=r"x\[0\]\[1\]\[0\]\[1\] = -0.001 .*'b'"):
        lib.mix(x)
    x[1, 0, 1] = np.nan
    with pytest.raises(ValueError, match=r"x\[0\]\[1\]\[0\]\[1\]"):
        lib.table(x)
    with pytest.raises(ValueError, match="one composition"):
        lib.table(np.ones((2, 2, 2, 2)))
    assert lib._handle is None          # nothing reached the device


def _kgrid(**kw):
    return KGrid(fa.Planet.from_hot_jupiter(), WL3, n_layers=6, n_g=4, **kw)


def test_kgrid_random_overlap_without_a_device():
    grid = _kgrid()
    p = grid.pressures
    rng = np.random.default_rng(9)
    kt = {n: np.sort(rng.lognormal(0.0, 1.0, (p.size, 2, 3, 4)), axis=-1) for n in ("a", "b")}
    mix = np.array([0.7, 0.3])[:, None, None]
    with pytest.raises(ValueError, match="set_mix needs"):
        grid.set_mix(mix)
    with pytest.raises(ValueError, match="overlap must be"):
        grid.load_opacities(ktables=kt, temperatures=T2, mix=mix, overlap="correlated")
    with pytest.raises(ValueError, match="overlap='random'"):
        grid.load_opacities(ktables=kt, temperatures=T2, mix=mix)            # premix: no ktables
    with pytest.raises(ValueError, match="needs mix="):
        grid.load_opacities(ktables=kt, temperatures=T2, overlap="random")
    with pytest.raises(ValueError, match="either cross_sections"):
        grid.load_opacities(mix=mix, overlap="random")
    with pytest.raises(ValueError, match="needs temperatures="):
        grid.load_opacities(ktables=kt, mix=mix, overlap="random")
    with pytest.raises(ValueError, match="neither mmr nor chemistry"):
        grid.load_opacities(ktables=kt, temperatures=T2, mix=mix, mmr=np.ones((1, 6)),
                            overlap="random")
    with pytest.raises(ValueError, match="must be finite and >= 0"):
        grid.load_opacities(ktables=kt, temperatures=T2, mix=-mix, overlap="random")
    wl = np.linspace(1.6, 2.4, 50)       # bins 0 and 2 hold no point
    xs = {n: CrossSection(np.ones((2, 2, 50), dtype=np.float32), T2, P2, wl, n)
          for n in ("1H2-16O", "12C-16O")}
    with pytest.raises(ValueError, match=r"bins 0, 2 hold no point"):
        grid.load_opacities(cross_sections=xs, mix=mix, overlap="random")
    assert grid.opacities is None and grid.klibrary is None
    out = grid.load_opacities(ktables=kt, temperatures=T2, mix=mix, overlap="random")
    assert list(out) == ["mix"] and isinstance(out["mix"], MixedKTable)
    assert grid.klibrary.names == ["a", "b"] and np.array_equal(grid.mmr, np.ones((1, 6)))
    assert np.array_equal(out["mix"].x[1], np.full((6, 2), 0.3))
    lib = grid.klibrary
    again = grid.set_mix(np.array([0.2, 0.8])[:, None, None])
    assert grid.klibrary is lib and again["mix"].library is lib
    assert np.array_equal(again["mix"].x[0], np.full((6, 2), 0.2))
    assert lib._handle is None
