"""K18 without a GPU: the NumPy restatement (tests/kdist_ref.py) against a brute-force per-bin
loop, the quadrature and column layout of KGrid, its refusals, and the seeded line-forest case
run through the oracle alone with its numbers asserted (tests/test_gpu_kdist.py holds the device
to the same case).
"""
import math

import numpy as np
import pytest

import frei_amd as fa
from frei_amd import constants as K
from frei_amd.binning import CrossSection, bin_counts
from frei_amd.kdist import KGrid, gauss_g
from tests import kdist_ref as R

PLANET = dict(T_star=5800.0, a_rstar=K.A_RSTAR_HOT_JUPITER, g=K.G_JUPITER,
              m_bar=K.M_BAR_HOT_JUPITER)


def brute_kdist(row, wl, wl_bins, g):
    """One row, bin by bin in plain Python: membership by comparison, sorted() with NaN last,
    the plan and the sample in Python floats."""
    out = np.full((len(wl_bins) - 1, len(g)), np.nan)
    for k in range(len(wl_bins) - 1):
        last = k == len(wl_bins) - 2
        vals = [float(v) for v, x in zip(row, wl)
                if wl_bins[k] < x and (x < wl_bins[k + 1] if last else x <= wl_bins[k + 1])]
        vals = [0.0 if v == 0 else v for v in vals]
        s = sorted(v for v in vals if not math.isnan(v)) + [v for v in vals if math.isnan(v)]
        n = len(s)
        for q, gq in enumerate(g):
            if n == 0:
                continue
            if n == 1:
                out[k, q] = s[0]
                continue
            t = gq * n - 0.5
            j = int(min(max(math.floor(t), 0), n - 2))
            f = min(max(t - j, 0.0), 1.0)
            d = s[j + 1] - s[j] if not (math.isinf(s[j + 1]) and math.isinf(s[j])) else math.nan
            out[k, q] = s[j] + f * d
    return out


def test_restatement_matches_brute_force():
    rng = np.random.default_rng(3)
    wl = np.sort(rng.uniform(1.0, 2.0, 400))
    wl_bins = np.array([0.9, 1.0 + 1e-9, 1.2, 1.2000001, 1.5, wl[300], 2.5])   # an edge on a point
    x = rng.lognormal(0.0, 2.0, (2, 1, 400)).astype(np.float32)
    x[0, 0, 10:40] = 0.5            # ties
    x[0, 0, 50] = -0.0
    x[0, 0, 51] = 0.0
    x[1, 0, 120] = np.nan
    x[1, 0, 350] = np.inf
    g = np.array([0.5, 0.01, 0.999, 0.3, 0.77])
    got, counts = R.kdist_ref(x, [1000.0, 2000.0], [1.0], wl, wl_bins, g, [900.0, 2100.0], [1.0])
    start, end = R.O.bin_ranges(wl, wl_bins)
    assert np.array_equal(counts, end - start) and np.array_equal(counts, bin_counts(wl, wl_bins))
    assert 0 in counts and counts.sum() == 400
    for t in range(2):
        want = brute_kdist(x[t, 0], wl, wl_bins, g)
        assert np.array_equal(got[0, t], want, equal_nan=True)
        assert np.array_equal(np.signbit(got[0, t]), np.signbit(want))
    assert np.isnan(got[0, 1]).any() and np.isinf(got[0, 1]).any()


def test_restatement_edges():
    g = np.array([0.2, 0.9])
    j, f = R.kdist_plan(2, g)                       # t = -0.1, 1.3: clamped to the one interval
    assert list(j) == [0, 0] and list(f) == [0.0, 1.0]
    j, f = R.kdist_plan(5, np.array([0.5]))         # t = 2: exactly s_2
    assert list(j) == [2] and list(f) == [0.0]
    rows = np.array([[3.0, -0.0, 1.0, np.nan, 2.0]], dtype=np.float32)
    k = R.kdist_rows(rows, [0, 0, 4, 1], [5, 3, 5, 1], np.array([0.5, 0.1]))
    assert k[0, 0, 0] == 2.0 and k[0, 0, 1] == 0.0 and not np.signbit(k[0, 0, 1])   # NaN last
    assert k[0, 1, 0] == 1.0                        # 3 points: the median
    assert np.array_equal(k[0, 2], [2.0, 2.0])      # 1 point
    assert np.isnan(k[0, 3]).all()                  # no point


def test_mix_restatement():
    a = np.array([[[1.0, 2.0, 0.0, np.inf]]], dtype=np.float32)
    b = np.array([[[0.5, 0.0, 0.0, 1.0]]], dtype=np.float32)
    out = R.mix_ref([a, b], [[[0.1]], [[0.3]]])
    assert out.dtype == np.float32
    assert out[0, 0, 0] == np.float32(0.1 * 1.0 + 0.3 * 0.5) and out[0, 0, 2] == 0
    assert np.isinf(out[0, 0, 3])


@pytest.mark.parametrize("n", [1, 4, 16])
def test_gauss_g_sums(n):
    g, w = gauss_g(n)
    assert g.shape == w.shape == (n,) and np.all((g > 0) & (g < 1)) and np.all(np.diff(g) > 0)
    assert abs(w.sum() - 1) < 1e-14 and abs((w * g).sum() - 0.5) < 1e-14


def test_gauss_g_split():
    g, w = gauss_g(8, split=0.9)
    assert g.size == 8 and np.all(np.diff(g) > 0) and np.all(g[:4] < 0.9) and np.all(g[4:] > 0.9)
    assert abs(w.sum() - 1) < 1e-14 and abs(w[:4].sum() - 0.9) < 1e-14
    assert abs((w * g ** 3).sum() - 0.25) < 1e-13       # exact for a cubic on each part
    with pytest.raises(ValueError):
        gauss_g(7, split=0.9)
    with pytest.raises(ValueError):
        gauss_g(8, split=1.0)


def _kgrid(**kw):
    return KGrid(fa.Planet.from_hot_jupiter(), np.array([1.0, 1.5, 2.5, 3.0]), n_layers=6, **kw)


def test_kgrid_layout_and_collapse():
    g, w = gauss_g(4)
    grid = _kgrid(n_g=4)
    assert grid.n_bins == 3 and grid.n_g == 4
    assert np.array_equal(grid.lam, [1.25, 2.0, 2.75])
    assert np.array_equal(grid.wl_bins, [1.0, 1.5, 2.5, 3.0])
    assert np.array_equal(grid.col_lam, np.repeat(grid.lam, 4))
    want = np.array([(d * K.UM) * wq for d in (0.5, 1.0, 0.5) for wq in w])
    assert np.array_equal(grid.col_weights, want)
    assert abs(grid.col_weights.sum() - 2.0 * K.UM) < 1e-18
    x = np.arange(24.0).reshape(2, 12) ** 2
    c = grid.collapse(x)
    assert c.shape == (2, 3)
    for m in range(2):
        for b in range(3):
            acc = 0.0
            for q in range(4):
                acc = acc + w[q] * x[m, b * 4 + q]
            assert c[m, b] == acc
    assert np.allclose(grid.collapse(np.ones(12)), 1.0, rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        grid.collapse(np.ones(11))
    own = KGrid(fa.Planet.from_hot_jupiter(), [1.0, 2.0, 3.0, 4.0], g=[0.25, 0.75],
                weights=[0.5, 0.5], n_layers=6)
    assert own.n_g == 2 and np.array_equal(own.col_lam, [1.5, 1.5, 2.5, 2.5, 3.5, 3.5])
    with pytest.raises(ValueError):
        KGrid(fa.Planet.from_hot_jupiter(), [1.0, 2.0, 3.0, 4.0], g=[0.5], n_layers=6)


def _xs(wl, name):
    T, p = np.array([1000.0, 2000.0]), np.array([1e-3, 1.0])
    return CrossSection(np.ones((2, 2, wl.size), dtype=np.float32), T, p, wl, name)


def test_kgrid_refuses_species_without_mix():
    wl = np.linspace(1.01, 2.99, 50)
    grid = _kgrid()
    with pytest.raises(ValueError, match="mix="):
        grid.load_opacities(cross_sections={"1H2-16O": _xs(wl, "1H2-16O"),
                                            "12C-16O": _xs(wl, "12C-16O")})
    assert grid.opacities is None


def test_kgrid_refuses_empty_bins():
    wl = np.linspace(1.6, 2.4, 50)       # bins 0 and 2 hold no point
    grid = _kgrid()
    with pytest.raises(ValueError, match=r"bins 0, 2 hold no point"):
        grid.load_opacities(cross_sections={"1H2-16O": _xs(wl, "1H2-16O")})
    assert grid.opacities is None


def test_kgrid_refusals_for_now():
    grid = _kgrid()
    with pytest.raises(NotImplementedError, match="KGrid"):
        fa.effective_temperature_milne(grid, None, None, None)
    with pytest.raises(NotImplementedError, match="quad_weights"):
        fa.batched_emission_spectra([grid, grid])


@pytest.fixture(scope="module")
def forest():
    case = R.forest_case()
    nat = R.oracle_top_flux(R.native_table(case), case["wl"], case, PLANET)
    nat.setflags(write=False)
    return case, nat


def _worst(x, ref):
    return float(np.max(np.abs(x / ref - 1.0)))


def test_forest_case_through_the_oracle(forest):
    """The worst relative error over the 8 bins of the band-mean F_up[top] against the native
    axis, after emit -> absorb -> emit at fixed T: mean opacity 0.570, 16 sampled points 0.0611,
    k-distribution with 4 / 8 / 16 Gauss points 1.03e-2 / 6.3e-3 / 1.9e-3."""
    case, nat = forest
    ref = R.band_mean(nat)
    lam_c = (case["wl_bins"][:-1] + case["wl_bins"][1:]) / 2
    e_mean = _worst(R.oracle_top_flux(R.mean_table(case), lam_c, case, PLANET), ref)
    cols = R.sampled_columns()
    e_samp = _worst(R.band_mean(R.oracle_top_flux(R.native_table(case)[:, :, cols],
                                                  case["wl"][cols], case, PLANET)), ref)
    e_k = {}
    for n_g in (4, 8, 16):
        g, w = gauss_g(n_g)
        k, counts = R.kdist_ref(case["xsec"], case["T_nodes"], case["p"], case["wl"],
                                case["wl_bins"], g, case["T_nodes"], case["p"])
        assert np.array_equal(counts, np.full(8, 512))
        f = R.oracle_top_flux(k.reshape(k.shape[:2] + (-1,)), np.repeat(lam_c, n_g), case, PLANET)
        e_k[n_g] = _worst((f.reshape(8, n_g) * w).sum(axis=-1), ref)
    print("mean", e_mean, "sampled", e_samp, "k", e_k)
    assert abs(e_mean - 0.570) < 5e-3
    assert abs(e_samp - 0.0611) < 5e-4
    assert abs(e_k[4] - 1.03e-2) < 1e-4
    assert abs(e_k[8] - 6.3e-3) < 1e-4
    assert abs(e_k[16] - 1.9e-3) < 1e-4
    # the bars the device run is held to
    assert e_k[16] <= 1e-2 and e_k[16] <= e_samp / 10 and e_mean > 0.1
