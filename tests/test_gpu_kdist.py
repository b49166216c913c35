"""K18 on the GPU: frei_xsec_mix and frei_xsec_kdist bitwise against the NumPy restatement
(tests/kdist_ref.py), the two kernel forms against each other, the independence properties, the
device path into an Engine, the unchanged default weights, and the seeded line-forest case
(figures through the oracle alone: tests/test_kdist_host.py).
"""
import numpy as np
import pytest

import frei_amd as fa
from frei_amd import constants as K
from frei_amd.binning import CrossSection, KTable
from frei_amd.engine import ABSORB, EMIT, Engine, trapz_weights
from frei_amd.kdist import KGrid, gauss_g
from tests import kdist_ref as R

pytestmark = pytest.mark.gpu

PLANET = dict(T_star=5800.0, a_rstar=K.A_RSTAR_HOT_JUPITER, g=K.G_JUPITER,
              m_bar=K.M_BAR_HOT_JUPITER)


def same_bits(a, b):
    return (np.array_equal(a, b, equal_nan=True) and
            np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b)))


# ------------------------------------------------------------------------------ mix
@pytest.fixture(scope="module")
def mix_case():
    rng = np.random.default_rng(21)
    T, p = np.array([900.0, 1500.0]), np.array([1e-3, 0.1, 10.0])
    wl = np.sort(rng.uniform(1.0, 2.0, 1000))
    vals = [rng.lognormal(0.0, 3.0, (2, 3, 1000)).astype(np.float32) for _ in range(3)]
    vals[0][:, :, 100:140] = 0.0
    vals[1][0, 1, 120] = 0.0
    vals[2][1, 2, 777] = np.inf
    w = rng.uniform(0.0, 1e-2, (3, 2, 3))
    w[1, 0, 0] = 0.0
    xs = [CrossSection(v, T, p, wl, f"s{k}") for k, v in enumerate(vals)]
    return dict(T=T, p=p, wl=wl, vals=vals, w=w, xs=xs)


def test_mix_bitwise(mix_case):
    c = mix_case
    mixed = CrossSection.mix(c["xs"], c["w"])
    assert mixed.opacity is None and mixed.isotopologue == "mix"
    got, want = mixed.values(), R.mix_ref(c["vals"], c["w"])
    assert got.dtype == np.float32 and same_bits(got, want)
    assert np.isinf(got[1, 2, 777]) and np.all(got[:, :, 100:140][c["vals"][1][:, :, 100:140] == 0]
                                               >= 0)
    # broadcast weights, one source: a scaled copy
    one = CrossSection.mix(c["xs"][:1], 0.25)
    assert same_bits(one.values(), R.mix_ref(c["vals"][:1], 0.25))
    # an ordinary cross-section: K6 bins it
    bins = np.linspace(1.0, 2.0, 6)
    lam = (bins[:-1] + bins[1:]) / 2
    ref = CrossSection(want, c["T"], c["p"], c["wl"])
    assert same_bits(mixed.bin(bins, lam, c["T"], c["p"]), ref.bin(bins, lam, c["T"], c["p"]))


def test_mix_errors(mix_case):
    c = mix_case
    other_T = CrossSection(c["vals"][0], np.array([900.0, 1600.0]), c["p"], c["wl"])
    with pytest.raises(RuntimeError, match=r"source 2 differs from source 0 at T_nodes\[1\]"):
        CrossSection.mix([c["xs"][0], c["xs"][1], other_T], c["w"])
    wl2 = c["wl"].copy()
    wl2[5] += 1e-9
    other_wl = CrossSection(c["vals"][0], c["T"], c["p"], wl2)
    with pytest.raises(RuntimeError, match=r"source 1 differs from source 0 at wl_hi\[5\]"):
        CrossSection.mix([c["xs"][0], other_wl], c["w"][:2])
    w = c["w"].copy()
    w[1, 1, 2] = -1e-3
    with pytest.raises(RuntimeError, match=r"weight\[1\]\[1\]\[2\]"):
        CrossSection.mix(c["xs"], w)
    w[1, 1, 2] = np.nan
    with pytest.raises(RuntimeError, match=r"weight\[1\]\[1\]\[2\]"):
        CrossSection.mix(c["xs"], w)
    with pytest.raises(ValueError):
        CrossSection.mix([], 1.0)
    assert same_bits(CrossSection.mix(c["xs"], c["w"]).values(), R.mix_ref(c["vals"], c["w"]))


# ------------------------------------------------------------------------------ k-dist
COUNTS = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 32768]
SRC_T, SRC_P = np.array([1000.0, 2000.0]), np.array([1e-2, 1.0])


def axis_for(counts):
    """An axis whose bins (k, k + 1] hold counts[k] points (none on an edge), and the edges."""
    wl = np.concatenate([k + (np.arange(n) + 0.5) / n for k, n in enumerate(counts)] + [[]])
    return wl, np.arange(len(counts) + 1.0)


@pytest.fixture(scope="module")
def kd_case():
    rng = np.random.default_rng(22)
    wl, bins = axis_for(COUNTS)
    assert wl.size == sum(COUNTS) and np.all(np.diff(wl) > 0)
    x = rng.lognormal(0.0, 2.0, (2, 2, wl.size)).astype(np.float32)
    first = np.concatenate([[0], np.cumsum(COUNTS)])
    for k, n in enumerate(COUNTS):      # runs of ties, zeros, a -0, one NaN, one inf
        if n >= 63:
            a = first[k]
            x[:, :, a + 5:a + 5 + n // 4] = x[:, :, a + 5:a + 6]
            x[0, :, a + 1] = 0.0
            x[0, 0, a + 2] = -0.0
    x[1, 1, first[7] + 100] = np.nan
    x[1, 0, first[12] + 9] = np.inf
    x[0, 1, first[3]] = -0.0            # in the 3-point bin
    x[1, 0, first[2]] = np.nan          # and where every g reaches them: the 2-point bin
    x[0, 0, first[1]] = np.inf          # and the 1-point bin
    x.setflags(write=False)
    xs = CrossSection(x, SRC_T, SRC_P, wl)
    return dict(wl=wl, bins=bins, x=x, xs=xs)


@pytest.mark.parametrize("n_g", [1, 8, 20])
def test_kdist_matches_restatement(kd_case, n_g):
    c = kd_case
    g = gauss_g(n_g)[0] if n_g > 1 else np.array([0.5])
    if n_g == 20:
        g = g[::-1].copy()              # any order
    T_t, p_t = np.array([1900.0, 900.0]), np.array([2.0, 1e-3])     # all four source rows
    got, counts = c["xs"].kdist(c["bins"], g, T_t, p_t)
    want, wcounts = R.kdist_ref(c["x"], SRC_T, SRC_P, c["wl"], c["bins"], g, T_t, p_t)
    assert np.array_equal(counts, COUNTS) and np.array_equal(wcounts, COUNTS)
    assert got.shape == (2, 2, len(COUNTS), n_g)
    assert same_bits(got, want)
    assert np.isnan(got[:, :, 0]).all() and np.isnan(got[:, :, 2]).any()
    assert np.isinf(got[:, :, 1]).any() and not np.isnan(got[:, :, 8:12]).any()
    if n_g == 20:                       # the last point of the 255-point bin is reached
        assert np.isnan(got[:, :, 7]).any()
    tab = KTable(c["xs"], c["bins"], g, T_t, p_t)
    assert np.array_equal(tab.counts, COUNTS)
    assert tab.shape == (2, 2, len(COUNTS) * n_g) and same_bits(tab.values, want.reshape(tab.shape))


def test_forms_give_the_same_bits(kd_case, monkeypatch):
    """Bins of at most 64 points, which both forms can take, through each form."""
    c = kd_case
    # the bins of 0 .. 64 points, the 65-point bin in halves, the 255-point bin in runs of 32
    fine = np.concatenate([np.linspace(0.0, 6.0, 7), [6.5, 7.0],
                           7.0 + np.arange(1, 8) * (32.0 / 255), [8.0]])
    g = gauss_g(8)[0]
    out = {}
    for form in ("wave", "block", "auto"):
        monkeypatch.setenv("FREI_KDIST_FORM", form)
        out[form], counts = c["xs"].kdist(fine, g, SRC_T, SRC_P)
        assert counts.max() <= 64 and counts.min() == 0 and 64 in counts and 32 in counts
    want, _ = R.kdist_ref(c["x"], SRC_T, SRC_P, c["wl"], fine, g, SRC_T, SRC_P)
    for form in out:
        assert same_bits(out[form], want), form
    monkeypatch.setenv("FREI_KDIST_FORM", "wave")
    with pytest.raises(RuntimeError, match=r"bin 6 holds 65 points"):
        c["xs"].kdist(c["bins"][:8], g, SRC_T, SRC_P)
    monkeypatch.setenv("FREI_KDIST_FORM", "sideways")
    with pytest.raises(RuntimeError, match="FREI_KDIST_FORM"):
        c["xs"].kdist(fine, g, SRC_T, SRC_P)


def test_large_bin_is_refused_and_the_library_goes_on():
    wl, bins = axis_for([5, 32769, 7])
    x = np.random.default_rng(23).uniform(0.0, 1.0, (1, 1, wl.size)).astype(np.float32)
    xs = CrossSection(x, [1000.0], [1.0], wl)
    g = gauss_g(4)[0]
    with pytest.raises(RuntimeError, match=r"bin 1 holds 32769 points"):
        xs.kdist(bins, g, [1000.0], [1.0])
    for bad in ([0.5, 1.0], [0.0], [np.nan]):
        with pytest.raises(RuntimeError, match=r"g\[\d\]"):
            xs.kdist(bins, bad, [1000.0], [1.0])
    with pytest.raises(RuntimeError, match="n_g"):
        xs.kdist(bins, np.linspace(0.01, 0.99, 65), [1000.0], [1.0])
    half = np.array([0.0, 1.0, 1.5, 2.0, 3.0])
    got, counts = xs.kdist(half, g, [1000.0], [1.0])
    want, _ = R.kdist_ref(x, [1000.0], [1.0], wl, half, g, [1000.0], [1.0])
    assert counts.max() <= 32768 and same_bits(got, want)


def test_independence(kd_case):
    c = kd_case
    g = gauss_g(8)[0]
    T_t, p_t = np.array([900.0, 1100.0, 1900.0]), np.array([1e-3, 2.0])
    whole, _ = c["xs"].kdist(c["bins"], g, T_t, p_t)
    # a bin's values do not change when bins are removed or added
    part, _ = c["xs"].kdist(c["bins"][3:9], g, T_t, p_t)
    assert same_bits(part, whole[:, :, 3:8])
    more = np.concatenate([[-1.0, -0.5], c["bins"][9:13]])
    ext, _ = c["xs"].kdist(more, g, T_t, p_t)
    assert same_bits(ext[:, :, 2:5], whole[:, :, 9:12])
    # targets that select one source row get identical rows
    assert same_bits(whole[:, 0], whole[:, 1]) and not same_bits(whole[:, 0], whole[:, 2])
    # the row chosen is the one CrossSection.bin chooses: sources whose rows differ by a factor
    wl = c["wl"][:2000]
    base = np.random.default_rng(24).uniform(1.0, 2.0, wl.size).astype(np.float32)
    fac = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]], dtype=np.float32)
    src_T, src_p = np.array([2000.0, 1000.0]), np.array([1.0, 1e-4, 1e-2])    # unsorted nodes
    xs = CrossSection(fac[:, :, None] * base, src_T, src_p, wl)
    bins = np.array([3.0, 6.0, 7.0])
    T_q, p_q = np.array([1500.0, 1499.0, 1501.0, 5000.0]), np.array([1e-3, 0.1, 1e-5, 0.05])
    k, _ = xs.kdist(bins, np.array([0.5]), T_q, p_q)
    b = xs.bin(bins, (bins[:-1] + bins[1:]) / 2, T_q, p_q, groupies=True)
    assert np.array_equal(k[:, :, 1, 0] / k[0, 0, 1, 0], b[:, :, 1] / b[0, 0, 1])
    assert len(np.unique(k[:, :, 1, 0])) > 3


# ------------------------------------------------------------------------------ device path
def _sweeps(eng, T):
    out = []
    for d in (EMIT, ABSORB):
        eng.set_temperatures(T)
        dT, bol, _ = eng.sweep(d, want_dtaus=False)
        out += [dT, bol]
    return out + list(eng.get_fluxes())


def test_device_path_matches_host_table(kd_case):
    c = kd_case
    g = gauss_g(4)[0]
    bins = c["bins"][3:12]                      # 8 bins of 3 .. 1023 points
    p_bar = np.logspace(0.5, -3, 7)
    T = np.linspace(1700.0, 1100.0, 7)
    tab = KTable(c["xs"], bins, g, SRC_T, p_bar)
    n_col = tab.wavelength.size
    lam = 1.0 + tab.wavelength / 10.0
    w = np.full(n_col, 1e-6)
    mmr = np.full((1, 7), 1e-3)
    dev = Engine(lam, p_bar, {"x": tab}, mmr=mmr, quad_weights=w)
    host = Engine(lam, p_bar, {"x": fa.OpacityTable(tab.values, p_bar, SRC_T, lam)}, mmr=mmr,
                  quad_weights=w)
    a, b = _sweeps(dev, T), _sweeps(host, T)
    for u, v in zip(a, b):
        assert same_bits(u, v)
    assert np.all(np.isfinite(a[-2][1:])) and np.ptp(a[-2][-1]) > 0
    # a column slice against the slice of the whole run (fluxes are per column)
    lo, hi = 5, 30
    part = Engine(lam, p_bar, {"x": tab}, mmr=mmr, quad_weights=w, lam_slice=(lo, hi))
    fu, fd = _sweeps(part, T)[-2:]
    assert same_bits(fu, a[-2][:, lo:hi]) and same_bits(fd, a[-1][:, lo:hi])
    for e in (dev, host, part):
        e.close()


def test_default_weights_unchanged():
    lam = np.logspace(np.log10(0.6), np.log10(9.0), 300)
    p_bar = np.logspace(1, -4, 8)
    tabs = fa.load_example_opacity(fa.Grid(fa.Planet.from_hot_jupiter(), lam=lam,
                                           pressures=p_bar))
    T = np.linspace(2000.0, 1000.0, 8)
    outs = []
    for kw in ({}, {"quad_weights": trapz_weights(lam * K.UM)}):
        eng = Engine(lam, p_bar, tabs, **kw)
        eng.set_temperatures(T)
        dT, bol, _ = eng.sweep(EMIT, want_dtaus=False)
        outs.append((dT, bol))
        eng.close()
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    assert np.all(outs[0][1][1:, 0] > 0)    # F_2_up of every step
    with pytest.raises(ValueError, match="quad_weights"):
        Engine(lam, p_bar, tabs, quad_weights=np.ones(299))


# ------------------------------------------------------------------------------ physics
def _device_top_flux(eng, T):
    for d in (EMIT, ABSORB, EMIT):
        eng.set_temperatures(T)
        eng.sweep(d, want_dtaus=False)
    return eng.get_fluxes()[0][-1].copy()


def _worst(x, ref):
    return float(np.max(np.abs(x / ref - 1.0)))


@pytest.fixture(scope="module")
def forest():
    case = R.forest_case()
    xs = CrossSection(case["xsec"], case["T_nodes"], case["p"], case["wl"], "x")
    planet = fa.Planet.from_hot_jupiter()
    assert (planet.g, planet.m_bar, planet.a_rstar) == (PLANET["g"], PLANET["m_bar"],
                                                        PLANET["a_rstar"])
    one = np.ones((1, R.N_LAYERS))
    kw = dict(g=planet.g, m_bar=planet.m_bar, mmr=one)

    def native(cols):
        lam = case["wl"][cols]
        tab = fa.OpacityTable(R.native_table(case)[:, :, cols], case["p"], case["T_nodes"], lam)
        eng = Engine(lam, case["p"], {"x": tab}, F_toa=fa.F_TOA(lam), **kw)
        f = _device_top_flux(eng, case["T"])
        return eng, f

    eng_nat, nat = native(np.arange(R.N_HI))
    grid = KGrid(planet, case["wl_bins"], n_g=16, pressures=case["p"],
                 init_temperatures=case["T"])
    grid.load_opacities(cross_sections={"x": xs}, mmr=one)
    kflux = _device_top_flux(grid.engine(), case["T"])
    return dict(case=case, xs=xs, planet=planet, kw=kw, native=native, eng_nat=eng_nat, nat=nat,
                grid=grid, kflux=kflux)


def test_forest_case_on_the_device(forest):
    """Band-mean F_up[top] after emit -> absorb -> emit at fixed T, worst relative error over the
    8 bins against the native axis, both on the device (the oracle's figures: k-distribution with
    16 Gauss points 1.9e-3, 16 sampled points 0.0611, mean opacity 0.570).  Bars: at most 1e-2, at
    most a tenth of the sampled run's error, and the mean-opacity run's error above 0.1."""
    f = forest
    case, grid = f["case"], f["grid"]
    # each device run matches the oracle's run on the same tables
    o_nat = R.oracle_top_flux(R.native_table(case), case["wl"], case, PLANET)
    assert _worst(f["nat"], o_nat) <= 1e-10
    ktab = grid.opacities["x"]
    assert np.array_equal(ktab.temperature, case["T_nodes"]) and ktab.g.size == 16
    o_k = R.oracle_top_flux(ktab.values, grid.col_lam, case, PLANET)
    assert _worst(f["kflux"], o_k) <= 1e-10
    ref = R.band_mean(f["nat"])
    e_k = _worst(grid.collapse(f["kflux"]), ref)
    eng_s, samp = f["native"](R.sampled_columns())
    eng_s.close()
    e_samp = _worst(R.band_mean(samp), ref)
    tab = fa.OpacityTable(R.mean_table(case), case["p"], case["T_nodes"], grid.lam)
    eng_m = Engine(grid.lam, case["p"], {"x": tab}, F_toa=fa.F_TOA(grid.lam), **f["kw"])
    e_mean = _worst(_device_top_flux(eng_m, case["T"]), ref)
    eng_m.close()
    print("k-distribution", e_k, "sampled", e_samp, "mean opacity", e_mean)
    assert e_k <= 1e-2
    assert e_k <= e_samp / 10
    assert e_mean > 0.1


def test_forest_case_transmission(forest):
    """The collapsed transmission_spectrum against the native axis' band-mean transit depth on
    the same case, dtaus of an emit at the case's T: finite and within the k-run's own bound of
    1e-2.  Measured on the device: worst relative error over the 8 bins 4.4e-5."""
    f = forest
    case, grid, planet = f["case"], f["grid"], f["planet"]
    T = case["T"]
    from frei_amd.transit import level_radii
    radii = level_radii(T, case["p"], planet.g, planet.m_bar, planet.R_p, None)
    f["eng_nat"].set_temperatures(T)
    _, _, d_nat = f["eng_nat"].sweep(EMIT)
    depth_nat = R.band_mean(f["eng_nat"].transit(radii, planet.R_star, d_nat))
    eng = grid.engine()
    eng.set_temperatures(T)
    _, _, d_k = eng.sweep(EMIT)
    spec = grid.transmission_spectrum(T, dtaus=d_k)
    assert spec.flux.shape == (8,) and np.array_equal(spec.wavelength, grid.lam)
    assert np.all(np.isfinite(spec.flux))
    err = _worst(spec.flux, depth_nat)
    print("transit depth", err, spec.flux, depth_nat)
    assert err <= 1e-2
