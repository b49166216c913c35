"""GPU tests of the stellar-spectrum binning (K8, frei_stellar.hip) and of irradiating a planet
with the binned spectrum.

Tolerance of the binning (derived, not measured): kernel and checker form the same terms
(dx * 0.5) * (y[i+1] + y[i]) (no contraction), so only the order of the n_k - 1 additions of a
bin differs; any two orders agree within 2 max(n_k, 4) eps sum_i |term_i| / span
(tests/stellar_ref.py ``bound``) — relative 2 n_k eps for positive flux.  The NaN pattern
(bins of fewer than two points, poisoned bins) must match exactly."""
import numpy as np
import pytest

from oracle import frei_oracle as O
from tests import stellar_ref as SR
from tests.parity import assert_grid_parity, grid_floor, perturbed_exp, rel

pytestmark = pytest.mark.gpu

FORMS = [0, 1, 2]


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


# ------------------------------------------------------------------ reference-made fixture
@pytest.fixture(scope="module")
def fixture_case(golden):
    """Per fixture grid: edges, lam, the reference's output, the plan's counts and the bound
    (aligned and compacted like the reference's output)."""
    g = golden("stellar_bin.npz")
    wl, flux = g["wl"], g["flux"]
    cases = {}
    for name in ("a", "b"):
        wl_bins, lam = g[f"{name}_wl_bins"], g[f"{name}_lam"]
        n = SR.counts(wl, wl_bins)
        _, scale = SR.bin_aligned(wl, flux, wl_bins)
        tol = SR.bound(n, scale)
        cases[name] = dict(wl_bins=wl_bins, lam=lam, ref=g[f"{name}_out"], n=n, tol=tol,
                           tol_c=SR.compact_padded(tol, n, lam.size))
    return wl, flux, cases


@pytest.fixture(scope="module")
def fixture_library(fa, fixture_case):
    wl, flux, _ = fixture_case
    lib = fa.StellarSpectra(wl, flux)
    yield lib
    lib.release()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ["a", "b"])
def test_fixture_parity(fixture_library, fixture_case, name, form):
    """Both fixture grids, each form forced and automatic, against the reference's own values."""
    c = fixture_case[2][name]
    got, n = fixture_library.bin(c["wl_bins"], form=form, counts=True)
    assert np.array_equal(n, c["n"])
    # automatic: form 2 from 4 points per non-empty bin on (grid a: 69.9, grid b: 1.5)
    auto = 2 if n.sum() / (n > 0).sum() >= 4.0 else 1
    assert fixture_library.form_used == (form or auto)
    assert auto == dict(a=2, b=1)[name]
    assert np.array_equal(np.isnan(got), np.broadcast_to(n < 2, got.shape))
    SR.assert_binned(SR.compact_padded(got, n, c["lam"].size), c["ref"], c["tol_c"],
                     f"grid {name} form {form}")


@pytest.mark.parametrize("name", ["a", "b"])
def test_binned_stellar_spectrum_reproduces_the_reference_output(fa, fixture_case, name):
    """The reference-named function: compacted, shifted where the grid starts below the
    spectrum, zero-padded to len(lam)."""
    wl, flux, cases = fixture_case
    c = cases[name]
    got = fa.binned_stellar_spectrum(wl, flux[1], c["wl_bins"], c["lam"])
    assert got.shape == c["lam"].shape
    SR.assert_binned(got, c["ref"][1], c["tol_c"][1], f"grid {name} spectrum 1")
    n_empty = int((c["n"] == 0).sum())
    assert np.array_equal(got[got.size - n_empty:], np.zeros(n_empty))
    both = fa.binned_stellar_spectrum(wl, flux, c["wl_bins"], c["lam"])
    SR.assert_binned(both, c["ref"], c["tol_c"], f"grid {name} library")
    model = type("Model", (), dict(wavelength=wl, flux=flux[1]))()
    assert np.array_equal(fa.get_binned_phoenix_spectrum(4000.0, 1e4, c["wl_bins"], c["lam"],
                                                         spectrum=model), got, equal_nan=True)


def test_no_point_in_any_bin_is_refused(fa, fixture_case):
    wl, flux, _ = fixture_case
    with pytest.raises(ValueError, match="no point"):
        fa.binned_stellar_spectrum(wl, flux[0], np.array([7.0, 8.0, 9.0]), np.array([7.5, 8.5]))


# ------------------------------------------------------------------ edges
EDGE_COUNTS = [300, 0, 1, 64, 2, 63, 3, 65, 128, 129]
ON_UPPER_EDGE = {0, 3, 9}      # bins whose last point sits exactly on their upper edge
N_BELOW, N_ABOVE = 150, 298    # the last point below sits exactly on wl_bins[0]


@pytest.fixture(scope="module")
def edge_case():
    """One hand-built axis: bins of 0, 1, 2, 3, 63, 64, 65, 128, 129 and 300 points, a point on
    an interior edge (lower bin), on wl_bins[0] (dropped), on wl_bins[-1] (kept), points below
    and above the grid, n_hi = 1203 (no multiple of 64).  Five spectra: four positive, the
    last changes sign."""
    rng = np.random.default_rng(5)
    wl_bins = 1.0 + np.cumsum(np.concatenate([[0.0], rng.uniform(0.05, 0.2, len(EDGE_COUNTS))]))
    parts = [np.linspace(0.4, wl_bins[0], N_BELOW)]
    for k, n in enumerate(EDGE_COUNTS):
        lo, hi = wl_bins[k], wl_bins[k + 1]
        if k in ON_UPPER_EDGE:
            t = np.linspace(0.0, 1.0, n + 1)[1:] ** 1.3
        else:
            t = np.linspace(0.0, 1.0, n + 2)[1:-1] ** 1.3
        x = lo + (hi - lo) * t
        if k in ON_UPPER_EDGE:
            x[-1] = hi
        parts.append(x)
    parts.append(wl_bins[-1] + 0.002 * np.arange(1, N_ABOVE + 1))
    wl = np.concatenate(parts)
    assert wl.size == 1203 and wl.size % 64 != 0 and np.all(np.diff(wl) > 0)
    assert wl[N_BELOW - 1] == wl_bins[0] and wl_bins[1] in wl and wl_bins[-1] in wl
    flux = 1e6 * wl ** -2 * rng.lognormal(0.0, 0.7, (5, wl.size))
    flux[4] *= np.sin(40.0 * wl)
    n = SR.counts(wl, wl_bins)
    assert list(n) == EDGE_COUNTS
    ref, scale = SR.bin_aligned(wl, flux, wl_bins)
    # the same library with one flux value of spectrum 1 inside the 65-point bin made NaN
    k_bad = EDGE_COUNTS.index(65)
    i_bad = int(SR.plan(wl, wl_bins)[k_bad]) + 31
    flux_nan = flux.copy()
    flux_nan[1, i_bad] = np.nan
    ref_nan, _ = SR.bin_aligned(wl, flux_nan, wl_bins)
    poisoned = np.isnan(ref_nan) & ~np.isnan(ref)
    assert poisoned.sum() == 1 and poisoned[1, k_bad]
    return dict(wl=wl, wl_bins=wl_bins, flux=flux, n=n, ref=ref, tol=SR.bound(n, scale),
                flux_nan=flux_nan, ref_nan=ref_nan, poisoned=(1, k_bad))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n_spec", [1, 3, 5])
def test_edges(fa, edge_case, n_spec, form):
    e = edge_case
    lib = fa.StellarSpectra(e["wl"], e["flux"][:n_spec])
    try:
        got, n = lib.bin(e["wl_bins"], form=form, counts=True)
        used = lib.form_used
        again = lib.bin(e["wl_bins"], form=form)
    finally:
        lib.release()
    assert got.shape == (n_spec, len(EDGE_COUNTS))
    assert np.array_equal(n, e["n"])
    assert used == (form or 2)            # 83.9 points per non-empty bin
    assert got.tobytes() == again.tobytes(), "two runs of one form differ"
    SR.assert_binned(got, e["ref"][:n_spec], e["tol"][:n_spec], f"n_spec {n_spec} form {form}")
    assert np.array_equal(np.isnan(got), np.broadcast_to(e["n"] < 2, got.shape))


def _variant(e, kind):
    """Other edges on the edge axis, so that form 2 runs with each of its lane-group sizes
    (chosen from the mean points per non-empty bin: 4 below 12, 8 below 28, 16 below 53, 32
    below 300, else a whole wave; the 10 bins above have 83.9): "coarse" is two bins of 300 and
    753 points (526.5: whole waves); "+k" appends k bins of two points each above the grid
    (+10: 40.8, +40: 17.0, +149: 6.7)."""
    wl, wl_bins = e["wl"], e["wl_bins"]
    if kind == "coarse":
        edges = np.array([wl_bins[0], wl_bins[1], wl[-1]])
        want = [300, 753]
    else:
        k = int(kind)
        edges = np.concatenate([wl_bins, wl_bins[-1] + 0.004 * np.arange(1, k + 1) + 0.001])
        want = EDGE_COUNTS + [2] * k
    n = SR.counts(wl, edges)
    assert list(n) == want
    return edges, n


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", ["coarse", "+10", "+40", "+149"])
def test_edges_with_every_lane_group_size(fa, edge_case, kind, form):
    e = edge_case
    edges, n = _variant(e, kind)
    ref, scale = SR.bin_aligned(e["wl"], e["flux"], edges)
    lib = fa.StellarSpectra(e["wl"], e["flux"])
    try:
        got, counts = lib.bin(edges, form=form, counts=True)
        used = lib.form_used
        again = lib.bin(edges, form=form)
    finally:
        lib.release()
    assert np.array_equal(counts, n)
    assert used == (form or 2)            # every variant's mean is above 4 points per bin
    assert got.tobytes() == again.tobytes(), "two runs of one form differ"
    SR.assert_binned(got, ref, SR.bound(n, scale), f"edges {kind} form {form}")


def test_one_dimensional_library_gives_one_dimensional_result(fa, edge_case):
    e = edge_case
    lib = fa.StellarSpectra(e["wl"], e["flux"][2])
    try:
        got = lib.bin(e["wl_bins"])
        ms, calls = lib.timing()
    finally:
        lib.release()
    assert got.shape == (len(EDGE_COUNTS),)
    SR.assert_binned(got, e["ref"][2], e["tol"][2], "1-D library")
    assert calls == 1 and ms > 0.0


def test_a_refused_call_leaves_the_library_usable(fa):
    """2 spectra x 400 points onto 20 bins, then onto 7: a call the library refuses in between
    leaves the handle, its kept plan and result buffers and the device as they were."""
    rng = np.random.default_rng(20)
    wl = np.sort(rng.uniform(1.0, 2.0, 400))
    flux = 10 ** rng.uniform(3, 4, (2, 400))
    bins, fewer = np.linspace(1.0, 2.0, 21), np.linspace(1.1, 1.9, 8)
    lib = fa.StellarSpectra(wl, flux)
    try:
        good = lib.bin(bins)
        assert good.shape == (2, 20) and np.all(np.isfinite(good))
        with pytest.raises(RuntimeError, match="form"):
            lib.bin(bins, form=3)
        assert np.array_equal(lib.bin(bins), good)
        with pytest.raises(RuntimeError, match="ascending"):
            lib.bin(bins[::-1].copy())
        small = lib.bin(fewer)                  # the kept buffers, reused for a smaller plan
        with pytest.raises(RuntimeError, match="form"):
            lib.bin(fewer, form=-1)
        assert np.array_equal(lib.bin(fewer), small)
        assert np.array_equal(lib.bin(bins), good)
        assert lib.timing()[1] == 5
    finally:
        lib.release()


@pytest.mark.parametrize("form", [1, 2])
def test_nan_flux_poisons_exactly_its_bin(fa, edge_case, form):
    e = edge_case
    lib = fa.StellarSpectra(e["wl"], e["flux_nan"])
    try:
        got = lib.bin(e["wl_bins"], form=form)
    finally:
        lib.release()
    SR.assert_binned(got, e["ref_nan"], e["tol"], f"NaN flux, form {form}")
    extra = np.isnan(got) & ~np.isnan(e["ref"])
    assert extra.sum() == 1 and extra[e["poisoned"]]


# ------------------------------------------------------------------ irradiation
N_LAYERS, N_LAM = 8, 300


def _grid(fa, planet, op=None):
    """8 layers x 300 wavelengths over 0.5-5 µm (inside the fixture spectra's 0.3-5.5 µm)."""
    gr = fa.Grid(planet, lam_min=0.5, lam_max=5.0, n_wl_bins=N_LAM, n_layers=N_LAYERS,
                 T_ref=2400)
    gr.load_opacities(opacities=fa.load_example_opacity(gr, scale_factor=1) if op is None else op)
    return gr


@pytest.fixture(scope="module")
def binned_on_grid(fa, fixture_library):
    """The fixture's three spectra binned, aligned, onto the irradiation grid."""
    gr = fa.Grid(fa.Planet.from_hot_jupiter(), lam_min=0.5, lam_max=5.0, n_wl_bins=N_LAM,
                 n_layers=N_LAYERS)
    F = fixture_library.bin(gr.wl_bins)
    assert F.shape == (3, N_LAM) and np.all(np.isfinite(F)) and np.all(F > 0)
    return F


def test_blackbody_as_stellar_spectrum_is_bitwise_the_blackbody_planet(fa):
    plain = _grid(fa, fa.Planet.from_hot_jupiter())
    pl = fa.Planet.from_hot_jupiter()
    pl.stellar_spectrum = np.pi * fa.B_star(pl.T_star, plain.lam)
    star = _grid(fa, pl)
    try:
        a = plain.emission_spectrum(n_timesteps=3)
        b = star.emission_spectrum(n_timesteps=3)
    finally:
        plain._close_engine()
        star._close_engine()
    assert np.array_equal(a[0].flux, b[0].flux)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


def _oracle(gr, Ft, n_timesteps):
    op = gr.opacities["1H2-16O"]
    tabs = {"1H2-16O": O.Table(op.values, op.pressure, op.temperature)}
    pl = gr.planet

    def run():
        return O.emission_spectrum(tabs, gr.init_temperatures, gr.pressures, gr.lam, Ft, pl.g,
                                   pl.m_bar, pl.alpha, n_timesteps=n_timesteps)
    res = run()
    with perturbed_exp():
        pert = run()
    return res, pert


def _f_toa(pl, F_star):
    return 2 / 3 * pl.a_rstar ** -2 * 1 / (2 * np.pi) * F_star


def test_binned_spectrum_irradiation_matches_oracle(fa, binned_on_grid):
    pl = fa.Planet(a_rstar=7.5, m_bar=fa.Planet.from_hot_jupiter().m_bar, g=2000.0,
                   T_star=4500.0, alpha=1, stellar_spectrum=binned_on_grid[1])
    gr = _grid(fa, pl)
    try:
        spec, T, th, dtaus = gr.emission_spectrum(n_timesteps=3)
        up, down = gr.engine().get_fluxes()
    finally:
        gr._close_engine()
    (osp, oT, oth, odt, ou, od, it), (psp, pT, _, _, pu, pd, _) = \
        _oracle(gr, _f_toa(pl, binned_on_grid[1]), 3)
    assert th.shape[1] // 2 == it
    # the spectrum is not the blackbody's: the run really took it
    assert rel(_f_toa(pl, binned_on_grid[1]), O.F_TOA(gr.lam, 4500.0, a_rstar=7.5)) > 0.05
    assert_grid_parity(spec.flux, osp, up, ou, down, od, "binned stellar irradiation",
                       grid_floor(osp, ou, od, psp, pu, pd), T=T, ref_T=oT, T_floor=rel(pT, oT))


def test_batched_planets_with_their_own_spectra_match_single_runs(fa, binned_on_grid):
    """Two planets under different binned spectra through batched_emission_spectra against
    each Grid's own emission_spectrum, compared as test_gpu_batch.py compares them: same
    iteration counts, and both within the reference's one-ulp floor of the oracle."""
    grids, op = [], None
    for m, (T_ref, g, a_r) in zip((0, 2), ((1800, 1500.0, 6.45), (2400, 3000.0, 9.0))):
        pl = fa.Planet(a_rstar=a_r, m_bar=fa.Planet.from_hot_jupiter().m_bar, g=g,
                       T_star=5000.0, alpha=1, stellar_spectrum=binned_on_grid[m])
        gr = fa.Grid(pl, lam_min=0.5, lam_max=5.0, n_wl_bins=N_LAM, n_layers=N_LAYERS,
                     T_ref=T_ref)
        if op is None:
            op = fa.load_example_opacity(gr, scale_factor=2)
        gr.load_opacities(opacities=op)
        grids.append(gr)
    res = fa.batched_emission_spectra(grids, n_timesteps=10)
    for m, gr, (spec, T, it) in zip((0, 2), grids, res):
        s1, T1, th1, _ = gr.emission_spectrum(n_timesteps=10)
        gr._close_engine()
        assert it == th1.shape[1] // 2
        (osp, oT, *_), (psp, pT, *_) = _oracle(gr, _f_toa(gr.planet, binned_on_grid[m]), 10)
        fT, fS = rel(pT, oT), rel(psp, osp)
        for t, sp_ in ((T, spec.flux), (T1, s1.flux)):
            assert rel(t, oT) <= max(1e-10, 2 * fT), (rel(t, oT), fT)
            assert rel(sp_, osp) <= max(1e-10, 2 * fS), (rel(sp_, osp), fS)
    assert not np.array_equal(res[0][0].flux, res[1][0].flux)
