"""GPU tests of the emergent intensities and the ray-traced flux (frei_emergent, K11):
Engine.emergent, BatchEngine.emergent, Grid.emergent_spectrum and BatchResult.emergent against
tests/emergent_ref.py, the plain NumPy restatement of the definition (the reference has no
counterpart; tests/test_emergent_host.py pins the restatement itself).

Tolerance, derived rather than measured.  Every step of the recurrence is a convex combination
of non-negative terms, so rounding stays within about n_layers x a few ulp of I; the Planck
exponent reaches about 32 at 0.5 um and 900 K, where ocml and glibc differ by a few ulp that exp
turns into about 1e-14.  So the device matches the restatement to rtol 1e-12, elementwise, on
intensity and flux, as K9 does.  Measured on MI355X (each test prints its maximum, pytest -s):
see the end of this docstring.

"Exactly B_1" for transparent shells is checked where it is defined on the device: the
intensities of a zero-dtaus call are bitwise those of the same call with every level at T_1, the
same at every angle, and match the restatement's B_1 within the tolerance (the device's Planck
function and glibc's differ by ulps, so no host value is the device's B_1 to the bit).

Measured maxima (relative): parity, intensity / flux: (4, 2, 1) 1.8e-16 / 2.3e-16, (7, 257, 3)
1.6e-15 / 4.2e-16, (30, 1000, 8) 1.2e-15 / 6.6e-16, (61, 513, 9) 4.3e-15 / 6.4e-16, (12, 300, 17)
7.3e-15 / 8.6e-16; transparent against B_1 3.3e-16, opaque against B_(nL-1) 3.0e-16, isothermal
flux against pi B 5.3e-16 and intensity against B 5.8e-16; batched rows 2.5e-15 / 6.0e-16; the C1
example's kept dtaus 9.3e-16 / 6.5e-16, over three grids 9.3e-16 / 7.5e-16.  Every bitwise
comparison held."""
import functools

import numpy as np
import pytest

from tests import emergent_ref as R

pytestmark = pytest.mark.gpu

RTOL = 1e-12


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _lam(n_lam):
    return np.logspace(np.log10(0.5), 1.0, n_lam)


def _grid(fa, n_layers, n_lam):
    lam = _lam(n_lam)
    p = np.logspace(np.log10(200.0), -6, n_layers)
    tabs = {"1H2-16O": fa.OpacityTable(np.ones((n_layers, 2, n_lam)), p, [1000.0, 2000.0])}
    return lam, p, tabs


def _angles(n_mu):
    """n_mu angles in (0, 1] ending at 1, with quadrature weights (any finite weights do)."""
    mu = np.linspace(1.0 / n_mu, 1.0, n_mu)
    w = np.linspace(0.5, 1.5, n_mu) / n_mu
    return mu, w


@functools.lru_cache(maxsize=None)
def _case(n_layers, n_lam, n_mu, n_atm=1, seed=0):
    """Seeded inputs and the restatement's answer, computed once per shape: dtaus log-uniform in
    [1e-8, 1e3] (row 0 NaN: it is never read), T a noisy 2500 -> 900 K ramp per atmosphere
    (T[0] NaN: never read)."""
    rng = np.random.default_rng(1000 * n_layers + n_lam + 7 * n_mu + seed)
    dt = 10 ** rng.uniform(-8, 3, (n_atm, n_layers, n_lam))
    dt[:, 0] = np.nan
    T = np.array([np.linspace(2500.0 - 300 * m, 900.0 + 100 * m, n_layers) +
                  80.0 * rng.standard_normal(n_layers) for m in range(n_atm)])
    T[:, 0] = np.nan
    mu, w = _angles(n_mu)
    ref = [R.emergent(dt[m], T[m], _lam(n_lam), mu, w) for m in range(n_atm)]
    for a in (dt, T, mu, w):
        a.setflags(write=False)
    return dt, T, mu, w, ref


def _err(x, ref):
    return float(np.max(np.abs(np.asarray(x) - ref) / np.abs(ref)))


def _close(x, ref, rtol=RTOL):
    return np.all(np.abs(np.asarray(x) - ref) <= rtol * np.abs(ref))


# ------------------------------------------------------------------ 1: restatement parity
@pytest.mark.parametrize("n_layers,n_lam,n_mu",
                         [(4, 2, 1), (7, 257, 3), (30, 1000, 8), (61, 513, 9), (12, 300, 17)])
def test_emergent_matches_the_restatement(fa, n_layers, n_lam, n_mu):
    """(4, 2, 1): the minimum layers, the smallest context (frei_ctx_create refuses n_lam = 1),
    one angle; (7, 257, 3): a last block of one lane, a partial tile; (30, 1000, 8): four blocks,
    one full tile; (61, 513, 9): a full tile plus a one-angle pass; (12, 300, 17): three passes."""
    dt, T, mu, w, ref = _case(n_layers, n_lam, n_mu)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    eng = fa.Engine(lam, p, tabs)
    try:
        flux, inten = eng.emergent(T[0], mu, w, dtaus=dt[0], want_intensity=True)
        flux_only = eng.emergent(T[0], mu, w, dtaus=dt[0])
        inten_only = eng.emergent(T[0], mu, dtaus=dt[0])
        flux2, inten2 = eng.emergent(T[0], mu, w, dtaus=dt[0], want_intensity=True)
    finally:
        eng.close()
    ri, rf = ref[0]
    assert flux.shape == (n_lam,) and inten.shape == (n_mu, n_lam)
    e_i, e_f = _err(inten, ri), _err(flux, rf)
    print(f"({n_layers}, {n_lam}, {n_mu}): intensity {e_i:.3e}  flux {e_f:.3e}")
    assert _close(inten, ri), e_i
    assert _close(flux, rf), e_f
    assert np.array_equal(flux_only, flux), "flux differs without the intensity output"
    assert np.array_equal(inten_only, inten), "intensity differs without the flux output"
    assert np.array_equal(flux2, flux) and np.array_equal(inten2, inten), "two calls differ"


# ------------------------------------------------------------------ 2: bounds and limits
def test_emergent_bounds_and_limits(fa):
    n_layers, n_lam, n_mu = 30, 257, 5
    dt, T, mu, w, _ = _case(n_layers, n_lam, n_mu)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    zero, thick = np.zeros((n_layers, n_lam)), np.full((n_layers, n_lam), 1e6)
    T1 = np.full(n_layers, T[0][1])
    gm, gw = fa.gauss_angles(4)
    eng = fa.Engine(lam, p, tabs)
    try:
        inten = eng.emergent(T[0], mu, dtaus=dt[0])
        clear = eng.emergent(T[0], mu, dtaus=zero)
        clear_iso = eng.emergent(T1, mu, dtaus=zero)
        opaque = eng.emergent(T[0], mu, dtaus=thick)
        iso_flux, iso_int = eng.emergent(np.full(n_layers, 1500.0), dtaus=dt[0],
                                         want_intensity=True)       # the default angles
    finally:
        eng.close()
    B = np.array([R.planck(lam, T[0][l]) for l in range(1, n_layers)])
    lo, hi = B.min(axis=0), B.max(axis=0)
    assert np.all(inten >= lo * (1 - 1e-13)) and np.all(inten <= hi * (1 + 1e-13))
    assert np.array_equal(clear, clear_iso), "transparent shells changed I"
    assert all(np.array_equal(clear[k], clear[0]) for k in range(n_mu))
    e0 = _err(clear[0], B[0])
    e1 = max(_err(opaque[k], B[-1]) for k in range(n_mu))
    Biso = R.planck(lam, 1500.0)
    e2, e3 = _err(iso_flux, np.pi * Biso), max(_err(iso_int[k], Biso) for k in range(4))
    print(f"transparent vs B_1 {e0:.3e}  opaque vs B_(nL-1) {e1:.3e}  "
          f"isothermal flux vs pi B {e2:.3e}  intensity vs B {e3:.3e}")
    assert e0 <= RTOL and e1 <= 1e-13 and e2 <= 1e-13 and e3 <= 1e-13
    assert iso_int.shape == (4, n_lam) and gm.shape == gw.shape == (4,)


# ------------------------------------------------------------------ 3: angle independence
def test_every_angle_is_independent_of_the_rest_of_the_call(fa):
    n_layers, n_lam = 30, 257
    dt, T, _, _, _ = _case(n_layers, n_lam, 5)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    three = np.array([0.2, 0.6, 1.0])
    many = np.linspace(0.05, 0.95, 17)
    many[[0, 8, 16]] = three
    w17 = np.full(17, 1.0 / 17)
    eng = fa.Engine(lam, p, tabs)
    try:
        i3 = eng.emergent(T[0], three, dtaus=dt[0])
        ones = [eng.emergent(T[0], three[k:k + 1], dtaus=dt[0]) for k in range(3)]
        i17 = eng.emergent(T[0], many, dtaus=dt[0])
        _, i17f = eng.emergent(T[0], many, w17, dtaus=dt[0], want_intensity=True)
    finally:
        eng.close()
    for k, pos in enumerate([0, 8, 16]):
        assert ones[k].shape == (1, n_lam)
        assert np.array_equal(i3[k], ones[k][0]), f"angle {k}: alone differs"
        assert np.array_equal(i3[k], i17[pos]), f"angle {k}: at position {pos} of 17 differs"
        assert np.array_equal(i3[k], i17f[pos]), f"angle {k}: with the flux differs"
    assert not np.array_equal(i3[0], i3[2])


# ------------------------------------------------------------------ 4: batched against single
def test_batched_emergent_is_bitwise_the_single_call(fa):
    n_layers, n_lam, n_atm, n_mu = 30, 700, 3, 9
    dt, T, mu, w, ref = _case(n_layers, n_lam, n_mu, n_atm, seed=5)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    beng = fa.BatchEngine(lam, p, tabs, g=np.array([900.0, 2478.65, 5200.0]))
    try:
        bf, bi = beng.emergent(T, mu, w, dtaus=dt, want_intensity=True)
        ms = beng.post_timing()
    finally:
        beng.close()
    assert bf.shape == (n_atm, n_lam) and bi.shape == (n_atm, n_mu, n_lam)
    assert ms > 0.0, "frei_post_timing does not cover the emergent kernel"
    eng = fa.Engine(lam, p, tabs)
    try:
        for m in range(n_atm):
            f, i = eng.emergent(T[m], mu, w, dtaus=dt[m], want_intensity=True)
            assert np.array_equal(bf[m], f), f"atmosphere {m}: flux not bitwise"
            assert np.array_equal(bi[m], i), f"atmosphere {m}: intensity not bitwise"
            e_i, e_f = _err(i, ref[m][0]), _err(f, ref[m][1])
            print(f"atmosphere {m}: intensity {e_i:.3e}  flux {e_f:.3e}")
            assert _close(i, ref[m][0]) and _close(f, ref[m][1]), (m, e_i, e_f)
    finally:
        eng.close()
    assert not np.array_equal(bf[0], bf[1])


# ------------------------------------------------------------------ 5: kept dtaus
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


def test_emergent_spectrum_from_the_kept_dtaus(fa):
    """The C1 example opacity at 30 x 500: after emission_spectrum the device copy of the dtaus
    gives bitwise what the returned host array gives, and both match the restatement."""
    gr, = _example_grids(fa, 1)
    try:
        with pytest.raises(RuntimeError, match="no device dtaus"):
            gr.emergent_spectrum(gr.init_temperatures)
        spec, T, _, dtaus = gr.emission_spectrum(n_timesteps=1)
        kept, kept_i = gr.emergent_spectrum(T, want_intensity=True)
        given = gr.emergent_spectrum(T, dtaus=dtaus.copy())
        alone = gr.emergent_spectrum(T, mu=[0.5, 1.0])
    finally:
        gr._close_engine()
    assert isinstance(kept, fa.Spectrum) and kept.flux.shape == (500,)
    assert np.array_equal(kept.wavelength, gr.lam)
    assert np.array_equal(kept.flux, given.flux), "device dtaus and host dtaus differ"
    mu, w = fa.gauss_angles(4)
    ri, rf = R.emergent(dtaus, T, gr.lam, mu, w)
    e_f, e_i = _err(kept.flux, rf), _err(kept_i, ri)
    ratio = kept.flux / np.asarray(spec.flux)
    print(f"grid emergent spectrum: flux {e_f:.3e}  intensity {e_i:.3e}; ray-traced over "
          f"two-stream flux {ratio.min():.3f} .. {ratio.max():.3f}")
    assert _close(kept.flux, rf), e_f
    assert _close(kept_i, ri), e_i
    assert alone.shape == (2, 500)
    assert _close(alone, R.emergent(dtaus, T, gr.lam, [0.5, 1.0])[0])


def test_batch_result_emergent_over_three_grids(fa):
    grids = _example_grids(fa, 3)
    mu, w = fa.gauss_angles(4)
    with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
        flux, inten = res.emergent(want_intensity=True)
        dts = [res.dtaus(m) for m in range(3)]
        Ts = np.array([res[m].final_T for m in range(3)])
        given = res.engine.emergent(Ts, mu, w, dtaus=np.array(dts))
    assert flux.shape == (3, 500) and inten.shape == (3, 4, 500)
    assert np.array_equal(flux, given), "device dtaus and host dtaus differ"
    for m, gr in enumerate(grids):
        ri, rf = R.emergent(dts[m], Ts[m], gr.lam, mu, w)
        e_f, e_i = _err(flux[m], rf), _err(inten[m], ri)
        print(f"grid {m}: batched emergent flux {e_f:.3e}  intensity {e_i:.3e}")
        assert _close(flux[m], rf) and _close(inten[m], ri), (m, e_f, e_i)


# ------------------------------------------------------------------ 6: wavelength slice
def test_emergent_on_a_wavelength_slice(fa):
    n_layers, n_lam, n_mu = 30, 1000, 8
    dt, T, mu, w, _ = _case(n_layers, n_lam, n_mu)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    full = fa.Engine(lam, p, tabs)
    try:
        ff, fi = full.emergent(T[0], mu, w, dtaus=dt[0], want_intensity=True)
    finally:
        full.close()
    part = fa.Engine(lam, p, tabs, lam_slice=(100, 357))
    try:
        pf, pi = part.emergent(T[0], mu, w, dtaus=dt[0][:, 100:357], want_intensity=True)
    finally:
        part.close()
    assert pf.shape == (257,) and pi.shape == (n_mu, 257)
    assert np.array_equal(pf, ff[100:357]) and np.array_equal(pi, fi[:, 100:357])


# ------------------------------------------------------------------ 7: errors, not faults
def test_emergent_errors(fa):
    from frei_amd import _native as N
    n_layers, n_lam, n_mu = 7, 257, 3
    dt, T, mu, w, ref = _case(n_layers, n_lam, n_mu)
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    eng = fa.Engine(lam, p, tabs)
    try:
        with pytest.raises(RuntimeError, match="no device dtaus"):
            eng.emergent(T[0], mu, w)
        for bad in (0.0, -0.5, 1.0 + 1e-12, np.nan, np.inf):
            m = mu.copy()
            m[1] = bad
            with pytest.raises(RuntimeError, match="mu must lie in"):
                eng.emergent(T[0], m, w, dtaus=dt[0])
        for bad in (np.nan, np.inf):
            ww = w.copy()
            ww[2] = bad
            with pytest.raises(RuntimeError, match="weights must be finite"):
                eng.emergent(T[0], mu, ww, dtaus=dt[0])
        for bad in (0.0, -100.0, np.nan, np.inf):
            Tb = T[0].copy()
            Tb[n_layers - 1] = bad
            with pytest.raises(RuntimeError, match="T must be finite and positive"):
                eng.emergent(Tb, mu, w, dtaus=dt[0])
        # shapes are caught in Python
        with pytest.raises(ValueError, match="T must hold"):
            eng.emergent(T[0][:-1], mu, w, dtaus=dt[0])
        with pytest.raises(ValueError, match="dtaus"):
            eng.emergent(T[0], mu, w, dtaus=dt[0][:, :-1])
        with pytest.raises(ValueError, match="weights"):
            eng.emergent(T[0], mu, w[:-1], dtaus=dt[0])
        with pytest.raises(ValueError, match="weights"):
            eng.emergent(T[0], None, w, dtaus=dt[0])
        for cnt in (0, 65):
            with pytest.raises(ValueError, match="1 to 64"):
                eng.emergent(T[0], np.full(cnt, 0.5), dtaus=dt[0])
        # the library's own argument checks, through the C ABI
        lib = N.lib()
        d, Th, m_, w_ = N.f64(dt[0]), N.f64(T[0]), N.f64(mu), N.f64(w)
        inten, flux = np.empty((n_mu, n_lam)), np.empty(n_lam)

        def call(T=Th, mu=m_, weights=w_, n=n_mu, intensity=inten, flux=flux):
            rc = lib.frei_emergent(eng._ctx, N.dptr(d), N.dptr(T), N.dptr(mu), N.dptr(weights),
                                   n, N.dptr(intensity), N.dptr(flux))
            return rc, lib.frei_last_error().decode()
        for kw, text in [(dict(T=None), "null"), (dict(mu=None), "null"),
                         (dict(intensity=None, flux=None, weights=None), "both null"),
                         (dict(weights=None), "weights and flux"),
                         (dict(flux=None), "weights and flux"),
                         (dict(n=0), "n_mu"), (dict(n=65), "n_mu"), (dict(n=-1), "n_mu")]:
            rc, msg = call(**kw)
            assert rc != 0 and text in msg, (kw, rc, msg)
        # the context stays usable
        f, i = eng.emergent(T[0], mu, w, dtaus=dt[0], want_intensity=True)
        assert _close(i, ref[0][0]) and _close(f, ref[0][1])
        rc, msg = call()
        assert rc == 0 and np.array_equal(inten, i) and np.array_equal(flux, f)
    finally:
        eng.close()
    beng = fa.BatchEngine(lam, p, tabs, g=np.array([1000.0, 2000.0]))
    try:
        with pytest.raises(RuntimeError, match="no device dtaus"):
            beng.emergent(np.array([T[0], T[0]]), mu, w)
    finally:
        beng.close()


def test_nan_and_inf_stay_in_their_columns(fa):
    n_layers, n_lam, n_mu = 7, 257, 3
    dt, T, mu, w, ref = _case(n_layers, n_lam, n_mu)
    d = dt[0].copy()
    d[3, 5], d[2, 200] = np.nan, np.inf
    lam, p, tabs = _grid(fa, n_layers, n_lam)
    eng = fa.Engine(lam, p, tabs)
    try:
        flux, inten = eng.emergent(T[0], mu, w, dtaus=d, want_intensity=True)
    finally:
        eng.close()
    assert np.all(np.isnan(inten[:, 5])) and np.isnan(flux[5])
    # an opaque shell hides what lies below it: the restatement's own answer for that column
    ri, rf = R.emergent(d[:, 200:201], T[0], lam[200:201], mu, w)
    assert np.all(np.isfinite(inten[:, 200])) and _close(inten[:, 200], ri[:, 0])
    assert _close(flux[200], rf[0])
    keep = np.ones(n_lam, dtype=bool)
    keep[[5, 200]] = False
    assert _close(inten[:, keep], ref[0][0][:, keep]) and _close(flux[keep], ref[0][1][keep])
