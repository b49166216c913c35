"""K15 on the GPU: frei_itp_apply in both forms and the automatic one against the plain NumPy
restatement (tests/interp_ref.py), bit for bit — both sides run the same IEEE multiplies and
adds in the same order, so there is no tolerance anywhere in this file except the instrument's
own chi-square bound in the end-to-end case.

Shapes vary one axis at a time about a base of 6 nodes x 5 queries x 4 corners x 70 wavelengths:
the wavelengths across a wave, form 1's pair of outputs and form 2's tile; the nodes up to the
tallest library form 2 stages and one beyond; the corners 1 to 16; the queries across form 1's
queries per block and form 2's waves per workgroup.
"""
import functools

import numpy as np
import pytest

from tests import interp_ref as R
from tests import observe_ref as OR

pytestmark = pytest.mark.gpu

FORMS_AND_AUTO = (1, 2, 0)
BASE = dict(n_node=6, n_query=5, n_corner=4, n_lam=70)


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _lam(n):
    return np.exp(np.linspace(np.log(1.0), np.log(1.2), n)) if n > 1 else np.array([1.0])


def _library(fa, X):
    """A ModelGrid on one axis of X.shape[0] nodes: plans are passed as idx=, w=."""
    return fa.ModelGrid([np.arange(X.shape[0], dtype=float)], _lam(X.shape[1]), spectra=X)


@functools.lru_cache(maxsize=None)
def _case(n_node, n_query, n_corner, n_lam, idx_kind="random"):
    """Seeded library, plan and reference.  The weights hold zeros, negative values and values
    above 1; idx is unsorted, or repeats a node within every query, or is one node throughout."""
    rng = np.random.default_rng([n_node, n_query, n_corner, n_lam])
    X = rng.normal(0.0, 1.0, (n_node, n_lam)) * np.exp(rng.uniform(-3.0, 3.0, (n_node, 1)))
    w = rng.uniform(-0.75, 1.75, (n_query, n_corner))
    w[rng.uniform(size=w.shape) < 0.2] = 0.0
    if idx_kind == "random":
        idx = rng.integers(0, n_node, (n_query, n_corner))
    elif idx_kind == "repeated":
        idx = rng.integers(0, n_node, (n_query, n_corner))
        idx[:, 1::2] = idx[:, 0::2][:, :idx[:, 1::2].shape[1]]
    else:
        idx = np.full((n_query, n_corner), n_node - 1)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    ref = R.interpolate(X, idx, w)
    for a in (X, idx, w, ref):
        a.setflags(write=False)
    return X, idx, w, ref


def _check_all_forms(fa, shape, idx_kind="random"):
    from frei_amd.modelgrid import automatic_form
    X, idx, w, ref = _case(*[shape[k] for k in ("n_node", "n_query", "n_corner", "n_lam")],
                           idx_kind)
    g = _library(fa, X)
    try:
        for form in FORMS_AND_AUTO:
            got = g.interpolate(idx=idx, w=w, form=form)
            auto = automatic_form(shape["n_node"], shape["n_lam"], shape["n_query"],
                                  shape["n_corner"])
            assert g.form_used == (form or auto)
            assert got.shape == ref.shape
            assert R.same_bits(got, ref), f"form {form} of {shape}, {idx_kind}"
        assert g.timing()[1] == 3 and g.timing()[0] > 0.0
    finally:
        g.release()


def _tile():
    from frei_amd.modelgrid import tile_width
    return tile_width(BASE["n_node"])


# ------------------------------------------------------------------ 1: shapes, one axis at a time
def _n_lam_values():
    T = _tile()
    return [1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3]


@pytest.mark.parametrize("n_lam", _n_lam_values())
def test_wavelength_counts(fa, n_lam):
    _check_all_forms(fa, dict(BASE, n_lam=n_lam))


@pytest.mark.parametrize("n_corner", [1, 2, 3, 8, 16])
def test_corner_counts(fa, n_corner):
    _check_all_forms(fa, dict(BASE, n_corner=n_corner))


def _n_query_values():
    from frei_amd.modelgrid import LDS_WAVES
    # 1; form 2's waves per workgroup - 1, + 0, + 1; one more than two whole rounds of its
    # per-workgroup query loop (the base's 5 is one more than form 1's 4 queries per block)
    return [1, LDS_WAVES - 1, LDS_WAVES, LDS_WAVES + 1, 2 * LDS_WAVES + 1]


@pytest.mark.parametrize("n_query", _n_query_values())
def test_query_counts(fa, n_query):
    _check_all_forms(fa, dict(BASE, n_query=n_query))


@pytest.mark.parametrize("idx_kind", ["random", "repeated", "equal"])
def test_index_patterns(fa, idx_kind):
    _check_all_forms(fa, BASE, idx_kind)


def test_node_counts(fa):
    """1, 2, every tile width's tallest library, and one more than the tallest of all: form 2
    must refuse that one and form 0 must take form 1."""
    from frei_amd.modelgrid import LDS_MAX_NODES, tile_width
    assert [tile_width(n) for n in (80, 81, 160, 161, LDS_MAX_NODES)] == [256, 128, 128, 64, 64]
    for n_node in (1, 2, 80, 81, 160, 161, LDS_MAX_NODES):
        _check_all_forms(fa, dict(BASE, n_node=n_node))
    X, idx, w, ref = _case(LDS_MAX_NODES + 1, 5, 4, 70)
    g = _library(fa, X)
    try:
        with pytest.raises(RuntimeError, match=f"at most {LDS_MAX_NODES} nodes in LDS"):
            g.interpolate(idx=idx, w=w, form=2)
        assert R.same_bits(g.interpolate(idx=idx, w=w, form=0), ref) and g.form_used == 1
        assert R.same_bits(g.interpolate(idx=idx, w=w, form=1), ref)
    finally:
        g.release()


def test_automatic_form_takes_the_lds_form_where_its_rule_says(fa):
    """The smallest shape past every threshold of the form-0 rule: the choice and the bits."""
    from frei_amd import modelgrid as M
    shape = dict(n_node=3, n_query=M.LDS_FROM_QUERIES, n_corner=M.LDS_FROM_CORNERS,
                 n_lam=256 * (M.LDS_FROM_TILES - 1) + 1)
    assert M.automatic_form(3, shape["n_lam"], shape["n_query"], shape["n_corner"]) == 2
    _check_all_forms(fa, shape)


# ------------------------------------------------------------------ 2: independence of rows
def test_rows_do_not_depend_on_the_batch(fa):
    X, idx, w, ref = _case(6, 17, 4, 70)
    # more nodes, none listed, all NaN; more queries behind the old ones
    X2 = np.concatenate([X, np.full((3, 70), np.nan)])
    rng = np.random.default_rng(2)
    idx2 = np.concatenate([idx, rng.integers(0, 9, (6, 4)).astype(np.int32)])
    w2 = np.concatenate([w, rng.uniform(0.0, 1.0, (6, 4))])
    g, g2 = _library(fa, X), _library(fa, X2)
    try:
        for form in FORMS_AND_AUTO:
            full = g.interpolate(idx=idx, w=w, form=form)
            assert R.same_bits(full, g.interpolate(idx=idx, w=w, form=form)), "a repeated call"
            for q in (0, 15, 16):
                alone = g.interpolate(idx=idx[q:q + 1], w=w[q:q + 1], form=form)
                assert R.same_bits(alone[0], full[q]), f"row {q} alone, form {form}"
            more = g2.interpolate(idx=idx2, w=w2, form=form)
            assert R.same_bits(more[:17], full), f"more queries and unused nodes, form {form}"
            assert np.isnan(more[17:]).any()
    finally:
        g.release(), g2.release()


def test_non_finite_values_stay_where_they_are(fa):
    """A NaN (and an inf) at X[2][33] reaches exactly the outputs (q, 33) of the queries that
    list node 2 — those that weight it with 0 included — and nothing else, in both forms."""
    X, _, _, _ = _case(6, 5, 4, 70)
    idx = np.array([[2, 0, 1, 3],       # lists it, weight 0
                    [0, 1, 3, 4],       # does not list it
                    [5, 4, 2, 2],       # lists it twice
                    [1, 1, 1, 1],       # does not
                    [0, 3, 5, 2],       # lists it, weight 0 in the last corner
                    [4, 5, 0, 3]], dtype=np.int32)
    w = np.array([[0.0, 0.5, 0.25, 0.25], [0.1, 0.2, 0.3, 0.4], [0.5, 0.5, -1.0, 2.0],
                  [1.0, 0.0, 0.0, 0.0], [0.3, 0.3, 0.4, 0.0], [0.25, 0.25, 0.25, 0.25]])
    lists = np.array([True, False, True, False, True, False])
    clean_ref = R.interpolate(X, idx, w)
    for bad in (np.nan, np.inf):
        Xb = X.copy()
        Xb[2, 33] = bad
        ref = R.interpolate(Xb, idx, w)
        g = _library(fa, Xb)
        try:
            for form in (1, 2):
                got = g.interpolate(idx=idx, w=w, form=form)
                assert R.same_bits(got, ref), form
                touched = ~np.isfinite(got)
                want = np.zeros_like(touched)
                want[lists, 33] = True
                assert np.array_equal(touched, want), (form, bad)
                assert R.same_bits(got[~want], clean_ref[~want])
        finally:
            g.release()


# ------------------------------------------------------------------ 3: the plan on the device
def test_a_query_on_a_node_returns_its_row(fa):
    rng = np.random.default_rng(3)
    axes = [np.array([1000.0, 1400.0, 2300.0]), np.array([2.5, 3.0])]
    X = rng.normal(0.0, 1.0, (6, 70))
    g = fa.ModelGrid(axes, _lam(70), spectra=X)
    theta = np.array([[t, s] for t in axes[0] for s in axes[1]] + [[9999.0, -1.0]])
    try:
        for form in FORMS_AND_AUTO:
            got = g.interpolate(theta, form=form)
            assert R.same_bits(got[:6], X), form
            assert R.same_bits(got[6], X[4]) and g.n_outside == 2     # clamped to (2300, 2.5)
    finally:
        g.release()


@pytest.mark.parametrize("shape", [(5,), (3, 4), (3, 2, 3), (2, 3, 2, 2), (3, 1, 2)])
def test_dyadic_multilinear_function_is_exact_on_the_device(fa, shape):
    axes, X, theta, exact = R.dyadic_case(shape)
    g = fa.ModelGrid(axes, _lam(X.shape[1]), spectra=X)
    try:
        for form in FORMS_AND_AUTO:
            assert R.same_bits(g.interpolate(theta, form=form), exact), form
    finally:
        g.release()


# ------------------------------------------------------------------ 4: kept rows and consumers
def _delta_instrument(fa, lam):
    """One channel per wavelength with weight 1: obs = (1 * x) / 1, the row itself."""
    n = lam.size
    return fa.Instrument(lam, np.arange(n), np.ones(n, dtype=np.int64), np.ones(n))


def test_kept_rows_are_the_downloaded_ones_and_feed_the_consumers(fa):
    from frei_amd.broaden import BroadeningKernel
    X, idx, w, ref = _case(6, 17, 4, 70)
    lam = _lam(70)
    rng = np.random.default_rng(4)
    g = _library(fa, X)
    delta = _delta_instrument(fa, lam)
    inst = fa.Instrument.top_hat(lam, [1.0, 1.05, 1.1], [1.06, 1.1, 1.2])
    cc = fa.CrossCorrelator(lam, rng.uniform(1.02, 1.18, 40), rng.normal(0.0, 1.0, (3, 40)),
                            np.linspace(-3000.0, 3000.0, 9), weights=rng.uniform(0.5, 1.5, 40))
    b = fa.Broadening(lam, BroadeningKernel(400.0, [0.05, 0.3, 0.6, 0.9, 1.0, 0.9, 0.6, 0.3,
                                                    0.05]))
    st = fa.OrbitStack(cc.velocities, [100.0, 150.0], np.linspace(-500.0, 500.0, 5),
                       phases=[0.1, 0.2, 0.3])
    scale = rng.uniform(0.5, 2.0, 17)
    offset = rng.uniform(-1.0, 1.0, 17)
    den = np.abs(rng.normal(1.0, 0.1, (2, 70))) + 0.5
    select = rng.integers(0, 2, 17)
    data, sigma = rng.normal(0.0, 1.0, 3), np.array([0.1, 0.2, np.inf])
    try:
        for form in (1, 2):
            host = g.interpolate(idx=idx, w=w, form=form)
            kept = g.interpolate(idx=idx, w=w, form=form, keep=True)
            assert kept.n_query == 17 and kept.n_lam == 70
            assert R.same_bits(delta.apply(kept), host), f"kept rows, form {form}"
            assert R.same_bits(host, ref)
        # Instrument.apply: a library, per-query select and scale, chi-square
        got = inst.apply(kept, den=den, select=select, scale=scale, data=data, sigma=sigma)
        want = inst.apply(host, den=den, select=select, scale=scale, data=data, sigma=sigma)
        assert R.same_bits(got[0], want[0]) and R.same_bits(got[1], want[1])
        # the observables over it: per-query radii, so (R_p / R_star)^2 can be fitted
        R_p = rng.uniform(0.8, 1.2, 17) * 7e9
        assert R.same_bits(inst.eclipse(kept, den[0], R_p, 7e10), inst.eclipse(host, den[0], R_p,
                                                                               7e10))
        assert R.same_bits(inst.transit(kept, F_star=den, select=select),
                           inst.transit(host, F_star=den, select=select))
        # Broadening.apply, to the host and kept in turn
        broad = b.apply(kept)
        assert R.same_bits(broad, b.apply(host))
        assert R.same_bits(delta.apply(b.apply(kept, keep=True)), broad)
        # correlate, then the stack from the kept sums
        for f in (1, 2):
            res = cc.correlate(kept, den=den, select=select, scale=scale, offset=offset, form=f)
            hand = cc.correlate(host, den=den, select=select, scale=scale, offset=offset, form=f)
            for x, y in zip((res.sfg, res.sg, res.sgg), (hand.sfg, hand.sg, hand.sgg)):
                assert R.same_bits(x, y), f
        on_device = st.stack(cc.correlate(kept, keep=True, want=()), "ccf")
        assert R.same_bits(on_device, st.stack(cc.correlate(host), "ccf"))
        assert on_device.shape == (17, 2, 5)
        # staleness reaches the consumers
        g.interpolate(idx=idx[:1], w=w[:1])
        with pytest.raises(RuntimeError, match="stale InterpolatedSpectra"):
            inst.apply(kept)
        # a kept result of another query count is refused by the library, naming both sides
        kept = g.interpolate(idx=idx[:3], w=w[:3], keep=True)
        # (the handle's result buffer is reused: a smaller call after a larger one keeps its own)
        assert R.same_bits(delta.apply(kept), ref[:3])
        from frei_amd import _native as N
        obs = np.empty((4, 3))
        rc = N.lib().frei_obs_apply_itp(inst.handle(), kept.handle(), 4, None, None, 0, None,
                                        None, None, None, 0, N.dptr(obs), None, None, None)
        assert rc != 0
        assert b"keeps 3 queries, not n_atm = 4" in N.lib().frei_last_error()
    finally:
        for o in (g, delta, inst, cc, b, st):
            o.release()


# ------------------------------------------------------------------ 5: nodes from a sweep
def _sweep_grids(fa):
    """2 x 2 nodes: T_ref x g, the last axis fastest."""
    lam, _, _ = fa.wavelength_grid(0.5, 10, 500)
    T_axis, g_axis = np.array([1400.0, 2300.0]), np.array([1500.0, 4000.0])
    grids, op = [], None
    for T_ref in T_axis:
        for g in g_axis:
            pl = fa.Planet.from_hot_jupiter()
            pl.g = float(g)
            gr = fa.Grid(pl, lam=lam, n_layers=30, T_ref=float(T_ref))
            if op is None:
                op = fa.load_example_opacity(gr)
            gr.load_opacities(opacities=op)
            grids.append(gr)
    return [T_axis, g_axis], grids


def test_nodes_from_a_sweep_left_on_the_device(fa):
    axes, grids = _sweep_grids(fa)
    lam = np.asarray(grids[0].lam, dtype=float)
    b = fa.Broadening(lam, fa.BroadeningKernel.gaussian(resolving_power=40.0))
    theta = np.array([[1850.0, 2750.0],      # the cell centre
                      [1400.0, 4000.0],      # a node
                      [2000.0, 1600.0]])
    made = []
    try:
        with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
            spectra = np.array([r.spectrum.flux for r in res], dtype=float)
            resident = res.model_grid(axes)
            broad_nodes = res.model_grid(axes, broadening=b)
            broad_host = b.apply(spectra)
            made += [resident, broad_nodes]
        # the sweep's context is closed: the grids own their copies
        from_host = fa.ModelGrid(axes, lam, spectra=spectra)
        from_broad_host = fa.ModelGrid(axes, lam, spectra=broad_host)
        made += [from_host, from_broad_host]
        idx, w, n_out = from_host.plan(theta)
        assert n_out == 0 and w[0].tolist() == [0.25] * 4
        ref = R.interpolate(spectra, idx, w)
        for form in (1, 2):
            got = resident.interpolate(theta, form=form)
            assert R.same_bits(got, from_host.interpolate(theta, form=form))
            assert R.same_bits(got, ref) and R.same_bits(got[1], spectra[1])
            assert np.all(np.isfinite(got)) and np.all(got[0] > 0.0)
            assert R.same_bits(broad_nodes.interpolate(theta, form=form),
                               from_broad_host.interpolate(theta, form=form))
        # set_nodes again replaces the library and ends what was kept
        kept = resident.interpolate(theta, keep=True)
        resident.set_nodes(spectra[::-1].copy())
        with pytest.raises(RuntimeError, match="stale"):
            kept.handle()
        assert R.same_bits(resident.interpolate(theta), R.interpolate(spectra[::-1], idx, w))
    finally:
        b.release()
        for g in made:
            g.release()


# ------------------------------------------------------------------ 6: the point of the feature
def test_chi2_over_a_lattice_finds_the_injected_point(fa):
    """3 x 3 nodes of positive spectra multilinear in theta (dyadic, so interpolation is exact),
    an instrument of 4 channels, data from the off-node theta* = (g0[0] + 1/2, g1[1] + 1/4) by
    the instrument's host restatement.  chi2 over a lattice of step 1/4 that holds theta* is
    within the instrument's bound (tests/observe_ref.chi2_bound) of the restatement's everywhere,
    0 within it at theta*, and smallest there."""
    axes, X, _, _ = R.dyadic_case((3, 3), n_lam=96, seed=6)
    X = X + 1024.0                       # positive; the weights sum to 1 exactly, so still exact
    assert np.all(X > 0.0)
    lam = _lam(96)
    lattice = np.array([[a, b] for a in np.arange(axes[0][0], axes[0][-1] + 0.125, 0.25)
                        for b in np.arange(axes[1][0], axes[1][-1] + 0.125, 0.25)])
    star = np.array([axes[0][0] + 0.5, axes[1][1] + 0.25])
    at = int(np.flatnonzero(np.all(lattice == star, axis=1))[0])
    inst = fa.Instrument.top_hat(lam, [1.0, 1.04, 1.09, 1.15], [1.04, 1.09, 1.15, 1.2])
    g = fa.ModelGrid(axes, lam, spectra=X)
    try:
        idx, w, _ = g.plan(lattice)
        rows = R.interpolate(X, idx, w)
        plan = (inst.first, inst.count, inst.weights)
        obs_ref = OR.apply(*plan, rows)
        data = obs_ref[at].copy()
        sigma = 1e-5 * data
        chi2_ref = OR.chi2(obs_ref, data, sigma)
        assert chi2_ref[at] == 0.0 and np.all(np.delete(chi2_ref, at) > 1.0)
        bound = OR.chi2_bound(obs_ref, data, sigma, OR.rtol_for(int(inst.count.max())))
        for form in FORMS_AND_AUTO:
            kept = g.interpolate(lattice, form=form, keep=True)
            obs, chi2 = inst.apply(kept, data=data, sigma=sigma)
            print(f"form {form}: chi2 at theta* {chi2[at]:.3e} (bound {bound[at]:.3e}), next "
                  f"smallest {np.delete(chi2, at).min():.3e}")
            assert np.all(np.abs(chi2 - chi2_ref) <= bound)
            assert chi2[at] <= bound[at]
            assert int(np.argmin(chi2)) == at
    finally:
        g.release(), inst.release()
