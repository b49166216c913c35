"""The references of tests/updateref.py against exact arithmetic and the oracle, and the input
conditions of tests/test_gpu_update_exact.py on its CPU stand-ins (the same inputs run through
the oracle): no GPU.

The branch and min() conditions are asserted per family where the family's purpose allows them
(isothermal and inverted profiles are radiative by construction, the steep one convective) and
over all families together: both branches and both outcomes of min(dt_rad, dt_conv) occur, the
mixed family alone has both branches.  No layer is excluded from any condition."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import frei_oracle as O
from tests import updateref as R


def _ulp(x):
    return math.ulp(abs(float(x)))


# ------------------------------------------------------------------ exact_dot
def test_exact_dot_is_the_rounded_fraction_sum():
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 64, 257):
        w = rng.uniform(-1, 1, n) * 10 ** rng.uniform(-9, -3, n)
        F = rng.uniform(-1, 1, n) * 10 ** rng.uniform(6, 12, n)
        F[0] = -F[0] if n > 1 else F[0]
        s, sa = R.exact_dot(w, F)
        fr = R.exact_dot_fraction(w, F)
        fa = sum((abs(Fraction(float(a)) * Fraction(float(b))) for a, b in zip(w, F)),
                 Fraction(0))
        assert s == float(fr) and sa == float(fa), n     # float(Fraction) rounds correctly
    # a sum whose leading terms cancel: only the low parts of the products survive
    a = np.array([1 + 2.0 ** -30, -(1 + 2.0 ** -30), 3.0])
    b = np.array([1 + 2.0 ** -29, 1 + 2.0 ** -29, 2.0 ** -80])
    assert R.exact_dot(a, b)[0] == 3 * 2.0 ** -80


# ------------------------------------------------------------------ weights
def _grids():
    rng = np.random.default_rng(5)
    for n in (2, 3, 1000):
        yield f"uniform{n}", np.linspace(0.5, 10, n) * 1e-4
        yield f"log{n}", O.wavelength_grid(0.5, 10, n)[0] * 1e-4 if n > 2 else \
            np.array([0.5, 10.0]) * 1e-4
        yield f"irregular{n}", np.sort(rng.uniform(0.3, 30, n)) * 1e-4 * \
            (1 + 1e-3 * np.arange(n))


@pytest.mark.parametrize("name,lam_cm", list(_grids()), ids=[g[0] for g in _grids()])
def test_trapz_weights_within_one_ulp_of_exact(name, lam_cm):
    from frei_amd.engine import trapz_weights
    assert np.all(np.diff(lam_cm) > 0)
    w = trapz_weights(lam_cm)
    ex = R.exact_trapz_weights(lam_cm)
    assert len(ex) == w.size
    worst = 0.0
    for j, (a, e) in enumerate(zip(w, ex)):
        err = abs(Fraction(float(a)) - e) / Fraction(_ulp(float(e)))
        worst = max(worst, float(err))
        assert err <= 1, (name, j, float(err))
    # the exact weights are np.trapz's: sum w_j y_j = sum (x_{j+1} - x_j) (y_{j+1} + y_j) / 2
    y = [Fraction(int(v)) for v in np.random.default_rng(1).integers(1, 100, w.size)]
    x = [Fraction(float(v)) for v in lam_cm]
    assert sum(a * b for a, b in zip(ex, y)) == sum(
        (x[j + 1] - x[j]) * (y[j + 1] + y[j]) / 2 for j in range(w.size - 1))
    print(f"{name}: worst weight error {worst:.3f} ulp")


def test_slice_weights_are_the_global_ones_at_slice_edges():
    """An Engine slices the global weights (engine.py: trapz_weights(lam_cm)[lo:hi]) — a context
    cannot be formed without a device, so the function's output is sliced the same way: the
    edge points of a slice carry interior weights of the global grid, and the slices' exact
    sums add up to the exact whole."""
    from frei_amd.engine import trapz_weights
    lam_cm = O.wavelength_grid(0.5, 10, 1000)[0] * 1e-4
    w = trapz_weights(lam_cm)
    ex = R.exact_trapz_weights(lam_cm)
    cuts = [0, 1, 257, 700, 1000]
    F = 10 ** np.random.default_rng(2).uniform(6, 12, 1000)
    parts = Fraction(0)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ws = w[slice(lo, hi)]
        for j in (lo, hi - 1):
            assert abs(Fraction(float(ws[j - lo])) - ex[j]) <= Fraction(_ulp(float(ex[j])))
            if 0 < j < 999:      # an interior weight of the global grid, not a slice-end half
                assert ws[j - lo] == w[j] and ex[j] == (Fraction(float(lam_cm[j + 1])) -
                                                        Fraction(float(lam_cm[j - 1]))) / 2
        s, _ = R.exact_dot(ws, F[lo:hi])
        fr = R.exact_dot_fraction(ws, F[lo:hi])
        assert s == float(fr)
        parts += fr
    assert parts == R.exact_dot_fraction(w, F)


# ------------------------------------------------------------------ row bookkeeping
@pytest.mark.parametrize("n_lam,nL", [(3, 5), (65, 37), (257, 34)])
def test_row_bookkeeping_matches_oracle_sweep(n_lam, nL):
    """The rows sweep_rows names in the flux arrays before / after a sweep are, bit for bit, the
    rows the oracle's _sweep hands to its bolometric sums (bol_fn hook)."""
    case = R.sum_case(n_lam, nL)
    for d in ("emit", "absorb"):
        o = R.oracle_sweep(case, d, case["g"], case["m_bar"], 1.0)
        sums = R.RowSums(np.ones(n_lam), case["up0"], case["down0"], o["up"], o["down"],
                         case["F_toa"])
        rows = R.sweep_rows(d, nL)
        assert sorted(rows) == sorted(o["rows"])
        for i, keys in rows.items():
            for q, key in enumerate(keys):
                if key is None:
                    assert d == "emit" and i == nL - 1 and q == 0
                    continue
                assert np.array_equal(sums.row(key), o["rows"][i][q]), (d, i, q)


# ------------------------------------------------------------------ bolometric-sum inputs
SUM_SIZES = [(3, 5), (63, 34), (65, 37), (255, 5), (257, 34), (513, 37), (1000, 5), (3000, 34),
             (66049, 4)]


@pytest.mark.parametrize("n_lam,nL", SUM_SIZES)
def test_sum_inputs_give_every_term_a_visible_share(n_lam, nL):
    """On the CPU stand-in of every size of the GPU cases: each term of each summed row is at
    least 100 n 2^-52 of the row's sum of |terms| — a dropped or doubled element moves the sum by
    100 times the bound asserted on the device — and the oracle's own trapezoid sums lie within
    that bound of the exact weighted sums."""
    from frei_amd.engine import trapz_weights
    case = R.sum_case(n_lam, nL)
    w = trapz_weights(case["lam"] * 1e-4)
    worst_share, worst = np.inf, 0.0
    for d in ("emit", "absorb"):
        o = R.oracle_sweep(case, d, case["g"], case["m_bar"], 1.0)
        sums = R.RowSums(w, case["up0"], case["down0"], o["up"], o["down"], case["F_toa"])
        for i, keys in R.sweep_rows(d, nL).items():
            for q, key in enumerate(keys):
                if key is None:
                    continue
                s, sa, tmin = sums(key)
                worst_share = min(worst_share, tmin / sa)
                assert tmin / sa >= 100 * n_lam * R.U, (d, i, q, tmin / sa)
                assert abs(o["bol"][i, q] - s) <= 3 * n_lam * R.U * sa, (d, i, q)
                worst = max(worst, abs(o["bol"][i, q] - s) / _ulp(s))
    print(f"{n_lam} x {nL}: smallest share {worst_share:.2e} (needs {100 * n_lam * R.U:.2e}); "
          f"np.trapz {worst:.1f} ulp from exact")


# ------------------------------------------------------------------ layer_dT_ref
def _family_layers(family):
    """Every (direction, g, m_bar, alpha, layer) of a family's stand-in: the oracle's dT and
    layer_dT_ref at the oracle's bolometric sums."""
    case = R.family_case(family, n_lam=128)       # (dT depends on the rows through bol alone)
    p_cgs = case["p"] * O.BAR
    ptop = R.oracle_p_top2(case["p"])
    out = []
    for g in R.GRAVITIES:
        for m_bar in R.M_BARS:
            for alpha in R.ALPHAS:
                for d in ("emit", "absorb"):
                    o = R.oracle_sweep(case, d, g, m_bar, alpha)
                    for i in o["rows"]:
                        args = R.step_inputs(d, i, case["T"], p_cgs, ptop)
                        ref = R.layer_dT_ref(o["bol"][i], *args, g, m_bar, alpha)
                        out.append((d, g, m_bar, alpha, i, o["dT"][i], ref))
    return out


@pytest.fixture(scope="module")
def family_layers():
    return {f: _family_layers(f) for f in R.FAMILIES}


@pytest.mark.parametrize("family", R.FAMILIES)
def test_layer_dT_ref_agrees_with_oracle_within_its_bound(family_layers, family):
    worst = 0.0
    for d, g, m_bar, alpha, i, dT, ref in family_layers[family]:
        assert np.isfinite(dT) and ref.bound > 0
        assert abs(dT - ref.value) <= ref.bound, (d, g, m_bar, alpha, i, dT, ref)
        worst = max(worst, abs(dT - ref.value) / ref.bound)
    print(f"{family}: oracle within {worst:.3f} of the bound")


@pytest.mark.parametrize("family", R.FAMILIES)
def test_family_input_conditions(family_layers, family):
    layers = family_layers[family]
    conv = [r.convective for *_, r in layers]
    for d, g, m_bar, alpha, i, dT, ref in layers:
        # no rounding can flip the branch; the bound is tight enough for the test to have teeth
        assert abs(ref.dg_rel) >= 1e-6, (d, g, m_bar, alpha, i, ref)
        assert ref.bound <= 1e-9 * abs(ref.value), (d, g, m_bar, alpha, i, ref)
    if family in ("isothermal", "inverted"):
        assert not any(conv)
    elif family == "superadiabatic":
        # every layer but emit's top one (T_2 = T_1 there: radiative by construction)
        assert all(r.convective != (d == "emit" and i == 23)
                   for d, g, m_bar, alpha, i, dT, r in layers)
    else:
        assert any(conv) and not all(conv)
    worst = max(r.bound / abs(r.value) for *_, r in layers)
    print(f"{family}: {sum(conv)} of {len(conv)} convective, bound <= {worst:.2e} relative, "
          f"min |dg| {min(abs(r.dg_rel) for *_, r in layers):.2e} g / c_p")


def test_families_cover_both_branches_and_both_min_outcomes(family_layers):
    refs = [r for f in R.FAMILIES for *_, r in family_layers[f]]
    assert any(r.convective for r in refs) and any(not r.convective for r in refs)
    picks = {r.conv_min for r in refs if r.convective}
    assert picks == {True, False}, picks
    for f in R.FAMILIES:
        c = [r.conv_min for *_, r in family_layers[f] if r.convective]
        print(f"{f}: min() took dt_conv in {sum(c)} and dt_rad in {len(c) - sum(c)} layers")


def test_layer_dT_m_bar_roles():
    """What the planet's m_bar and delta_temperature's default one (Q7) each decide.  rho0 cp0 =
    (dp / g) m0 g / (k T lnp) * 7 k / (2 m0) holds no m0 at all, so forming rho0 and cp0 with
    the planet's m_bar instead of the default changes dT by rounding alone (a few ulp, inside any
    bound): no accuracy test can see that swap, on the device or here.  The planet's m_bar
    itself cancels on the radiative branch too (dz and c_p both go as 1 / m_bar) and reaches dT
    through the mixing length of a convective layer, lmix ~ alpha / m_bar: there doubling it
    moves dT by far more than the bound, which is what the doubled-m_bar cases hold."""
    m0 = float(O.M_BAR_DEFAULT)
    Fb = (3.1e8, 1.2e8, 2.9e8, 1.5e8)
    rad = (1500.0, 1400.0, 1e6, 7e5, 2479.0)
    conv = (1500.0, 1100.0, 1e6, 7e5, 2479.0)
    for args in (rad, conv):
        a = R.layer_dT_ref(Fb, *args, 2 * m0, 1.0)
        assert abs(a.value - O.layer_dT(Fb, *args, 2 * m0, 1.0)) <= a.bound
    a, b = R.layer_dT_ref(Fb, *rad, 2 * m0, 1.0), R.layer_dT_ref(Fb, *rad, m0, 1.0)
    assert not a.convective and abs(a.value - b.value) <= a.bound
    a, b = R.layer_dT_ref(Fb, *conv, 2 * m0, 1.0), R.layer_dT_ref(Fb, *conv, m0, 1.0)
    assert a.convective and abs(a.value - b.value) > 1e6 * a.bound
    # the swap itself, in double: rho0 and cp0 from 2 m0 instead of m0
    for m in (m0, 2 * m0):
        rc = O.rho_p(1e6, 7e5, 1500.0, 2479.0, m) * O.c_p(m)
        assert abs(rc - 3.5 * 3e5 / 2479.0 * 2479.0 / (1500.0 * np.log(1e6 / 7e5))) <= 8 * R.U * rc


def test_zero_flux_layer_is_exactly_zero():
    """x = 0: the guard gives f = 1 and dT = 0 (without it, 1e5 / 0 ** 0.9 = inf and inf * 0)."""
    r = R.layer_dT_ref((0.0, 0.0, 0.0, 0.0), 1.0, 1.0, 1e6, 7e5, 2479.0, R.M_BAR, 1.0)
    assert r.value == 0.0 and r.bound == 0.0 and not r.convective
    assert O.layer_dT((0.0, 0.0, 0.0, 0.0), 1.0, 1.0, 1e6, 7e5, 2479.0, R.M_BAR, 1.0) == 0.0


def test_zero_flux_stand_in_is_zero_everywhere():
    """The GPU x == 0 case on the oracle: T = 1 K, F_TOA = 0, zero fluxes — Planck's expm1
    overflows at every wavelength, every row and sum is 0, and every dT is exactly 0."""
    case = dict(R.family_case("isothermal", n_lam=128))
    nL, n_lam = case["up0"].shape
    case.update(T=np.ones(nL), up0=np.zeros((nL, n_lam)), down0=np.zeros((nL, n_lam)),
                F_toa=np.zeros(n_lam))
    assert np.all(O.H * O.C / (case["lam"] * 1e-4 * O.K_B * 1.0) > 1400)
    for d in ("emit", "absorb"):
        with np.errstate(over="ignore"):
            o = R.oracle_sweep(case, d, R.G_J, R.M_BAR, 1.0)
        assert np.all(o["up"] == 0) and np.all(o["down"] == 0) and np.all(o["bol"] == 0)
        assert np.all(o["dT"] == 0)


# ------------------------------------------------------------------ replay_convergence
@pytest.fixture(scope="module")
def full_histories():
    """The 40-iteration histories of both cases (no stop): every other setting's run is a
    prefix of them."""
    return {k: R.oracle_run(R.conv_case(k), 10 ** 6, -1.0)[0] for k in ("flips", "dT")}


@pytest.mark.parametrize("kind,nzc,thr", [("flips", 2, -1.0), ("dT", 10 ** 6, 3.0)])
def test_replay_reproduces_the_oracle_iteration_count(full_histories, kind, nzc, thr):
    """Two oracle runs, one stopped by the flip count alone and one by |dT| alone."""
    hist, n_iter = R.oracle_run(R.conv_case(kind), nzc, thr)
    assert hist.shape == (20, 2 * n_iter) and 1 < n_iter < R.CONV_STEPS
    assert R.replay_convergence(hist, nzc, thr) == n_iter
    assert R.replay_convergence(hist[:, :2 * (n_iter - 1)], nzc, thr) is None
    assert np.array_equal(hist, full_histories[kind][:, :2 * n_iter])
    adt = R.abs_dT_of_history(hist)
    if kind == "flips":
        assert not np.all(adt[:, -1] < 3.0)          # the |dT| test would not have stopped it
    else:
        assert np.all(adt[:, -1] < thr) and R.replay_convergence(hist, 10 ** 6, -1.0) is None
    print(f"{kind}: n_zero_crossings {nzc} convergence_dT {thr} stops after {n_iter}")


@pytest.mark.parametrize("kind", ["flips", "dT"])
def test_convergence_cases_stop_where_the_gpu_cases_need_them(full_histories, kind):
    """Every setting of the GPU cases, replayed on the oracle's 40-iteration history: the
    flip-stopped runs stop on flips before the 40 iterations are over, at different iterations,
    and no |dT| lies within 1e-9 of a threshold."""
    hist = full_histories[kind]
    assert hist.shape == (20, 2 * R.CONV_STEPS) and np.all(np.isfinite(hist))
    stops = {s: R.replay_convergence(hist, *s) for s in R.CONV_SETTINGS}
    print(kind, stops)
    adt = R.abs_dT_of_history(hist)
    assert not np.any(np.abs(adt - 3.0) < 1e-9)
    if kind == "flips":
        flip = [stops[(z, -1.0)] for z in (0, 1, 2, 5)]
        assert all(k is not None and k < R.CONV_STEPS for k in flip)
        assert flip == sorted(flip) and len(set(flip)) >= 3 and flip[0] > 1
        assert stops[(10 ** 6, 3.0)] is None and stops[(2, 3.0)] == stops[(2, -1.0)]
    else:
        assert all(stops[(z, -1.0)] is None for z in (0, 1, 2, 5))
        assert 1 < stops[(10 ** 6, 3.0)] < R.CONV_STEPS
        assert stops[(2, 3.0)] == stops[(10 ** 6, 3.0)]


