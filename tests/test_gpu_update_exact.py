"""The update of the T-P loop against exact references (tests/updateref.py), one level above
tests/test_gpu_math.py: (a) the bolometric sums ``bol`` of ``frei_sweep`` against the exactly
rounded sum of w_j F_j over the flux rows the device itself holds, in every sweep form and for
wavelength slices; (b) the per-layer dT against ``oracle.layer_dT`` in 60-digit arithmetic with a
running rounding-error bound, on profiles that take each branch on purpose; (c) the convergence
bookkeeping (iter / conv / history) against the oracle's ``converged()`` replayed on the device's
own history.  The inputs are those whose CPU stand-ins tests/test_update_ref_host.py checks (the
row bookkeeping against oracle._sweep, every term's share of its row sum, |dg| >= 1e-6 g / c_p,
bound <= 1e-9 relative, both branches, both outcomes of min()).

Bounds, none taken from the code under test:
  bol   |bol - exact| <= n_lam 2^-52 sum |w_j F_j|: the any-order bound of n products and n - 1
        additions.  Every term is >= 100 n 2^-52 of its row's sum (asserted on the rows read
        back), so a dropped or doubled element misses the bound a hundredfold.
  dT    |dT - ref| <= 2 x bound; the bound is first order (the factor 2 covers the second order),
        0.5 ulp for + - * / sqrt and 2 ulp for log and pow — no document under the ROCm
        installation states the device library's bounds for them, so updateref's fallback holds.
  conv  n_iter equals the replay's first stop exactly; the history has 2 n_iter columns; no |dT|
        lies within 1e-9 of convergence_dT, so the replay's |T_before - T_after| decides as the
        device's |dT| does.

Forms are selected by the options of the README's FREI_* knobs and asserted through
``Engine.path()`` as far as it reports them (lanes per wavelength, producer/consumer consumers,
two wavelengths per lane, contraction, trailing update) and through ``chain_count`` /
``tail_count``; path() does not report FREI_RED_STAGE / FREI_RED_ROWS or FREI_FUSED_UPDATE, which
are set on forms it does report.

Not reachable through the ABI and left out:
  - bol and dT of the chained, trailing and batched updates are not readable (``frei_sweep``
    returns them for the separate and fused update kernels only): they stay held bitwise to the
    forms here by test_gpu_chain.py, test_gpu_tail.py and the batch tests; their bookkeeping is
    held here through the history.
  - multi-rank sums: test_gpu_multirank.py.
  - a one-wavelength slice: frei_ctx_create refuses n_lam < 2 (asserted below), so the cut at 1
    yields the slices [0, 2) — which holds the left end weight and the first interior one — and
    [1, 257) instead of [0, 1) and [1, 257); the slices then overlap at j = 1, and the
    additivity of the exact slice sums is checked on the cuts 0, 1, 257, 700, n of the rows
    themselves.
  - forming rho0 / cp0 with the planet's m_bar instead of the default cannot be seen by any
    accuracy test: rho0 cp0 = 3.5 dp / (T lnp) holds no m_bar (test_update_ref_host.py
    test_layer_dT_m_bar_roles).  The doubled-m_bar cases hold m_bar's real path, the mixing
    length of the convective layers.

Measured on MI355X (each test prints its figures, pytest -s), errors in ulps of the exact sum:
  bol, default form      3 / 63 / 255 / 1000 x 5: 1; 63 / 257 / 3000 x 34: 2; 65 / 513 x 37: 3;
                         66 049 x 4 (two lanes per wavelength, 517 partial-sum columns): 1
  bol, per form          (worst of 257 x 34 and 1000 x 37; lam2 of 1000 x 37 and 3000 x 34)
                         one lane 3; 2 lanes x 4 / 8 waves 3 / 3; 4 lanes x 4 / 8 waves 3 / 3;
                         one lane staged / rows / full 3 / 3 / 3; 4 lanes rows / full 4 / 2;
                         two wavelengths per lane 2; producer/consumer 1 / 2 / 4 consumers
                         3 / 2 / 3; per-species (precontract 0) 3; fused update 0 / 1 3 / 3;
                         one lane with the separate update 3
  bol, slices            [0, 2), [1, 257), [257, 700), [700, 1000): 1 each
                         (the terms are positive, so the bound is n_lam to 2 n_lam ulp of the
                         sum; the oracle's np.trapz on the stand-in rows is 1 to 4 ulp from exact)
  dT error / bound       isothermal 0.075, inverted 0.099, steep (convective) 0.027, mixed 0.054
                         (four convective layers per sweep, min() taking dt_conv in one and
                         dt_rad in three), the same with the fused and the separate update kernel
                         (the oracle's own double evaluation on the stand-ins: 0.073, 0.079,
                         0.011, 0.059); the bound itself is <= 1.6e-10 |dT| in every layer
  x == 0                 every flux, sum and dT exactly 0, both update kernels
  convergence            20 x 512: flips case n_iter 12, 14, 14, 18 for n_zero_crossings 0, 1, 2,
                         5, 40 for (1e6, 3.0), 14 for (2, 3.0); |dT| case 40 four times, then 7
                         and 7 — the same in the default (chained), separate-update, unchained
                         and chained one-lane forms; 30 x 5000 producer/consumer with and
                         without the trailing update: 8, 9, 9, 13, 40, 9; batched 7, 14, 21, 31
  log / pow ulp bounds   2 and 2 (updateref.py's fallback: no document under the ROCm
                         installation states them)
Arithmetic-only mutations of a scratch copy of the kernels, loaded through FREI_HIP_LIB:
  - the weight of a 256-wavelength block's last wavelength multiplied by 0 (every sweep kernel
    but the two-wavelength one): 23 tests fail — the default form from 257 wavelengths up, every
    form but lam2, the slices;
  - ``flips >= n_zero_crossings`` for ``>`` at its single site (layer_bookkeep, called by
    update_kernel, update_fused_body and tail_update_slot): all 12 cases of
    test_convergence_bookkeeping_matches_replay (the six CONV_FORMS, flips and dT, each at its
    first run: n_iter 1 instead of 40 with n_zero_crossings 0) and the batched test fail;
  - the mixing length formed with the default m_bar instead of the planet's: the steep and the
    mixed family fail with both update kernels;
  - rho0 / cp0 formed with the planet's m_bar: nothing fails, as the algebra above says.
"""
import functools
import math

import numpy as np
import pytest

from oracle import frei_oracle as O
from tests import updateref as R

pytestmark = pytest.mark.gpu

EMIT, ABSORB = 0, 1
DIRS = ((EMIT, "emit"), (ABSORB, "absorb"))


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _ulp(x):
    return math.ulp(abs(float(x)))


@functools.lru_cache(maxsize=None)
def _sum_case(n_lam, nL):
    return R.sum_case(n_lam, nL)


def _engine(fa, case, g=R.G_J, m_bar=R.M_BAR, **kw):
    tabs = {n: fa.OpacityTable(v, case["p"], case["Tn"]) for n, v in case["vals"].items()}
    return fa.Engine(case["lam"], case["p"], tabs, g=g, m_bar=m_bar, F_toa=case["F_toa"], **kw)


def _sweeps(eng, case, alpha=1.0, lo=0, hi=None):
    """One sweep each way from the case's state -> {direction: dict(dT, bol, up, down)}."""
    out = {}
    for d, _ in DIRS:
        eng.set_temperatures(case["T"])
        eng.set_fluxes(case["up0"][:, lo:hi], case["down0"][:, lo:hi])
        dT, bol, _ = eng.sweep(d, alpha=alpha, want_dtaus=False)
        up, down = eng.get_fluxes()
        out[d] = dict(dT=dT, bol=bol, up=up, down=down)
    return out


def _check_sums(res, case, w, lo=0, hi=None, what=""):
    """bol of both sweeps against exact_dot over the rows read back; worst error in ulps."""
    n, nL = w.size, len(case["p"])
    worst, share = 0.0, np.inf
    for d, name in DIRS:
        r = res[d]
        assert np.all(np.isfinite(r["bol"])) and np.all(np.isfinite(r["up"]))
        sums = R.RowSums(w, case["up0"][:, lo:hi], case["down0"][:, lo:hi], r["up"], r["down"],
                         case["F_toa"][lo:hi])
        for i, keys in R.sweep_rows(name, nL).items():
            for q, key in enumerate(keys):
                if key is None:        # the top emit layer's F_2_up is not stored
                    continue
                s, sa, tmin = sums(key)
                share = min(share, tmin / sa)
                assert tmin / sa >= 100 * n * R.U, (what, name, i, q, tmin / sa)
                err = abs(r["bol"][i, q] - s)
                assert err <= n * R.U * sa, (what, name, i, q, r["bol"][i, q], s, err / _ulp(s))
                worst = max(worst, err / _ulp(s))
        skipped = 0 if name == "emit" else nL - 1
        assert np.all(r["bol"][skipped] == 0) and r["dT"][skipped] == 0
    return worst, share


# ------------------------------------------------------------------ (a) bolometric sums
SIZES = [(3, 5), (63, 34), (65, 37), (255, 5), (257, 34), (513, 37), (1000, 5), (3000, 34),
         (66049, 4)]


@pytest.mark.parametrize("n_lam,nL", SIZES)
def test_bolometric_sums_exact_default_form(fa, n_lam, nL):
    """Every size in the form the context chooses by itself (66 049 wavelengths: more than 256
    partial-sum columns, the strided block-partial loop of the reduction)."""
    case = _sum_case(n_lam, nL)
    eng = _engine(fa, case)
    try:
        path = eng.path()
        res = _sweeps(eng, case)
        w = eng.wtr
    finally:
        eng.close()
    assert path["fast"] and path["contracted"], path
    worst, share = _check_sums(res, case, w, what=f"default {n_lam}x{nL}")
    print(f"default {n_lam} x {nL} (quad {path['quad']} paired {path['paired']}): bol within "
          f"{worst:.2f} ulp of exact (bound {n_lam} ulp of sum|wF|), smallest share {share:.1e}")


def _lanes(p):
    return 4 if p["quad"] else 2 if p["paired"] else 1


ONE = dict(group_q=1)
FORMS = {
    "one_lane": (ONE, lambda p: _lanes(p) == 1 and not p["pipe"] and not p["lam2"]),
    "q2_w4": (dict(group_q=2, group_waves=4), lambda p: _lanes(p) == 2 and not p["pipe"]),
    "q2_w8": (dict(group_q=2, group_waves=8), lambda p: _lanes(p) == 2 and not p["pipe"]),
    "q4_w4": (dict(group_q=4, group_waves=4), lambda p: _lanes(p) == 4 and not p["pipe"]),
    "q4_w8": (dict(group_q=4, group_waves=8), lambda p: _lanes(p) == 4 and not p["pipe"]),
    "one_lane_stage": (dict(ONE, red_stage=1), lambda p: _lanes(p) == 1 and not p["pipe"]),
    "one_lane_rows": (dict(ONE, red_stage=0, red_rows=1), lambda p: _lanes(p) == 1),
    "one_lane_full": (dict(ONE, red_stage=0, red_rows=0), lambda p: _lanes(p) == 1),
    "q4_rows": (dict(group_q=4, red_stage=0, red_rows=1), lambda p: _lanes(p) == 4),
    "q4_full": (dict(group_q=4, red_stage=0, red_rows=0), lambda p: _lanes(p) == 4),
    "lam2": (dict(ONE, shared=0, lam2=1), lambda p: p["lam2"] and not p["lds_steps"]),
    "pipe1": (dict(pipe=1), lambda p: p["pipe"] == 1),
    "pipe2": (dict(pipe=2), lambda p: p["pipe"] == 2),
    "pipe4": (dict(pipe=4), lambda p: p["pipe"] == 4),
    "precontract0": (dict(precontract=0), lambda p: p["fast"] and not p["contracted"]),
    "fused0": (dict(fused_update=0), lambda p: p["contracted"]),
    "fused1": (dict(fused_update=1), lambda p: p["contracted"]),
    "one_lane_fused0": (dict(ONE, fused_update=0), lambda p: _lanes(p) == 1),
}
FORM_SIZES = [(257, 34), (1000, 37)]
LAM2_SIZES = [(1000, 37), (3000, 34)]          # two wavelengths per lane: even counts only


@pytest.mark.parametrize("form", list(FORMS))
def test_bolometric_sums_exact_every_form(fa, form):
    """Every sweep form at two ragged sizes (no multiple of a block, odd and even step counts)."""
    opts, taken = FORMS[form]
    for n_lam, nL in (LAM2_SIZES if form == "lam2" else FORM_SIZES):
        case = _sum_case(n_lam, nL)
        eng = _engine(fa, case)
        try:
            for k, v in opts.items():
                eng.set_option(k, v)
            path = eng.path()
            res = _sweeps(eng, case)
            w = eng.wtr
        finally:
            eng.close()
        assert path["fast"] and taken(path), (form, path)
        worst, share = _check_sums(res, case, w, what=f"{form} {n_lam}x{nL}")
        print(f"{form} {n_lam} x {nL}: bol within {worst:.2f} ulp of exact")


def test_bolometric_sums_of_wavelength_slices(fa):
    """lam_slice contexts without a communicator sum their own slice only (frei_runtime.hip:
    nranks stays 1, so update_kernel's rank loop and the fused update add no peer sums): each
    slice's bol is the exact dot of its slice of the global weights with its own rows."""
    n_lam, nL = 1000, 5
    case = _sum_case(n_lam, nL)
    from frei_amd.engine import trapz_weights
    wg = trapz_weights(case["lam"] * 1e-4)
    with pytest.raises(RuntimeError, match="n_lam"):
        _engine(fa, case, lam_slice=(0, 1))          # a one-wavelength context is refused
    for lo, hi in ((0, 2), (1, 257), (257, 700), (700, n_lam)):
        eng = _engine(fa, case, lam_slice=(lo, hi))
        try:
            res = _sweeps(eng, case, lo=lo, hi=hi)
            w = eng.wtr
        finally:
            eng.close()
        assert np.array_equal(w, wg[lo:hi])
        worst, _ = _check_sums(res, case, w, lo, hi, what=f"slice {lo}:{hi}")
        print(f"slice [{lo}, {hi}): bol within {worst:.2f} ulp of exact")
    # the exact slice sums add up to the exact whole, on the whole context's own rows
    eng = _engine(fa, case)
    try:
        res = _sweeps(eng, case)
    finally:
        eng.close()
    cuts = [0, 1, 257, 700, n_lam]
    for row in (res[EMIT]["up"][2], res[ABSORB]["down"][1], case["down0"][3]):
        parts = sum(R.exact_dot_fraction(wg[a:b], row[a:b]) for a, b in zip(cuts[:-1], cuts[1:]))
        assert float(parts) == R.exact_dot(wg, row)[0]


# ------------------------------------------------------------------ (b) dT
def _check_dT(res, case, p_cgs, g, m_bar, alpha, what):
    nL = len(case["p"])
    ptop = R.device_p_top2(p_cgs)
    worst, kinds = 0.0, set()
    for d, name in DIRS:
        r = res[d]
        assert np.all(np.isfinite(r["dT"]))
        for i in R.sweep_rows(name, nL):
            args = R.step_inputs(name, i, case["T"], p_cgs, ptop)
            ref = R.layer_dT_ref(r["bol"][i], *args, g, m_bar, alpha)
            # the device's own sums leave the branch and the bound where the stand-ins had them
            assert abs(ref.dg_rel) >= 1e-6 and ref.bound <= 1e-9 * abs(ref.value), (what, i, ref)
            err = abs(r["dT"][i] - ref.value)
            assert err <= 2 * ref.bound, (what, name, i, r["dT"][i], ref, err / ref.bound)
            worst = max(worst, err / ref.bound)
            kinds.add((ref.convective, ref.conv_min))
    return worst, kinds


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_layer_dT_within_reference_bound(fa, family, fused):
    """24 layers x 1024 wavelengths, g = 300, 2479, 1e4, m_bar the default and twice it, alpha =
    0.5, 1, 2, both update kernels: dT against layer_dT_ref at the device's own bol."""
    case = R.family_case(family)
    worst, kinds = 0.0, set()
    for g in R.GRAVITIES:
        for m_bar in R.M_BARS:
            eng = _engine(fa, case, g=g, m_bar=m_bar)
            try:
                eng.set_option("fused_update", fused)
                p_cgs = np.array(eng.p_cgs)
                runs = [(alpha, _sweeps(eng, case, alpha)) for alpha in R.ALPHAS]
            finally:
                eng.close()
            for alpha, res in runs:
                w, k = _check_dT(res, case, p_cgs, g, m_bar, alpha,
                                 f"{family} g {g} m_bar {m_bar} alpha {alpha} fused {fused}")
                worst, kinds = max(worst, w), kinds | k
    conv = {c for c, _ in kinds}
    assert conv == {"isothermal": {False}, "inverted": {False}, "superadiabatic": {True, False},
                    "mixed": {True, False}}[family], kinds
    print(f"{family} fused_update {fused}: worst |dT - ref| / bound {worst:.3f}; "
          f"(convective, min took dt_conv) seen: {sorted(kinds, key=str)}")


@pytest.mark.parametrize("fused", [1, 0])
def test_zero_flux_gives_exactly_zero_dT(fa, fused):
    """The x == 0 guard: T = 1 K everywhere, F_TOA = 0 and zero fluxes.  Planck's expm1
    overflows at every wavelength (h c / (lambda k T) >= 1438), so B = 0, every flux row and
    every bolometric sum is 0, x = 0, and dT must be exactly 0 — 1e5 / pow(0, 0.9) * 0 is NaN."""
    case = dict(R.family_case("isothermal"))
    nL, n_lam = case["up0"].shape
    case.update(T=np.ones(nL), up0=np.zeros((nL, n_lam)), down0=np.zeros((nL, n_lam)),
                F_toa=np.zeros(n_lam))
    eng = _engine(fa, case)
    try:
        eng.set_option("fused_update", fused)
        res = _sweeps(eng, case)
    finally:
        eng.close()
    for d, name in DIRS:
        r = res[d]
        assert np.all(r["up"] == 0) and np.all(r["down"] == 0), name
        assert np.all(r["bol"] == 0), name
        assert np.all(np.isfinite(r["dT"])) and np.all(r["dT"] == 0), (name, r["dT"])


# ------------------------------------------------------------------ (c) convergence
def _check_run(r, nzc, thr, what):
    hist, n_iter = r["temp_hist"], r["n_iter"]
    assert hist.shape[1] == 2 * n_iter and np.all(np.isfinite(hist)), what
    k = R.replay_convergence(hist, nzc, thr)
    assert n_iter == (k if k is not None else R.CONV_STEPS), (what, n_iter, k)
    assert not np.any(np.abs(R.abs_dT_of_history(hist) - thr) < 1e-9), what
    return n_iter


CONV_FORMS = {
    # options, (nL, n_lam) of the flips / dT case, what the counters must show
    "default": (dict(), (20, 512), (20, 512)),
    "fused0": (dict(fused_update=0), (20, 512), (20, 512)),
    "chain0": (dict(chain=0), (20, 512), (20, 512)),
    "chain2_one_lane": (dict(group_q=1, chain=2), (20, 512), (20, 512)),
    "pipe4_tail1": (dict(pipe=4, tail=1), (30, 5000), (20, 5000)),
    "pipe4_tail0": (dict(pipe=4, tail=0), (30, 5000), (20, 5000)),
}


@pytest.mark.parametrize("kind", ["flips", "dT"])
@pytest.mark.parametrize("form", list(CONV_FORMS))
def test_convergence_bookkeeping_matches_replay(fa, form, kind):
    """frei_run's n_iter against the oracle's converged() replayed over the device's own history,
    for every (n_zero_crossings, convergence_dT) setting, 40 iterations at most.  The tail forms
    run the producer/consumer sweep at test_gpu_tail.py's 5000 wavelengths (30 layers where the
    case oscillates; the |dT|-stopped case keeps 20 layers, whose steps its start is sized for).
    Every layer stays in the replay: the end layers' differences are exact zeros."""
    opts, size_f, size_d = CONV_FORMS[form]
    nL, n_lam = size_f if kind == "flips" else size_d
    case = R.conv_case(kind, nL, n_lam)
    eng = _engine(fa, case)
    stops = {}
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        path = eng.path()
        c0, t0 = eng.chain_count(), eng.tail_count()
        for nzc, thr in R.CONV_SETTINGS:
            r = eng.run(case["T"], n_timesteps=R.CONV_STEPS, n_zero_crossings=nzc,
                        convergence_dT=thr, alpha=R.CONV_ALPHA, want_dtaus=False)
            stops[(nzc, thr)] = _check_run(r, nzc, thr, f"{form} {kind} {nzc} {thr}")
        chained, tailed = eng.chain_count() - c0, eng.tail_count() - t0
    finally:
        eng.close()
    assert path["fast"] and path["contracted"], path
    if form in ("default", "chain2_one_lane"):
        assert chained > 0 and tailed == 0, (chained, tailed)
    elif form == "pipe4_tail1":
        assert path["pipe"] == 4 and path["tail"] and tailed > 0 and chained == 0, (path, tailed)
    else:
        assert chained == 0 and tailed == 0, (chained, tailed)
    if form.startswith("pipe4"):
        assert path["pipe"] == 4, path
    if form == "chain2_one_lane":
        assert _lanes(path) == 1, path
    flip = [stops[(z, -1.0)] for z in (0, 1, 2, 5)]
    if kind == "flips":     # they stop on flips, before the 40 iterations are over
        assert all(1 < k < R.CONV_STEPS for k in flip) and flip == sorted(flip), stops
        assert stops[(10 ** 6, 3.0)] == R.CONV_STEPS
    elif nL == 20:
        assert all(k == R.CONV_STEPS for k in flip) and 1 < stops[(10 ** 6, 3.0)] < R.CONV_STEPS
    print(f"{form} {kind} {nL} x {n_lam}: n_iter {stops}")


def test_batched_convergence_matches_replay(fa):
    """Four atmospheres whose start temperatures (1300 to 1600 K) make them stop on flips at
    different iterations: each n_iter[m] is the replay of its own history."""
    case = R.conv_case("flips")
    T0 = np.array([np.full(20, t) for t in (1300.0, 1400.0, 1500.0, 1600.0)])
    tabs = {n: fa.OpacityTable(v, case["p"], case["Tn"]) for n, v in case["vals"].items()}
    eng = fa.BatchEngine(case["lam"], case["p"], tabs, g=np.full(4, R.G_J), m_bar=R.M_BAR,
                         F_toa=case["F_toa"])
    try:
        r = eng.run(T0, n_timesteps=R.CONV_STEPS, n_zero_crossings=2, convergence_dT=-1.0,
                    alpha=R.CONV_ALPHA, want_hist=True)
    finally:
        eng.close()
    n = [_check_run(dict(temp_hist=r["temp_hist"][m], n_iter=int(r["n_iter"][m])), 2, -1.0,
                    f"batch atmosphere {m}") for m in range(4)]
    assert len(set(n)) == 4 and all(1 < k < R.CONV_STEPS for k in n), n
    print(f"batched: n_iter {n}")
