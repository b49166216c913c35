"""Exact references of the T-P update (test infrastructure, plain Python, no GPU): the
bolometric sums of a sweep, the per-layer dT physics and the convergence bookkeeping.

``exact_dot``           the correctly rounded sum of w_j F_j over one row (error-free products,
                        ``math.fsum``), with sum |w_j F_j|; ``exact_dot_fraction`` is the same
                        sum as an unrounded Fraction.
``layer_dT_ref``        ``oracle.frei_oracle.layer_dT`` in mpmath at 60 digits from the doubles
                        given, with a first-order running bound of the rounding error of its
                        double evaluation.
``replay_convergence``  the oracle's ``converged()`` replayed over the first k column pairs of a
                        temperature history, k = 1..n.
``sweep_rows``          which flux rows each step of an emit / absorb sweep sums, from the flux
                        arrays before and after the sweep.
"""
import functools
import math
from collections import namedtuple
from fractions import Fraction

import mpmath
import numpy as np

from oracle import frei_oracle as O

U = 2.0 ** -52                    # one ulp of a double, relative to the result (upper bound)
_SPLIT = 134217729.0              # 2^27 + 1 (Veltkamp)


# ------------------------------------------------------------------ bolometric sums
def _two_product(a, b):
    """Dekker's error-free product on arrays: a * b = hi + lo exactly (no FMA needed; exact
    while no intermediate overflows or underflows: |a b| in [1e-250, 1e250] is asserted)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    hi = a * b
    nz = hi != 0
    assert np.all((np.abs(hi[nz]) > 1e-250) & (np.abs(hi[nz]) < 1e250)), "two-product range"
    t = _SPLIT * a
    a1 = t - (t - a)
    a2 = a - a1
    t = _SPLIT * b
    b1 = t - (t - b)
    b2 = b - b1
    lo = a2 * b2 - (((hi - a1 * b1) - a2 * b1) - a1 * b2)
    return hi, lo


def exact_dot(w, F):
    """(sum_j w_j F_j, sum_j |w_j F_j|), each the correctly rounded value of the exact sum:
    every product is split into hi + lo without error and math.fsum adds the 2 n parts exactly,
    rounding once."""
    hi, lo = _two_product(w, F)
    s = np.where(hi < 0, -1.0, 1.0)          # |hi + lo| = sign(hi) (hi + lo): |lo| <= ulp(hi) / 2
    return (math.fsum(np.concatenate([hi, lo]).tolist()),
            math.fsum(np.concatenate([s * hi, s * lo]).tolist()))


def exact_dot_fraction(w, F):
    """sum_j w_j F_j as an unrounded Fraction (small n: the cross-check of exact_dot and the
    slice sums' additivity)."""
    return sum((Fraction(float(a)) * Fraction(float(b)) for a, b in zip(w, F)), Fraction(0))


def exact_trapz_weights(lam_cm):
    """The trapezoid weights of np.trapz on the grid as Fractions of the doubles given: the ends
    (lam_1 - lam_0) / 2 and (lam_{n-1} - lam_{n-2}) / 2, interior (lam_{j+1} - lam_{j-1}) / 2."""
    x = [Fraction(float(v)) for v in lam_cm]
    n = len(x)
    w = []
    for j in range(n):
        lo = x[j - 1] if j > 0 else x[0]
        hi = x[j + 1] if j < n - 1 else x[n - 1]
        w.append((hi - lo) / 2)
    return w


def sweep_rows(direction, nL):
    """{layer i: (F_2_up, F_2_down, F_1_up, F_1_down)} — where the four rows (bol's order) that
    the step of layer i sums are found in the flux arrays before ("up_old", "down_old") and
    after ("up_new", "down_new") one sweep, as (array, row) keys; ("toa", 0) is F_TOA.
    oracle._sweep: emit walks upward and reads the old F_down above it; absorb walks downward
    and reads the old F_up of its own layer.  The top emit layer's F_2_up is not stored: None."""
    rows = {}
    if direction == "emit":
        for i in range(1, nL):
            top = i == nL - 1
            rows[i] = (None if top else ("up_new", i + 1),
                       ("toa", 0) if top else ("down_old", i + 1),
                       ("up_new", i), ("down_new", i))
    else:
        for i in range(nL - 2, -1, -1):
            rows[i] = (("up_new", i + 1), ("down_new", i + 1), ("up_old", i), ("down_new", i))
    return rows


class RowSums:
    """exact_dot(w, row) of the rows sweep_rows names, each row summed once."""

    def __init__(self, w, up_old, down_old, up_new, down_new, F_toa):
        self.w = np.asarray(w, dtype=float)
        self.arrays = dict(up_old=up_old, down_old=down_old, up_new=up_new, down_new=down_new,
                           toa=np.asarray(F_toa, dtype=float)[None, :])
        self._sums = {}

    def row(self, key):
        return self.arrays[key[0]][key[1]]

    def __call__(self, key):
        """(exact sum, sum of |terms|, smallest |term|) of the row ``key``."""
        if key not in self._sums:
            r = self.row(key)
            s, sa = exact_dot(self.w, r)
            self._sums[key] = (s, sa, float(np.min(np.abs(self.w * r))))
        return self._sums[key]


# ------------------------------------------------------------------ layer physics
_mp = mpmath.mpf


def _at_60_digits(fn):
    """Run ``fn`` at 60 decimal digits, leaving mpmath's global precision as it was."""
    @functools.wraps(fn)
    def wrapped(*args, **kwargs):
        with mpmath.workdps(60):
            return fn(*args, **kwargs)
    return wrapped

# ulp bounds of the double operations.  + - * / and sqrt are correctly rounded (the build has
# -ffp-contract=off and no fast-math): half an ulp.  No document under the ROCm installation
# states the device library's bounds for log and pow, so both take 2 ulp.
ULP_BASIC = 0.5
ULP_LOG = 2.0
ULP_POW = 2.0

LayerRef = namedtuple("LayerRef", "value bound convective dg_rel conv_min")


class _V:
    """A high-precision value with an absolute bound of the error its double evaluation has."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v = _mp(v)
        self.e = _mp(e)

    def _done(self, ulps):
        self.e += ulps * U * abs(self.v)
        return self


def _c(x):
    return x if isinstance(x, _V) else _V(float(x))


def _add(a, b):
    a, b = _c(a), _c(b)
    return _V(a.v + b.v, a.e + b.e)._done(ULP_BASIC)


def _sub(a, b):
    a, b = _c(a), _c(b)
    return _V(a.v - b.v, a.e + b.e)._done(ULP_BASIC)     # a cancellation keeps a.e + b.e


def _mul(a, b):
    a, b = _c(a), _c(b)
    return _V(a.v * b.v, abs(a.v) * b.e + abs(b.v) * a.e)._done(ULP_BASIC)


def _div(a, b):
    a, b = _c(a), _c(b)
    q = a.v / b.v
    return _V(q, a.e / abs(b.v) + abs(q) * b.e / abs(b.v))._done(ULP_BASIC)


def _sqrt(a):
    r = mpmath.sqrt(a.v)
    return _V(r, a.e / (2 * r))._done(ULP_BASIC)


def _log(a):
    return _V(mpmath.log(a.v), a.e / abs(a.v))._done(ULP_LOG)


def _pow(a, y):
    """a ** y for an exact double exponent y."""
    r = mpmath.power(a.v, _mp(y))
    return _V(r, abs(y) * abs(r) * a.e / abs(a.v) if a.v != 0 else 0)._done(ULP_POW)


def _delta_z(T, lnp, g, m_bar):
    return _mul(_div(_mul(O.K_B, T), _mul(m_bar, g)), lnp)


def _c_p(m_bar):
    return _mul(_div(7.0, _mul(2.0, m_bar)), O.K_B)


@_at_60_digits
def layer_dT_ref(Fb, T1, T2, p1, p2, g, m_bar, alpha):
    """oracle.frei_oracle.layer_dT from the doubles given, in mpmath at 60 digits, with the
    oracle's double constants (K_B, SIGMA_SB, M_BAR_DEFAULT = the double 2.4 * M_P).

    Alongside the value a first-order running error bound of the double evaluation is carried:
    every rounded operation adds its ulp bound times |result| 2^-52, and the errors of the
    operands propagate by the usual rules (sum of absolute errors through + and -, so the
    cancellations in (F2u - F2d) - (F1u - F1d), dF_rad + dF_conv and (T1 - T2) / dz - g / c_p
    amplify as they do; relative errors add through * and /, halve through sqrt, scale by |y|
    through pow(., y), and log turns a relative error into an absolute one).  The operations are
    the device's (frei_kernels.hip layer_pre / layer_dT_post), which are the oracle's with
    lmix * lmix for lmix ** 2 and sqrt for ** 0.5: lnp = log(p1 / p2) is formed once in double (a
    division and a log) and used by both delta_z calls; dz, c_p, rho, dg, lmix, dF_conv, dt_rad
    (pow(T1, 3)), dt_conv, dF_rad, div, x = div dz, f = 1e5 / pow(|x|, 0.9), min(dt_rad,
    dt_conv) (its error is at most the larger of its operands'), rho0 and cp0 with the default
    m_bar, and 1 / rho0 / cp0 * div * dt.

    ulp bounds: 0.5 for + - * / sqrt; 2 for log and pow — no document under the ROCm
    installation states the device library's bounds, so the fallback holds for both.

    Returns LayerRef(value, bound, convective, dg_rel, conv_min): value and bound as floats
    (the bound rounded up), the branch taken (dg > 0), dg / (g / c_p) — the relative distance of
    dg from the switch — and whether min() took dt_conv (None on the radiative branch)."""
    F2u, F2d, F1u, F1d = (float(v) for v in Fb)
    T1, T2, p1, p2, g, m_bar, alpha = (float(v) for v in (T1, T2, p1, p2, g, m_bar, alpha))
    lnp = _log(_div(p1, p2))
    dz = _delta_z(T1, lnp, g, m_bar)
    cp = _c_p(m_bar)
    dp_g = _div(_sub(p1, p2), g)
    rho = _div(dp_g, dz)
    g_cp = _div(g, cp)
    dg = _sub(_div(_sub(T1, T2), dz), g_cp)
    conv = dg.v > 0
    dt_rad = _div(_div(_div(_mul(cp, p1), O.SIGMA_SB), g), _pow(_c(T1), 3.0))
    conv_min = None
    if conv:
        lmix = _div(_mul(_mul(alpha, O.K_B), T1), _mul(m_bar, g))
        dF_conv = _mul(_mul(_mul(_mul(rho, cp), _mul(lmix, lmix)), _sqrt(_div(g, T1))),
                       _pow(dg, 1.5))
        dt_conv = _sqrt(_div(_div(T1, g), dg))
        conv_min = bool(dt_conv.v < dt_rad.v)
        dt_min = _V(min(dt_rad.v, dt_conv.v), max(dt_rad.e, dt_conv.e))
    else:
        dF_conv = _V(0)
        dt_min = dt_rad
    dF_rad = _sub(_sub(F2u, F2d), _sub(F1u, F1d))
    div = _div(_add(dF_rad, dF_conv), dz)
    x = _mul(div, dz)
    if x.v != 0:
        ax = _V(abs(x.v), x.e)
        f = _div(1e5, _pow(ax, 0.9))
    else:
        f = _V(1)
    dt = _mul(f, dt_min)
    m0 = float(O.M_BAR_DEFAULT)
    rho0 = _div(dp_g, _delta_z(T1, lnp, g, m0))
    out = _mul(_mul(_div(_div(1.0, rho0), _c_p(m0)), div), dt)
    bound = float(out.e) * (1 + 2.0 ** -40)
    return LayerRef(float(out.v), bound, bool(conv), float(dg.v / g_cp.v), conv_min)


def step_inputs(direction, i, T, p_cgs, p_top2):
    """(T1, T2, p1, p2) of layer i's step (oracle._sweep): the top emit layer takes the
    extrapolated ``p_top2`` = p[-1] p[-2] / p[-3] with T2 = T1.  The caller forms p_top2 as the
    code under comparison does: the oracle in bar, then scaled (``oracle_p_top2``); the device
    from the cgs pressures (``device_p_top2``) — the two doubles can differ by an ulp."""
    nL = len(T)
    if direction == "emit" and i == nL - 1:
        return T[i], T[i], p_cgs[i], p_top2
    return T[i], T[i + 1], p_cgs[i], p_cgs[i + 1]


def oracle_p_top2(p_bar):
    return (p_bar[-1] * p_bar[-2] / p_bar[-3]) * O.BAR


def device_p_top2(p_cgs):
    return p_cgs[-1] * p_cgs[-2] / p_cgs[-3]


# ------------------------------------------------------------------ convergence bookkeeping
def replay_convergence(temp_hist, n_zero_crossings, convergence_dT):
    """The first k (1-based) at which oracle.converged() holds on the first k column pairs
    [T_before, T_after] of ``temp_hist`` (n_layers, 2 n), or None when it never does.  |dT| of
    the k-th absorb sweep is |T_before - T_after| of its pair.  Every layer stays in the replay:
    the bottom layer never moves in absorb, so its differences are 0 (np.sign 0 against +-1)."""
    th = np.asarray(temp_hist, dtype=float)
    n = th.shape[1] // 2
    for k in range(1, n + 1):
        hists = [th[:, 2 * q:2 * q + 2] for q in range(k)]
        dT = th[:, 2 * k - 2] - th[:, 2 * k - 1]
        if O.converged(hists, dT, n_zero_crossings, convergence_dT):
            return k
    return None


def abs_dT_of_history(temp_hist):
    """|T_before - T_after| of every absorb pair, (n_layers, n)."""
    th = np.asarray(temp_hist, dtype=float)
    return np.abs(th[:, 0::2] - th[:, 1::2])


# ------------------------------------------------------------------ shared inputs
# The host tests run these inputs through the oracle (the CPU stand-ins of the GPU cases); the
# GPU tests run the same inputs through the engine.
G_J, M_BAR = 2478.6519476149147, 4.0142926168559996e-24
SPIKE_AT = (0, 63, 64, 255, 256, -1)


def flux_rows(rng, nL, n_lam):
    """Random positive rows inside 1e8..1e12 (up) and 1e6..1e11 (down): every row has its own
    level, drawn over the whole range less one decade, and spreads over one decade within the
    row.  (Elements drawn over the whole range within one row would put the smallest of 66 049
    terms — 1e-4 of the mean flux, times an end weight of 0.08 of the mean weight, over n — below
    the share 100 n 2^-52 of the row sum that the tests require of every term; two decades
    within the row still miss it by a third after the sweep has attenuated the short
    wavelengths.)  Every row then gets one spike of 1e4 times its mean, at j = 0, 63, 64, 255,
    256, n - 1 in turn (those that exist)."""
    up = 10 ** rng.uniform(8, 11, (nL, 1)) * 10 ** rng.uniform(0, 1, (nL, n_lam))
    down = 10 ** rng.uniform(6, 10, (nL, 1)) * 10 ** rng.uniform(0, 1, (nL, n_lam))
    at = sorted({j % n_lam for j in SPIKE_AT if j < n_lam})
    for k, a in enumerate((up, down)):
        for i in range(nL):
            j = at[(i + 3 * k) % len(at)]
            a[i, j] = 1e4 * a[i].mean()
    return up, down


def sum_case(n_lam, nL, S=2):
    """Inputs of the bolometric-sum cases: the grids, temperatures and separable tables of
    tests/test_gpu_parity.py test_ragged_shapes_sweeps_match_oracle with S species on shared
    nodes, and flux_rows.  The grid starts at 1 um, not 0.5: below it the thick cool layers of the
    four-layer case leave terms (Planck's tail) under the share the tests require of every term."""
    rng = np.random.default_rng(1000 * n_lam + nL)
    lam, _, _ = O.wavelength_grid(1.0, 10, n_lam)
    p = O.pressure_grid(nL, -6, np.log10(200))
    T = O.temperature_grid(p, 1700.0, 0.1, 0.1) * (1 + 0.03 * rng.standard_normal(nL))
    Tn = np.linspace(0.7 * T.min(), 1.3 * T.max(), 5)
    names = ["1H2-16O", "12C-16O", "Na"][:S]
    vals = {n: O.separable_table(10 ** rng.uniform(-3, 2, lam.size), (p / 1.0) ** 0.1,
                                 (Tn / 1000) ** 0.5) for n in names}
    up0, down0 = flux_rows(rng, nL, n_lam)
    return dict(lam=lam, p=p, T=T, Tn=Tn, vals=vals, up0=up0, down0=down0, F_toa=O.F_TOA(lam),
                g=G_J, m_bar=M_BAR)


FAMILIES = ("isothermal", "inverted", "superadiabatic", "mixed")
ALPHAS = (0.5, 1.0, 2.0)
GRAVITIES = (300.0, 2479.0, 1e4)
M_BARS = (float(O.M_BAR_DEFAULT), 2 * float(O.M_BAR_DEFAULT))


def family_case(family, nL=24, n_lam=1024):
    """Inputs of the dT cases (g, m_bar and alpha are the caller's).  Isothermal and inverted
    (T rising outward) profiles are radiative in every layer; T ~ p^0.4 is steeper than the
    adiabat (2/7) and convective in every layer but emit's top one, whose T_2 = T_1; the oracle's
    temperature_grid with 5 % noise has both.  The steep profile spans four decades of pressure
    (1e-3 to 10 bar, 4000 K to 100 K) and so does the noisy one (1e-6 to 1e-2 bar), the others
    the usual 1e-6 to 200 bar."""
    assert family in FAMILIES
    rng = np.random.default_rng(7 + FAMILIES.index(family))
    lam, _, _ = O.wavelength_grid(0.5, 10, n_lam)
    if family == "superadiabatic":
        p = O.pressure_grid(nL, -3, 1)
        T = 4000.0 * (p / p[0]) ** 0.4
    elif family == "mixed":
        # four decades in 23 steps: the noise between neighbours (7 % rms) passes the adiabat's
        # 11 % less the profile's own 4 % in about one layer of seven (this draw: four of the 24
        # layers, at both ends and in the middle, none within 10 % of the switch)
        p = O.pressure_grid(nL, -6, -2)
        noise = np.random.default_rng(8).standard_normal(nL)
        T = O.temperature_grid(p, 1800.0, 0.1, 0.1) * (1 + 0.05 * noise)
    else:
        p = O.pressure_grid(nL, -6, np.log10(200))
        if family == "isothermal":
            T = np.full(nL, 1500.0)
        else:
            T = np.geomspace(900.0, 2200.0, nL)
    Tn = np.linspace(0.7 * T.min(), 1.3 * T.max(), 7)
    vals = {n: O.separable_table(10 ** rng.uniform(-2, 2, lam.size), (p / 1.0) ** 0.1,
                                 (Tn / 1000) ** 0.5) for n in ("1H2-16O", "12C-16O")}
    up0 = 10 ** rng.uniform(8, 12, (nL, n_lam))
    down0 = 10 ** rng.uniform(6, 11, (nL, n_lam))
    return dict(lam=lam, p=p, T=T, Tn=Tn, vals=vals, up0=up0, down0=down0, F_toa=O.F_TOA(lam))


CONV_SETTINGS = ((0, -1.0), (1, -1.0), (2, -1.0), (5, -1.0), (10 ** 6, 3.0), (2, 3.0))
CONV_ALPHA = 1.0
CONV_STEPS = 40


def conv_case(kind, nL=20, n_lam=512):
    """Inputs of the convergence cases.  A layer's step is |dT| ~ 1e5 |x|^0.1 p / (dp sigma T^3)
    (delta_t_i's 1e5 / |x|^0.9 leaves the flux divergence x only its sign and a tenth power), so
    a layer walks to its equilibrium at a nearly fixed pace and then steps across it and back:
    the temperatures oscillate where the start lies within 40 steps of equilibrium, whatever
    the mixing length (these layers are radiative, so ``alpha`` — 1 here — does not enter).
    "flips": isothermal 1400 K on 1e-3..0.1 bar, 25 K steps around an equilibrium near 1100 K:
    every layer has flipped once after 12 iterations and six times after 18, and |dT| never
    falls under 3 K.  "dT": the star 128 times brighter, 2700 K (the bottom layer, the only one
    that cools, 3300 K): the layers heat monotonically, their steps shrink with T^-3 from 3.1 K,
    and the last falls under 3 K at the seventh iteration; no layer but the end ones flips."""
    assert kind in ("flips", "dT")
    rng = np.random.default_rng(31)
    lam, _, _ = O.wavelength_grid(0.5, 10, n_lam)
    p = O.pressure_grid(nL, -3, -1)
    if kind == "flips":
        T0, scale = np.full(nL, 1400.0), 1.0
    else:
        T0, scale = np.full(nL, 2700.0), 128.0
        T0[0] = 3300.0
    Tn = np.linspace(0.3 * T0.min(), 2.5 * T0.max(), 9)
    vals = {n: O.separable_table(10 ** rng.uniform(-3, 1, lam.size), (p / 1.0) ** 0.1,
                                 (Tn / 1000.0) ** 0.5) for n in ("1H2-16O", "12C-16O")}
    return dict(lam=lam, p=p, T=T0, Tn=Tn, vals=vals, F_toa=scale * O.F_TOA(lam))


def oracle_run(case, n_zero_crossings, convergence_dT):
    """(temp_hist, n_iter) of the oracle's emission_spectrum on a conv_case."""
    o = O.emission_spectrum(oracle_tables(case), case["T"], case["p"], case["lam"],
                            case["F_toa"], G_J, M_BAR, CONV_ALPHA, n_timesteps=CONV_STEPS,
                            n_zero_crossings=n_zero_crossings, convergence_dT=convergence_dT)
    return o[2], o[6]


def oracle_tables(case):
    return {n: O.Table(v, case["p"], case["Tn"]) for n, v in case["vals"].items()}


def oracle_sweep(case, direction, g, m_bar, alpha):
    """One oracle sweep from the case's state -> dict(up, down: the new flux arrays, dT, bol
    [n_layers][4]: the oracle's own trapezoid sums, rows {layer: the four rows handed to the
    sums}), captured through the bol_fn hook."""
    fn = O.emit if direction == "emit" else O.absorb
    lam_cm = case["lam"] * 1e-4
    steps = []          # (rows, sums) in the order the sweep visits its layers

    def bol_fn(*rows):
        rows = tuple(np.array(r, dtype=float) for r in rows)      # (copies: absorb rewrites F_up)
        sums = tuple(O.trapz(r, lam_cm) for r in rows)
        steps.append((rows, sums))
        return sums

    up, down, _, _, dT = fn(oracle_tables(case), case["T"], case["p"], case["lam"], case["F_toa"],
                            g, m_bar, alpha, case["up0"].copy(), case["down0"].copy(),
                            bol_fn=bol_fn)
    nL = len(case["p"])
    layers = list(range(1, nL)) if direction == "emit" else list(range(nL - 2, -1, -1))
    assert len(steps) == len(layers)
    bol, cap = np.zeros((nL, 4)), {}
    for i, (rows, sums) in zip(layers, steps):
        cap[i] = rows
        bol[i] = sums
    return dict(up=up, down=down, dT=dT, bol=bol, rows=cap)
