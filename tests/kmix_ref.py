"""NumPy restatement of K19 (include/frei_hip.h: frei_klib_mix), in the header's operation order:
random overlap of k-tables with resort-and-rebin.  The integer parts (fixed-point weights, pair
weights, prefix sums, overlaps) are Python ints, so they are exact by construction; the float
parts are float64 in the header's order.  Also the two-species line-forest case the physics is
held to (tests/test_kmix_host.py through the oracle alone, tests/test_gpu_kmix.py on the device).
"""
import math

import numpy as np

from tests import kdist_ref as R


def fixed_weights(w):
    """W_q = llrint(w_q 2^30) as Python ints (round half to even, as llrint in the default
    rounding mode)."""
    return [int(np.rint(float(x) * 2.0 ** 30)) for x in np.asarray(w, dtype=np.float64)]


def intervals(W):
    """E_q = Wt sum_{q' < q} W_q', q = 0 .. n_g, in units of Wt^2."""
    Wt, acc, E = sum(W), 0, []
    for q in range(len(W) + 1):
        E.append(Wt * acc)
        if q < len(W):
            acc += W[q]
    return E


def order(v):
    """The pairs' indices ordered by (v, e): -0 as +0, NaN last, ties to the smaller e."""
    return sorted(range(len(v)), key=lambda e: (math.isnan(v[e]), 0.0 if math.isnan(v[e])
                                                else v[e] + 0.0, e))


def fold(a, b, W):
    """One species folded in: a'[n_g] from a[n_g], b[n_g] (float64) and the weights W (ints).
    Also returns what the tests look at: v[n_g^2], the order, u[n_g^2] (ints) and, per q, the
    list of (e, overlap) it summed."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n_g = len(W)
    Wt, E = sum(W), intervals(W)
    with np.errstate(all="ignore"):
        v = (a[:, None] + b[None, :]).ravel()
        lnv = np.log(v)
    u = [W[e // n_g] * W[e % n_g] for e in range(n_g * n_g)]
    perm = order([float(x) for x in v])
    acc = [np.float64(0.0)] * n_g
    parts = [[] for _ in range(n_g)]
    C, q = 0, 0
    with np.errstate(all="ignore"):
        for e in perm:
            lo, hi = C, C + u[e]
            while E[q + 1] <= lo:           # the first interval the pair overlaps
                q += 1
            k = q
            while k < n_g and E[k] < hi:
                ov = min(hi, E[k + 1]) - max(lo, E[k])
                acc[k] = acc[k] + np.float64(float(ov)) * lnv[e]
                parts[k].append((e, ov))
                k += 1
            C = hi
        out = np.array([np.exp(acc[k] / np.float64(float(W[k] * Wt))) for k in range(n_g)])
    assert C == Wt * Wt
    return out, dict(v=v, order=perm, u=u, parts=parts, lnv=lnv)


def ln_max(v):
    """max |ln v| over the finite, positive v (0 when there is none)."""
    v = np.asarray(v, dtype=np.float64)
    ok = np.isfinite(v) & (v > 0)
    return float(np.max(np.abs(np.log(v[ok])))) if ok.any() else 0.0


def step_bound(n_g, lnmax):
    """The rounding of one fold: (n_g^2 + 4) 2^-52 max(1, max |ln v|)."""
    return (n_g * n_g + 4) * 2.0 ** -52 * max(1.0, lnmax)


def kmix_ref(K, x, w):
    """-> (out[n_p][n_T][n_bins][n_g], lnmax[n_p][n_T][n_bins]) of the tables K[n_src][n_p][n_T]
    [n_bins][n_g] at the composition x[n_src][n_p][n_T] (the C layout); lnmax is the largest
    |ln v| any fold of the item met."""
    K = np.asarray(K, dtype=np.float64)
    x = np.broadcast_to(np.asarray(x, dtype=np.float64), K.shape[:3])
    W = fixed_weights(w)
    n_src, n_p, n_T, n_bins, n_g = K.shape
    out = np.empty(K.shape[1:])
    lnmax = np.zeros(K.shape[1:4])
    with np.errstate(all="ignore"):
        for kp in range(n_p):
            for kt in range(n_T):
                for b in range(n_bins):
                    a = x[0, kp, kt] * K[0, kp, kt, b]
                    for s in range(1, n_src):
                        a, st = fold(a, x[s, kp, kt] * K[s, kp, kt, b], W)
                        lnmax[kp, kt, b] = max(lnmax[kp, kt, b], ln_max(st["v"]))
                    out[kp, kt, b] = a
    return out, lnmax


# ----------------------------------------------------------------- the two-species forest case
def second_forest(case, seed=12):
    """A second species beside kdist_ref.forest_case(): an independent seeded forest of 90 lines
    on the same axis and nodes (float32 [n_T][n_p][n_hi])."""
    rng = np.random.default_rng(seed)
    wl, p, T_nodes = case["wl"], case["p"], case["T_nodes"]
    c = rng.uniform(2.5, 3.0, 90)
    S = rng.lognormal(0.5, 2.0, 90)
    E = rng.uniform(0.0, 4000.0, 90)
    g0 = 2e-4 * rng.uniform(0.5, 1.5, 90)
    x = np.empty((T_nodes.size, p.size, wl.size), dtype=np.float32)
    for a, Tn in enumerate(T_nodes):
        s = S * np.exp(-1.4388 * E * (1.0 / Tn - 1.0 / 1200.0))
        for b, pn in enumerate(p):
            w = g0 * pn * (1200.0 / Tn) ** 0.5 + 3e-5 * (Tn / 1200.0) ** 0.5
            prof = s[:, None] * w[:, None] / np.pi / ((wl[None, :] - c[:, None]) ** 2 +
                                                      w[:, None] ** 2)
            x[a, b] = (1e-4 + 1e-3 * prof.sum(axis=0)).astype(np.float32)
    x.setflags(write=False)
    return x


FOREST_MIX = (0.6, 0.4)     # the two species' mass mixing ratios, the same at every node


def forest_pair():
    """kdist_ref.forest_case() with the second species: ``xsec2`` and the true mixture
    ``xsec`` = K18's premix of the two at FOREST_MIX (what the native-axis run uses); the
    first species alone is ``xsec1``."""
    case = dict(R.forest_case())
    case["xsec1"] = case["xsec"]
    case["xsec2"] = second_forest(case)
    case["xsec"] = R.mix_ref([case["xsec1"], case["xsec2"]],
                             np.array(FOREST_MIX)[:, None, None])
    case["xsec"].setflags(write=False)
    return case


def species_tables(case, g):
    """The two species' k-tables [2][n_p][n_T][n_bins][n_g] on the case's own nodes."""
    return np.stack([R.kdist_ref(case[k], case["T_nodes"], case["p"], case["wl"],
                                 case["wl_bins"], g, case["T_nodes"], case["p"])[0]
                     for k in ("xsec1", "xsec2")])
