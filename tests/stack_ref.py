"""Plain restatement of the orbital stack (include/frei_hip.h, frei_stack_apply): Python loops and
``math`` written from the definition alone — the statistic of the cross-correlation sums and the
stack over the exposures, every operation in the header's order — and a bounded high-precision
form of the statistic (mpmath at 60 digits with a first-order running bound of the rounding
error of its double evaluation, the machinery of tests/updateref.py unchanged).

Operation bounds: 0.5 ulp for + - * / and sqrt, 2 ulp for log (updateref's defaults).  The
kernel uses the compiler's correctly rounded fp64 division and square root, not ``fm::div`` or
``fm::sqrt`` of frei_math.h, so no 1-ulp allowance is needed.  Nothing here imports frei_amd.
"""
import math

import numpy as np

from tests.updateref import _V, _add, _at_60_digits, _div, _log, _mul, _sqrt, _sub

CCF, LOGLIKE = 1, 2
EPS = 2.0 ** -53


# ------------------------------------------------------------------ statistic
def statistic(which, sfg, sg, sgg, W, S_wf, S_wff, n_eff):
    """values[n_atm][n_exp][n_vel] of statistic ``which`` (CCF or LOGLIKE) in doubles, by the
    header's operations in the header's order."""
    sfg = np.asarray(sfg, dtype=float)
    out = np.empty(sfg.shape)
    W, half = float(W), -(float(n_eff) / 2.0)
    for m in range(sfg.shape[0]):
        for e in range(sfg.shape[1]):
            swf, swff = float(S_wf[e]), float(S_wff[e])
            sq = swf * swf
            V_f = swff - sq / W
            for v in range(sfg.shape[2]):
                g = float(sg[m][v])
                gbar = g / W
                gs = gbar * swf
                C_fg = float(sfg[m][e][v]) - gs
                gg = g * gbar
                V_g = float(sgg[m][v]) - gg
                if which == CCF:
                    p = V_f * V_g
                    out[m][e][v] = C_fg / math.sqrt(p)
                else:
                    c2 = 2.0 * C_fg
                    d = V_f - c2
                    q = (d + V_g) / W
                    out[m][e][v] = half * math.log(q)
    return out


@_at_60_digits
def statistic_ref(which, sfg, sg, sgg, W, S_wf, S_wff, n_eff):
    """(value, bound), each [n_atm][n_exp][n_vel]: the statistic in mpmath at 60 digits from the
    doubles given, rounded to double, and the first-order bound of the rounding error of its
    evaluation in doubles in the header's order (cancellation in C_fg, V_g, V_f and the log's
    argument enters through the propagation)."""
    sfg = np.asarray(sfg, dtype=float)
    val, bnd = np.empty(sfg.shape), np.empty(sfg.shape)
    half = -(float(n_eff) / 2.0)                      # exact
    for m in range(sfg.shape[0]):
        for e in range(sfg.shape[1]):
            swf, swff = float(S_wf[e]), float(S_wff[e])
            V_f = _sub(swff, _div(_mul(swf, swf), float(W)))
            for v in range(sfg.shape[2]):
                g = float(sg[m][v])
                gbar = _div(g, float(W))
                C_fg = _sub(float(sfg[m][e][v]), _mul(gbar, swf))
                V_g = _sub(float(sgg[m][v]), _mul(g, gbar))
                if which == CCF:
                    r = _div(C_fg, _sqrt(_mul(V_f, V_g)))
                else:
                    r = _mul(half, _log(_div(_add(_sub(V_f, _mul(2.0, C_fg)), V_g), float(W))))
                val[m][e][v], bnd[m][e][v] = float(r.v), float(r.e)
    return val, bnd


# ------------------------------------------------------------------ stack
def brackets(vel, dv, v_obs, vsys):
    """(j [n_kp][n_exp][n_vsys] int, t [n_kp][n_exp][n_vsys], outside [n_kp][n_exp][n_vsys]
    bool): u = (vsys[s] + dv[k][e]) + v_obs[e] clamped to the grid, j the largest index with
    vel[j] <= u limited to n_vel - 2 (the device's bisection), t = (u - vel[j]) / (vel[j+1] -
    vel[j]); ``outside`` where u was clamped."""
    n = len(vel)
    vl = [float(x) for x in vel]
    K, E, S = len(dv), len(v_obs), len(vsys)
    j = np.empty((K, E, S), dtype=int)
    t = np.empty((K, E, S))
    outside = np.zeros((K, E, S), dtype=bool)
    for k in range(K):
        for e in range(E):
            for s in range(S):
                u = (float(vsys[s]) + float(dv[k][e])) + float(v_obs[e])
                if u < vl[0] or u > vl[n - 1]:
                    outside[k][e][s] = True
                    u = vl[0] if u < vl[0] else vl[n - 1]
                lo, hi = 0, n - 2
                while lo < hi:
                    mid = (lo + hi + 1) >> 1
                    if vl[mid] <= u:
                        lo = mid
                    else:
                        hi = mid - 1
                j[k][e][s] = lo
                t[k][e][s] = (u - vl[lo]) / (vl[lo + 1] - vl[lo])
    return j, t, outside


def stack(values, j, t):
    """map[n_atm][n_kp][n_vsys] of values[n_atm][n_exp][n_vel] on the brackets (j, t): val =
    f[j] + t * (f[j+1] - f[j]), summed over the exposures in ascending order by plain
    additions from 0."""
    values = np.asarray(values, dtype=float)
    K, E, S = j.shape
    out = np.empty((values.shape[0], K, S))
    for m in range(values.shape[0]):
        f = [[float(x) for x in row] for row in values[m]]
        for k in range(K):
            for s in range(S):
                acc = 0.0
                for e in range(E):
                    i = int(j[k][e][s])
                    d = f[e][i + 1] - f[e][i]
                    td = float(t[k][e][s]) * d
                    val = f[e][i] + td
                    acc = acc + val
                out[m][k][s] = acc
    return out


def magnitude(a, j):
    """sum_e (|a[m][e][j]| + |a[m][e][j+1]|) -> [n_atm][n_kp][n_vsys], for a[n_atm][n_exp][n_vel]
    (the values, or a bound on them) on the brackets j[n_kp][n_exp][n_vsys]."""
    a = np.abs(np.asarray(a, dtype=float))
    E = j.shape[1]
    out = np.zeros((a.shape[0], j.shape[0], j.shape[2]))
    for e in range(E):
        out += a[:, e, :][:, j[:, e, :]] + a[:, e, :][:, j[:, e, :] + 1]
    return out


def stack_bound(values, j):
    """The bound on |map - map_ref| for the same values: u and j are identical in exact
    arithmetic and the sums run in the same order, so only t's division and the knock-on
    roundings can differ: (n_exp + 4) 2^-53 sum_e (|f_j| + |f_{j+1}|)."""
    return (j.shape[1] + 4) * EPS * magnitude(values, j)


def stacked_statistic_bound(value_ref, value_bound, j):
    """The bound on |map - stack(value_ref)| when the stacked values are within ``value_bound``
    of ``value_ref``: the stack's own bound on the reference values plus what an error of that
    size in f_j and f_{j+1} moves a linear interpolation by at most (t in [0, 1]: no more than
    the two errors together), summed over the exposures."""
    return stack_bound(value_ref, j) + magnitude(value_bound, j)
