"""Plain restatement of the Doppler cross-correlation (include/frei_hip.h, frei_ccf_apply):
Python loops written from the definition alone, every sum by math.fsum (the correctly rounded
sum of the rounded terms).  Also the plan of frei_amd.crosscorr.CrossCorrelator, the statistics of
CrossCorrelation and the K_p-V_sys map as explicit loops.  Nothing here imports frei_amd."""
import math

import numpy as np

C_KMS = 299792.458


def plan(lam, wl_data, velocities):
    """(idx [n_vel][n_pix], frac [n_vel][n_pix], n_clamped [n_vel]): s = wl / (1 + v / c)
    clamped to the axis, idx the largest index with lam[idx] <= s limited to n_lam - 2,
    frac = (s - lam[idx]) / (lam[idx + 1] - lam[idx])."""
    n = len(lam)
    idx = np.empty((len(velocities), len(wl_data)), dtype=np.int32)
    frac = np.empty((len(velocities), len(wl_data)))
    n_clamped = np.zeros(len(velocities), dtype=int)
    for v in range(len(velocities)):
        d_v = 1.0 / (1.0 + float(velocities[v]) / C_KMS)
        for p in range(len(wl_data)):
            s = float(wl_data[p]) * d_v
            if s < lam[0] or s > lam[n - 1]:
                n_clamped[v] += 1
                s = float(lam[0]) if s < lam[0] else float(lam[n - 1])
            lo, hi = 0, n - 1          # lam[lo] <= s holds (s >= lam[0]); bisect upwards
            while lo < hi:
                mid = (lo + hi + 1) // 2
                if lam[mid] <= s:
                    lo = mid
                else:
                    hi = mid - 1
            j = min(lo, n - 2)
            idx[v][p] = j
            frac[v][p] = (s - float(lam[j])) / (float(lam[j + 1]) - float(lam[j]))
    return idx, frac, n_clamped


def template(x, den=None, select=None, scale=None, offset=None):
    """y[n_atm][n_lam] = scale_m (x[m] / den[select_m]) - offset_m; an absent operand drops
    its operation."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    den = None if den is None else np.atleast_2d(np.asarray(den, dtype=float))
    y = np.empty(x.shape)
    for m in range(x.shape[0]):
        sel = 0 if select is None else int(select[m])
        for j in range(x.shape[1]):
            v = float(x[m][j])
            if den is not None:
                v = v / float(den[sel][j])
            if scale is not None:
                v = float(scale[m]) * v
            if offset is not None:
                v = v - float(offset[m])
            y[m][j] = v
    return y


def _fsum(terms):
    """math.fsum; NaN where a term is NaN or inf (fsum refuses inf - inf)."""
    if any(math.isnan(t) or math.isinf(t) for t in terms):
        return float("nan")
    return math.fsum(terms)


def sums(y, idx, frac, a, w):
    """(S_fg [n_atm][n_exp][n_vel], S_g [n_atm][n_vel], S_gg [n_atm][n_vel]) of the definition
    for templates y[n_atm][n_lam]."""
    y = np.atleast_2d(np.asarray(y, dtype=float))
    a = np.atleast_2d(np.asarray(a, dtype=float))
    n_atm, (n_vel, n_pix), n_exp = y.shape[0], idx.shape, a.shape[0]
    sfg = np.empty((n_atm, n_exp, n_vel))
    sg, sgg = np.empty((n_atm, n_vel)), np.empty((n_atm, n_vel))
    al = [[float(a[e][p]) for p in range(n_pix)] for e in range(n_exp)]
    wl = [float(w[p]) for p in range(n_pix)]
    for m in range(n_atm):
        ym = [float(v) for v in y[m]]
        for v in range(n_vel):
            g = []
            for p in range(n_pix):
                j, t = int(idx[v][p]), float(frac[v][p])
                d = ym[j + 1] - ym[j]
                td = t * d
                g.append(ym[j] + td)
            for e in range(n_exp):
                sfg[m][e][v] = _fsum([al[e][p] * g[p] for p in range(n_pix)])
            sg[m][v] = _fsum([wl[p] * g[p] for p in range(n_pix)])
            sgg[m][v] = _fsum([(wl[p] * g[p]) * g[p] for p in range(n_pix)])
    return sfg, sg, sgg


def bounds(y, idx, a, w):
    """The bounds on |S - S_ref|, shaped like the sums: (n_pix + 32) 2^-53 sum_p |c_p| (|y_j| +
    |y_{j+1}|) with c_p = a[e][p] (S_fg), w[p] (S_g) and w[p] (|y_j| + |y_{j+1}|) (S_gg).
    (|g| <= |y_j| + |y_{j+1}| for t in [0, 1]; each side sums n_pix terms of that size within
    (n_pix - 1) 2^-53 of their absolute sum, g and the products round a few times more, and the
    device's y may differ from the restatement's by a few roundings: 32 covers them.)"""
    y = np.atleast_2d(np.asarray(y, dtype=float))
    a = np.atleast_2d(np.asarray(a, dtype=float))
    n_pix = idx.shape[1]
    eps = (n_pix + 32) * 2.0 ** -53
    mag = np.abs(y)[:, idx] + np.abs(y)[:, idx + 1]          # [n_atm][n_vel][n_pix]
    b_fg = eps * np.einsum("ep,mvp->mev", np.abs(a), mag)
    b_g = eps * np.einsum("p,mvp->mv", np.abs(np.asarray(w, dtype=float)), mag)
    b_gg = eps * np.einsum("p,mvp->mv", np.abs(np.asarray(w, dtype=float)), mag * mag)
    return b_fg, b_g, b_gg


def host_sums(flux, w):
    """(W, S_wf [n_exp], S_wff [n_exp]) with a = w flux."""
    flux = np.atleast_2d(np.asarray(flux, dtype=float))
    W = math.fsum(float(v) for v in w)
    S_wf = [math.fsum(float(w[p]) * float(f[p]) for p in range(len(w))) for f in flux]
    S_wff = [math.fsum((float(w[p]) * float(f[p])) * float(f[p]) for p in range(len(w)))
             for f in flux]
    return W, np.array(S_wf), np.array(S_wff)


def ccf(sfg, sg, sgg, W, S_wf, S_wff):
    """C_fg / sqrt(V_f V_g), [n_atm][n_exp][n_vel]."""
    out = np.empty(np.shape(sfg))
    for m in range(out.shape[0]):
        for e in range(out.shape[1]):
            V_f = S_wff[e] - S_wf[e] * S_wf[e] / W
            for v in range(out.shape[2]):
                gbar = sg[m][v] / W
                C_fg = sfg[m][e][v] - gbar * S_wf[e]
                V_g = sgg[m][v] - sg[m][v] * gbar
                out[m][e][v] = C_fg / math.sqrt(V_f * V_g)
    return out


def loglike(sfg, sg, sgg, W, S_wf, S_wff, n_pix):
    """-(n_pix / 2) log((V_f - 2 C_fg + V_g) / W), [n_atm][n_exp][n_vel]."""
    out = np.empty(np.shape(sfg))
    for m in range(out.shape[0]):
        for e in range(out.shape[1]):
            V_f = S_wff[e] - S_wf[e] * S_wf[e] / W
            for v in range(out.shape[2]):
                gbar = sg[m][v] / W
                C_fg = sfg[m][e][v] - gbar * S_wf[e]
                V_g = sgg[m][v] - sg[m][v] * gbar
                out[m][e][v] = -(n_pix / 2.0) * math.log((V_f - 2.0 * C_fg + V_g) / W)
    return out


def _interp(x, xp, fp):
    """np.interp for one x on ascending xp: the end values beyond the ends."""
    n = len(xp)
    if x <= xp[0]:
        return float(fp[0])
    if x >= xp[n - 1]:
        return float(fp[n - 1])
    j = 0
    for k in range(n - 1):
        if xp[k] <= x:
            j = k
    slope = (float(fp[j + 1]) - float(fp[j])) / (float(xp[j + 1]) - float(xp[j]))
    return slope * (x - float(xp[j])) + float(fp[j])


def kp_vsys_map(values, velocities, phases, Kp, Vsys, v_obs):
    """[n_atm][n_Kp][n_Vsys]: the sum over exposures of values[m][e] interpolated at
    Vsys + Kp sin(2 pi phase_e) + v_obs_e."""
    values = np.asarray(values, dtype=float)
    out = np.zeros((values.shape[0], len(Kp), len(Vsys)))
    for m in range(values.shape[0]):
        for k in range(len(Kp)):
            for s in range(len(Vsys)):
                tot = 0.0
                for e in range(len(phases)):
                    v = Vsys[s] + Kp[k] * math.sin(2.0 * math.pi * phases[e]) + v_obs[e]
                    tot += _interp(v, velocities, values[m][e])
                out[m][k][s] = tot
    return out
