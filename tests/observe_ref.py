"""Plain restatement of the synthetic-observation definition (include/frei_hip.h,
frei_obs_apply): Python and NumPy loops written from the definition alone, summed in ascending t
and ascending k.  Also the three weight constructions of frei_amd.observe.Instrument as explicit
loops over the axis.  Nothing here imports frei_amd."""
import math

import numpy as np


def trapz_weights(lam):
    """np.trapz's weight of every point: half the distance to each neighbour."""
    n = len(lam)
    w = [0.0] * n
    for j in range(n - 1):
        d = lam[j + 1] - lam[j]
        w[j] += d / 2
        w[j + 1] += d / 2
    return w


def apply(first, count, weights, x, num=None, den=None, select=None, scale=None):
    """obs[n_atm][K] of the definition."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    n_atm, K = x.shape[0], len(first)
    num = None if num is None else np.atleast_2d(num)
    den = None if den is None else np.atleast_2d(den)
    obs = np.empty((n_atm, K))
    off = 0
    for k in range(K):
        f, c = int(first[k]), int(count[k])
        for m in range(n_atm):
            sel = 0 if select is None else int(select[m])
            N = D = 0.0
            for t in range(c):
                w = float(weights[off + t])
                term = w * float(x[m][f + t])
                if num is not None:
                    term = term * float(num[sel][f + t])
                N = N + term
                D = D + (w * float(den[sel][f + t]) if den is not None else w)
            v = N / D if not (math.isnan(N) or math.isnan(D)) else float("nan")
            obs[m][k] = (1.0 if scale is None else float(scale[m])) * v
        off += c
    return obs


def chi2(obs, data, sigma):
    """chi2[n_atm]; a channel of infinite sigma contributes exactly 0."""
    obs = np.atleast_2d(obs)
    out = np.empty(obs.shape[0])
    for m in range(obs.shape[0]):
        s = 0.0
        for k in range(obs.shape[1]):
            if math.isinf(sigma[k]):
                continue
            r = (float(obs[m][k]) - float(data[k])) / float(sigma[k])
            s = s + r * r
        out[m] = s
    return out


def chi2_bound(obs_ref, data, sigma, rtol):
    """The bound on |chi2 - chi2_ref| when every obs lies within rtol (relative) of obs_ref:
    sum_k (2 |r_k| e_k + e_k^2) + (K + 4) 2^-52 chi2_ref, e_k = rtol |obs_ref| / sigma_k."""
    obs_ref = np.atleast_2d(obs_ref)
    K = obs_ref.shape[1]
    ref = chi2(obs_ref, data, sigma)
    out = np.empty(obs_ref.shape[0])
    for m in range(obs_ref.shape[0]):
        b = 0.0
        for k in range(K):
            if math.isinf(sigma[k]):
                continue
            e = rtol * abs(float(obs_ref[m][k])) / float(sigma[k])
            r = (float(obs_ref[m][k]) - float(data[k])) / float(sigma[k])
            b += 2 * abs(r) * e + e * e
        out[m] = b + (K + 4) * 2.0 ** -52 * ref[m]
    return out


def rtol_for(c_max):
    """(4 c_max + 20) 2^-53: device and restatement each within (c + 4) 2^-53 of the exact sum
    of non-negative terms, the ratio and the scale two more roundings each side."""
    return (4 * c_max + 20) * 2.0 ** -53


# ---------------------------------------------------------------- weight constructions
def _pack(chans):
    first = [a for a, _ in chans]
    count = [len(w) for _, w in chans]
    weights = [v for _, w in chans for v in w]
    return first, count, weights


def top_hat(lam, lo, hi):
    """w = tw_j for lo_k <= lam_j <= hi_k.  ValueError naming an empty channel."""
    tw = trapz_weights(lam)
    chans = []
    for k in range(len(lo)):
        idx = [j for j in range(len(lam)) if lo[k] <= lam[j] <= hi[k]]
        if not idx:
            raise ValueError(f"channel {k} is empty")
        chans.append((idx[0], [tw[j] for j in idx]))
    return _pack(chans)


def from_throughput(lam, curves):
    """w = tw_j * interp(lam_j, wl, T, left=0, right=0); support from the first to the last
    non-zero weight."""
    tw = trapz_weights(lam)
    chans = []
    for k, (wl, T) in enumerate(curves):
        w = [tw[j] * float(np.interp(lam[j], wl, T, left=0, right=0)) for j in range(len(lam))]
        nz = [j for j in range(len(lam)) if w[j] != 0.0]
        if not nz:
            raise ValueError(f"channel {k} is empty")
        chans.append((nz[0], w[nz[0]:nz[-1] + 1]))
    return _pack(chans)


def gaussian(lam, centres, fwhm=None, resolving_power=None, n_sigma=4.0):
    """s_k = fwhm_k / (2 sqrt(2 ln 2)), fwhm_k = c_k / R; w = tw_j exp(-((lam_j - c_k) / s_k)^2
    / 2) for |lam_j - c_k| <= n_sigma s_k."""
    tw = trapz_weights(lam)
    chans = []
    for k, c in enumerate(centres):
        fw = c / resolving_power if fwhm is None else (fwhm[k] if np.ndim(fwhm) else fwhm)
        s = fw / (2.0 * math.sqrt(2.0 * math.log(2.0)))
        idx = [j for j in range(len(lam)) if abs(lam[j] - c) <= n_sigma * s]
        if not idx:
            raise ValueError(f"channel {k} is empty")
        w = []
        for j in idx:
            z = (lam[j] - c) / s
            w.append(tw[j] * math.exp(-0.5 * (z * z)))
        chans.append((idx[0], w))
    return _pack(chans)
