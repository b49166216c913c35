"""Plain NumPy restatement of the transmission-spectrum definition (the header comment of
frei_transit in include/frei_hip.h), written from the definition alone: explicit loops over
the tangent level i and the shell j in the stated order, vectorised over wavelength only.  The
checker of tests/test_gpu_transit.py; it imports nothing of the package under test.

Notation: nL = n_layers; levels 1 .. nL with radii r_1 < ... < r_nL (``radii[k]`` = r_{k+1});
shell l (1 <= l <= nL - 1) lies between levels l and l + 1 and has the vertical optical depth
``dtaus[l]``; row 0 of ``dtaus`` is never read."""
import numpy as np

K_B = 1.380649e-16   # erg K^-1 (CODATA 2018)


def radii(T, p_bar, g, m_bar, R_p, P_ref=None):
    """r_1 .. r_nL: r_1 = R_p - z_ref, r_{l+1} = r_l + dz_l with dz_l = k_B T_l / (m_bar g)
    ln(p_l / p_{l+1}), p_nL = p_{nL-1} p_{nL-2} / p_{nL-3}; z_ref = 0 or the height of P_ref
    above level 1."""
    T, p = np.asarray(T, dtype=float), np.asarray(p_bar, dtype=float)
    nL = p.size
    pl = {l: p[l] for l in range(1, nL)}
    pl[nL] = p[nL - 1] * p[nL - 2] / p[nL - 3]
    dz = {l: K_B * T[l] / (m_bar * g) * np.log(pl[l] / pl[l + 1]) for l in range(1, nL)}
    z_ref = 0.0
    if P_ref is not None:
        if not (pl[nL] <= P_ref <= pl[1]):
            raise ValueError("P_ref outside the levels")
        z = 0.0
        for l in range(1, nL):
            if pl[l + 1] <= P_ref:
                z_ref = z + dz[l] * np.log(pl[l] / P_ref) / np.log(pl[l] / pl[l + 1])
                break
            z = z + dz[l]
    r = [R_p - z_ref]
    for l in range(1, nL):
        r.append(r[-1] + dz[l])
    return np.array(r)


def chord_weights(r):
    """G[i][j] for 1 <= i <= j <= nL - 1 (dict keyed by (i, j)); ``r[k - 1]`` = r_k."""
    nL = len(r)
    R = {k: float(r[k - 1]) for k in range(1, nL + 1)}

    def s(i, k):
        return np.sqrt((R[k] - R[i]) * (R[k] + R[i]))
    return {(i, j): 2.0 * (R[j + 1] + R[j]) / (s(i, j + 1) + s(i, j))
            for i in range(1, nL) for j in range(i, nL)}


def transit(dtaus, r, R_star):
    """(depth[n_lam], tau_slant[nL - 1][n_lam]) of one atmosphere; tau_slant row k is tangent
    level k + 1."""
    dtaus = np.asarray(dtaus, dtype=float)
    nL, n = dtaus.shape
    assert len(r) == nL
    G = chord_weights(r)
    tau = {}
    for i in range(1, nL):
        t = G[(i, i)] * dtaus[i]
        for j in range(i + 1, nL):
            t = t + G[(i, j)] * dtaus[j]
        tau[i] = t
    f = {i: -np.expm1(-tau[i]) for i in range(1, nL)}
    f[nL] = np.zeros(n)
    R = {k: float(r[k - 1]) for k in range(1, nL + 1)}
    A = np.full(n, R[1] * R[1])
    for i in range(1, nL):
        A = A + (f[i] * R[i] + f[i + 1] * R[i + 1]) * (R[i + 1] - R[i])
    depth = A / (R_star * R_star)
    return depth, np.array([tau[i] for i in range(1, nL)])
