"""Writes tests/golden/voigt_case.npz: the exact cross-section of one line (K17,
frei_xsec_create_lines in include/frei_hip.h) for tests/test_lines_host.py and
tests/test_gpu_lines.py.  Needs mpmath (50 digits); run from the repository root:

    python tests/golden/make_voigt_goldens.py

One line at 2000 cm^-1, two T nodes, eight p nodes and an axis of ~1600 points whose distances
from the line run from 0 over 1e-6 cm^-1 to beyond the cutoff on both sides, with extra points
at x = 8 (1 +- 1e-3) (the |z| = 8 branch boundary at small y) and a hair inside and outside the
cutoff.  The (x, y) the definition forms cover x from 0 to > 1e4 and y from 1.4e-8 to 9.9e3, with
p nodes on both sides of y = 1e-3.

Stored: the inputs; ``x`` [n_T][n_hi] and ``y`` [n_T][n_p], the fp64 (x, y) the definition's
operations form; ``K`` [n_T][n_p][n_hi], Re w(x + iy) exact at those fp64 (x, y); ``inside``
[n_hi], the definition's fp64 cutoff comparison; ``values`` [n_T][n_p][n_hi], the definition
evaluated exactly (50 digits) from the fp64 inputs and the fp64 nu_i = 1e4 / wl_hi[i], rounded to
fp64 (0 outside the cutoff).  Every nonzero value is a normal float32.
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from frei_amd.constants import AMU, C, H, K_B  # noqa: E402
from tests import lines_ref  # noqa: E402

mp.mp.dps = 50


def faddeeva_re(x, y):
    """Re w(x + iy) to ~45 digits: exp(-z^2) erfc(-iz), or the asymptotic series
    w = (i / (z sqrt(pi))) sum_k (2k - 1)!! / (2 z^2)^k for |z| > 50 (its terms fall below 1e-60
    long before they start to grow at k ~ |z|^2)."""
    z = mp.mpc(x, y)
    if abs(z) <= 50:
        return (mp.exp(-z * z) * mp.erfc(-1j * z)).real
    s, term, k = mp.mpc(1), mp.mpc(1), 0
    while abs(term) > mp.mpf(10) ** -60:
        k += 1
        term = term * (2 * k - 1) / (2 * z * z)
        s += term
    return (1j / (z * mp.sqrt(mp.pi)) * s).real


def main():
    nu0, S_ref, E_low, gamma_ref, n_exp = 2000.0, 1e-19, 350.0, 0.07, 0.7
    mass_amu, T_ref, cutoff = 28.0, 296.0, 40.0
    T_nodes = np.array([300.0, 1500.0])
    q_ratio = np.array([0.98, 0.11])
    p_nodes = np.array([4e-9, 1e-6, 3e-5, 5e-5, 1e-2, 1.0, 50.0, 400.0])

    _, ia, _ = lines_ref.line_parameters([nu0], [S_ref], [E_low], [gamma_ref], [n_exp], mass_amu,
                                         T_ref, q_ratio, T_nodes)
    alpha = 1.0 / ia[:, 0]
    d = np.concatenate([
        np.exp(np.linspace(np.log(1e-6), np.log(45.0), 780)),
        8.0 * alpha * (1 - 1e-3), 8.0 * alpha * (1 + 1e-3),
        cutoff * (1 + np.array([-1e-3, -1e-9, 0.0, 1e-9, 1e-3]))])
    target = np.unique(np.concatenate([nu0 - d, [nu0], nu0 + d]))[::-1]     # nu descending
    wl = 1e4 / target
    wl[np.argmin(np.abs(target - nu0))] = 5.0                               # 1e4 / 5 = nu0: x = 0
    assert np.all(np.diff(wl) > 0)
    nu = lines_ref.wavenumbers(wl)
    assert (nu == nu0).sum() == 1

    # the fp64 (x, y) of the definition and its cutoff comparison
    A, ia, ga = lines_ref.line_parameters([nu0], [S_ref], [E_low], [gamma_ref], [n_exp],
                                          mass_amu, T_ref, q_ratio, T_nodes)
    dnu = np.abs(nu - nu0)
    inside = dnu <= cutoff
    assert inside.sum() < nu.size and inside[0] == inside[-1] == False  # noqa: E712
    x = dnu[None, :] * ia[:, :1]
    y = ga[:, :1] * p_nodes[None, :]
    K = np.zeros((2, p_nodes.size, nu.size))
    for t in range(2):
        for k in range(p_nodes.size):
            for i in range(nu.size):
                K[t, k, i] = float(faddeeva_re(mp.mpf(x[t, i]), mp.mpf(y[t, k])))
        print("K", t, flush=True)

    # the definition, exactly
    f = mp.mpf
    c2 = f(H) * f(C) / f(K_B)
    m = f(mass_amu) * f(AMU)
    values = np.zeros_like(K)
    for t in range(2):
        T = f(T_nodes[t])
        S = (f(S_ref) * f(q_ratio[t]) * mp.exp(-c2 * f(E_low) * (1 / T - 1 / f(T_ref))) *
             mp.expm1(-c2 * f(nu0) / T) / mp.expm1(-c2 * f(nu0) / f(T_ref)))
        al = f(nu0) * mp.sqrt(2 * f(K_B) * T / m) / f(C)
        gT = f(gamma_ref) * mp.exp(f(n_exp) * mp.log(f(T_ref) / T))
        for k in range(p_nodes.size):
            yy = gT * f(p_nodes[k]) / al
            for i in np.nonzero(inside)[0]:
                xx = abs(f(nu[i]) - f(nu0)) / al
                values[t, k, i] = float(S / (al * mp.sqrt(mp.pi)) * faddeeva_re(xx, yy) / m)
        print("values", t, flush=True)
    nz = values[values != 0]
    assert nz.min() >= 2.0 ** -100 and nz.max() < 2.0 ** 127, (nz.min(), nz.max())
    assert x.max() > 1e4 and y.min() < 1e-7 * 1.5 and y.max() > 1e3

    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "voigt_case.npz")
    np.savez_compressed(out, nu0=np.array([nu0]), S_ref=np.array([S_ref]), E_low=np.array([E_low]),
                        gamma_ref=np.array([gamma_ref]), n_exp=np.array([n_exp]),
                        mass_amu=np.array(mass_amu), T_ref=np.array(T_ref),
                        cutoff=np.array(cutoff), q_ratio=q_ratio, T_nodes=T_nodes,
                        p_nodes=p_nodes, wl_hi=wl, x=x, y=y, K=K, inside=inside, values=values)
    print(out, os.path.getsize(out), "bytes;", nu.size, "points; x max", x.max(), "y range",
          y.min(), y.max(), "values", nz.min(), nz.max())


if __name__ == "__main__":
    main()
