"""Plain NumPy restatement of the emergent-intensity definition (the header comment of
frei_emergent in include/frei_hip.h), written from the definition alone: explicit loops over the
angle k and the shell l in the stated order, vectorised over wavelength only.  The checker of
tests/test_gpu_emergent.py, itself pinned by tests/test_emergent_host.py; it imports nothing of
the package under test.

Notation: nL = n_layers; levels l = 1 .. nL - 1 carry T_l = T[l], the virtual top level nL has
T_nL = T_{nL-1}; shell l (1 <= l <= nL - 1) lies between levels l and l + 1 and has the vertical
optical depth ``dtaus[l]``; row 0 of ``dtaus`` and ``T[0]`` are never read."""
import numpy as np

H = 6.62607015e-27       # erg s        (CODATA 2018)
C = 29979245800.0        # cm s^-1
K_B = 1.380649e-16       # erg K^-1
UM = 1e-4                # cm per micron

# 1/2!, -1/3!, ..., +1/11!: v(x) = x/2 - x^2/6 + x^3/24 - ... - x^10/11!
_V_COEF = []
_f = 1.0
for _k in range(2, 12):
    _f *= _k
    _V_COEF.append((1.0 if _k % 2 == 0 else -1.0) / _f)


def planck(lam_um, T):
    """B = c1 / expm1((h c / lk) * (1 / T)) with c1 = 2 h c^2 / lam^5 and lk = lam k_B, lam in
    cm: the constants a context is given (frei_set_grid)."""
    lam_cm = np.asarray(lam_um, dtype=float) * UM
    c1 = 2 * H * C ** 2 / np.power(lam_cm, 5)
    lk = lam_cm * K_B
    return c1 / np.expm1((H * C / lk) * (1.0 / T))


def v_of(x):
    """v = 1 - em / x with em = -expm1(-x): by the series through the x^10 / 11! term in Horner
    form for x <= 1/8, by the formula above that; v(0) = 0, v(inf) = 1."""
    x = np.asarray(x, dtype=float)
    small = x <= 0.125
    xs = np.where(small, x, 0.0)
    s = np.full(x.shape, _V_COEF[-1])
    for c in _V_COEF[-2::-1]:
        s = s * xs + c
    s = s * xs
    with np.errstate(divide="ignore", invalid="ignore"):
        big = 1.0 - (-np.expm1(-x)) / x
    return np.where(small, s, big)


def weights_of(x):
    """(e, u, v) of one step: e = exp(-x), v as above, u = em - v."""
    x = np.asarray(x, dtype=float)
    e = np.exp(-x)
    em = -np.expm1(-x)
    v = v_of(x)
    return e, em - v, v


def emergent(dtaus, T, lam_um, mu, weights=None):
    """(intensity[n_mu][n_lam], flux[n_lam] or None) of one atmosphere."""
    dtaus = np.asarray(dtaus, dtype=float)
    T = np.asarray(T, dtype=float)
    mu = np.asarray(mu, dtype=float)
    nL, n = dtaus.shape
    assert T.shape == (nL,)
    B = {l: planck(lam_um, T[l]) for l in range(1, nL)}
    B[nL] = B[nL - 1]
    inten = np.empty((mu.size, n))
    for k in range(mu.size):
        I = B[1].copy()
        for l in range(1, nL):
            with np.errstate(over="ignore"):
                x = dtaus[l] / mu[k]
            e, u, v = weights_of(x)
            I = I * e + (B[l] * u + B[l + 1] * v)
        inten[k] = I
    flux = None
    if weights is not None:
        c = np.asarray(weights, dtype=float) * mu
        s = c[0] * inten[0]
        for k in range(1, mu.size):
            s = s + c[k] * inten[k]
        flux = 2 * np.pi * s
    return inten, flux
