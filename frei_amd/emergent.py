"""Emergent intensities at viewing angles and the ray-traced (disk-integrated) spectrum: the
formal solution along rays through the final emit's optical depths on the GPU (frei_emergent,
K11).

The reference has no counterpart; the definition is the header comment of ``frei_emergent`` in
include/frei_hip.h.  The dtaus are absorption optical depths (twostream.py:371-373), so this is
the pure-absorption formal solution: scattering enters neither as extinction nor as source.
:func:`gauss_angles` is the default quadrature; the engines' ``emergent`` methods take whatever
angles and weights they are handed.
"""
import numpy as np

from . import _native as N
from .units import value

__all__ = ["gauss_angles"]


def gauss_angles(n):
    """(mu, weights) of the ``n``-point Gauss-Legendre rule mapped to (0, 1): nodes ascending,
    sum(weights) = 1 and sum(weights * mu) = 1/2, so an isothermal atmosphere's flux
    ``2 pi sum_k weights[k] mu[k] I(mu[k])`` is ``pi B``."""
    n = int(n)
    if n < 1:
        raise ValueError("gauss_angles needs n >= 1")
    x, w = np.polynomial.legendre.leggauss(n)
    return 0.5 * (x + 1.0), 0.5 * w


def emergent_call(eng, n_atm, T, mu, weights, dtaus, want_intensity):
    """frei_emergent on ``eng``'s context -> (flux[n_atm][n_lam] or None,
    intensity[n_atm][n_mu][n_lam] or None).  ``mu`` None: gauss_angles(4) with its weights;
    ``mu`` without ``weights``: intensities only."""
    nL, n = eng.n_layers, eng.n_lam
    if mu is None:
        if weights is not None:
            raise ValueError("weights need the mu they belong to")
        mu, weights = gauss_angles(4)
    mu = N.f64(mu).reshape(-1)
    if not 1 <= mu.size <= 64:
        raise ValueError(f"mu must hold 1 to 64 angles, not {mu.size}")
    w = None
    if weights is not None:
        w = N.f64(weights).reshape(-1)
        if w.size != mu.size:
            raise ValueError(f"weights must hold one value per angle ({mu.size}), not {w.size}")
    Th = N.f64(value(T, "K")).reshape(-1)
    if Th.size != n_atm * nL:
        raise ValueError(f"T must hold {n_atm} x {nL} temperatures, not {Th.size}")
    d = None
    if dtaus is not None:
        d = N.f64(dtaus)
        if d.size != n_atm * nL * n:
            raise ValueError(f"dtaus must have shape {(n_atm, nL, n)}, not {d.shape}")
    flux = np.empty((n_atm, n)) if w is not None else None
    inten = np.empty((n_atm, mu.size, n)) if (want_intensity or w is None) else None
    N.check(N.lib().frei_emergent(eng._ctx, N.dptr(d), N.dptr(Th), N.dptr(mu), N.dptr(w),
                                  mu.size, N.dptr(inten), N.dptr(flux)))
    return flux, inten


def pick(flux, inten, m=None):
    """What the ``emergent`` methods return: flux, intensity or (flux, intensity); row ``m`` of
    each for a single context."""
    if m is not None:
        flux = None if flux is None else flux[m]
        inten = None if inten is None else inten[m]
    if flux is None:
        return inten
    return flux if inten is None else (flux, inten)
