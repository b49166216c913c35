"""Transmission (transit-depth) spectra: the chord geometry on the host, the slant optical
depths and the effective area on the GPU (frei_transit, K9).

The reference has no counterpart; the definition is the header comment of ``frei_transit`` in
include/frei_hip.h, in frei's conventions: layer 0 is the bottom, g and m_bar are constant, the
emit top layer's virtual level sits at p[-1] * p[-2] / p[-3] (twostream.py:358-363) and a
shell's thickness is ``delta_z_i`` (twostream.py:180-187).  :func:`level_radii` is the only place
the radii are formed; the engines' ``transit`` methods take them as they are.
"""
import numpy as np

from . import _native as N
from .constants import K_B
from .units import scalar, value

__all__ = ["level_radii"]


def level_radii(T, p_bar, g, m_bar, R_p, P_ref=None):
    """Radii r[n_layers] (cm) of the levels 1 .. n_layers of an atmosphere in hydrostatic
    equilibrium: level l <= n_layers - 1 at ``p_bar[l]``, the virtual top level at
    ``p_bar[-1] * p_bar[-2] / p_bar[-3]``; ``r[k]`` is the radius of level k + 1.

    Shell l between levels l and l + 1 is ``k_B T[l] / (m_bar g) * ln(p_l / p_{l+1})`` thick.
    ``R_p`` (cm) is the radius at the pressure ``P_ref`` (bar), by default at level 1
    (``p_bar[1]``); a ``P_ref`` between two levels is placed linearly in ln p inside its shell,
    one outside [top level, level 1] is a ValueError."""
    T = np.asarray(value(T, "K"), dtype=float)
    p = np.asarray(value(p_bar, "bar"), dtype=float)
    g, m_bar, R_p = scalar(g, "cm / s2"), scalar(m_bar, "g"), scalar(R_p, "cm")
    nL = p.size
    if nL < 4 or T.shape != p.shape:
        raise ValueError("T and p_bar must be [n_layers] with n_layers >= 4")
    p_lev = np.concatenate([p[1:], [p[-1] * p[-2] / p[-3]]])   # p_lev[k] = p_{k+1}
    ln = np.log(p_lev[:-1] / p_lev[1:])                        # ln(p_l / p_{l+1}), l = 1 ..
    dz = K_B * T[1:] / (m_bar * g) * ln
    z_ref = 0.0
    if P_ref is not None:
        P_ref = scalar(P_ref, "bar")
        if not (p_lev[-1] <= P_ref <= p_lev[0]):
            raise ValueError(f"P_ref = {P_ref} bar lies outside the levels "
                             f"[{p_lev[-1]:.6g}, {p_lev[0]:.6g}] bar")
        k = min(int(np.count_nonzero(p_lev >= P_ref)) - 1, nL - 2)   # its shell: level k + 1
        z = 0.0
        for l in range(k):
            z = z + dz[l]
        z_ref = z + dz[k] * np.log(p_lev[k] / P_ref) / ln[k]
    r = np.empty(nL)
    r[0] = R_p - z_ref
    for l in range(nL - 1):
        r[l + 1] = r[l] + dz[l]
    return r


def default_radius(arg, planet, attr, what):
    """The argument, else the Planet's value; ValueError with neither."""
    v = arg if arg is not None else getattr(planet, attr, None)
    if v is None:
        raise ValueError(f"transmission spectrum needs {what}: pass {attr} or give the Planet one")
    return scalar(v, "cm")


def transit_call(eng, n_atm, radii, R_star, dtaus, want_tau):
    """frei_transit on ``eng``'s context -> depth[n_atm][n_lam] (and tau_slant[n_atm]
    [n_layers - 1][n_lam] with ``want_tau``)."""
    nL, n = eng.n_layers, eng.n_lam
    r = N.f64(value(radii, "cm")).reshape(-1)
    if r.size != n_atm * nL:
        raise ValueError(f"radii must hold {n_atm} x {nL} level radii, not {r.size}")
    d = None
    if dtaus is not None:
        d = N.f64(dtaus)
        if d.size != n_atm * nL * n:
            raise ValueError(f"dtaus must have shape {(n_atm, nL, n)}, not {d.shape}")
    depth = np.empty((n_atm, n))
    tau = np.empty((n_atm, nL - 1, n)) if want_tau else None
    N.check(N.lib().frei_transit(eng._ctx, N.dptr(d), N.dptr(r), scalar(R_star, "cm"),
                                 N.dptr(depth), N.dptr(tau)))
    return depth, tau
