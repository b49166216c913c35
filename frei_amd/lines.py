"""Cross-sections from line lists (K17, ``frei_amd/csrc/frei_lines.hip``).

A :class:`LineList` holds one species' lines in the HITRAN / ExoMol style — position, strength
at a reference temperature, lower-state energy, Lorentz half-width and its temperature exponent —
with the species' mass and partition function.  :meth:`LineList.cross_section` computes the
float32 ``opacity[temperature][pressure][wavelength]`` table on the device (Voigt profiles summed
line by line inside a wing cutoff; the definition is in ``include/frei_hip.h``,
``frei_xsec_create_lines``) and returns it as a :class:`~frei_amd.binning.CrossSection` whose
values never leave the device unless asked for: ``binned_opacity(cross_sections=...)`` and
``Grid.load_opacities(cross_sections=...)`` take it like an uploaded one.

The reference downloads this table pre-computed (opacity.py:345-372, 493-540); nothing here
downloads anything.
"""
import ctypes

import numpy as np

from . import _native as N
from .binning import CrossSection
from .units import value

__all__ = ["LineList"]

ATM_IN_BAR = 1.01325


def _finite(name, a):
    bad = np.nonzero(~np.isfinite(a))[0]
    if bad.size:
        raise ValueError(f"{name}[{bad[0]}] = {a[bad[0]]} is not finite")


def _require(name, a, ok, why):
    _finite(name, a)
    bad = np.nonzero(~ok(a))[0]
    if bad.size:
        raise ValueError(f"{name}[{bad[0]}] = {a[bad[0]]} {why}")


class LineList:
    """Lines of one species: ``nu0`` (cm^-1), ``S`` (cm molecule^-1 at ``T_ref``), ``E_low``
    (cm^-1), ``gamma`` (Lorentz HWHM, cm^-1 per bar at ``T_ref``), ``n_exp`` (its temperature
    exponent: gamma(T) = gamma (T_ref / T)^n_exp); ``mass`` in amu; ``partition`` = (T_tab, Q_tab),
    the partition function Q on ascending temperatures (K).  The lines are stable-sorted by
    position."""

    def __init__(self, nu0, S, E_low, gamma, n_exp, mass, T_ref=296.0, partition=None):
        arrs = [np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in (nu0, S, E_low, gamma,
                                                                        n_exp)]
        n = arrs[0].size
        if n < 1:
            raise ValueError("a line list needs at least one line")
        for name, a in zip(("nu0", "S", "E_low", "gamma", "n_exp"), arrs):
            if a.ndim != 1 or a.size != n:
                raise ValueError(f"{name} must be one-dimensional with {n} entries like nu0")
        nu0, S, E_low, gamma, n_exp = arrs
        _require("nu0", nu0, lambda a: a > 0, "must be > 0")
        _require("S", S, lambda a: a >= 0, "must be >= 0")
        _finite("E_low", E_low)
        _require("gamma", gamma, lambda a: a > 0, "must be > 0")
        _finite("n_exp", n_exp)
        self.mass = float(mass)
        self.T_ref = float(T_ref)
        if not (np.isfinite(self.mass) and self.mass > 0):
            raise ValueError("mass must be finite and > 0 (amu)")
        if not (np.isfinite(self.T_ref) and self.T_ref > 0):
            raise ValueError("T_ref must be finite and > 0 (K)")
        if partition is None:
            raise ValueError("partition=(T_tab, Q_tab) is required")
        T_tab, Q_tab = (np.atleast_1d(np.asarray(a, dtype=np.float64)) for a in partition)
        if T_tab.ndim != 1 or T_tab.shape != Q_tab.shape or T_tab.size < 2:
            raise ValueError("partition needs T_tab and Q_tab of one length >= 2")
        _require("partition T_tab", T_tab, lambda a: a > 0, "must be > 0")
        if not np.all(np.diff(T_tab) > 0):
            raise ValueError("partition T_tab must be strictly ascending")
        _require("partition Q_tab", Q_tab, lambda a: a > 0, "must be > 0")
        self._T_tab, self._lnQ = T_tab, np.log(Q_tab)
        if not T_tab[0] <= self.T_ref <= T_tab[-1]:
            raise ValueError(f"T_ref = {self.T_ref} K lies outside the partition table "
                             f"[{T_tab[0]}, {T_tab[-1]}] K")
        order = np.argsort(nu0, kind="stable")
        self.nu0, self.S, self.E_low, self.gamma, self.n_exp = (
            np.ascontiguousarray(a[order]) for a in (nu0, S, E_low, gamma, n_exp))

    def __len__(self):
        return self.nu0.size

    def q_ratio(self, temperature):
        """Q(T_ref) / Q(T), ln Q interpolated linearly in T; raises outside the table."""
        T = np.atleast_1d(np.asarray(value(temperature, "K"), dtype=np.float64))
        bad = np.nonzero(~((T >= self._T_tab[0]) & (T <= self._T_tab[-1])))[0]
        if bad.size:
            raise ValueError(f"temperature[{bad[0]}] = {T[bad[0]]} K lies outside the partition "
                             f"table [{self._T_tab[0]}, {self._T_tab[-1]}] K")
        lnq = np.interp(T, self._T_tab, self._lnQ)
        lnq_ref = np.interp(self.T_ref, self._T_tab, self._lnQ)
        return np.exp(lnq_ref - lnq)

    def cross_section(self, temperature, pressure, wavelength, cutoff=25.0, device=0,
                      isotopologue=None):
        """The cross-section (cm^2 g^-1) on nodes ``temperature`` (K) x ``pressure`` (bar) and
        the axis ``wavelength`` (µm, strictly ascending), every line's Voigt profile summed
        within ``cutoff`` cm^-1 of its position, computed on ``device``.  The returned
        CrossSection holds no host copy (``.opacity`` is None); ``.values()`` downloads it."""
        T = np.ascontiguousarray(np.atleast_1d(value(temperature, "K")), dtype=np.float64)
        p = np.ascontiguousarray(np.atleast_1d(value(pressure, "bar")), dtype=np.float64)
        wl = np.ascontiguousarray(np.atleast_1d(value(wavelength, "um")), dtype=np.float64)
        qr = np.ascontiguousarray(self.q_ratio(T))
        cutoff = float(cutoff)
        timing = {}

        def make(dev):
            h, ms = ctypes.c_void_p(), ctypes.c_double(0.0)
            N.check(N.lib().frei_xsec_create_lines(
                ctypes.byref(h), dev, self.nu0.size, N.dptr(self.nu0), N.dptr(self.S),
                N.dptr(self.E_low), N.dptr(self.gamma), N.dptr(self.n_exp), self.mass,
                self.T_ref, cutoff, N.dptr(qr), T.size, p.size, wl.size, N.dptr(T), N.dptr(p),
                N.dptr(wl), ctypes.byref(ms)))
            timing[dev] = ms.value
            return h

        xs = CrossSection._from_lines(make, T, p, wl, isotopologue)
        xs.handle(device)
        xs.kernel_ms = timing[device]     # HIP-event time of the main kernel
        return xs

    @classmethod
    def from_hitran_par(cls, path, mass, partition, T_ref=296.0):
        """Read the fixed-width 160-character HITRAN ``.par`` records of a local file: position
        (columns 4-15), intensity at 296 K (16-25), air-broadened half-width (36-40, cm^-1 per
        atm, converted to per bar), lower-state energy (46-55) and the half-width's temperature
        exponent (56-59)."""
        nu0, S, E_low, gamma, n_exp = [], [], [], [], []
        with open(path) as f:
            for k, rec in enumerate(f):
                rec = rec.rstrip("\r\n")
                if not rec.strip():
                    continue
                if len(rec) != 160:
                    raise ValueError(f"{path}: record {k + 1} has {len(rec)} characters, not 160")
                try:
                    nu0.append(float(rec[3:15]))
                    S.append(float(rec[15:25]))
                    gamma.append(float(rec[35:40]) / ATM_IN_BAR)
                    E_low.append(float(rec[45:55]))
                    n_exp.append(float(rec[55:59]))
                except ValueError as e:
                    raise ValueError(f"{path}: record {k + 1}: {e}") from None
        return cls(nu0, S, E_low, gamma, n_exp, mass, T_ref=T_ref, partition=partition)
