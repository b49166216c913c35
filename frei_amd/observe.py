"""Synthetic observations: spectra taken to the channels of an instrument on the GPU (K10,
``frei_amd/csrc/frei_observe.hip``) and scored against data.

An :class:`Instrument` is K channels on a native wavelength axis: channel k covers the
contiguous native indices ``first[k] .. first[k] + count[k] - 1`` with one weight per covered
index, stored back to back.  Plan and weights are uploaded once and stay in HBM; ``apply``
forms, per atmosphere m and channel k,

    obs[m][k] = scale_m * (sum_t w x[m] num[select_m]) / (sum_t w den[select_m])

and on request ``chi2[m] = sum_k ((obs[m][k] - data[k]) / sigma[k])^2``.  The reference has no
counterpart; the definition is the header comment of ``frei_obs_apply`` in include/frei_hip.h.
The three observables are thin layers over that one call: the channel-mean flux, the
secondary-eclipse depth (a ratio of band integrals, not a mean of ratios) and the band-averaged
transit depth.  The constructors (top-hat bands, throughput curves, a Gaussian line-spread
function) build plan and weights on the host in NumPy, O(number of weights).
"""
import ctypes

import numpy as np

from . import _native as N
from ._device import (DeviceObject, broadened_source, i32ptr, library_rows, per_atmosphere,
                      kept_suffix, resident_or_host, select_rows, unknown_kind)
from .engine import trapz_weights
from .transit import default_radius
from .twostream import BB
from .units import value

__all__ = ["Instrument"]

FLUX = "erg / (s cm3)"
_i64p = ctypes.POINTER(ctypes.c_int64)


def _axis(lam):
    lam = N.f64(value(lam, "um"))
    if lam.ndim != 1 or lam.size < 1:
        raise ValueError("lam must be a 1-D wavelength axis")
    if np.any(np.diff(lam) <= 0):
        raise ValueError("lam must be strictly ascending")
    return lam


def _window(lam, lo, hi, inside):
    """[a, b): the points of ``lam`` for which ``inside`` holds, searched around [lo, hi] (the
    predicate decides at the edges, so the plan is exactly the definition's)."""
    a = max(int(np.searchsorted(lam, lo, "left")) - 1, 0)
    b = min(int(np.searchsorted(lam, hi, "right")) + 1, lam.size)
    hit = np.nonzero(inside(lam[a:b]))[0]
    return (a + int(hit[0]), a + int(hit[-1]) + 1) if hit.size else (a, a)


def star_flux(planet, lam):
    """The star's surface flux on the grid (erg s^-1 cm^-3): ``planet.stellar_spectrum``, else
    ``pi * B_star(T_star, lam)``."""
    s = getattr(planet, "stellar_spectrum", None)
    if s is not None:
        return np.asarray(s, dtype=float)
    return np.pi * BB(planet.T_star)(lam)


def star_library(planets, lam):
    """(library [n_lib][n_lam], select [n_atm]) of the planets' stars: distinct stellar spectra
    (by identity, else by T_star) once each, in order of first use."""
    keys, rows, select = [], [], []
    for pl in planets:
        if pl is None:
            raise ValueError("the observable needs each atmosphere's Planet (its star)")
        s = getattr(pl, "stellar_spectrum", None)
        key = ("T", pl.T_star) if s is None else ("id", id(s))
        if key not in keys:
            keys.append(key)
            rows.append(star_flux(pl, lam))
        select.append(keys.index(key))
    return N.f64(np.array(rows)), np.array(select, dtype=np.int32)


class Instrument(DeviceObject):
    """K channels on the native axis ``lam`` ([n_lam], µm): ``first`` and ``count`` [K] and the
    channels' ``weights`` back to back ([sum(count)], finite, >= 0, each channel's sum > 0),
    resident on ``device``.  Channels may overlap and come in any order."""

    _destroy = "frei_obs_destroy"

    def __init__(self, lam, first, count, weights, device=0):
        super().__init__(device)
        self.lam = N.f64(value(lam, "um"))
        self.first = np.ascontiguousarray(first, dtype=np.int64)
        self.count = np.ascontiguousarray(count, dtype=np.int64)
        self.weights = N.f64(weights)
        if self.lam.ndim != 1 or self.first.ndim != 1 or self.first.shape != self.count.shape:
            raise ValueError("lam must be [n_lam], first and count [n_channels]")
        if self.first.size < 1:
            raise ValueError("an instrument needs at least one channel")
        if self.weights.ndim != 1 or self.weights.size != int(np.maximum(self.count, 0).sum()):
            raise ValueError("weights must hold one value per covered point: "
                             f"{int(np.maximum(self.count, 0).sum())}, not {self.weights.size}")

    @property
    def n_channels(self):
        return self.first.size

    @property
    def n_lam(self):
        return self.lam.size

    # ------------------------------------------------------------------ constructors
    @classmethod
    def _build(cls, lam, spans, weights_of, what, device, trim):
        """Channels from candidate spans [a, b): their weights, cut (``trim``) to the span from
        the first to the last non-zero one."""
        tw = trapz_weights(lam)
        first, count, ws = [], [], []
        for k, (a, b) in enumerate(spans):
            w = weights_of(k, a, b, tw) if b > a else np.empty(0)
            nz = np.nonzero(w)[0] if trim else np.arange(w.size)
            if nz.size == 0:
                raise ValueError(f"channel {k} {what}")
            first.append(a + int(nz[0]))
            count.append(int(nz[-1]) - int(nz[0]) + 1)
            ws.append(w[nz[0]:nz[-1] + 1])
        return cls(lam, first, count, np.concatenate(ws), device=device)

    @classmethod
    def top_hat(cls, lam, lo, hi, device=0):
        """Bands ``lo[k] <= lam <= hi[k]`` (µm, edges included) with the axis' trapezoid
        weights.  A band holding no point is a ValueError naming it."""
        lam = _axis(lam)
        lo, hi = np.atleast_1d(value(lo, "um")), np.atleast_1d(value(hi, "um"))
        if lo.shape != hi.shape or lo.ndim != 1:
            raise ValueError("lo and hi must be [n_channels]")
        tw = trapz_weights(lam)
        first, count, ws = [], [], []
        for k in range(lo.size):
            a = int(np.searchsorted(lam, lo[k], "left"))
            b = int(np.searchsorted(lam, hi[k], "right"))
            if b <= a:
                raise ValueError(f"channel {k} holds no point of the axis: "
                                 f"[{lo[k]:.6g}, {hi[k]:.6g}] um")
            first.append(a)
            count.append(b - a)
            ws.append(tw[a:b])
        return cls(lam, first, count, np.concatenate(ws), device=device)

    @classmethod
    def from_throughput(cls, lam, curves, device=0):
        """Channels from throughput curves ``curves[k] = (wl, T)`` (µm, ascending; any scale):
        ``w = tw * np.interp(lam, wl, T, left=0, right=0)``; a channel's support runs from its
        first to its last non-zero weight (zeros inside stay)."""
        lam = _axis(lam)
        curves = [(np.asarray(value(wl, "um"), dtype=float), np.asarray(T, dtype=float))
                  for wl, T in curves]
        spans = [(int(np.searchsorted(lam, wl[0], "left")),
                  int(np.searchsorted(lam, wl[-1], "right"))) for wl, _ in curves]

        def weights_of(k, a, b, tw):
            wl, T = curves[k]
            return tw[a:b] * np.interp(lam[a:b], wl, T, left=0, right=0)
        return cls._build(lam, spans, weights_of, "has no non-zero weight on the axis", device,
                          True)

    @classmethod
    def gaussian(cls, lam, centres, fwhm=None, resolving_power=None, n_sigma=4.0, device=0):
        """Gaussian line-spread functions at ``centres`` (µm) of width ``fwhm`` (µm, scalar or
        per channel) or ``fwhm_k = centre_k / resolving_power``, cut at ``n_sigma`` standard
        deviations: ``w = tw * exp(-((lam - c) / s)^2 / 2)`` for ``|lam - c| <= n_sigma s``."""
        lam = _axis(lam)
        c = np.atleast_1d(value(centres, "um"))
        if (fwhm is None) == (resolving_power is None):
            raise ValueError("pass either fwhm or resolving_power")
        fw = c / float(resolving_power) if fwhm is None else np.broadcast_to(value(fwhm, "um"),
                                                                            c.shape)
        s = fw / (2.0 * np.sqrt(2.0 * np.log(2.0)))
        spans = []
        for k in range(c.size):
            h = n_sigma * s[k]
            spans.append(_window(lam, c[k] - h, c[k] + h,
                                 lambda x, ck=c[k], h=h: np.abs(x - ck) <= h))

        def weights_of(k, a, b, tw):
            z = (lam[a:b] - c[k]) / s[k]
            return tw[a:b] * np.exp(-0.5 * (z * z))
        return cls._build(lam, spans, weights_of, "holds no point of the axis", device, False)

    def for_columns(self, n_g, weights):
        """The instrument on the columns of a k-distribution (K20): the axis is
        ``repeat(lam, n_g)`` (column ``b * n_g + q`` is bin b at g-point q), channel k covers the
        columns of its bins — ``first * n_g``, ``count * n_g`` — and column (b, q) weighs
        ``W_b w_q``: ``repeat(w_chan, n_g) * tile(weights, count)``.  With per-wavelength ``num``
        and ``den`` repeated onto the columns, x on the columns gives
        ``sum_b W_b sum_q w_q x_bq num_b / sum_b W_b sum_q w_q den_b``: the band value of the
        collapsed spectrum up to rounding, which never has to exist on the device.  Host plan
        construction only."""
        w_q = N.f64(np.atleast_1d(weights))
        n_g = int(n_g)
        if n_g < 1 or w_q.shape != (n_g,):
            raise ValueError(f"weights must be [n_g = {n_g}], one per quadrature point")
        if not np.all(np.isfinite(w_q) & (w_q > 0)):
            raise ValueError("the quadrature weights must be finite and positive")
        return Instrument(np.repeat(self.lam, n_g), self.first * n_g, self.count * n_g,
                          np.repeat(self.weights, n_g) * np.tile(w_q, self.weights.size),
                          device=self.device)

    # ------------------------------------------------------------------ device
    def _create(self, h):
        """frei_obs* of the instrument (plan and weights uploaded once)."""
        return N.lib().frei_obs_create(
            ctypes.byref(h), self.device, self.lam.size, self.first.size,
            self.first.ctypes.data_as(_i64p), self.count.ctypes.data_as(_i64p),
            N.dptr(self.weights))

    def apply(self, x, num=None, den=None, select=None, scale=None, data=None, sigma=None,
              form=0, engine=None):
        """The instrument applied to ``x`` ([n_lam] or [n_atm][n_lam]) -> ``obs`` ([K] or
        [n_atm][K]); ``(obs, chi2)`` with ``data`` and ``sigma`` ([K]; ``sigma = inf`` drops a
        channel).  ``num`` and ``den`` are optional libraries ([n_lam] or [n_lib][n_lam]),
        ``select`` [n_atm] the library row of each atmosphere (default row 0), ``scale`` a
        factor per atmosphere.  ``x=None`` with ``engine=`` (an Engine or BatchEngine on the
        whole axis) takes the emergent spectra resident in the engine's flux state; a
        :class:`~frei_amd.broaden.BroadenedSpectra` as ``x`` takes what
        ``Broadening.apply(keep=True)`` left on the device, an
        :class:`~frei_amd.modelgrid.InterpolatedSpectra` what
        ``ModelGrid.interpolate(keep=True)`` left there (its queries are the atmospheres).  ``form``
        0 picks the kernel from the points per channel, 1 forces one lane per channel, 2 one
        group of lanes per channel (``form_used`` records the choice)."""
        kept = kept_suffix(x)
        x, ctx, brd, n_atm, single, _ = resident_or_host(
            x, engine, self.n_lam, ("an instrument", "a channel"))
        num = library_rows(num, "num", self.n_lam)
        den = library_rows(den, "den", self.n_lam)
        n_lib = 0
        if num is not None or den is not None:
            n_lib = (num if num is not None else den).shape[0]
            if num is not None and den is not None and num.shape != den.shape:
                raise ValueError("num and den must hold the same number of rows")
        sel = select_rows(select, n_atm)
        sc = per_atmosphere(scale, n_atm)
        if (data is None) != (sigma is None):
            raise ValueError("chi2 needs both data and sigma")
        K = self.n_channels
        chi2 = None
        if data is not None:
            data, sigma = N.f64(data), N.f64(sigma)
            if data.shape != (K,) or sigma.shape != (K,):
                raise ValueError(f"data and sigma must be [{K}], one value per channel")
            chi2 = np.empty(n_atm)
        obs = np.empty((n_atm, K))
        used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        tail = (N.dptr(num), N.dptr(den), n_lib, i32ptr(sel), N.dptr(sc), N.dptr(data),
                N.dptr(sigma), int(form), N.dptr(obs), N.dptr(chi2), ctypes.byref(used),
                ctypes.byref(ms))
        if brd is not None:
            N.check(getattr(N.lib(), "frei_obs_apply" + kept)(self.handle(), brd, n_atm, *tail))
        else:
            N.check(N.lib().frei_obs_apply(self.handle(), ctx, N.dptr(x), n_atm, *tail))
        self._record(used, ms)
        if single:
            obs = obs[0]
            chi2 = None if chi2 is None else float(chi2[0])
        return obs if chi2 is None else (obs, chi2)

    # ------------------------------------------------------------------ observables
    def eclipse(self, F_planet, F_star, R_p, R_star, select=None, **kw):
        """Secondary-eclipse depths: (band integral of F_planet / band integral of F_star) *
        (R_p / R_star)^2.  ``F_star`` [n_lam] or a library [n_lib][n_lam] with ``select``;
        radii in cm or Quantities, scalars or one per atmosphere."""
        ratio = np.asarray(value(R_p, "cm")) / np.asarray(value(R_star, "cm"))
        F_star = None if F_star is None else value(F_star, FLUX)
        if kept_suffix(F_planet) is None:       # spectra kept on the device pass as they are
            F_planet = value(F_planet, FLUX)
        return self.apply(F_planet, den=F_star, select=select, scale=ratio * ratio, **kw)

    def transit(self, depth, F_star=None, select=None, **kw):
        """Band-averaged transit depths, weighted by the stellar flux ``F_star`` (a library
        with ``select``, as in :meth:`eclipse`) or, without it, by the channel weights alone."""
        F_star = None if F_star is None else N.f64(value(F_star, FLUX))
        return self.apply(depth, num=F_star, den=F_star, select=select, **kw)


def eclipse_scale(planets, R_p, R_star):
    """(R_p / R_star)^2 per atmosphere; radii default to each Planet's (ValueError without)."""
    A = len(planets)

    def per_atm(x):
        return [None] * A if x is None else list(np.broadcast_to(value(x, "cm"), (A,)))
    Rp = [default_radius(x, pl, "R_p", "the planet's radius")
          for x, pl in zip(per_atm(R_p), planets)]
    Rs = [default_radius(x, pl, "R_star", "the star's radius")
          for x, pl in zip(per_atm(R_star), planets)]
    return np.array([(a / b) * (a / b) for a, b in zip(Rp, Rs)])


def observe(instrument, kind, planets, lam, x=None, engine=None, weighting=None, data=None,
            sigma=None, R_p=None, R_star=None, broadening=None):
    """The observable ``kind`` ("flux", "eclipse" or "transit") of ``x`` (or of ``engine``'s
    resident spectra) for atmospheres whose stars are ``planets``'.  With ``broadening`` (a
    :class:`~frei_amd.broaden.Broadening`, K13) the spectrum is broadened first and stays on the
    device."""
    x, engine, star = broadened_source(kind, planets, lam, x, engine, R_p, R_star, broadening)
    kw = dict(data=data, sigma=sigma, engine=engine)
    if kind in ("flux", "eclipse"):
        return instrument.apply(x, **star, **kw)
    if kind == "transit":
        has_star = all(pl is not None for pl in planets)
        if weighting is None:
            weighting = "stellar" if has_star else "flat"
        if weighting == "flat":
            return instrument.apply(x, **kw)
        if weighting != "stellar":
            raise ValueError(f"unknown weighting {weighting!r}: 'stellar' or 'flat'")
        lib, select = star_library(planets, lam)
        return instrument.apply(x, num=lib, den=lib, select=select, **kw)
    raise unknown_kind(kind)
