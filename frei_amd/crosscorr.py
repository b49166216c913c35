"""Doppler cross-correlation of batched spectra with high-resolution data on the GPU (K12,
``frei_amd/csrc/frei_crosscorr.hip``).

A :class:`CrossCorrelator` is a time series of ``n_exp`` exposures on ``n_pix`` detector pixels
and a grid of ``n_vel`` trial velocities on a native wavelength axis.  For every velocity the
plan holds, per pixel, the native bracket ``idx`` and the weight ``frac`` of its upper point at
which the pixel samples the shifted template; plan, weighted data and weights are uploaded once
and stay in HBM.  ``correlate`` forms, per atmosphere m, exposure e and velocity v,

    g = y[m][j] + t (y[m][j+1] - y[m][j]),    y = scale_m (x[m] / den[select_m]) - offset_m
    S_fg[m][e][v] = sum_p a[e][p] g,   S_g[m][v] = sum_p w[p] g,   S_gg[m][v] = sum_p (w[p] g) g

and :class:`CrossCorrelation` turns the sums into the cross-correlation coefficient and the
log-likelihood on the host.  The reference has no counterpart; the definition is the header
comment of ``frei_ccf_apply`` in include/frei_hip.h.  The plan is built on the host: ``t`` is
ill-conditioned (a rounding of the shifted wavelength moves it by about R 2^-53), so the device
and any restatement must use the very same ``t``, and the plan can be checked without a GPU.
"""
import ctypes

import numpy as np

from . import _native as N
from ._device import (DeviceObject, broadened_source, i32ptr, library_rows, per_atmosphere,
                      kept_suffix, resident_or_host, select_rows, unknown_kind)
from .units import value

__all__ = ["CrossCorrelator", "CrossCorrelation", "KeptSums", "kp_vsys_map", "FORMS",
           "PIXEL_CHUNK", "C_KMS"]

C_KMS = 299792.458     # km/s
# the kernel forms that exist (frei_ccf_apply's `form`; 0 picks among them)
FORMS = (1, 2)
# pixels per chunk of the device sums (frei_crosscorr.hip kChunk): the order of summation
# changes at its multiples
PIXEL_CHUNK = 4096
_SUMS = ("sfg", "sg", "sgg")


def doppler_plan(lam, wl_data, velocities):
    """(idx [n_vel][n_pix] int32, frac [n_vel][n_pix], n_clamped [n_vel]) of pixels at
    ``wl_data`` sampling a template on ``lam`` shifted by ``velocities`` (km/s, positive
    receding): ``s = wl_data / (1 + v / c)`` clamped to the axis, ``idx`` the largest index with
    ``lam[idx] <= s`` limited to n_lam - 2, ``frac = (s - lam[idx]) / (lam[idx+1] - lam[idx])``."""
    d_v = 1.0 / (1.0 + velocities / C_KMS)
    s = wl_data[None, :] * d_v[:, None]
    n_clamped = np.count_nonzero((s < lam[0]) | (s > lam[-1]), axis=1)
    s = np.minimum(np.maximum(s, lam[0]), lam[-1])
    j = np.minimum(np.searchsorted(lam, s, "right") - 1, lam.size - 2)
    t = (s - lam[j]) / (lam[j + 1] - lam[j])
    return np.ascontiguousarray(j, dtype=np.int32), np.ascontiguousarray(t), n_clamped


class KeptSums:
    """What ``CrossCorrelator.correlate(keep=True)`` left on the device: the sums ``names`` of
    ``n_atm`` atmospheres, for :meth:`frei_amd.stack.OrbitStack.stack`.  It goes stale at the
    owner's next ``correlate`` or ``release``; using a stale one raises."""

    def __init__(self, owner, serial, n_atm, single, names):
        self.owner, self.serial, self.n_atm, self.single = owner, serial, n_atm, single
        self.names = tuple(names)

    def handle(self):
        """frei_ccf* of the owner, after the staleness check."""
        if self.owner._serial != self.serial or self.owner._handle is None:
            raise RuntimeError("stale kept sums: their CrossCorrelator has correlated again or "
                               "was released since")
        return self.owner._handle


class CrossCorrelation:
    """The sums of one :meth:`CrossCorrelator.correlate` call — ``sfg`` [n_atm][n_exp][n_vel],
    ``sg`` and ``sgg`` [n_atm][n_vel] (without the atmosphere axis for a 1-D ``x``; None where
    not asked for) — with ``velocities`` and the model-independent host sums ``W = sum w``,
    ``S_wf[e] = sum a[e]`` and ``S_wff[e] = sum a[e] flux[e]``.

    With ``gbar = S_g / W``: ``C_fg = S_fg - gbar S_wf``, ``V_g = S_gg - S_g gbar`` and
    ``V_f = S_wff - S_wf^2 / W`` are the weighted covariance and variances times W.

    Cancellation: ``V_g`` is a difference of two nearly equal numbers when the template's lines
    are shallow against its continuum (with lines of a few per cent on a flat continuum about
    0.3 % of ``S_gg`` survives), and ``C_fg`` likewise.  ``offset=`` in ``correlate`` (for
    example each template's mean over the data's span) removes the continuum before the sums
    are formed and is the remedy.

    ``kept`` is the :class:`KeptSums` of a ``correlate(..., keep=True)`` (None otherwise): the
    sums as they lie on the device, which :meth:`frei_amd.stack.OrbitStack.stack` turns into
    K_p-V_sys maps without a copy to the host (K14)."""

    def __init__(self, sfg, sg, sgg, velocities, W, S_wf, S_wff, n_pix, kept=None):
        self.sfg, self.sg, self.sgg = sfg, sg, sgg
        self.velocities = velocities
        self.W, self.S_wf, self.S_wff, self.n_pix = W, S_wf, S_wff, n_pix
        self.kept = kept

    def _moments(self):
        if self.sfg is None or self.sg is None or self.sgg is None:
            raise ValueError("the statistic needs all three sums (want=)")
        gbar = self.sg / self.W
        C_fg = self.sfg - gbar[..., None, :] * self.S_wf[:, None]
        V_g = (self.sgg - self.sg * gbar)[..., None, :]
        V_f = (self.S_wff - self.S_wf * self.S_wf / self.W)[:, None]
        return C_fg, V_f, V_g

    def ccf(self):
        """The weighted cross-correlation coefficient ``C_fg / sqrt(V_f V_g)``,
        [n_atm][n_exp][n_vel]."""
        C_fg, V_f, V_g = self._moments()
        return C_fg / np.sqrt(V_f * V_g)

    def loglike(self):
        """``-(n_pix / 2) log((V_f - 2 C_fg + V_g) / W)``, [n_atm][n_exp][n_vel]: the
        log-likelihood of Brogi & Line (2019), exact for unit weights."""
        C_fg, V_f, V_g = self._moments()
        return -(self.n_pix / 2.0) * np.log((V_f - 2.0 * C_fg + V_g) / self.W)


class CrossCorrelator(DeviceObject):
    """High-resolution data against Doppler-shifted templates on the native axis ``lam``
    ([n_lam], µm or a Quantity, strictly ascending).  ``wl_data`` [n_pix] (µm) in any order
    (several spectral orders back to back, overlapping or not), ``flux`` [n_exp][n_pix] or
    [n_pix], ``velocities`` [n_vel] in km/s (positive receding), ``weights`` [n_pix] (finite,
    >= 0; default ones).  ``a = weights * flux`` and ``w = weights`` are what the device holds.
    Beyond the axis the template is held constant; ``n_clamped`` [n_vel] counts the pixels for
    which that happened, so a caller can drop those velocities."""

    _destroy = "frei_ccf_destroy"

    def __init__(self, lam, wl_data, flux, velocities, weights=None, device=0):
        super().__init__(device)
        self.lam = N.f64(value(lam, "um"))
        if self.lam.ndim != 1 or self.lam.size < 2:
            raise ValueError("lam must be a 1-D wavelength axis of at least 2 points")
        if np.any(np.diff(self.lam) <= 0):
            raise ValueError("lam must be strictly ascending")
        self.wl_data = N.f64(value(wl_data, "um"))
        if self.wl_data.ndim != 1 or self.wl_data.size < 1:
            raise ValueError("wl_data must be [n_pix]")
        self.flux = np.ascontiguousarray(np.atleast_2d(N.f64(flux)))
        if self.flux.ndim != 2 or self.flux.shape[1] != self.wl_data.size:
            raise ValueError(f"flux must be [n_pix] or [n_exp][n_pix] with n_pix = "
                             f"{self.wl_data.size}, not {self.flux.shape}")
        self.velocities = N.f64(np.atleast_1d(velocities))
        if self.velocities.ndim != 1 or self.velocities.size < 1:
            raise ValueError("velocities must be [n_vel]")
        if np.any(self.velocities <= -C_KMS):
            raise ValueError("velocities must exceed -c")
        self.weights = (np.ones(self.wl_data.size) if weights is None else N.f64(weights))
        if self.weights.shape != self.wl_data.shape:
            raise ValueError(f"weights must be [{self.wl_data.size}], one value per pixel")
        self.idx, self.frac, self.n_clamped = doppler_plan(self.lam, self.wl_data,
                                                           self.velocities)
        self.a = np.ascontiguousarray(self.weights * self.flux)
        self.W = float(np.sum(self.weights))
        self.S_wf = np.sum(self.a, axis=1)
        self.S_wff = np.sum(self.a * self.flux, axis=1)
        self._serial = 0
        self._keep_on = False

    @property
    def n_lam(self):
        return self.lam.size

    @property
    def n_pix(self):
        return self.wl_data.size

    @property
    def n_vel(self):
        return self.velocities.size

    @property
    def n_exp(self):
        return self.flux.shape[0]

    # ------------------------------------------------------------------ device
    def _create(self, h):
        """frei_ccf* of the correlator (plan, data and weights uploaded once)."""
        return N.lib().frei_ccf_create(
            ctypes.byref(h), self.device, self.n_lam, self.n_pix, self.n_vel, i32ptr(self.idx),
            N.dptr(self.frac), self.n_exp, N.dptr(self.a), N.dptr(self.weights))

    def release(self):
        self._serial += 1     # whatever was kept ends with the handle
        self._keep_on = False
        super().release()

    def correlate(self, x, den=None, select=None, scale=None, offset=None, form=0, engine=None,
                  want=_SUMS, keep=False):
        """The sums of ``x`` ([n_lam] or [n_atm][n_lam]) against the data ->
        :class:`CrossCorrelation`.  The template is ``scale_m (x[m] / den[select_m]) -
        offset_m``: ``den`` an optional library ([n_lam] or [n_lib][n_lam]) with ``select``
        [n_atm] the row of each atmosphere (default row 0), ``scale`` and ``offset`` optional
        numbers per atmosphere; an absent one drops its operation.  ``x=None`` with ``engine=``
        (an Engine or BatchEngine on the whole axis) takes the emergent spectra resident in the
        engine's flux state; a :class:`~frei_amd.broaden.BroadenedSpectra` as ``x`` takes what
        ``Broadening.apply(keep=True)`` left on the device, an
        :class:`~frei_amd.modelgrid.InterpolatedSpectra` what
        ``ModelGrid.interpolate(keep=True)`` left there.  ``form`` 0 picks the kernel, a
        member of ``FORMS`` forces it (``form_used`` records the choice).  ``want`` names the
        sums to compute (``"sfg"``, ``"sg"``, ``"sgg"``; the others are None and cost
        nothing).  ``keep=True`` also leaves the computed sums on the device (the result's
        ``kept``, for :meth:`frei_amd.stack.OrbitStack.stack`, K14) until the next ``correlate``
        or ``release``; ``want=()`` is then allowed: all three sums are computed and kept and
        none is copied back."""
        want = (want,) if isinstance(want, str) else tuple(want)
        if any(k not in _SUMS for k in want):
            raise ValueError(f"want holds names other than {_SUMS}: {want}")
        kept = kept_suffix(x)
        x, ctx, brd, n_atm, single, _ = resident_or_host(
            x, engine, self.n_lam, ("a correlator", "a pixel's bracket"))
        den = library_rows(den, "den", self.n_lam)
        n_lib = 0 if den is None else den.shape[0]
        sel = select_rows(select, n_atm)
        sc, off = per_atmosphere(scale, n_atm), per_atmosphere(offset, n_atm)
        V, E = self.n_vel, self.n_exp
        out = dict(sfg=np.empty((n_atm, E, V)) if "sfg" in want else None,
                   sg=np.empty((n_atm, V)) if "sg" in want else None,
                   sgg=np.empty((n_atm, V)) if "sgg" in want else None)
        used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        tail = (N.dptr(den), n_lib, i32ptr(sel), N.dptr(sc), N.dptr(off), int(form),
                N.dptr(out["sfg"]), N.dptr(out["sg"]), N.dptr(out["sgg"]), ctypes.byref(used),
                ctypes.byref(ms))
        handle = self.handle()
        self._serial += 1                          # whatever was kept ends with this call
        if bool(keep) != self._keep_on:            # switching keep mode off frees what was kept
            N.check(N.lib().frei_ccf_keep(handle, 1 if keep else 0))
            self._keep_on = bool(keep)
        if brd is not None:
            N.check(getattr(N.lib(), "frei_ccf_apply" + kept)(handle, brd, n_atm, *tail))
        else:
            N.check(N.lib().frei_ccf_apply(handle, ctx, N.dptr(x), n_atm, *tail))
        self._record(used, ms)
        if single:
            out = {k: None if v is None else v[0] for k, v in out.items()}
        kept = KeptSums(self, self._serial, n_atm, single, want or _SUMS) if keep else None
        return CrossCorrelation(out["sfg"], out["sg"], out["sgg"], self.velocities, self.W,
                                self.S_wf, self.S_wff, self.n_pix, kept=kept)


def kp_vsys_map(values, velocities, phases, Kp, Vsys, v_obs=0.0):
    """A CCF or log-likelihood ``values`` [..., n_exp, n_vel] on ``velocities`` (ascending,
    km/s) stacked along the planet's orbit: for every (K_p, V_sys) the sum over exposures of
    ``np.interp(Vsys + Kp sin(2 pi phases[e]) + v_obs[e], velocities, values[..., e, :])`` ->
    [..., n_Kp, n_Vsys].  ``phases`` [n_exp] are orbital phases (0 at mid-transit), ``v_obs``
    a scalar or [n_exp] (for example minus the barycentric correction)."""
    values = np.asarray(values, dtype=float)
    velocities = np.asarray(velocities, dtype=float)
    phases = np.atleast_1d(np.asarray(phases, dtype=float))
    Kp = np.atleast_1d(np.asarray(Kp, dtype=float))
    Vsys = np.atleast_1d(np.asarray(Vsys, dtype=float))
    n_exp = phases.size
    if values.ndim < 2 or values.shape[-2:] != (n_exp, velocities.size):
        raise ValueError(f"values must be [..., {n_exp}, {velocities.size}], not {values.shape}")
    v_obs = np.broadcast_to(np.asarray(v_obs, dtype=float), (n_exp,))
    lead = values.shape[:-2]
    flat = values.reshape((-1, n_exp, velocities.size))
    out = np.zeros((flat.shape[0], Kp.size, Vsys.size))
    for r in range(flat.shape[0]):
        for k in range(Kp.size):
            for e in range(n_exp):
                v = Vsys + Kp[k] * np.sin(2.0 * np.pi * phases[e]) + v_obs[e]
                out[r, k] += np.interp(v, velocities, flat[r, e])
    return out.reshape(lead + (Kp.size, Vsys.size))


def cross_correlate(cc, kind, planets, lam, x=None, engine=None, R_p=None, R_star=None,
                    offset=None, broadening=None, **kw):
    """The templates of ``kind`` ("flux", "eclipse" or "transit") of ``x`` (or of ``engine``'s
    resident spectra) for atmospheres whose stars are ``planets``', through ``cc``.  With
    ``broadening`` (a :class:`~frei_amd.broaden.Broadening`, K13) the spectrum — for "transit"
    minus the depth — is broadened first and stays on the device; the pre-pass follows."""
    if kind == "transit":     # minus the depth, before any broadening
        x = -np.asarray(getattr(x, "value", x), dtype=float)
    x, engine, star = broadened_source(kind, planets, lam, x, engine, R_p, R_star, broadening)
    if kind == "transit":
        return cc.correlate(x, offset=offset, **kw)
    if kind in ("flux", "eclipse"):
        return cc.correlate(x, offset=offset, engine=engine, **star, **kw)
    raise unknown_kind(kind)
