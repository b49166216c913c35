"""What the device-side objects share (StellarSpectra, Instrument, CrossCorrelator, Broadening,
OrbitStack, ModelGrid, PhaseCurve):
the handle's lifecycle and the kernel timing (:class:`DeviceObject`), the choice between spectra
resident on the device and a host array (:func:`resident_or_host`), and the argument checks of
the calls that take a library, a ``select`` and numbers per atmosphere.  A new post-processing
call starts from here and from ``csrc/frei_host.h``.
"""
import ctypes

import numpy as np

from . import _native as N


class DeviceObject:
    """A handle of the native library created on first use.  Subclasses give ``_create(h)``
    (the library's create call filling ``h``; its status is returned) and ``_destroy`` (the
    name of the library's destroy function)."""

    _destroy = None

    def __init__(self, device):
        self.device = device
        self.form_used = None
        self._handle = None
        self._ms = 0.0
        self._calls = 0

    def handle(self):
        """The native handle (its data uploaded once)."""
        if self._handle is None:
            h = ctypes.c_void_p()
            N.check(self._create(h))
            self._handle = h
        return self._handle

    def release(self):
        if self._handle is not None:
            getattr(N.lib(), self._destroy)(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def timing(self, reset=False):
        """(milliseconds, calls) of the kernels since the last reset (HIP events around the
        kernels only: uploads and read-back excluded)."""
        ms, n = self._ms, self._calls
        if reset:
            self._ms, self._calls = 0.0, 0
        return ms, n

    def _record(self, used, ms):
        """After a call: the form it took and its kernel time (the ctypes values it filled)."""
        self.form_used = used.value
        self._ms += ms.value
        self._calls += 1


def kept_suffix(x):
    """The suffix of the C entry points that read ``x`` where it lies on the device: ``"_brd"``
    for a :class:`~frei_amd.broaden.BroadenedSpectra`, ``"_itp"`` for an
    :class:`~frei_amd.modelgrid.InterpolatedSpectra`, ``"_phs"`` for a
    :class:`~frei_amd.phasecurve.PhaseSpectra`; None for anything else."""
    return getattr(x, "suffix", None) if hasattr(x, "owner") and hasattr(x, "serial") else None


def resident_or_host(x, engine, n_lam, consumer):
    """Where a call's spectra come from -> ``(x2d, ctx, kept, n_atm, single, unit)``, one of the
    first three set: spectra kept on the device as ``x`` — a
    :class:`~frei_amd.broaden.BroadenedSpectra`, an
    :class:`~frei_amd.modelgrid.InterpolatedSpectra` or a
    :class:`~frei_amd.phasecurve.PhaseSpectra`, told apart by :func:`kept_suffix` — (their
    owner's handle, after the staleness check), ``x=None`` with ``engine=`` (the engine's
    context), or a host array [n_lam] or [n_atm][n_lam] (a Quantity's numbers as they are, its
    unit in ``unit``).  ``consumer`` is ``(noun with its article, what may straddle slices)``."""
    if hasattr(x, "owner") and hasattr(x, "serial"):
        return None, None, x.handle(), x.n_atm, x.single, None
    if x is None:
        if engine is None:
            raise ValueError("pass x, or engine= for its resident spectra")
        if engine.n_lam != engine.lam_um.size:
            raise ValueError(f"a wavelength-slice engine cannot feed {consumer[0]}: "
                             f"{consumer[1]} may straddle slices")
        return (None, engine._ctx, None, getattr(engine, "n_atm", 1),
                not hasattr(engine, "n_atm"), None)
    unit = getattr(x, "unit", None)
    x = N.f64(getattr(x, "value", x))
    if x.ndim not in (1, 2) or x.shape[-1] != n_lam:
        raise ValueError(f"x must be [n_lam] or [n_atm][n_lam] with n_lam = {n_lam}, "
                         f"not {x.shape}")
    x2d = np.ascontiguousarray(np.atleast_2d(x))
    return x2d, None, None, x2d.shape[0], x.ndim == 1, unit


def library_rows(a, name, n_lam):
    """A library ``a`` ([n_lam] or [n_lib][n_lam]; None stays None) as [n_lib][n_lam]."""
    if a is None:
        return None
    a = np.ascontiguousarray(np.atleast_2d(N.f64(getattr(a, "value", a))))
    if a.ndim != 2 or a.shape[1] != n_lam:
        raise ValueError(f"{name} must be [n_lam] or [n_lib][n_lam] with n_lam = "
                         f"{n_lam}, not {a.shape}")
    return a


def select_rows(select, n_atm):
    """``select`` as int32 [n_atm] (None stays None)."""
    if select is None:
        return None
    sel = np.ascontiguousarray(select, dtype=np.int32)
    if sel.shape != (n_atm,):
        raise ValueError(f"select must have {n_atm} entries")
    return sel


def per_atmosphere(v, n_atm):
    """A number per atmosphere (a scalar is repeated; None stays None) as float64 [n_atm]."""
    if v is None:
        return None
    return N.f64(np.broadcast_to(np.asarray(v, dtype=float), (n_atm,)))


def i32ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


KINDS = ("flux", "eclipse", "transit")


def unknown_kind(kind):
    return ValueError(f"unknown kind {kind!r}: 'flux', 'eclipse' or 'transit'")


def broadened_source(kind, planets, lam, x, engine, R_p, R_star, broadening):
    """The opening of ``observe()`` and ``cross_correlate()`` -> ``(x, engine, star)``: with
    ``broadening`` (a :class:`~frei_amd.broaden.Broadening`, K13) the spectrum is broadened first
    and stays on the device; ``star`` holds ``den``, ``select`` and ``scale`` of the stars for
    "eclipse" and is empty otherwise.  The eclipse scale's errors come before any device work."""
    from .observe import eclipse_scale, star_library
    if broadening is not None and kind not in KINDS:
        raise unknown_kind(kind)
    star = {}
    if kind == "eclipse":
        star["scale"] = eclipse_scale(planets, R_p, R_star)
    if broadening is not None:
        x, engine = broadening.apply(x, engine=engine, keep=True), None
    if kind == "eclipse":
        star["den"], star["select"] = star_library(planets, lam)
    return x, engine, star
