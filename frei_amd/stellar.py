"""Stellar model spectra binned on the GPU (frei/phoenix.py ``get_binned_phoenix_spectrum``).

A :class:`StellarSpectra` is a library of high-resolution spectra on one shared wavelength
axis (PHOENIX models share theirs), uploaded once and kept in HBM as float64
``flux[n_spec][n_hi]``.  K8 (``frei_amd/csrc/frei_stellar.hip``) bins all of them onto a
grid's wavelength bins in one launch: per bin the trapezoid integral over its points divided
by their span (phoenix.py:13-17), bins right-closed as ``pandas.cut`` makes them.

``.bin`` returns the result aligned with the bins (NaN where a bin holds fewer than two
points), which is what ``Planet(stellar_spectrum=...)`` takes.  ``binned_stellar_spectrum`` is
the reference's own output: the non-empty bins' values in bin order, zero-padded to
``len(lam)`` (phoenix.py:47-51), so a grid that starts below the spectrum shifts the result as
the reference does.  Nothing here reads files or the network: the spectrum comes from the
caller (``spectrum=``) or from ``expecto`` when that package is installed.
"""
import ctypes

import numpy as np

from . import _native as N
from ._device import DeviceObject
from .units import unit_of, value, with_unit

__all__ = ["StellarSpectra", "binned_stellar_spectrum", "get_binned_phoenix_spectrum"]

FLUX = "erg / (s cm3)"


class StellarSpectra(DeviceObject):
    """High-resolution spectra ``flux`` ([n_hi] or [n_spec][n_hi], erg s^-1 cm^-3) on
    ``wavelength`` ([n_hi], µm, strictly ascending), resident on ``device``."""

    _destroy = "frei_sspec_destroy"

    def __init__(self, wavelength, flux, device=0):
        super().__init__(device)
        self.wavelength = N.f64(value(wavelength, "um"))
        f = N.f64(value(flux, FLUX))
        if f.ndim not in (1, 2):
            raise ValueError("flux must be [n_hi] or [n_spec][n_hi]")
        self.single = f.ndim == 1
        self.flux = np.ascontiguousarray(np.atleast_2d(f))
        if self.wavelength.ndim != 1 or self.flux.shape[1] != self.wavelength.size:
            raise ValueError("flux must have one value per wavelength along its last axis")

    @property
    def n_spec(self):
        return self.flux.shape[0]

    def _create(self, h):
        """frei_sspec* of the library (uploaded once)."""
        return N.lib().frei_sspec_create(ctypes.byref(h), self.device, N.dptr(self.flux),
                                         self.flux.shape[0], self.flux.shape[1],
                                         N.dptr(self.wavelength))

    def bin(self, wl_bins, form=0, counts=False, out=True):
        """Every spectrum binned onto ``wl_bins`` (n_bins + 1 edges, µm), aligned with the
        bins: [n_bins] for a 1-D library, else [n_spec][n_bins]; NaN where a bin holds fewer
        than two points.  ``form`` 0 picks the kernel from the points per bin, 1 forces one
        lane per bin, 2 one wave per bin (``form_used`` records the choice).  ``counts=True``
        also returns the points per bin; ``out=False`` leaves the result on the device
        (timing) and returns None in its place."""
        wl_bins = N.f64(value(wl_bins, "um"))
        if wl_bins.ndim != 1 or wl_bins.size < 2:
            raise ValueError("wl_bins must hold at least two edges")
        nb = wl_bins.size - 1
        res = np.empty((self.n_spec, nb)) if out else None
        cnt = np.empty(nb, dtype=np.int64)
        used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        N.check(N.lib().frei_sspec_bin(
            self.handle(), N.dptr(wl_bins), nb, int(form), N.dptr(res),
            cnt.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(used),
            ctypes.byref(ms)))
        self._record(used, ms)
        if res is not None and self.single:
            res = res[0]
        return (res, cnt) if counts else res


def binned_stellar_spectrum(wavelength, flux, wl_bins, lam, device=0):
    """phoenix.py:43-52 for a spectrum ``flux`` on ``wavelength``: the values of the non-empty
    bins of ``wl_bins`` in bin order, zero-padded at the end to ``len(lam)``.  A Quantity when
    ``flux`` is one."""
    lib = StellarSpectra(wavelength, flux, device=device)
    try:
        aligned, counts = lib.bin(wl_bins, counts=True)
    finally:
        lib.release()
    keep = counts > 0          # groupby_bins drops empty groups (O(n_bins) on the host)
    if not keep.any():
        raise ValueError("no point of the spectrum falls in any wavelength bin")
    n_lam = len(value(lam, "um"))
    vals = aligned[..., keep]
    if vals.shape[-1] > n_lam:
        raise ValueError("index can't contain negative values")    # np.pad's own refusal
    pad = [(0, 0)] * (vals.ndim - 1) + [(0, n_lam - vals.shape[-1])]
    return with_unit(np.pad(vals, pad), unit_of(FLUX, flux))


def get_binned_phoenix_spectrum(T_eff, g, wl_bins, lam, cache=True, spectrum=None):
    """Binned PHOENIX spectrum of effective temperature ``T_eff`` and surface gravity ``g``
    (phoenix.py:20-52).  ``spectrum`` is the model itself, an object with ``.wavelength`` and
    ``.flux`` (what ``expecto.get_spectrum`` returns); without it ``expecto`` is imported and
    asked for the model, as the reference does.  This package downloads nothing itself."""
    if spectrum is None:
        try:
            from expecto import get_spectrum
        except ImportError as e:
            raise ImportError("get_binned_phoenix_spectrum needs the expecto package to fetch "
                              "the PHOENIX model; pass the model as spectrum= (an object with "
                              ".wavelength and .flux) instead") from e
        spectrum = get_spectrum(float(value(T_eff, "K")),
                                log_g=float(np.log10(value(g, "cm / s2"))), cache=cache)
    return binned_stellar_spectrum(spectrum.wavelength, spectrum.flux, wl_bins, lam)
