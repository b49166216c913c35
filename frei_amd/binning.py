"""Opacity binning on the GPU (frei/opacity.py:66-170 ``binned_opacity``; frei/interp.py
``groupby_bins_agg``; opacity.py:33-42 ``mapfunc_exact``).

A :class:`CrossSection` is one species' high-resolution cross-section in the layout the
reference's ``opacity_dir_to_netcdf`` writes (opacity.py:395-483): float32
``opacity[temperature][pressure][wavelength]`` with wavelengths in µm ascending.  It is
uploaded once per device and stays in HBM; K6 (``frei_amd/csrc/frei_binning.hip``) bins
it onto a Grid's wavelength bins and selects the nearest source (T, p) node for every
grid node.  ``binned_opacity`` returns :class:`BinnedTable` objects: the Engine bins them
straight into its device tables (no host round trip); ``.values`` materialises the
(pressure, temperature, wavelength) array on the host when asked.  K18
(``frei_amd/csrc/frei_kdist.hip``) gives a second road from the same resident values:
``CrossSection.mix`` premixes species, ``CrossSection.kdist`` and :class:`KTable` sort every bin
into a k-distribution (``frei_amd.kdist`` holds the grid that runs on it).
"""
import ctypes
import glob
import os

import numpy as np

from . import _native as N
from .chemistry import iso_to_species
from .units import value

__all__ = ["CrossSection", "BinnedTable", "KTable", "binned_opacity", "open_cross_section",
           "GROUPIES", "EXACT"]

GROUPIES, EXACT = 0, 1


class CrossSection:
    """High-resolution cross-section of one species (the reference's netCDF Dataset)."""

    def __init__(self, opacity, temperature, pressure, wavelength, isotopologue=None):
        self.opacity = np.ascontiguousarray(opacity, dtype=np.float32)
        self.temperature = np.ascontiguousarray(value(temperature, "K"), dtype=np.float64)
        self.pressure = np.ascontiguousarray(value(pressure, "bar"), dtype=np.float64)
        self.wavelength = np.ascontiguousarray(value(wavelength, "um"), dtype=np.float64)
        self.isotopologue = isotopologue
        self._synthetic = None
        self._lines = None
        if self.opacity.shape != (self.temperature.size, self.pressure.size,
                                  self.wavelength.size):
            raise ValueError("opacity must be (temperature, pressure, wavelength)")
        self._handles = {}

    @classmethod
    def synthetic(cls, temperature, pressure, wavelength, seed=0, isotopologue=None):
        """Device-generated line forest (benchmarks): no host copy of the values."""
        obj = cls.__new__(cls)
        obj.temperature = np.ascontiguousarray(temperature, dtype=np.float64)
        obj.pressure = np.ascontiguousarray(pressure, dtype=np.float64)
        obj.wavelength = np.ascontiguousarray(wavelength, dtype=np.float64)
        obj.opacity = None
        obj.isotopologue = isotopologue
        obj._synthetic = int(seed)
        obj._lines = None
        obj._handles = {}
        return obj

    @classmethod
    def _from_lines(cls, make, temperature, pressure, wavelength, isotopologue=None):
        """Computed on the device from a line list (``LineList.cross_section``): ``make(device)``
        returns the frei_xsec*; no host copy of the values."""
        obj = cls.synthetic(temperature, pressure, wavelength, isotopologue=isotopologue)
        obj._synthetic = None
        obj._lines = make
        return obj

    @classmethod
    def mix(cls, sources, weights, isotopologue="mix", device=0):
        """The premixed cross-section ``sum_s weights[s] * sources[s]`` of CrossSections on
        shared nodes and one axis, computed on ``device`` (frei_xsec_mix, K18).  ``weights``
        (mass mixing ratios at the sources' own nodes) broadcasts to (n_src, n_T, n_p).  A
        k-distribution needs the mixture: the k(g) of several species do not add.  The result
        holds no host copy (``.opacity`` is None); ``.values()`` downloads it."""
        sources = list(sources)
        if not sources:
            raise ValueError("CrossSection.mix needs at least one source")
        s0 = sources[0]
        w = N.f64(np.broadcast_to(np.asarray(weights, dtype=float),
                                  (len(sources), s0.temperature.size, s0.pressure.size)))
        timing = {}

        def make(dev):
            h, ms = ctypes.c_void_p(), ctypes.c_double(0.0)
            src = (ctypes.c_void_p * len(sources))(*[x.handle(dev).value for x in sources])
            N.check(N.lib().frei_xsec_mix(ctypes.byref(h), len(sources), src, N.dptr(w),
                                          ctypes.byref(ms)))
            timing[dev] = ms.value
            return h

        xs = cls._from_lines(make, s0.temperature, s0.pressure, s0.wavelength, isotopologue)
        xs.handle(device)
        xs.kernel_ms = timing[device]     # HIP-event time of the kernel
        return xs

    def handle(self, device=0):
        """frei_xsec* of this cross-section on ``device`` (uploaded once)."""
        h = self._handles.get(device)
        if h is None:
            lib = N.lib()
            h = ctypes.c_void_p()
            nT, npr, nhi = self.temperature.size, self.pressure.size, self.wavelength.size
            if self._lines is not None:
                h = self._lines(device)
            elif self._synthetic is not None:
                N.check(lib.frei_xsec_create_synthetic(
                    ctypes.byref(h), device, nT, npr, nhi, N.dptr(self.temperature),
                    N.dptr(self.pressure), N.dptr(self.wavelength), self._synthetic))
            else:
                N.check(lib.frei_xsec_create(
                    ctypes.byref(h), device, N.fptr(self.opacity), nT, npr, nhi,
                    N.dptr(self.temperature), N.dptr(self.pressure), N.dptr(self.wavelength)))
            self._handles[device] = h
        return h

    def release(self):
        for h in self._handles.values():
            N.lib().frei_xsec_destroy(h)
        self._handles = {}

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def bin(self, wl_bins, lam, temperatures, pressures, groupies=True, device=0, out=True):
        """Binned (pressure, temperature, λ) table on the host (``out=False``: leave it on
        the device, for timing)."""
        wl_bins = N.f64(value(wl_bins, "um"))
        lam = N.f64(value(lam, "um"))
        T = N.f64(value(temperatures, "K"))
        p = N.f64(value(pressures, "bar"))
        if wl_bins.size != lam.size + 1:
            raise ValueError("wl_bins must have one more edge than lam has points")
        res = np.empty((p.size, T.size, lam.size)) if out else None
        N.check(N.lib().frei_xsec_bin(self.handle(device), GROUPIES if groupies else EXACT,
                                      N.dptr(wl_bins), N.dptr(lam), lam.size, N.dptr(T), T.size,
                                      N.dptr(p), p.size, N.dptr(res)))
        return res

    def kdist(self, wl_bins, g, temperatures, pressures, device=0, out=True):
        """The k-distribution (frei_xsec_kdist, K18; the definition is in include/frei_hip.h):
        per bin of ``wl_bins`` (µm) the values sorted ascending and sampled at the quadrature
        points ``g`` (each in (0, 1)) -> (k[pressure][temperature][bin][g], counts[bin]), the
        points per bin (``out=False``: k stays on the device, for timing, and is None)."""
        wl_bins = N.f64(value(wl_bins, "um"))
        g = N.f64(np.atleast_1d(g))
        T = N.f64(np.atleast_1d(value(temperatures, "K")))
        p = N.f64(np.atleast_1d(value(pressures, "bar")))
        n_bins = wl_bins.size - 1
        res = np.empty((p.size, T.size, n_bins, g.size)) if out else None
        counts = np.zeros(max(n_bins, 0), dtype=np.int64)
        N.check(N.lib().frei_xsec_kdist(
            self.handle(device), N.dptr(wl_bins), n_bins, g.size, N.dptr(g), N.dptr(T), T.size,
            N.dptr(p), p.size, N.dptr(res),
            counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return res, counts

    def values(self, t=None, p=None, device=0):
        """The resident float32 values read back from ``device`` (frei_xsec_values): the whole
        (temperature, pressure, wavelength) table, the (pressure, wavelength) rows of
        temperature node ``t``, the (temperature, wavelength) rows of pressure node ``p``, or
        the one row of node (t, p)."""
        h = self.handle(device)
        ts = range(self.temperature.size) if t is None else [int(t)]
        ps = range(self.pressure.size) if p is None else [int(p)]
        out = np.empty((len(ts), len(ps), self.wavelength.size), dtype=np.float32)
        for a, kt in enumerate(ts):
            for b, kp in enumerate(ps):
                N.check(N.lib().frei_xsec_values(h, kt, kp, 0, self.wavelength.size,
                                                 N.fptr(out[a, b])))
        if t is not None:
            out = out[0]
        if p is not None:
            out = out[..., 0, :]
        return out

    def timing(self, on, device=0):
        ms, n = ctypes.c_double(0), ctypes.c_int(0)
        N.check(N.lib().frei_xsec_timing(self.handle(device), int(on), ctypes.byref(ms),
                                         ctypes.byref(n)))
        return ms.value, n.value


class BinnedTable:
    """A species' opacity binned onto a grid: nodes ``pressure`` (bar) x ``temperature``
    (K), wavelengths ``wavelength`` (µm).  The Engine bins it directly into HBM."""

    dims = ("pressure", "temperature", "wavelength")

    def __init__(self, xsec, wl_bins, lam, temperatures, pressures, groupies=True, device=0):
        self.xsec = xsec
        self.wl_bins = N.f64(value(wl_bins, "um"))
        self.wavelength = N.f64(value(lam, "um"))
        self.temperature = N.f64(value(temperatures, "K"))
        self.pressure = N.f64(value(pressures, "bar"))
        self.groupies = bool(groupies)
        self.device = device
        self._values = None

    @property
    def mode(self):
        return GROUPIES if self.groupies else EXACT

    @property
    def shape(self):
        return (self.pressure.size, self.temperature.size, self.wavelength.size)

    @property
    def values(self):
        if self._values is None:
            self._values = self.xsec.bin(self.wl_bins, self.wavelength, self.temperature,
                                         self.pressure, self.groupies, self.device)
        return self._values


class KTable:
    """A cross-section's k-distribution on a grid's bins (K18): nodes ``pressure`` (bar) x
    ``temperature`` (K), and per bin of ``wl_bins`` (µm) one column per quadrature point of
    ``g``, column ``b * n_g + q`` for bin b at g_q; ``wavelength`` repeats each bin's centre
    n_g times.  The Engine writes it directly into HBM (frei_set_table_kdist)."""

    dims = ("pressure", "temperature", "wavelength")

    def __init__(self, xsec, wl_bins, g, temperatures, pressures, device=0):
        self.xsec = xsec
        self.wl_bins = N.f64(value(wl_bins, "um"))
        self.g = N.f64(np.atleast_1d(g))
        self.temperature = N.f64(np.atleast_1d(value(temperatures, "K")))
        self.pressure = N.f64(np.atleast_1d(value(pressures, "bar")))
        self.wavelength = np.repeat((self.wl_bins[:-1] + self.wl_bins[1:]) / 2, self.g.size)
        self.device = device
        self._values = None
        self._counts = None

    @property
    def n_bins(self):
        return self.wl_bins.size - 1

    @property
    def shape(self):
        return (self.pressure.size, self.temperature.size, self.wavelength.size)

    @property
    def values(self):
        """(pressure, temperature, n_bins * n_g) on the host."""
        if self._values is None:
            v, _ = self.xsec.kdist(self.wl_bins, self.g, self.temperature, self.pressure,
                                   self.device)
            self._values = v.reshape(self.shape)
        return self._values

    @property
    def counts(self):
        """Points of the cross-section's axis per bin (host arithmetic on the axis alone;
        ``CrossSection.kdist`` returns the device call's own)."""
        if self._counts is None:
            self._counts = bin_counts(self.xsec.wavelength, self.wl_bins)
        return self._counts


def bin_counts(wavelength, wl_bins):
    """Points per bin under K6's membership (pandas.cut right-closed on the cropped axis): bin k
    holds ``wl_bins[k] < wl <= wl_bins[k + 1]``, the last bin ``wl < wl_bins[-1]``."""
    wl, b = np.asarray(wavelength, dtype=float), np.asarray(wl_bins, dtype=float)
    start = np.searchsorted(wl, b[:-1], side="right")
    end = np.searchsorted(wl, b[1:], side="right")
    end[-1] = np.searchsorted(wl, b[-1], side="left")
    return np.maximum(end - start, 0).astype(np.int64)


def open_cross_section(path):
    """Read one species file: ``.npz`` (arrays opacity/temperature/pressure/wavelength) or a
    classic netCDF3 file with the opacity_dir_to_netcdf variables (scipy.io).  HDF5-based
    netCDF4 (the reference's zlib output) needs a reader this image lacks: convert it to
    .npz elsewhere."""
    iso = os.path.basename(path).split("_")[0]
    if path.endswith(".npz"):
        d = np.load(path, allow_pickle=False)
        return CrossSection(d["opacity"], d["temperature"], d["pressure"], d["wavelength"], iso)
    with open(path, "rb") as f:
        magic = f.read(4)
    if magic[:3] != b"CDF":
        raise ValueError(f"{path}: not a netCDF3 file (netCDF4/HDF5 cannot be read here; "
                         "convert to .npz with arrays opacity/temperature/pressure/wavelength)")
    from scipy.io import netcdf_file
    with netcdf_file(path, "r", mmap=False) as nc:
        v = nc.variables
        return CrossSection(np.array(v["opacity"][:]), np.array(v["temperature"][:]),
                            np.array(v["pressure"][:]), np.array(v["wavelength"][:]), iso)


def binned_opacity(temperatures, pressures, wl_bins, lam, groupies=True, species=None,
                   path=None, cross_sections=None, device=0):
    """Opacity for all available species binned to ``lam`` (opacity.py:66-170).

    ``cross_sections`` ({isotopologue: CrossSection}) replaces reading files from ``path``
    (default ``~/.frei/*.nc``, then ``*.npz``).  ``species`` filters by species name
    (``iso_to_species``, chemistry.py:13-21).  Returns {isotopologue: BinnedTable}."""
    if cross_sections is None:
        if path is None:
            path = os.path.join(os.path.expanduser("~"), ".frei", "*.nc")
        paths = sorted(glob.glob(path))
        if not paths and path.endswith(".nc"):
            paths = sorted(glob.glob(path[:-3] + ".npz"))
        cross_sections = {}
        for pth in paths:
            iso = os.path.basename(pth).split("_")[0]
            if species is None or iso_to_species(iso) in species:
                cross_sections[iso] = open_cross_section(pth)
    elif species is not None:
        cross_sections = {k: v for k, v in cross_sections.items()
                          if iso_to_species(k) in species}
    if not cross_sections:
        raise FileNotFoundError(f"no opacity cross-sections found at {path!r}")
    return {iso: BinnedTable(x, wl_bins, lam, temperatures, pressures, groupies, device)
            for iso, x in cross_sections.items()}
