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
into a k-distribution (``frei_amd.kdist`` holds the grid that runs on it).  K19
(``frei_amd/csrc/frei_kmix.hip``) mixes species from their k-tables alone: a :class:`KLibrary`
keeps the tables resident and folds them by random overlap into a :class:`MixedKTable`.
"""
import ctypes
import glob
import os

import numpy as np

from . import _native as N
from .chemistry import iso_to_species
from .units import value

__all__ = ["CrossSection", "BinnedTable", "KTable", "KLibrary", "MixedKTable", "MixedKTables",
           "binned_opacity",
           "open_cross_section", "fixed_point_weights", "GROUPIES", "EXACT"]

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


def fixed_point_weights(weights):
    """K19's fixed-point quadrature weights ``W_q = rint(w_q 2^30)`` (uint64; the definition is in
    include/frei_hip.h): every w_q finite and positive, every W_q >= 1 and sum(W) <= 2^31."""
    w = np.asarray(weights, dtype=float)
    W, total = [], 0
    for q, wq in enumerate(w):
        if not np.isfinite(wq) or not wq > 0.0 or wq > 2.0:
            raise ValueError(f"weights[{q}] = {wq} must be finite and positive, and the weights "
                             "sum to at most 2")
        W.append(int(np.rint(wq * 2.0 ** 30)))
        if W[-1] < 1:
            raise ValueError(f"weights[{q}] = {wq} is below the fixed-point step 2^-30")
        total += W[-1]
        if total > 2 ** 31:
            raise ValueError(f"the weights up to weights[{q}] sum to more than 2")
    return np.array(W, dtype=np.uint64)


class KLibrary:
    """Several species' k-tables on shared nodes, bins and one quadrature, resident on
    ``device`` (frei_klib, K19).  ``tables`` is ``{name: CrossSection | array[n_p][n_T][n_bins]
    [n_g]}``: a CrossSection is sorted on the device straight into its slot (K18's
    k-distribution at the library's nodes, bins and ``g``), an array is uploaded.  ``wl_bins``
    (µm) are the bin edges, ``g`` (strictly ascending in (0, 1)) and ``weights`` the quadrature,
    ``temperatures`` (K) x ``pressures`` (bar) the nodes.  :meth:`mix` folds the species by
    random overlap with resort-and-rebin (the definition is in include/frei_hip.h) for any
    number of compositions; :meth:`table` gives the :class:`MixedKTable` an Engine takes.
    Nothing touches the device before the first mix."""

    def __init__(self, tables, wl_bins, g, weights, temperatures, pressures, device=0):
        if not tables:
            raise ValueError("KLibrary needs tables={name: CrossSection or array}")
        self.names = list(tables)
        self.wl_bins = N.f64(value(wl_bins, "um"))
        self.g = N.f64(np.atleast_1d(g))
        self.weights = N.f64(np.atleast_1d(weights))
        self.temperature = N.f64(np.atleast_1d(value(temperatures, "K")))
        self.pressure = N.f64(np.atleast_1d(value(pressures, "bar")))
        if self.wl_bins.ndim != 1 or self.wl_bins.size < 2 or np.any(np.diff(self.wl_bins) <= 0):
            raise ValueError("wl_bins must be strictly ascending bin edges of at least 1 bin")
        if self.g.ndim != 1 or self.g.shape != self.weights.shape:
            raise ValueError("g and weights must be 1-D arrays of one length")
        if not 1 <= self.g.size <= 64:
            raise ValueError(f"n_g = {self.g.size} lies outside [1, 64]")
        for q, gq in enumerate(self.g):
            if not (np.isfinite(gq) and 0.0 < gq < 1.0) or (q and not gq > self.g[q - 1]):
                raise ValueError(f"g[{q}] = {gq} must be finite, in (0, 1) and above the g "
                                 "before it")
        self.fixed_weights = fixed_point_weights(self.weights)
        if self.temperature.ndim != 1 or self.pressure.ndim != 1:
            raise ValueError("temperatures and pressures must be 1-D")
        self.n_bins, self.n_g = self.wl_bins.size - 1, self.g.size
        self.shape = (self.pressure.size, self.temperature.size, self.n_bins, self.n_g)
        self.sources = {}     # {name: array or CrossSection} (tables(x) is the K20 method)
        for name, t in tables.items():
            if not isinstance(t, CrossSection):
                t = N.f64(t)
                if t.shape != self.shape:
                    raise ValueError(f"table {name!r} has shape {t.shape}, not (n_p, n_T, n_bins, "
                                     f"n_g) = {self.shape}")
            self.sources[name] = t
        self.wavelength = np.repeat((self.wl_bins[:-1] + self.wl_bins[1:]) / 2, self.n_g)
        self.device = device
        self.kernel_ms = None
        self._handle = None

    @property
    def n_src(self):
        return len(self.names)

    @property
    def resident_bytes(self):
        """Bytes of the species' tables in HBM."""
        return 8 * self.n_src * int(np.prod(self.shape))

    def handle(self):
        """frei_klib* on the library's device (created and filled once)."""
        if self._handle is None:
            lib, h = N.lib(), ctypes.c_void_p()
            N.check(lib.frei_klib_create(
                ctypes.byref(h), self.device, self.n_src, self.pressure.size,
                self.temperature.size, self.n_bins, self.n_g, N.dptr(self.wl_bins), N.dptr(self.g),
                N.dptr(self.weights), N.dptr(self.pressure), N.dptr(self.temperature)))
            self._handle = h
            for s, t in enumerate(self.sources.values()):
                if isinstance(t, CrossSection):
                    N.check(lib.frei_klib_set_kdist(h, s, t.handle(self.device)))
                else:
                    N.check(lib.frei_klib_set(h, s, N.dptr(t)))
        return self._handle

    def release(self):
        if self._handle is not None:
            N.lib().frei_klib_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def composition(self, x):
        """``x`` — mass mixing ratios at the nodes, (n_src, n_T, n_p) or (n_comp, n_src, n_T,
        n_p), broadcast as ``CrossSection.mix`` broadcasts its weights — checked (finite, >= 0)
        and transposed to the C layout [n_comp][n_src][n_p][n_T] -> (array, batched)."""
        x = np.asarray(x, dtype=float)
        one = (self.n_src, self.temperature.size, self.pressure.size)
        batched = x.ndim == 4
        if x.ndim > 4:
            raise ValueError(f"x has {x.ndim} axes: (n_src, n_T, n_p) or (n_comp, n_src, n_T, n_p)")
        try:
            x = np.broadcast_to(x, ((x.shape[0],) if batched else (1,)) + one)
        except ValueError:
            raise ValueError(f"x of shape {x.shape} does not broadcast to (n_src, n_T, n_p) = "
                             f"{one}") from None
        if x.shape[0] < 1:
            raise ValueError("x holds no composition")
        bad = np.argwhere(~(np.isfinite(x) & (x >= 0)))
        if bad.size:
            c, s, t, p = bad[0]
            raise ValueError(f"x[{c}][{s}][{t}][{p}] = {x[c, s, t, p]} (composition, species "
                             f"{self.names[s]!r}, T node, p node) must be finite and >= 0")
        return N.f64(x.transpose(0, 1, 3, 2)), batched

    def mix(self, x, form=0, out=True):
        """The mixture's k-table(s) on the host: (n_p, n_T, n_bins, n_g), or (n_comp, ...) for a
        batch of compositions (``out=False``: they stay on the device, for timing, and None is
        returned).  ``form``: 0 automatic (the wave form for n_g <= 2, the block form above),
        1 the wave form (n_g <= 8), 2 the block form; the same bits.
        ``kernel_ms`` receives the HIP-event time of the kernel."""
        xc, batched = self.composition(x)
        res = np.empty((xc.shape[0],) + self.shape) if out else None
        ms = ctypes.c_double(0.0)
        N.check(N.lib().frei_klib_mix(self.handle(), xc.shape[0], N.dptr(xc), N.dptr(res),
                                      int(form), ctypes.byref(ms)))
        self.kernel_ms = ms.value
        if res is None or batched:
            return res
        return res[0]

    def table(self, x):
        """One composition's mixture as the table an Engine takes (no host round trip)."""
        return MixedKTable(self, x)

    def tables(self, x):
        """A batch of compositions (n_comp, n_src, n_T, n_p) as the per-atmosphere tables a
        BatchEngine takes (K20; no host round trip)."""
        return MixedKTables(self, x)


class MixedKTables:
    """``n_comp`` compositions of a :class:`KLibrary`, one per atmosphere of a batch (K20): the
    batched counterpart of :class:`MixedKTable`.  A BatchEngine has the device mix each
    atmosphere's table straight into HBM (frei_set_table_kmix_batch); ``x`` is kept in the C
    layout [n_comp][n_src][n_p][n_T]."""

    dims = ("pressure", "temperature", "wavelength")

    def __init__(self, library, x):
        self.library = library
        x = np.asarray(x, dtype=float)
        if x.ndim != 4:
            raise ValueError(f"x of shape {x.shape} is not a batch of compositions: "
                             "(n_comp, n_src, n_T, n_p)")
        self.x, _ = library.composition(x)
        self.pressure = library.pressure
        self.temperature = library.temperature
        self.wavelength = library.wavelength
        self.wl_bins, self.g = library.wl_bins, library.g
        self.device = library.device

    @property
    def n_comp(self):
        return self.x.shape[0]

    @property
    def n_bins(self):
        return self.library.n_bins

    def __getitem__(self, m):
        """Composition ``m`` as a :class:`MixedKTable`."""
        return MixedKTable(self.library, self.x[m].transpose(0, 2, 1))


class MixedKTable:
    """One composition of a :class:`KLibrary` mixed by random overlap (K19): nodes ``pressure``
    (bar) x ``temperature`` (K), columns as a :class:`KTable`'s.  The Engine has the device mix
    it directly into HBM (frei_set_table_kmix); ``values`` materialises it on the host."""

    dims = ("pressure", "temperature", "wavelength")

    def __init__(self, library, x):
        self.library = library
        xc, batched = library.composition(x)
        if batched:
            raise ValueError("a MixedKTable holds one composition: x is (n_src, n_T, n_p)")
        self.x = xc[0]                      # [n_src][n_p][n_T], the C layout
        self.pressure = library.pressure
        self.temperature = library.temperature
        self.wavelength = library.wavelength
        self.wl_bins, self.g = library.wl_bins, library.g
        self.device = library.device
        self._values = None

    @property
    def n_bins(self):
        return self.library.n_bins

    @property
    def shape(self):
        return (self.pressure.size, self.temperature.size, self.wavelength.size)

    @property
    def values(self):
        """(pressure, temperature, n_bins * n_g) on the host."""
        if self._values is None:
            self._values = self.library.mix(self.x.transpose(0, 2, 1)).reshape(self.shape)
        return self._values


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
