"""Phase curves on the GPU (K16, ``frei_amd/csrc/frei_phase.hip``): the columns of a batched run
seen as the cells of a tidally locked planet's surface and integrated over the visible disk at
every orbital phase.

A :class:`PhaseCurve` holds the geometry — per phase ``p`` and cell ``c`` the cosine ``mu[p][c]``
of the angle between the cell's normal and the observer, and the weight ``coef[p][c]`` (solid
angle times ``mu``) — and forms

    out[p][j] = sum over the cells with mu[p][c] > 0, ascending, of coef[p][c] I_pc[j]

on the device, ``I_pc`` being the emergent intensity (K11) of atmosphere ``select[c]`` at the
angle ``mu[p][c]``.  There is no 2 pi: a uniform planet gives the flux of ``emergent()``.  With
``keep=True`` the result stays there (:class:`PhaseSpectra`) and feeds ``Instrument.apply``,
``Broadening.apply`` and ``CrossCorrelator.correlate`` as ``x``: the phases take the role of the
atmospheres, and only band light curves cross to the host.  The reference has no counterpart; the
definition is the header comment of ``frei_phs_apply`` in include/frei_hip.h.
"""
import ctypes

import numpy as np

from . import _native as N
from ._device import DeviceObject, i32ptr
from .units import value

__all__ = ["PhaseCurve", "PhaseSpectra", "lonlat_cells", "PHASE_TILE"]

# phases a block holds in registers (frei_phase.hip kTile)
PHASE_TILE = 8


def lonlat_cells(n_lon, n_lat):
    """An equal-angle grid of ``n_lat`` x ``n_lon`` cells -> ``(lon, lat, area)``, each
    [n_lat * n_lon] in latitude-major order (cell ``j * n_lon + k`` is latitude band ``j``,
    south to north, and longitude ``k``): the cell centres in radians, longitudes in (-pi, pi)
    with the substellar point at 0, and the exact solid angles
    ``dlon * (sin lat_hi - sin lat_lo)``, which sum to 4 pi."""
    n_lon, n_lat = int(n_lon), int(n_lat)
    if n_lon < 1 or n_lat < 1:
        raise ValueError("lonlat_cells needs n_lon >= 1 and n_lat >= 1")
    dlon = 2.0 * np.pi / n_lon
    lon_c = -np.pi + (np.arange(n_lon) + 0.5) * dlon
    edges = -0.5 * np.pi + np.arange(n_lat + 1) * (np.pi / n_lat)
    edges[-1] = 0.5 * np.pi
    lat_c = 0.5 * (edges[:-1] + edges[1:])
    band = dlon * (np.sin(edges[1:]) - np.sin(edges[:-1]))
    lon = np.tile(lon_c, n_lat)
    lat = np.repeat(lat_c, n_lon)
    area = np.repeat(band, n_lon)
    return lon, lat, area


class PhaseSpectra:
    """What ``PhaseCurve.integrate(keep=True)`` left on the device, [n_phase][n_lam]: pass it as
    ``x`` to ``Instrument.apply``, ``Broadening.apply`` or ``CrossCorrelator.correlate``; the
    phases are their atmospheres.  It goes stale at the owner's next ``integrate`` or
    ``release``; using a stale one raises."""

    suffix = "_phs"     # the C entry points that read it: frei_*_apply_phs

    def __init__(self, owner, serial, n_phase, n_lam):
        self.owner, self.serial, self.n_atm, self.single = owner, serial, n_phase, False
        self.n_lam = n_lam

    @property
    def n_phase(self):
        return self.n_atm

    def handle(self):
        """frei_phs* of the owner, after the staleness check."""
        if self.owner._serial != self.serial or self.owner._handle is None:
            raise RuntimeError("stale PhaseSpectra: its PhaseCurve has integrated again or was "
                               "released since")
        return self.owner._handle


class PhaseCurve(DeviceObject):
    """The disk integral of a set of columns at a set of orbital phases.

    Cells at ``lon``, ``lat`` (radians) with solid angles ``area`` (:func:`lonlat_cells` gives
    an equal-angle grid) on a tidally locked planet whose substellar point is at longitude 0,
    seen at ``phases`` (orbital phase in turns; 0 is mid-transit, 0.5 mid-eclipse) from an orbit
    of ``inclination`` degrees: the sub-observer longitude is ``pi + 2 pi phase``, the
    sub-observer latitude ``beta = pi/2 - i``, and

        mu   = sin(beta) sin(lat) + cos(beta) cos(lat) cos(lon - phi)     (limited to 1)
        coef = area * mu

    ``mu=`` and ``coef=`` [n_phase][n_cell] take any geometry directly instead (an eccentric
    orbit, limb-darkened weights, a partial eclipse by the star folded into ``coef``).  A pair is
    visible exactly when ``mu > 0``; ``n_visible[p]`` counts the cells phase ``p`` sees.
    ``select`` [n_cell] names each cell's atmosphere (default: cell ``c`` is atmosphere ``c``);
    several cells may share one."""

    _destroy = "frei_phs_destroy"

    def __init__(self, lon=None, lat=None, area=None, phases=None, inclination=90.0, select=None,
                 mu=None, coef=None, device=0):
        super().__init__(device)
        if (mu is None) != (coef is None):
            raise ValueError("pass mu= and coef= together")
        if mu is not None:
            self.lon = self.lat = self.area = self.phases = None
            self.mu, self.coef = N.f64(mu), N.f64(coef)
            if self.mu.ndim != 2 or self.mu.shape != self.coef.shape:
                raise ValueError(f"mu and coef must both be [n_phase][n_cell], not "
                                 f"{self.mu.shape} and {self.coef.shape}")
        else:
            if lon is None or lat is None or area is None or phases is None:
                raise ValueError("pass lon, lat, area and phases, or mu= and coef=")
            self.lon, self.lat, self.area = N.f64(lon), N.f64(lat), N.f64(area)
            self.phases = N.f64(np.atleast_1d(phases))
            if (self.lon.ndim != 1 or self.lat.shape != self.lon.shape or
                    self.area.shape != self.lon.shape or self.phases.ndim != 1):
                raise ValueError("lon, lat and area must be [n_cell] and phases [n_phase]")
            phi = np.pi + 2.0 * np.pi * self.phases
            beta = np.deg2rad(90.0 - float(inclination))
            m = (np.sin(beta) * np.sin(self.lat)[None, :] +
                 np.cos(beta) * np.cos(self.lat)[None, :] *
                 np.cos(self.lon[None, :] - phi[:, None]))
            self.mu = N.f64(np.minimum(m, 1.0))
            self.coef = N.f64(self.area[None, :] * self.mu)
        self.inclination = float(inclination)
        if select is None:
            select = np.arange(self.n_cell)
        self.select = np.ascontiguousarray(select, dtype=np.int32)
        if self.select.shape != (self.n_cell,):
            raise ValueError(f"select must have {self.n_cell} entries (one per cell)")
        self.n_visible = np.count_nonzero(self.mu > 0.0, axis=1)
        self._serial = 0

    @property
    def n_phase(self):
        return self.mu.shape[0]

    @property
    def n_cell(self):
        return self.mu.shape[1]

    # ------------------------------------------------------------------ device
    def _create(self, h):
        """frei_phs* of the geometry (checked on the host; uploaded by the first integrate)."""
        return N.lib().frei_phs_create(ctypes.byref(h), self.device, self.n_cell, self.n_phase,
                                       i32ptr(self.select), N.dptr(self.mu), N.dptr(self.coef))

    def release(self):
        self._serial += 1     # whatever was kept ends with the handle
        super().release()

    def integrate(self, engine, T, dtaus=None, keep=False):
        """The phase spectra [n_phase][n_lam] of ``engine``'s columns: an Engine (one column for
        the whole planet, ``T`` [n_layers]) or a BatchEngine (``T`` [n_atm][n_layers]);
        ``dtaus`` a host array [n_atm][n_layers][n_lam], or None for the dtaus the last run left
        on the device, as ``emergent``.  ``keep=True`` leaves the result on the device and
        returns a :class:`PhaseSpectra`; nothing is copied back."""
        n_atm = getattr(engine, "n_atm", 1)
        nL, n = engine.n_layers, engine.n_lam
        Th = N.f64(value(T, "K")).reshape(-1)
        if Th.size != n_atm * nL:
            raise ValueError(f"T must hold {n_atm} x {nL} temperatures, not {Th.size}")
        d = None
        if dtaus is not None:
            d = N.f64(dtaus)
            if d.size != n_atm * nL * n:
                raise ValueError(f"dtaus must have shape {(n_atm, nL, n)}, not {d.shape}")
        out = None if keep else np.empty((self.n_phase, n))
        used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        handle = self.handle()
        self._serial += 1                          # whatever was kept ends with this call
        N.check(N.lib().frei_phs_apply(handle, engine._ctx, N.dptr(d), N.dptr(Th), N.dptr(out),
                                       1 if keep else 0, 0, ctypes.byref(used),
                                       ctypes.byref(ms)))
        self._record(used, ms)
        return PhaseSpectra(self, self._serial, self.n_phase, n) if keep else out
