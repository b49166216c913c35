"""Spectra interpolated between the models of a grid sweep on the GPU (K15,
``frei_amd/csrc/frei_interp.hip``).

A sweep gives spectra at the nodes of a parameter grid (T_ref x log g x [M/H], say); a fit needs
the spectrum at arbitrary points between them, thousands per sampler step, each scored by the
same instruments and correlators.  A :class:`ModelGrid` holds the node spectra on the device,
plans a multilinear interpolation on the host (:meth:`ModelGrid.plan`: per query the ``2^d``
corner nodes and their weights) and forms

    out[q][i] = sum_c w[q][c] X[idx[q][c]][i]

on the device, corners in ascending ``c``, one multiply and one add per term.  With
``keep=True`` the result stays there (:class:`InterpolatedSpectra`) and feeds
``Instrument.apply``, ``CrossCorrelator.correlate`` and ``Broadening.apply`` as ``x``: the
queries take the role of the atmospheres, and only chi-squares, sums and maps cross to the host.
The reference has no counterpart; the definition is the header comment of ``frei_itp_apply`` in
include/frei_hip.h.
"""
import ctypes

import numpy as np

from . import _native as N
from ._device import DeviceObject, i32ptr, kept_suffix, resident_or_host
from .units import value

__all__ = ["ModelGrid", "InterpolatedSpectra", "FORMS", "MAX_CORNERS", "LDS_BYTES", "LDS_WAVES",
           "LDS_MAX_NODES", "LDS_FROM_TILES", "LDS_FROM_QUERIES", "LDS_FROM_CORNERS",
           "tile_width", "automatic_form"]

# the kernel forms that exist (frei_itp_apply's `form`; 0 picks among them)
FORMS = (1, 2)
# the most corners a query may hold (include/frei_hip.h FREI_ITP_MAX_CORNERS): 2^4
MAX_CORNERS = 16
# form 2 (include/frei_hip.h FREI_ITP_LDS_BYTES, _WAVES, _MAX_NODES): the LDS a tile's slab of
# the library may take, the waves of a workgroup (each takes one query at a time), and the
# tallest library whose narrowest tile (64 wavelengths) still fits
LDS_BYTES = 163840
LDS_WAVES = 16
LDS_MAX_NODES = 320
# form 0 takes form 2 where it fits, the axis gives LDS_FROM_TILES tiles or more (a workgroup per
# CU), and the call holds LDS_FROM_QUERIES queries and LDS_FROM_CORNERS corners or more
# (frei_interp.hip kLdsFromTiles, kLdsFromQueries, kLdsFromCorners); form 1 otherwise.  Measured
# at 256 nodes x 100k wavelengths (tools/interp_probe.py, profiles/r15/interp/README.md): form 2
# wins at 16 corners from 64 queries on, ties at 8 corners, loses at 2 corners and for a single
# query; the thresholds are the midpoints of the timed neighbours
LDS_FROM_TILES = 256
LDS_FROM_QUERIES = 32
LDS_FROM_CORNERS = 12


def tile_width(n_node):
    """Form 2's tile: the widest of 256, 128 and 64 wavelengths whose slab of ``n_node`` rows
    fits ``LDS_BYTES``; 0 where the library is too tall for form 2."""
    for t in (256, 128, 64):
        if n_node * t * 8 <= LDS_BYTES:
            return t
    return 0


def automatic_form(n_node, n_lam, n_query, n_corner):
    """The form that ``form=0`` takes for a library of ``n_node`` spectra of ``n_lam`` points
    and a plan of ``n_query`` queries of ``n_corner`` corners."""
    t = tile_width(n_node)
    if t == 0:
        return 1
    tiles = -(-n_lam // t)
    return 2 if (tiles >= LDS_FROM_TILES and n_query >= LDS_FROM_QUERIES and
                 n_corner >= LDS_FROM_CORNERS) else 1


class InterpolatedSpectra:
    """What ``ModelGrid.interpolate(keep=True)`` left on the device, [n_query][n_lam]: pass it
    as ``x`` to ``Instrument.apply``, ``CrossCorrelator.correlate`` or ``Broadening.apply``; the
    queries are their atmospheres.  It goes stale at the owner's next ``interpolate``,
    ``set_nodes`` or ``release``; using a stale one raises."""

    suffix = "_itp"     # the C entry points that read it: frei_*_apply_itp

    def __init__(self, owner, serial, n_query):
        self.owner, self.serial, self.n_atm, self.single = owner, serial, n_query, False

    @property
    def n_query(self):
        return self.n_atm

    @property
    def n_lam(self):
        return self.owner.n_lam

    def handle(self):
        """frei_itp* of the owner, after the staleness check."""
        if self.owner._serial != self.serial or self.owner._handle is None:
            raise RuntimeError("stale InterpolatedSpectra: its ModelGrid has interpolated again, "
                               "taken new nodes or was released since")
        return self.owner._handle


class ModelGrid(DeviceObject):
    """Node spectra on a rectilinear parameter grid.  ``axes`` holds 1 to 4 strictly ascending
    1-D arrays; node ``m`` is the C-order index over them (the last axis fastest) and the node
    spectra [n_node][n_lam] on ``lam`` ([n_lam], µm or a Quantity) come from one of: ``spectra=``
    a host array (uploaded on first use), ``spectra=`` a
    :class:`~frei_amd.broaden.BroadenedSpectra` (what ``Broadening.apply(keep=True)`` left on the
    device), or ``engine=`` a BatchEngine whose run left its emergent spectra there — the two
    device sources are copied at once, device to device, so the engine may be reused or closed
    afterwards.  An axis of one node takes no part in the interpolation: it has no corner bit and
    its coordinate is only checked for finiteness."""

    _destroy = "frei_itp_destroy"

    def __init__(self, axes, lam, spectra=None, engine=None, device=0):
        super().__init__(device)
        self.axes = [N.f64(a) for a in axes]
        if not 1 <= len(self.axes) <= 4:
            raise ValueError(f"a model grid has 1 to 4 axes, not {len(self.axes)}")
        for a, g in enumerate(self.axes):
            if g.ndim != 1 or g.size < 1:
                raise ValueError(f"axis {a} must be a 1-D array of at least one node")
            if not np.all(np.isfinite(g)) or np.any(np.diff(g) <= 0):
                raise ValueError(f"axis {a} must be finite and strictly ascending")
        self.shape = tuple(g.size for g in self.axes)
        self.n_node = int(np.prod(self.shape))
        self.lam = N.f64(value(lam, "um"))
        if self.lam.ndim != 1 or self.lam.size < 1:
            raise ValueError("lam must be a 1-D wavelength axis")
        self.n_outside = 0
        self._serial = 0
        self._pending = None
        self._nodes_set = False
        self.set_nodes(spectra, engine)

    @property
    def n_lam(self):
        return self.lam.size

    @property
    def n_axes(self):
        return len(self.axes)

    @property
    def participating(self):
        """The axes of more than one node, in order: axis ``a`` of them is bit
        ``d_eff - 1 - a`` of the corner number."""
        return [a for a, g in enumerate(self.axes) if g.size > 1]

    @property
    def n_corner(self):
        return 1 << len(self.participating)

    # ------------------------------------------------------------------ host plan
    def plan(self, theta):
        """The multilinear plan of ``theta`` [n_query][d] -> ``(idx, w, n_outside)``: ``idx``
        int32 and ``w`` float64 [n_query][2^d_eff], ``d_eff`` the axes of more than one node.
        Per such axis ``a``, by exactly these operations: theta is clamped to ``[g[0], g[-1]]``
        (``n_outside`` counts the coordinates that were); ``j`` is the largest index with
        ``g[j] <= theta``, limited to ``len - 2``; ``t = (theta - g[j]) / (g[j+1] - g[j])``.
        Corner ``c`` takes the upper node on axis ``a`` where bit ``d_eff - 1 - a`` of ``c`` is
        set; its weight is the product over ``a`` ascending, left to right, of ``t_a`` or
        ``1 - t_a``.  NaN coordinates raise."""
        theta = N.f64(theta)
        if theta.ndim != 2 or theta.shape[1] != self.n_axes or theta.shape[0] < 1:
            raise ValueError(f"theta must be [n_query][{self.n_axes}] with at least one query, "
                             f"not {theta.shape}")
        if np.any(np.isnan(theta)):
            q, a = np.argwhere(np.isnan(theta))[0]
            raise ValueError(f"theta[{q}][{a}] is NaN")
        strides = np.ones(self.n_axes, dtype=np.int64)
        for a in range(self.n_axes - 2, -1, -1):
            strides[a] = strides[a + 1] * self.shape[a + 1]
        part = self.participating
        d_eff = len(part)
        js, ts, n_outside = [], [], 0
        for a, g in enumerate(self.axes):
            th = theta[:, a]
            if g.size == 1:
                if not np.all(np.isfinite(th)):
                    q = int(np.argwhere(~np.isfinite(th))[0][0])
                    raise ValueError(f"theta[{q}][{a}] is not finite")
                continue
            n_outside += int(np.count_nonzero((th < g[0]) | (th > g[-1])))
            th = np.minimum(np.maximum(th, g[0]), g[-1])
            j = np.clip(np.searchsorted(g, th, "right") - 1, 0, g.size - 2)
            ts.append((th - g[j]) / (g[j + 1] - g[j]))
            js.append(j)
        Q = theta.shape[0]
        idx = np.zeros((Q, 1 << d_eff), dtype=np.int64)
        w = np.empty((Q, 1 << d_eff))
        for c in range(1 << d_eff):
            wc = None
            for k, a in enumerate(part):
                up = (c >> (d_eff - 1 - k)) & 1
                idx[:, c] += (js[k] + up) * strides[a]
                f = ts[k] if up else 1.0 - ts[k]
                wc = f if wc is None else wc * f
            w[:, c] = 1.0 if wc is None else wc
        return np.ascontiguousarray(idx, dtype=np.int32), w, n_outside

    # ------------------------------------------------------------------ device
    def _create(self, h):
        """frei_itp* of the grid (the library is filled by set_nodes)."""
        return N.lib().frei_itp_create(ctypes.byref(h), self.device, self.n_lam, self.n_node)

    def release(self):
        self._serial += 1     # whatever was kept ends with the handle
        self._nodes_set = False
        super().release()

    def set_nodes(self, spectra=None, engine=None):
        """New node spectra from ``spectra`` (a host array [n_node][n_lam], uploaded on first
        use, or a :class:`~frei_amd.broaden.BroadenedSpectra`) or ``engine`` (its resident
        spectra): the library is replaced and whatever was kept ends."""
        kept = kept_suffix(spectra)
        if kept == "_itp":
            raise TypeError("an InterpolatedSpectra cannot be a model grid's nodes: pass an array")
        if kept == "_phs":
            raise TypeError("a PhaseSpectra cannot be a model grid's nodes: pass an array")
        x, ctx, brd, n_rows, _, _ = resident_or_host(
            spectra, engine, self.n_lam, ("a model grid", "its wavelength axis"))
        if n_rows != self.n_node:
            raise ValueError(f"{n_rows} spectra for {self.n_node} nodes: the row count must be "
                             f"the product of the axis lengths {self.shape}")
        self._serial += 1
        self._nodes_set = False
        self._pending = x
        if x is None:         # a device source is copied now: it may not outlive this call
            N.check(N.lib().frei_itp_set_nodes(self.handle(), ctx, brd, None))
            self._nodes_set = True

    def handle(self):
        """The native handle, its library filled."""
        h = super().handle()
        if self._pending is not None and not self._nodes_set:
            N.check(N.lib().frei_itp_set_nodes(h, None, None, N.dptr(self._pending)))
            self._nodes_set = True
        return h

    def interpolate(self, theta=None, form=0, keep=False, idx=None, w=None):
        """The spectra at ``theta`` [n_query][d] -> [n_query][n_lam] (``n_outside`` records
        how many coordinates were clamped), or at any plan ``idx=``, ``w=`` [n_query][n_corner]
        (simplices, a barycentric scheme; up to ``MAX_CORNERS`` corners; the device applies the
        weights as they are).  ``form`` 0 picks the kernel, a member of ``FORMS`` forces it
        (``form_used`` records the choice; the forms give the same bits).  ``keep=True`` leaves
        the result on the device and returns an :class:`InterpolatedSpectra`; nothing is copied
        back."""
        if (idx is None) != (w is None) or (theta is None) == (idx is None):
            raise ValueError("pass theta, or idx= and w= together")
        if theta is not None:
            idx, w, self.n_outside = self.plan(theta)
        else:
            idx = np.ascontiguousarray(idx, dtype=np.int32)
            w = N.f64(w)
            if idx.ndim != 2 or idx.shape != w.shape:
                raise ValueError(f"idx and w must both be [n_query][n_corner], not {idx.shape} "
                                 f"and {w.shape}")
        Q, C = idx.shape
        out = None if keep else np.empty((Q, self.n_lam))
        used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        handle = self.handle()
        self._serial += 1                          # whatever was kept ends with this call
        N.check(N.lib().frei_itp_apply(handle, Q, C, i32ptr(idx), N.dptr(w), int(form),
                                       N.dptr(out), 1 if keep else 0, ctypes.byref(used),
                                       ctypes.byref(ms)))
        self._record(used, ms)
        return InterpolatedSpectra(self, self._serial, Q) if keep else out
