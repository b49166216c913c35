"""Rotational and instrumental broadening of batched spectra on the GPU (K13,
``frei_amd/csrc/frei_broaden.hip``).

A :class:`BroadeningKernel` is a host-side table of a kernel in velocity (a Gaussian line-spread
function, Gray's rotational profile, any profile, or a convolution of them).  A
:class:`Broadening` binds one to a native wavelength axis: with ``u = c ln(lam)`` and the
trapezoid weights ``tw`` of the axis in ``u``,

    out[m][i] = (sum_j w_ij x[m][j]) / norm[i],    w_ij = tw[j] K(u[j] - u[i]),

``K`` the table interpolated linearly, ``j`` over the window ``|u[j] - u[i]| <= H`` (the table's
half-width) truncated at the ends of the axis, ``norm[i] = sum_j w_ij``.  Only ``u``, ``tw``, the
windows, ``norm`` and the table live on the device; the weights are formed in registers.  The
reference has no counterpart; the definition is the header comment of ``frei_brd_apply`` in
include/frei_hip.h.  With ``keep=True`` the result stays on the device and feeds
``CrossCorrelator.correlate`` or ``Instrument.apply`` without crossing to the host.
"""
import ctypes

import numpy as np

from . import _native as N
from ._device import DeviceObject, i32ptr, kept_suffix, resident_or_host
from .crosscorr import C_KMS
from .units import value

__all__ = ["BroadeningKernel", "Broadening", "BroadenedSpectra", "FORMS", "MAX_COUNT", "C_KMS",
           "MFMA_FROM_ATMOSPHERES", "MFMA_FROM_POINTS", "MFMA_WIDE_POINTS", "automatic_form"]

# the kernel forms that exist (frei_brd_apply's `form`; 0 picks among them)
FORMS = (1, 2)
# the most points a window may hold (include/frei_hip.h FREI_BRD_MAX_COUNT)
MAX_COUNT = 4096
# form 0 takes form 2 from MFMA_FROM_ATMOSPHERES atmospheres where the windows hold
# MFMA_FROM_POINTS points or more on average, and from 2 atmospheres where they hold
# MFMA_WIDE_POINTS or more (frei_broaden.hip kMfmaFromAtmospheres, kMfmaFromPoints,
# kMfmaWidePoints); form 1 otherwise
MFMA_FROM_ATMOSPHERES = 5
MFMA_FROM_POINTS = 21.0
MFMA_WIDE_POINTS = 81.0


def automatic_form(n_atm, mean_points):
    """The form that ``form=0`` takes for ``n_atm`` atmospheres and windows of ``mean_points``
    points on average (``count.mean()``)."""
    return 2 if ((n_atm >= MFMA_FROM_ATMOSPHERES and mean_points >= MFMA_FROM_POINTS) or
                 (n_atm >= 2 and mean_points >= MFMA_WIDE_POINTS)) else 1


_FWHM = 2.0 * np.sqrt(2.0 * np.log(2.0))      # FWHM of a Gaussian in standard deviations


class BroadeningKernel:
    """A kernel in velocity tabulated at ``(k - h) dv`` km/s, ``k = 0 .. 2 h``: ``values`` holds
    an odd number (>= 3) of finite, non-negative samples, ``dv > 0``.  Between samples the
    kernel is linear, beyond the table zero.  Its scale is immaterial (the device renormalises
    every output); the constructors return densities of unit integral."""

    def __init__(self, dv, values):
        self.dv = float(dv)
        self.values = N.f64(values)
        if not self.dv > 0.0 or not np.isfinite(self.dv):
            raise ValueError("dv must be > 0")
        if self.values.ndim != 1 or self.values.size < 3 or self.values.size % 2 == 0:
            raise ValueError("values must hold an odd number (>= 3) of samples")
        if not np.all(np.isfinite(self.values)) or np.any(self.values < 0.0):
            raise ValueError("values must be finite and >= 0")

    @property
    def h(self):
        return (self.values.size - 1) // 2

    @property
    def half_width(self):
        """H = h dv, in km/s (formed as the device library forms it)."""
        return float(self.h) * self.dv

    @property
    def velocities(self):
        return (np.arange(self.values.size) - self.h) * self.dv

    def integral(self):
        """The trapezoid integral of the table."""
        v = self.values
        return float(self.dv * (np.sum(v) - 0.5 * (v[0] + v[-1])))

    def __call__(self, v):
        """The kernel at velocities ``v`` (linear in the table, zero beyond it)."""
        return np.interp(np.asarray(v, dtype=float), self.velocities, self.values, left=0.0,
                         right=0.0)

    @classmethod
    def from_profile(cls, dv, values):
        return cls(dv, values)

    @classmethod
    def gaussian(cls, fwhm_kms=None, resolving_power=None, n_sigma=4.0, oversample=16):
        """A Gaussian of full width at half maximum ``fwhm_kms`` (km/s) or ``c /
        resolving_power``, cut at ``n_sigma`` standard deviations, ``oversample`` samples per
        standard deviation."""
        if (fwhm_kms is None) == (resolving_power is None):
            raise ValueError("pass either fwhm_kms or resolving_power")
        fwhm = C_KMS / float(resolving_power) if fwhm_kms is None else float(fwhm_kms)
        if not fwhm > 0.0:
            raise ValueError("the width must be > 0")
        s = fwhm / _FWHM
        dv = s / float(oversample)
        h = max(1, int(np.ceil(n_sigma * float(oversample))))
        v = (np.arange(2 * h + 1) - h) * dv
        z = v / s
        return cls(dv, np.exp(-0.5 * (z * z)) / (s * np.sqrt(2.0 * np.pi)))

    @classmethod
    def rotation(cls, vsini, epsilon=0.6, n_half=512):
        """Gray's rotational profile of a rigid sphere with linear limb darkening ``epsilon``,
        ``[2 (1 - e) sqrt(1 - (v/V)^2) + (pi e / 2) (1 - (v/V)^2)] / (pi V (1 - e / 3))`` for
        ``|v| < V = vsini`` (km/s), on ``2 n_half + 1`` samples from -V to V."""
        V = float(vsini)
        if not V > 0.0:
            raise ValueError("vsini must be > 0")
        h = int(n_half)
        r = (np.arange(2 * h + 1) - h) / float(h)
        a = np.maximum(1.0 - r * r, 0.0)
        e = float(epsilon)
        vals = (2.0 * (1.0 - e) * np.sqrt(a) + 0.5 * np.pi * e * a) / (np.pi * V * (1.0 - e / 3.0))
        return cls(V / h, vals)

    def convolve(self, other):
        """The convolution with ``other`` on the finer of the two spacings (both tables taken
        there by linear interpolation, then the discrete convolution times ``dv``), on the host:
        rotation and line-spread function in one kernel."""
        dv = min(self.dv, other.dv)

        def on(k):
            h = int(np.ceil(k.half_width / dv - 1e-9))
            return k((np.arange(2 * h + 1) - h) * dv)
        return BroadeningKernel(dv, np.maximum(np.convolve(on(self), on(other)) * dv, 0.0))


def axis_weights(u):
    """Trapezoid weights of the ascending axis ``u``: ``(u[j+1] - u[j-1]) / 2`` inside,
    ``(u[1] - u[0]) / 2`` and ``(u[-1] - u[-2]) / 2`` at the ends."""
    tw = np.empty_like(u)
    tw[1:-1] = 0.5 * (u[2:] - u[:-2])
    tw[0] = 0.5 * (u[1] - u[0])
    tw[-1] = 0.5 * (u[-1] - u[-2])
    return tw


def windows(u, H):
    """(first, count) int32 of the runs ``|u[j] - u[i]| <= H`` on the ascending axis ``u``: a
    binary search for ``u[i] -+ H`` and then the criterion itself — that very subtraction — at
    the four points about the two ends until nothing moves (the search compares with a rounded
    ``u[i] -+ H`` and may be off by a point)."""
    n = u.size
    lo = np.searchsorted(u, u - H, "left").astype(np.int64)
    hi = np.searchsorted(u, u + H, "right").astype(np.int64) - 1     # inclusive
    idx = np.arange(n)
    lo, hi = np.minimum(lo, idx), np.maximum(hi, idx)
    while True:
        grow_lo = (lo > 0) & (np.abs(u[np.maximum(lo - 1, 0)] - u) <= H)
        cut_lo = ~grow_lo & (lo < idx) & ~(np.abs(u[lo] - u) <= H)
        grow_hi = (hi < n - 1) & (np.abs(u[np.minimum(hi + 1, n - 1)] - u) <= H)
        cut_hi = ~grow_hi & (hi > idx) & ~(np.abs(u[hi] - u) <= H)
        if not (grow_lo.any() or cut_lo.any() or grow_hi.any() or cut_hi.any()):
            break
        lo = lo - grow_lo + cut_lo
        hi = hi + grow_hi - cut_hi
    return lo.astype(np.int32), (hi - lo + 1).astype(np.int32)


def tap_weights(u, tw, i, j, inv_dv, tab):
    """``w_ij`` for index arrays ``i``, ``j``, by the operations of the definition."""
    h = float((tab.size - 1) // 2)
    d = u[j] - u[i]
    q = d * inv_dv + h
    k = np.clip(np.floor(q), 0.0, float(tab.size - 2))
    f = q - k
    k = k.astype(np.int64)
    K = tab[k] + f * (tab[k + 1] - tab[k])
    return tw[j] * K


class BroadenedSpectra:
    """What ``Broadening.apply(keep=True)`` left on the device, [n_atm][n_lam]: pass it as ``x``
    to ``CrossCorrelator.correlate`` or ``Instrument.apply``.  It goes stale at the owner's next
    ``apply`` or ``release``; using a stale one raises."""

    suffix = "_brd"     # the C entry points that read it: frei_*_apply_brd

    def __init__(self, owner, serial, n_atm, single):
        self.owner, self.serial, self.n_atm, self.single = owner, serial, n_atm, single

    @property
    def n_lam(self):
        return self.owner.n_lam

    def handle(self):
        """frei_brd* of the owner, after the staleness check."""
        if self.owner._serial != self.serial or self.owner._handle is None:
            raise RuntimeError("stale BroadenedSpectra: its Broadening has applied again or was "
                               "released since")
        return self.owner._handle


class Broadening(DeviceObject):
    """``kernel`` (:class:`BroadeningKernel`) on the native axis ``lam`` ([n_lam], µm or a
    Quantity, strictly ascending).  The plan is built on the host, vectorised: ``u``, ``tw``,
    ``first``, ``count`` (and ``norm``, computed on first use by the device library's
    operations) are exposed for inspection."""

    _destroy = "frei_brd_destroy"

    def __init__(self, lam, kernel, device=0):
        super().__init__(device)
        self.lam = N.f64(value(lam, "um"))
        if self.lam.ndim != 1 or self.lam.size < 2:
            raise ValueError("lam must be a 1-D wavelength axis of at least 2 points")
        if np.any(np.diff(self.lam) <= 0) or not np.all(np.isfinite(self.lam)) or self.lam[0] <= 0:
            raise ValueError("lam must be positive, finite and strictly ascending")
        self.kernel = kernel
        self.dv = kernel.dv
        self.inv_dv = 1.0 / kernel.dv
        self.tab = kernel.values
        self.u = N.f64(C_KMS * np.log(self.lam))
        self.tw = axis_weights(self.u)
        self.first, self.count = windows(self.u, kernel.half_width)
        self._norm = None
        self._serial = 0

    @property
    def n_lam(self):
        return self.lam.size

    @property
    def norm(self):
        """``norm[i] = sum_j w_ij`` in ascending ``j`` with plain additions, [n_lam]: the
        operations of ``frei_brd_create`` (one vectorised pass per tap)."""
        if self._norm is None:
            s = np.zeros(self.n_lam)
            i_all = np.arange(self.n_lam)
            for t in range(int(self.count.max())):
                i = i_all[self.count > t]
                s[i] = s[i] + tap_weights(self.u, self.tw, i, self.first[i] + t, self.inv_dv,
                                          self.tab)
            self._norm = s
        return self._norm

    # ------------------------------------------------------------------ device
    def _create(self, h):
        """frei_brd* of the broadener (axis, windows, norm and table uploaded once)."""
        return N.lib().frei_brd_create(
            ctypes.byref(h), self.device, self.n_lam, N.dptr(self.u), N.dptr(self.tw),
            i32ptr(self.first), i32ptr(self.count), self.tab.size, self.dv, self.inv_dv,
            N.dptr(self.tab))

    def device_norm(self):
        """``norm`` as ``frei_brd_create`` formed it (read back from the device)."""
        out = np.empty(self.n_lam)
        N.check(N.lib().frei_brd_norm(self.handle(), N.dptr(out)))
        return out

    def release(self):
        self._serial += 1     # whatever was kept ends with the handle
        super().release()

    def apply(self, x=None, engine=None, form=0, keep=False):
        """``x`` ([n_lam] or [n_atm][n_lam]) broadened -> an array of the same shape (a
        Quantity's numbers as they are, its unit put back).  ``x=None`` with ``engine=`` (an
        Engine or BatchEngine on the whole axis) takes the emergent spectra resident in the
        engine's flux state; an :class:`~frei_amd.modelgrid.InterpolatedSpectra` as ``x`` takes
        what ``ModelGrid.interpolate(keep=True)`` left on the device, a
        :class:`~frei_amd.phasecurve.PhaseSpectra` what ``PhaseCurve.integrate(keep=True)`` left
        there.  ``form`` 0 picks the
        kernel, a member of ``FORMS`` forces it
        (``form_used`` records the choice).  ``keep=True`` leaves the result on the device and
        returns a :class:`BroadenedSpectra` for ``CrossCorrelator.correlate`` or
        ``Instrument.apply``; nothing is copied back."""
        kept = kept_suffix(x)
        if kept == "_brd":
            raise TypeError("a BroadenedSpectra cannot be broadened again: pass an array")
        x, ctx, src, n_atm, single, unit = resident_or_host(
            x, engine, self.n_lam, ("a broadener", "a window"))
        out = None if keep else np.empty((n_atm, self.n_lam))
        used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        handle = self.handle()
        self._serial += 1                          # whatever was kept ends with this call
        tail = (n_atm, int(form), N.dptr(out), 1 if keep else 0, ctypes.byref(used),
                ctypes.byref(ms))
        if src is not None:
            N.check(getattr(N.lib(), "frei_brd_apply" + kept)(handle, src, *tail))
        else:
            N.check(N.lib().frei_brd_apply(handle, ctx, N.dptr(x), *tail))
        self._record(used, ms)
        if keep:
            return BroadenedSpectra(self, self._serial, n_atm, single)
        if single:
            out = out[0]
        return out if unit is None else out * unit
