"""K_p-V_sys maps on the GPU: the detection statistic of the cross-correlation sums and its stack
over the exposures along trial orbits (K14, ``frei_amd/csrc/frei_stack.hip``).

An :class:`OrbitStack` binds the trial velocities of a :class:`~frei_amd.crosscorr.CrossCorrelator`
to a grid of trial orbits: ``dv[k][e]``, the planet's line-of-sight velocity of trial ``k`` at
exposure ``e`` (``Kp[k] sin(2 pi phases[e])`` for a circular orbit, or any ``shifts``), the
observer's ``v_obs[e]`` and the systemic velocities ``Vsys[s]``.  ``stack`` forms, per
atmosphere,

    map[k][s] = sum_e interp(Vsys[s] + dv[k][e] + v_obs[e], velocities, values[e])

for ``values`` given, or for the CCF or the log-likelihood of a
:class:`~frei_amd.crosscorr.CrossCorrelation` — from its host sums, or from the sums that
``correlate(..., keep=True)`` left on the device, which then never cross to the host.  It is the
device counterpart of :func:`frei_amd.crosscorr.kp_vsys_map` (which stays the host path); the
definition, with the order of every operation, is the header comment of ``frei_stack_apply`` in
include/frei_hip.h.  ``dv`` is formed here, on the host, so the device and any restatement share
one ``sin``.
"""
import ctypes

import numpy as np

from . import _native as N
from ._device import DeviceObject

__all__ = ["OrbitStack", "FORMS", "STATISTICS", "ATM_TILE", "LDS_VELOCITIES"]

# the kernel forms that exist (frei_stack_apply's `form`; 0 picks among them): 1 searches the
# velocities in LDS, 2 in global memory; the same bits
FORMS = (1, 2)
# frei_stack_apply's `statistic`
STATISTICS = {"values": 0, "ccf": 1, "loglike": 2}
# atmospheres per lane of the stack kernel (frei_stack.hip kAT)
ATM_TILE = 8
# the longest velocity grid form 1 holds in LDS (include/frei_hip.h FREI_STACK_LDS_VEL)
LDS_VELOCITIES = 2048


class OrbitStack(DeviceObject):
    """``velocities`` [n_vel] (km/s, strictly ascending, any spacing) against trial orbits
    ``Kp`` [n_Kp] and systemic velocities ``Vsys`` [n_Vsys] (any order).  Exactly one of
    ``phases`` [n_exp] (orbital phases, 0 at mid-transit: ``dv = Kp[:, None] * np.sin(2 pi
    phases)[None, :]``) and ``shifts`` [n_Kp][n_exp] (``dv`` itself, for any other orbit) is
    given; ``v_obs`` is a scalar or [n_exp].  ``n_outside`` [n_Kp] counts the (e, s) samples
    that fall off the velocity grid (where the end value is held), so a caller can drop those
    trials."""

    _destroy = "frei_stack_destroy"

    def __init__(self, velocities, Kp, Vsys, phases=None, v_obs=0.0, shifts=None, device=0):
        super().__init__(device)
        self.velocities = N.f64(np.atleast_1d(velocities))
        if self.velocities.ndim != 1 or self.velocities.size < 2:
            raise ValueError("velocities must be [n_vel] with at least 2 points")
        if np.any(np.diff(self.velocities) <= 0):
            raise ValueError("velocities must be strictly ascending")
        self.Kp = N.f64(np.atleast_1d(Kp))
        self.Vsys = N.f64(np.atleast_1d(Vsys))
        if self.Kp.ndim != 1 or self.Kp.size < 1 or self.Vsys.ndim != 1 or self.Vsys.size < 1:
            raise ValueError("Kp must be [n_Kp] and Vsys [n_Vsys]")
        if (phases is None) == (shifts is None):
            raise ValueError("pass exactly one of phases and shifts")
        if phases is not None:
            self.phases = N.f64(np.atleast_1d(phases))
            if self.phases.ndim != 1 or self.phases.size < 1:
                raise ValueError("phases must be [n_exp]")
            self.dv = N.f64(self.Kp[:, None] * np.sin(2.0 * np.pi * self.phases)[None, :])
        else:
            self.phases = None
            self.dv = N.f64(shifts)
            if self.dv.ndim != 2 or self.dv.shape[0] != self.Kp.size or self.dv.shape[1] < 1:
                raise ValueError(f"shifts must be [n_Kp][n_exp] with n_Kp = {self.Kp.size}, not "
                                 f"{self.dv.shape}")
        self.v_obs = N.f64(np.broadcast_to(np.asarray(v_obs, dtype=float), (self.n_exp,)))
        u = (self.Vsys[None, None, :] + self.dv[:, :, None]) + self.v_obs[None, :, None]
        self.n_outside = np.count_nonzero(
            (u < self.velocities[0]) | (u > self.velocities[-1]), axis=(1, 2))

    @property
    def n_vel(self):
        return self.velocities.size

    @property
    def n_exp(self):
        return self.dv.shape[1]

    @property
    def n_kp(self):
        return self.Kp.size

    @property
    def n_vsys(self):
        return self.Vsys.size

    # ------------------------------------------------------------------ device
    def _create(self, h):
        """frei_stack* of the stacker (checked on the host; uploaded by the first stack)."""
        return N.lib().frei_stack_create(
            ctypes.byref(h), self.device, self.n_exp, self.n_vel, N.dptr(self.velocities),
            self.n_kp, N.dptr(self.dv), N.dptr(self.v_obs), self.n_vsys, N.dptr(self.Vsys))

    def stack(self, values, statistic=None, want_values=False, form=0):
        """The map(s) of ``values``: a host array [n_exp][n_vel] -> [n_Kp][n_Vsys] or
        [n_atm][n_exp][n_vel] -> [n_atm][n_Kp][n_Vsys], stacked as it is; or a
        :class:`~frei_amd.crosscorr.CrossCorrelation` with ``statistic`` ``"ccf"`` or
        ``"loglike"`` (its ``W``, ``S_wf``, ``S_wff`` and ``n_pix`` enter the statistic), the
        sums taken from the device when it came from ``correlate(..., keep=True)`` and from its
        host arrays otherwise.  ``want_values=True`` returns ``(map, values)`` with the
        statistic [n_atm][n_exp][n_vel] that was stacked.  ``form`` 0 picks the kernel, a member
        of ``FORMS`` forces it (``form_used`` records the choice)."""
        E, V = self.n_exp, self.n_vel
        kept = sfg = sg = sgg = S_wf = S_wff = None
        W = n_eff = 0.0
        if hasattr(values, "sfg") and hasattr(values, "S_wf"):
            res = values
            if statistic not in ("ccf", "loglike"):
                raise ValueError('a CrossCorrelation needs statistic="ccf" or "loglike"')
            stat = STATISTICS[statistic]
            if np.shape(res.velocities) != (V,) or not np.array_equal(res.velocities,
                                                                       self.velocities):
                raise ValueError("the correlation's velocities are not the stacker's")
            W, n_eff = float(res.W), float(res.n_pix)
            S_wf, S_wff = N.f64(res.S_wf), N.f64(res.S_wff)
            if S_wf.shape != (E,) or S_wff.shape != (E,):
                raise ValueError(f"the correlation has {S_wf.size} exposures, the stacker {E}")
            if getattr(res, "kept", None) is not None:
                kept = res.kept.handle()               # raises when stale
                n_atm, single = res.kept.n_atm, res.kept.single
            else:
                if res.sfg is None or res.sg is None or res.sgg is None:
                    raise ValueError("the statistic needs all three sums (want=)")
                sfg, sg, sgg = N.f64(res.sfg), N.f64(res.sg), N.f64(res.sgg)
                single = sfg.ndim == 2
                if (sfg.ndim not in (2, 3) or sfg.shape[-2:] != (E, V) or
                        sg.shape != sfg.shape[:-2] + (V,) or sgg.shape != sg.shape):
                    raise ValueError("the correlation's sums do not have the stacker's shape")
                sfg = np.ascontiguousarray(sfg.reshape((-1, E, V)))
                n_atm = sfg.shape[0]
                sg = np.ascontiguousarray(sg.reshape((n_atm, V)))
                sgg = np.ascontiguousarray(sgg.reshape((n_atm, V)))
        else:
            if statistic not in (None, "values"):
                raise ValueError("an array is stacked as it is: statistic applies to a "
                                 "CrossCorrelation")
            stat = 0
            sfg = N.f64(getattr(values, "value", values))
            if sfg.ndim not in (2, 3) or sfg.shape[-2:] != (E, V):
                raise ValueError(f"values must be [n_exp][n_vel] or [n_atm][n_exp][n_vel] with "
                                 f"n_exp = {E}, n_vel = {V}, not {sfg.shape}")
            single = sfg.ndim == 2
            sfg = np.ascontiguousarray(sfg.reshape((-1, E, V)))
            n_atm = sfg.shape[0]
        out = np.empty((n_atm, self.n_kp, self.n_vsys))
        vals = np.empty((n_atm, E, V)) if want_values else None
        used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        N.check(N.lib().frei_stack_apply(
            self.handle(), kept, n_atm, N.dptr(sfg), N.dptr(sg), N.dptr(sgg), stat, W,
            N.dptr(S_wf), N.dptr(S_wff), n_eff, N.dptr(out), N.dptr(vals), int(form),
            ctypes.byref(used), ctypes.byref(ms)))
        self._record(used, ms)
        if single:
            out, vals = out[0], None if vals is None else vals[0]
        return (out, vals) if want_values else out
