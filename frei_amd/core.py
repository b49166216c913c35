"""User API: Planet, Grid, emission_spectrum, effective temperature (frei/core.py).

``Grid.emission_spectrum`` runs the whole radiative-equilibrium T-P loop on the GPU
(frei_run: device-resident sweeps, bolometric reductions, dT, convergence test).
"""
import numpy as np

from .constants import (A_RSTAR_HOT_JUPITER, FLUX_UNIT, G_JUPITER, M_BAR_HOT_JUPITER, R_JUPITER,
                        R_SUN, SIGMA_SB, UM)
from .engine import Engine, f_toa
from .tp import pressure_grid, temperature_grid
from .transit import default_radius, level_radii
from .twostream import BB
from .units import scalar, unit_of, value, with_unit

__all__ = ["Grid", "Planet", "Spectrum", "effective_temperature", "wavelength_grid", "F_TOA",
           "B_star", "contribution_function"]


def wavelength_grid(min_micron=0.5, max_micron=10, n_bins=500, lam=None):
    """Log-spaced wavelengths (µm), bin edges and resolution (core.py:34-45; Q14)."""
    if lam is None:
        lam = np.logspace(np.log10(min_micron), np.log10(max_micron), n_bins)
    lam = np.asarray(value(lam, "um"), dtype=float)
    d0 = lam[1] - lam[0]
    wl_bins = np.concatenate([[lam.min() - d0], lam]) + d0 / 2
    m = lam.shape[0] // 2
    R = float(lam[m] / (lam[m + 1] - lam[m]))
    return lam, wl_bins, R


def F_TOA(lam, T_star=5800.0, f=2 / 3, a_rstar=A_RSTAR_HOT_JUPITER, F_star=None):
    """Irradiation at the top of the atmosphere, erg s^-1 cm^-3 (core.py:48-55).  ``F_star``
    ([n_lam], erg s^-1 cm^-3) is the star's surface flux on ``lam`` and takes the place of the
    blackbody's ``pi * B_star(T_star, lam)``."""
    if F_star is None:
        return f_toa(value(lam, "um"), scalar(T_star, "K"), f, a_rstar)
    F_star = checked_stellar_spectrum(F_star, len(value(lam, "um")))
    return f * a_rstar ** -2 * 1 / (2 * np.pi) * F_star


def checked_stellar_spectrum(F_star, n_lam=None):
    """``F_star`` as a float array [n_lam] in erg s^-1 cm^-3; a non-finite value (a bin of the
    grid that the binned spectrum does not cover) is refused."""
    F_star = np.asarray(value(F_star, "erg / (s cm3)"), dtype=float)
    if F_star.ndim != 1 or (n_lam is not None and F_star.shape != (n_lam,)):
        raise ValueError("stellar spectrum must be [n_lam], one value per grid wavelength"
                         f"{'' if n_lam is None else f' ({n_lam})'}, got shape {F_star.shape}")
    bad = np.nonzero(~np.isfinite(F_star))[0]
    if bad.size:
        shown = ", ".join(str(k) for k in bad[:8]) + (", ..." if bad.size > 8 else "")
        raise ValueError(f"stellar spectrum does not cover the grid: bins {shown} hold fewer "
                         "than 2 points")
    return F_star


def B_star(T_star, lam):
    """Stellar blackbody (core.py:58-62)."""
    return BB(T_star)(lam)


class Planet:
    """Planetary system (core.py:65-106). m_bar in g, g in cm s^-2, T_star in K.
    ``stellar_spectrum`` ([n_lam], erg s^-1 cm^-3) is the star's surface flux binned onto the
    grid's wavelengths (``StellarSpectra.bin``); without it the star is a blackbody of T_star.
    ``R_p`` and ``R_star`` (cm or Quantities) are the radii of planet and star: the defaults of
    the transmission spectra (``Grid.transmission_spectrum``, ``BatchResult.transmission``)."""

    def __init__(self, a_rstar, m_bar, g, T_star, alpha, stellar_spectrum=None, R_p=None,
                 R_star=None):
        self.a_rstar = float(a_rstar)
        self.m_bar = scalar(m_bar, "g")
        self.g = scalar(g, "cm / s2")
        self.T_star = scalar(T_star, "K")
        self.alpha = alpha
        self.stellar_spectrum = (None if stellar_spectrum is None
                                 else checked_stellar_spectrum(stellar_spectrum))
        self.R_p = None if R_p is None else scalar(R_p, "cm")
        self.R_star = None if R_star is None else scalar(R_star, "cm")

    @classmethod
    def from_hot_jupiter(cls):
        """M_J, R_J, m_bar = 2.4 m_p, g = g_J, T_star = 5800 K, a = 0.03 AU (core.py:92-106)."""
        return cls(a_rstar=A_RSTAR_HOT_JUPITER, m_bar=M_BAR_HOT_JUPITER, g=G_JUPITER,
                   T_star=5800.0, alpha=1, R_p=R_JUPITER, R_star=R_SUN)


class Spectrum:
    """Minimal Spectrum1D stand-in: ``flux`` (erg s^-1 cm^-3) on ``wavelength`` (µm)."""

    def __init__(self, flux, spectral_axis):
        self.flux = np.asarray(flux)
        self.spectral_axis = np.asarray(spectral_axis)

    @property
    def wavelength(self):
        return self.spectral_axis


class Grid:
    """Grid over temperatures, pressures and wavelengths (core.py:109-338).

    Units: wavelengths µm, pressures bar, temperatures K.  ``device`` selects the GPU."""

    def __init__(self, planet, lam=None, pressures=None, init_temperatures=None,
                 lam_min=0.5, lam_max=10, n_wl_bins=500, P_toa=1e-6, P_boa=200,
                 n_layers=30, T_ref=2300, P_ref=0.1, alpha=0.1, device=0):
        self.planet = planet
        if lam is None:
            self.lam, self.wl_bins, self.R = wavelength_grid(
                min_micron=scalar(lam_min, "um"), max_micron=scalar(lam_max, "um"),
                n_bins=n_wl_bins)
        else:
            self.lam, self.wl_bins, self.R = wavelength_grid(lam=lam)
        if pressures is None:
            self.pressures = pressure_grid(n_layers=n_layers,
                                           P_toa=np.log10(scalar(P_toa, "bar")),
                                           P_boa=np.log10(scalar(P_boa, "bar")))
        else:
            self.pressures = np.asarray(value(pressures, "bar"), dtype=float)
        if init_temperatures is None:
            self.init_temperatures = temperature_grid(self.pressures, T_ref, P_ref, alpha)
        else:
            self.init_temperatures = np.asarray(value(init_temperatures, "K"), dtype=float)
        self.opacities = None
        self.mmr = None
        self.chemistry = None
        self.device = device
        self._engine = None
        self._last_dtaus = None

    def __repr__(self):
        return (f"<Grid in T=[{self.init_temperatures[0]:.0f}...{self.init_temperatures[-1]:.0f}] K, "
                f"p=[{self.pressures[0]:.2g}...{self.pressures[-1]:.2g}] bar, "
                f"lam=[{self.lam[0]}...{self.lam[-1]}] um>")

    def load_opacities(self, species=None, path=None, opacities=None, client=None,
                       force_reload=False, groupies=False, mmr=None, cross_sections=None,
                       chemistry=None):
        """Attach opacity tables (core.py:198-231).  ``opacities`` is the reference's dict
        of (pressure, temperature, wavelength) tables; otherwise high-resolution
        cross-sections (files at ``path`` or ``cross_sections``) are binned on the GPU
        straight into the engine's tables (opacity.py:66-170).  The mixing ratios come from
        ``chemistry`` — a provider on the reference's ``chemistry(T, p, species, m_bar=...)``
        signature, called wherever the reference's kappa calls it (opacity.py:246-248; the
        drop-in passes frei's own) — or ``mmr`` (per-species, per-layer
        arrays or a ChemistryTable); with neither, the reference's mock."""
        if (self.opacities is None and opacities is None) or force_reload:
            from .binning import binned_opacity
            self.opacities = binned_opacity(self.init_temperatures, self.pressures,
                                            self.wl_bins, self.lam, species=species,
                                            path=path, groupies=groupies,
                                            cross_sections=cross_sections, device=self.device)
        else:
            self.opacities = opacities
        if mmr is not None and chemistry is not None:
            raise ValueError("pass either mmr or a chemistry provider, not both")
        self.mmr = mmr
        self.chemistry = chemistry
        self._close_engine()
        return self.opacities

    def _close_engine(self):
        if self._engine is not None:
            self._engine.close()
            self._engine = None
        self._last_dtaus = None   # its device copy went with the engine

    def engine(self):
        if self._engine is None:
            pl = self.planet
            self._engine = Engine(self.lam, self.pressures, self.opacities, g=pl.g,
                                  m_bar=pl.m_bar,
                                  F_toa=F_TOA(self.lam, T_star=pl.T_star, a_rstar=pl.a_rstar,
                                              F_star=getattr(pl, "stellar_spectrum", None)),
                                  mmr=self.mmr, chemistry=self.chemistry, device=self.device)
        return self._engine

    def emission_spectrum(self, n_timesteps=1, n_zero_crossings=2, convergence_dT=3.0):
        """Emission spectrum after iterating toward radiative equilibrium (core.py:233-338)
        -> (spectrum, final_temps, temperature_history, dtaus)."""
        if self.opacities is None:
            raise ValueError("Must load opacities before computing emission spectrum.")
        if n_timesteps < 1:
            raise ValueError("n_timesteps must be >= 1")
        out = self.engine().run(self.init_temperatures, n_timesteps=n_timesteps,
                                n_zero_crossings=n_zero_crossings,
                                convergence_dT=scalar(convergence_dT, "K"),
                                alpha=self.planet.alpha)
        th = out["temp_hist"]
        th = th.T[th[0] != 0].T   # core.py:320-321
        self._last_dtaus = out["dtaus"]
        return (Spectrum(out["spectrum"], self.lam), out["final_T"], th, out["dtaus"])

    def contribution_function(self, final_temps, dtaus=None):
        """Contribution function of the last emission_spectrum (plot.py:63-79)."""
        return contribution_function(self, self._last_dtaus if dtaus is None else dtaus,
                                     final_temps)

    def transmission_spectrum(self, final_temps, dtaus=None, R_p=None, R_star=None, P_ref=None):
        """Transmission spectrum of the converged atmosphere: a :class:`Spectrum` whose ``flux``
        is the transit depth (R_eff / R_star)^2 per wavelength (frei_transit; the reference has
        no counterpart).  ``dtaus`` defaults to the last emission_spectrum's (its device copy is
        used); ``R_p`` and ``R_star`` (cm or Quantities) default to the Planet's; ``P_ref``
        (bar) is the pressure R_p refers to (by default level 1, ``pressures[1]``)."""
        pl = self.planet
        radii = level_radii(final_temps, self.pressures, pl.g, pl.m_bar,
                            default_radius(R_p, pl, "R_p", "the planet's radius"), P_ref)
        R_star = default_radius(R_star, pl, "R_star", "the star's radius")
        eng, d = _post_engine(self, self._last_dtaus if dtaus is None else dtaus)
        return Spectrum(eng.transit(radii, R_star, d), self.lam)

    def emergent_spectrum(self, final_temps, dtaus=None, mu=None, weights=None,
                          want_intensity=False):
        """Ray-traced emission spectrum of the converged atmosphere: a :class:`Spectrum` whose
        ``flux`` is ``2 pi sum_k weights[k] mu[k] I(mu[k])`` of the emergent intensities at the
        viewing angles ``mu`` (frei_emergent, pure absorption; the reference has no counterpart),
        in emission_spectrum's unit (a Quantity when ``final_temps`` is one).  ``dtaus`` defaults
        to the last emission_spectrum's (its device copy is used); ``mu`` and ``weights`` default
        to :func:`frei_amd.gauss_angles` (4).  ``want_intensity`` also returns the intensities
        [n_mu][n_lam]: (spectrum, intensity); ``mu`` without ``weights`` returns them alone."""
        eng, d = _post_engine(self, self._last_dtaus if dtaus is None else dtaus)
        out = eng.emergent(final_temps, mu=mu, weights=weights, dtaus=d,
                           want_intensity=want_intensity)
        if mu is not None and weights is None:
            return out
        flux, inten = out if want_intensity else (out, None)
        spec = Spectrum(flux, self.lam)
        spec.flux = with_unit(spec.flux, unit_of(FLUX_UNIT, final_temps))
        return (spec, inten) if want_intensity else spec

    def observe(self, instrument, spectrum, kind="eclipse", data=None, sigma=None, R_p=None,
                R_star=None, broadening=None):
        """``spectrum`` (the :class:`Spectrum` of emission_spectrum or transmission_spectrum)
        through ``instrument`` (:class:`~frei_amd.observe.Instrument`, K10) -> obs [K], or
        (obs, chi2) with ``data`` and ``sigma`` [K].  ``kind``: "flux" the channel means,
        "eclipse" (band integral of F_p / band integral of F_star) (R_p / R_star)^2, "transit"
        the band-averaged transit depth weighted by the stellar flux.  The star is the Planet's
        ``stellar_spectrum``, else ``pi * B_star(T_star)``; the radii default to the Planet's.
        ``broadening`` (:class:`~frei_amd.broaden.Broadening`, K13) broadens the spectrum on the
        device first."""
        from .observe import observe
        return observe(instrument, kind, [self.planet], self.lam,
                       x=np.asarray(getattr(spectrum, "flux", spectrum), dtype=float),
                       data=data, sigma=sigma, R_p=R_p, R_star=R_star, broadening=broadening)

    def cross_correlate(self, cc, spectrum, kind="eclipse", R_p=None, R_star=None, offset=None,
                        broadening=None, keep=False, **kw):
        """``spectrum`` (the :class:`Spectrum` of emission_spectrum or transmission_spectrum)
        against high-resolution data over a grid of trial velocities (``cc``:
        :class:`~frei_amd.crosscorr.CrossCorrelator`, K12) ->
        :class:`~frei_amd.crosscorr.CrossCorrelation`.  ``kind``: "flux" the spectrum as it is,
        "eclipse" F_p / F_star (R_p / R_star)^2, "transit" minus the transit depth.  Star and
        radii as in :meth:`observe`; ``broadening`` broadens the spectrum (for "transit" minus
        the depth) on the device first.  ``keep=True`` (and any further keyword) goes to
        :meth:`~frei_amd.crosscorr.CrossCorrelator.correlate`: the sums stay on the device for
        :meth:`~frei_amd.stack.OrbitStack.stack` (K14)."""
        from .crosscorr import cross_correlate
        return cross_correlate(cc, kind, [self.planet], self.lam,
                               x=np.asarray(getattr(spectrum, "flux", spectrum), dtype=float),
                               R_p=R_p, R_star=R_star, offset=offset, broadening=broadening,
                               keep=keep, **kw)

    def emission_dashboard(self, *args, **kwargs):
        raise NotImplementedError("plotting is out of scope for the MI355X engine (SURVEY.md §2)")


def _post_engine(grid, dtaus):
    """The grid's engine and the dtaus argument for the device: None when ``dtaus`` is the
    array the last emission_spectrum returned (its device copy is used)."""
    eng = grid.engine()
    same = dtaus is getattr(grid, "_last_dtaus", None)
    return eng, (None if same else np.asarray(dtaus, dtype=float))


def effective_temperature_milne(grid, spec, dtaus, final_temps):
    """Photosphere temperature from Milne's tau ~ 2/3 (core.py:386-405).  The per-wavelength
    np.interp over layers runs on the GPU (frei_milne_pressure); the weighted mean and the
    final interpolation are O(n_lambda) host work, as in the reference."""
    if hasattr(grid, "col_weights"):
        raise NotImplementedError(
            "effective_temperature_milne on a KGrid: the Milne mean weights wavelengths, not the "
            "columns of a k-distribution (bin width x quadrature weight); use "
            "KGrid.effective_temperature_milne, or batched_k_spectra(..., post=True) for a batch")
    lam = np.asarray(grid.lam)
    p = np.asarray(grid.pressures)
    eng, d = _post_engine(grid, dtaus)
    pressure_milne = eng.milne_pressure(p, d)
    # weights: F_lambda -> lambda F_lambda (erg s^-1 cm^-2, astropy spectral_density)
    lam_flux = np.asarray(spec.flux) * (lam * UM)
    return np.interp(np.average(pressure_milne, weights=lam_flux), p[::-1],
                     np.asarray(final_temps)[::-1])


def contribution_function(grid, dtaus, final_temps):
    """Normalised contribution function of the final atmosphere (plot.py:63-79), computed
    on the GPU: array (n_layers, n_lambda), rows bottom-first like ``grid.pressures`` (the
    reference plots ``cf[::-1]``)."""
    eng, d = _post_engine(grid, dtaus)
    return eng.contribution(np.asarray(grid.pressures), np.asarray(final_temps), d)


def planck_temperature(lam_um, flux):
    """(trapezoid integral of ``flux`` over ``lam_um`` / sigma_SB)^(1/4), K."""
    lam_cm = np.asarray(lam_um) * UM
    f = np.asarray(flux)
    bol = np.sum(np.diff(lam_cm) * (f[1:] + f[:-1]) / 2.0)
    return (bol / SIGMA_SB) ** 0.25


def effective_temperature_planck(grid, spec):
    """Stefan-Boltzmann inversion of the bolometric flux (core.py:408-414)."""
    return planck_temperature(grid.lam, spec.flux)


def collapse_columns(x, weights):
    """[..., n_bins * n_g] -> [..., n_bins]: the g-average ``sum_q w_q x[b n_g + q]`` of a
    k-distribution's columns, q ascending, on the host."""
    x, w = np.asarray(x), np.asarray(weights, dtype=float)
    if x.shape[-1] % w.size:
        raise ValueError(f"{x.shape[-1]} columns are no whole number of bins of {w.size} points")
    x = x.reshape(x.shape[:-1] + (x.shape[-1] // w.size, w.size))
    out = np.zeros(x.shape[:-1], dtype=np.result_type(x.dtype, float))
    for q in range(w.size):
        out = out + w[q] * x[..., q]
    return out


def milne_on_columns(p_milne, flux, lam_um, weights, pressures, final_temps):
    """Milne's photosphere temperature on the columns of a k-distribution (K20):
    ``p_b = sum_q w_q p_milne[b n_g + q]`` (q ascending, as :func:`collapse_columns` sums), then
    the reference's formula on the bins (core.py:386-405): ``interp(average(p_b, weights =
    lam_b F_b))`` with ``flux`` = F_b the collapsed spectrum on the bin centres ``lam_um``."""
    p_b = collapse_columns(p_milne, weights)
    lam_flux = np.asarray(flux) * (np.asarray(lam_um) * UM)
    p = np.asarray(pressures)
    return np.interp(np.average(p_b, weights=lam_flux), p[::-1], np.asarray(final_temps)[::-1])


def effective_temperature(grid, spec, dtaus, final_temps):
    """Mean of the Milne and Stefan-Boltzmann estimates, K (core.py:417-439)."""
    return float(np.mean([effective_temperature_milne(grid, spec, dtaus, final_temps),
                          effective_temperature_planck(grid, spec)]))
