"""Correlated-k grids (K18): a :class:`KGrid` runs the engine on the columns of a
k-distribution instead of on wavelengths.

Per wavelength bin the cross-section is sorted into a monotone k(g), g the fraction of the
bin's points below k, and sampled at a few quadrature points g_q with weights w_q
(``frei_amd/csrc/frei_kdist.hip``; the definition is in ``include/frei_hip.h``).  Column
``b * n_g + q`` of a KGrid is bin b at g_q: it carries the bin centre's wavelength, Planck
function, Rayleigh cross-section and irradiation, the opacity k_b(g_q), and the weight
``Δλ_b w_q`` in the bolometric sums.  No kernel of the engine looks at a neighbouring column, so
such a column is an ordinary column to all of them.

The approximation: species are premixed at the table's (T, p) nodes (``CrossSection.mix``), k is
interpolated in (p, T) at fixed g, and the spectral order inside a bin is taken to be the same
in every layer (the layers' k are perfectly correlated).  With ``overlap="random"`` (K19) the
species are mixed from their own k-tables instead, their lines taken as uncorrelated
(:class:`~frei_amd.binning.KLibrary`); a new composition then re-mixes the small tables and
neither re-reads nor re-sorts a native cross-section (``KGrid.set_mix``).
"""
import numpy as np

from .binning import CrossSection, KLibrary, KTable, MixedKTable, bin_counts
from .constants import UM
from .core import F_TOA, Grid, Spectrum
from .emergent import gauss_angles
from .engine import Engine
from .units import value

__all__ = ["KGrid", "KTable", "KLibrary", "MixedKTable", "gauss_g"]


def gauss_g(n, split=None):
    """Quadrature points and weights (g, w) on (0, 1), sum(w) = 1: the ``n``-point
    Gauss-Legendre rule of :func:`~frei_amd.gauss_angles`, or with ``split=x`` (0 < x < 1, n
    even) n/2 points on (0, x) and n/2 on (x, 1) — more points where k(g) rises steeply, just
    below g = 1."""
    n = int(n)
    if split is None:
        return gauss_angles(n)
    x = float(split)
    if not 0.0 < x < 1.0:
        raise ValueError("gauss_g: split must lie in (0, 1)")
    if n < 2 or n % 2:
        raise ValueError("gauss_g: a split rule needs an even n >= 2")
    g, w = gauss_angles(n // 2)
    return np.concatenate([x * g, x + (1.0 - x) * g]), np.concatenate([x * w, (1.0 - x) * w])


class KGrid(Grid):
    """A :class:`~frei_amd.Grid` whose columns are the (bin, g-point) pairs of a k-distribution.

    ``wl_bins`` (µm, ascending) are the bin edges; ``g`` and ``weights`` the quadrature on
    (0, 1) (default ``gauss_g(n_g)``).  ``lam`` are the ``n_bins`` bin centres, so the collapsed
    spectra go through ``observe`` and ``cross_correlate`` as any Grid's; ``col_lam =
    repeat(lam, n_g)`` and ``col_weights = (Δλ_b cm) w_q`` are the per-column wavelengths and
    quadrature weights the engine gets.  The pressure and temperature arguments are Grid's."""

    def __init__(self, planet, wl_bins, g=None, weights=None, n_g=8, **grid_kw):
        wl_bins = np.asarray(value(wl_bins, "um"), dtype=float)
        if wl_bins.ndim != 1 or wl_bins.size < 4 or np.any(np.diff(wl_bins) <= 0):
            raise ValueError("wl_bins must be strictly ascending bin edges of at least 3 bins")
        if "lam" in grid_kw:
            raise ValueError("a KGrid's wavelengths are its bin centres: pass wl_bins, not lam")
        super().__init__(planet, lam=(wl_bins[:-1] + wl_bins[1:]) / 2, **grid_kw)
        self.wl_bins = wl_bins
        if g is None:
            if weights is not None:
                raise ValueError("weights without g: pass both or neither")
            g, weights = gauss_g(n_g)
        elif weights is None:
            raise ValueError("g without weights: pass both or neither")
        self.g = np.asarray(g, dtype=float)
        self.weights = np.asarray(weights, dtype=float)
        if self.g.ndim != 1 or self.g.shape != self.weights.shape:
            raise ValueError("g and weights must be 1-D arrays of one length")
        self.n_bins, self.n_g = self.lam.size, self.g.size
        self.col_lam = np.repeat(self.lam, self.n_g)
        self.col_weights = np.outer(np.diff(wl_bins) * UM, self.weights).ravel()
        self.klibrary = None

    def load_opacities(self, cross_sections=None, mix=None, mmr=None, temperatures=None,
                       pressures=None, chemistry=None, ktables=None, overlap="premix"):
        """Attach the k-tables of ``cross_sections`` ({name: CrossSection}).  One cross-section
        becomes a :class:`KTable` under its own name, with ``mmr`` (or ``chemistry``) as in
        Grid.load_opacities.  Several need ``mix`` — their mass mixing ratios at the sources' own
        nodes, broadcast to (n_src, n_T, n_p) — and become the one species ``"mix"`` with mixing
        ratio 1: the mixture is sorted, not the species.  The table's nodes are ``pressures``
        (default: the grid's layers, each taking its nearest source node as in Grid) x
        ``temperatures`` (default: the cross-section's own nodes, so that k is interpolated in T
        at fixed g).  A bin that holds no point of the cross-section's axis is refused.

        ``overlap="random"`` (K19) mixes the species from their own k-tables by random overlap
        with resort-and-rebin instead of premixing the native cross-sections: from
        ``cross_sections`` (each sorted once into a :class:`KLibrary` slot) or from
        ``ktables={name: array[n_p][n_T][n_bins][n_g]}`` on the nodes ``temperatures`` x
        ``pressures`` (default: the grid's layers).  ``mix`` is required; the library is kept as
        ``grid.klibrary`` and the one species ``"mix"`` has mixing ratio 1.  :meth:`set_mix`
        then changes the composition."""
        if overlap not in ("premix", "random"):
            raise ValueError(f"overlap must be 'premix' or 'random', not {overlap!r}")
        if overlap == "random":
            return self._load_random(cross_sections, ktables, mix, mmr, temperatures, pressures,
                                     chemistry)
        if ktables is not None:
            raise ValueError("ktables= holds no native cross-section to premix: pass "
                             "overlap='random'")
        if not cross_sections:
            raise ValueError("KGrid.load_opacities needs cross_sections={name: CrossSection}")
        xs = dict(cross_sections)
        if len(xs) > 1 and mix is None:
            raise ValueError(
                f"{len(xs)} cross-sections without mix=: the k(g) of several species do not add "
                "(that would treat their lines as perfectly correlated); pass mix= (their mass "
                "mixing ratios at the table nodes) and the mixture is sorted as one species")
        if mix is not None:
            if mmr is not None or chemistry is not None:
                raise ValueError("mix= already holds the mixing ratios: the species 'mix' has "
                                 "mixing ratio 1, pass neither mmr nor chemistry")
            xs = {"mix": CrossSection.mix(list(xs.values()), mix, device=self.device)}
            mmr = np.ones((1, self.pressures.size))
        if mmr is not None and chemistry is not None:
            raise ValueError("pass either mmr or a chemistry provider, not both")
        p = self.pressures if pressures is None else value(pressures, "bar")
        tables = {name: KTable(x, self.wl_bins, self.g,
                               x.temperature if temperatures is None else temperatures, p,
                               self.device)
                  for name, x in xs.items()}
        for name, tab in tables.items():
            bad = np.nonzero(tab.counts == 0)[0]
            if bad.size:
                shown = ", ".join(str(k) for k in bad[:8]) + (", ..." if bad.size > 8 else "")
                raise ValueError(f"cross-section {name!r} does not cover the grid: bins {shown} "
                                 "hold no point")
        self.opacities = tables
        self.mmr = mmr
        self.chemistry = chemistry
        self._close_engine()
        return self.opacities

    def _load_random(self, cross_sections, ktables, mix, mmr, temperatures, pressures, chemistry):
        if bool(cross_sections) == bool(ktables):
            raise ValueError("overlap='random' needs either cross_sections={name: CrossSection} "
                             "or ktables={name: array}")
        if mix is None:
            raise ValueError("overlap='random' needs mix=: the species' mass mixing ratios at "
                             "the table nodes, (n_src, n_T, n_p)")
        if mmr is not None or chemistry is not None:
            raise ValueError("mix= already holds the mixing ratios: the species 'mix' has "
                             "mixing ratio 1, pass neither mmr nor chemistry")
        p = self.pressures if pressures is None else value(pressures, "bar")
        if ktables:
            if temperatures is None:
                raise ValueError("ktables= needs temperatures=: the tables' T nodes")
            tables = dict(ktables)
        else:
            tables = dict(cross_sections)
            if temperatures is None:
                temperatures = next(iter(tables.values())).temperature
            for name, x in tables.items():
                bad = np.nonzero(bin_counts(x.wavelength, self.wl_bins) == 0)[0]
                if bad.size:
                    shown = ", ".join(str(k) for k in bad[:8]) + (", ..." if bad.size > 8 else "")
                    raise ValueError(f"cross-section {name!r} does not cover the grid: bins "
                                     f"{shown} hold no point")
        lib = KLibrary(tables, self.wl_bins, self.g, self.weights, temperatures, p, self.device)
        table = lib.table(mix)
        if self.klibrary is not None:
            self.klibrary.release()
        self.klibrary = lib
        self.opacities = {"mix": table}
        self.mmr = np.ones((1, self.pressures.size))
        self.chemistry = None
        self._close_engine()
        return self.opacities

    def set_mix(self, mix):
        """A new composition of the kept library (``load_opacities(..., overlap="random")``): the
        species' k-tables are re-mixed on the device when the engine is next built; no native
        cross-section is read or sorted again.  Closes the engine."""
        if self.klibrary is None:
            raise ValueError("set_mix needs the library load_opacities(..., overlap='random') "
                             "keeps")
        self.opacities = {"mix": self.klibrary.table(mix)}
        self._close_engine()
        return self.opacities

    def engine(self):
        if self._engine is None:
            pl = self.planet
            ft = F_TOA(self.lam, T_star=pl.T_star, a_rstar=pl.a_rstar,
                       F_star=getattr(pl, "stellar_spectrum", None))
            self._engine = Engine(self.col_lam, self.pressures, self.opacities, g=pl.g,
                                  m_bar=pl.m_bar, F_toa=np.repeat(ft, self.n_g), mmr=self.mmr,
                                  chemistry=self.chemistry, device=self.device,
                                  quad_weights=self.col_weights)
        return self._engine

    def collapse(self, x):
        """[..., n_bins * n_g] -> [..., n_bins]: the g-average ``sum_q w_q x[b n_g + q]``, q
        ascending, on the host — the band mean of a result that is linear in the column."""
        x = np.asarray(x)
        if x.shape[-1] != self.n_bins * self.n_g:
            raise ValueError(f"collapse needs {self.n_bins * self.n_g} columns, got {x.shape[-1]}")
        x = x.reshape(x.shape[:-1] + (self.n_bins, self.n_g))
        out = np.zeros(x.shape[:-1], dtype=np.result_type(x.dtype, float))
        for q in range(self.n_g):
            out = out + self.weights[q] * x[..., q]
        return out

    def _collapsed(self, spec):
        flux = spec.flux
        unit = getattr(flux, "unit", None)
        out = self.collapse(getattr(flux, "value", flux))
        return Spectrum(out if unit is None else out * unit, self.lam)

    def emission_spectrum(self, n_timesteps=1, n_zero_crossings=2, convergence_dT=3.0):
        """Grid.emission_spectrum on the k-distribution's columns -> (spectrum, final_temps,
        temperature_history, dtaus): the spectrum is the band mean on ``lam`` (collapsed);
        ``dtaus`` stays per column, [n_layers][n_bins * n_g]."""
        spec, T, th, dtaus = super().emission_spectrum(n_timesteps, n_zero_crossings,
                                                       convergence_dT)
        return self._collapsed(spec), T, th, dtaus

    def transmission_spectrum(self, *args, **kw):
        """Grid.transmission_spectrum, collapsed: the band-mean transit depth on ``lam`` (the
        depth is linear in the column's transmission)."""
        return self._collapsed(super().transmission_spectrum(*args, **kw))

    def emergent_spectrum(self, final_temps, dtaus=None, mu=None, weights=None,
                          want_intensity=False):
        """Grid.emergent_spectrum, the flux collapsed onto ``lam``; intensities stay per
        column, [n_mu][n_bins * n_g]."""
        out = super().emergent_spectrum(final_temps, dtaus=dtaus, mu=mu, weights=weights,
                                        want_intensity=want_intensity)
        if mu is not None and weights is None:
            return out
        if want_intensity:
            return self._collapsed(out[0]), out[1]
        return self._collapsed(out)

    def contribution_function(self, final_temps, dtaus=None):
        """Grid.contribution_function per column, [n_layers][n_bins * n_g] (it is normalised
        per column, so it has no band mean)."""
        return super().contribution_function(final_temps, dtaus)
