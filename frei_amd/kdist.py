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

from .batch import BatchEngine, BatchRecord, BatchResult
from .binning import CrossSection, KLibrary, KTable, MixedKTable, MixedKTables, bin_counts
from .constants import UM
from .core import (F_TOA, Grid, Spectrum, _post_engine, collapse_columns,
                   effective_temperature_planck, milne_on_columns)
from .emergent import gauss_angles
from .engine import Engine
from .units import scalar, value

__all__ = ["KGrid", "KTable", "KLibrary", "MixedKTable", "MixedKTables", "gauss_g",
           "batched_k_spectra", "KBatchResult"]


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
        self._owns_library = False
        self.mix = None

    def load_opacities(self, cross_sections=None, mix=None, mmr=None, temperatures=None,
                       pressures=None, chemistry=None, ktables=None, overlap="premix",
                       klibrary=None):
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
        then changes the composition.

        ``klibrary=`` (K20) attaches an existing :class:`KLibrary` instead, with ``mix`` this
        grid's composition: it must have the grid's ``wl_bins``, ``g``, ``weights`` and device,
        and the layers must sit on its pressure nodes.  Several KGrids can share one library
        object (:func:`batched_k_spectra` then runs them as one batch); the grid does not own
        it.  The composition is kept as ``grid.mix``, as ``overlap="random"`` keeps it."""
        if klibrary is not None:
            return self._attach_library(klibrary, cross_sections, ktables, mix, mmr, chemistry)
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
        return self._keep_library(lib, lib.table(mix), mix, owned=True)

    def _keep_library(self, lib, table, mix, owned):
        if self.klibrary is not None and self.klibrary is not lib and self._owns_library:
            self.klibrary.release()
        self.klibrary, self._owns_library = lib, owned
        self.mix = np.array(mix, dtype=float)
        self.opacities = {"mix": table}
        self.mmr = np.ones((1, self.pressures.size))
        self.chemistry = None
        self._close_engine()
        return self.opacities

    def _attach_library(self, lib, cross_sections, ktables, mix, mmr, chemistry):
        if cross_sections or ktables:
            raise ValueError("klibrary= already holds the species' k-tables: pass neither "
                             "cross_sections nor ktables")
        if mix is None:
            raise ValueError("klibrary= needs mix=: the species' mass mixing ratios at the "
                             "library's nodes, (n_src, n_T, n_p)")
        if mmr is not None or chemistry is not None:
            raise ValueError("mix= already holds the mixing ratios: the species 'mix' has "
                             "mixing ratio 1, pass neither mmr nor chemistry")
        if not isinstance(lib, KLibrary):
            raise ValueError("klibrary= must be a KLibrary")
        for name in ("wl_bins", "g", "weights"):
            if not np.array_equal(getattr(lib, name), getattr(self, name)):
                raise ValueError(f"the library's {name} are not the grid's")
        if lib.device != self.device:
            raise ValueError(f"the library lives on device {lib.device}, the grid on device "
                             f"{self.device}")
        off = [l for l, p in enumerate(self.pressures) if p not in lib.pressure]
        if off:
            raise ValueError(f"layer {off[0]} (p = {self.pressures[off[0]]:.6g} bar) does not sit "
                             "on a pressure node of the library")
        return self._keep_library(lib, lib.table(mix), mix, owned=False)

    def set_mix(self, mix):
        """A new composition of the kept library (``load_opacities(..., overlap="random")`` or
        ``klibrary=``): the species' k-tables are re-mixed on the device when the engine is next
        built; no native cross-section is read or sorted again.  Closes the engine."""
        if self.klibrary is None:
            raise ValueError("set_mix needs the library load_opacities(..., overlap='random') "
                             "keeps")
        self.opacities = {"mix": self.klibrary.table(mix)}
        self.mix = np.array(mix, dtype=float)
        self._close_engine()
        return self.opacities

    def effective_temperature_milne(self, spec, dtaus, final_temps):
        """Milne's photosphere temperature on the k-distribution's columns (K20):
        ``p_b = sum_q w_q p_milne[b n_g + q]`` from the device's per-column Milne pressures, then
        the reference's formula on the bins with ``spec`` the collapsed spectrum
        (:func:`frei_amd.core.milne_on_columns`)."""
        eng, d = _post_engine(self, dtaus)
        p = np.asarray(self.pressures)
        return milne_on_columns(eng.milne_pressure(p, d), getattr(spec, "flux", spec), self.lam,
                                self.weights, p, final_temps)

    def effective_temperature(self, spec, dtaus, final_temps):
        """Mean of :meth:`effective_temperature_milne` and the Stefan-Boltzmann estimate of the
        collapsed spectrum, K."""
        return float(np.mean([self.effective_temperature_milne(spec, dtaus, final_temps),
                              effective_temperature_planck(self, spec)]))

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
        return collapse_columns(x, self.weights)

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


# ------------------------------------------------------------------------------ batches (K20)
NO_LINES = ("a k-distribution has no line positions: {} needs spectra on a wavelength axis "
            "(run a Grid at the native resolution)")


class KBatchResult(BatchResult):
    """The :class:`~frei_amd.batch.BatchRecord` list of ``batched_k_spectra(..., post=True)``:
    a :class:`~frei_amd.batch.BatchResult` whose engine runs on the columns of a
    k-distribution.  Each record's spectrum is collapsed onto ``lam`` (the bin centres);
    ``T_milne`` follows :func:`frei_amd.core.milne_on_columns` and ``T_planck`` the collapsed
    spectrum.  ``dtaus(m)``, ``contribution(m)`` and the intensities of :meth:`emergent` stay per
    column.  :meth:`set_mix` and :meth:`rerun` change compositions and run again on the same
    context (a batch of grids that share a :class:`KLibrary`)."""

    def __init__(self, records, engine, planets, lam, weights, run_args=None):
        super().__init__(records, engine, planets)
        self.lam = np.asarray(lam, dtype=float)
        self.weights = np.asarray(weights, dtype=float)
        self.n_g = self.weights.size
        self.run_args = run_args
        self._instruments = {}

    def collapse(self, x):
        """[..., n_bins * n_g] -> [..., n_bins]: ``sum_q w_q x[b n_g + q]``, q ascending."""
        return collapse_columns(x, self.weights)

    def transmission(self, R_p=None, R_star=None, P_ref=None):
        """Every atmosphere's band-mean transit depth on ``lam``, [n_atm][n_bins]:
        BatchResult.transmission per column, collapsed."""
        return self.collapse(super().transmission(R_p=R_p, R_star=R_star, P_ref=P_ref))

    def emergent(self, mu=None, weights=None, want_intensity=False):
        """BatchResult.emergent with the flux collapsed onto ``lam``; the intensities stay per
        column, [n_atm][n_mu][n_bins * n_g]."""
        out = super().emergent(mu=mu, weights=weights, want_intensity=want_intensity)
        if mu is not None and weights is None:
            return out
        if want_intensity:
            return self.collapse(out[0]), out[1]
        return self.collapse(out)

    def column_instrument(self, instrument):
        """``instrument`` (on ``lam``) on the engine's columns (``Instrument.for_columns``),
        built once per instrument."""
        if instrument.n_lam != self.lam.size:
            raise ValueError(f"the instrument's axis has {instrument.n_lam} points, the bins' "
                             f"{self.lam.size}: it must be an Instrument on lam")
        key = id(instrument)
        if key not in self._instruments:
            self._instruments[key] = (instrument,
                                      instrument.for_columns(self.n_g, self.weights))
        return self._instruments[key][1]

    def observe(self, instrument, kind="eclipse", depth=None, weighting=None, data=None,
                sigma=None, R_p=None, R_star=None, broadening=None):
        """BatchResult.observe for an ``instrument`` on ``lam``: it runs on the columns on the
        device through ``Instrument.for_columns``, the stars' spectra (on ``lam``) repeated onto
        the columns, so the collapsed spectrum never has to exist there.  ``depth`` for
        ``kind="transit"`` is per column, [n_atm][n_bins * n_g] (default: the engine's)."""
        from .observe import eclipse_scale, star_library
        from ._device import unknown_kind
        if broadening is not None:
            raise ValueError(NO_LINES.format("broadening="))
        inst = self.column_instrument(instrument)
        A, eng = len(self), self.engine
        planets = self.planets if self.planets is not None else [None] * A
        kw = dict(data=data, sigma=sigma)

        def columns(lib):
            return np.repeat(lib, self.n_g, axis=-1)
        if kind == "flux":
            return inst.apply(None, engine=eng, **kw)
        if kind == "eclipse":
            scale = eclipse_scale(planets, R_p, R_star)
            lib, select = star_library(planets, self.lam)
            return inst.apply(None, den=columns(lib), select=select, scale=scale, engine=eng, **kw)
        if kind != "transit":
            raise unknown_kind(kind)
        if depth is None:
            depth = BatchResult.transmission(self, R_p=R_p, R_star=R_star)
        if weighting is None:
            weighting = "stellar" if all(pl is not None for pl in planets) else "flat"
        if weighting == "flat":
            return inst.apply(depth, **kw)
        if weighting != "stellar":
            raise ValueError(f"unknown weighting {weighting!r}: 'stellar' or 'flat'")
        lib, select = star_library(planets, self.lam)
        return inst.apply(depth, num=columns(lib), den=columns(lib), select=select, **kw)

    def cross_correlate(self, *args, **kw):
        raise ValueError(NO_LINES.format("cross_correlate"))

    def phase_curve(self, *args, **kw):
        raise ValueError("phase curves on the columns of a k-distribution are not implemented: "
                         "integrate the collapsed spectra of emergent() on the host")

    def model_grid(self, axes, broadening=None):
        """A :class:`~frei_amd.modelgrid.ModelGrid` on ``lam`` whose nodes are the records'
        collapsed spectra (uploaded from the host), atmosphere ``m`` the node of C-order index
        ``m`` over ``axes``."""
        from .modelgrid import ModelGrid
        if broadening is not None:
            raise ValueError(NO_LINES.format("broadening="))
        nodes = np.array([np.asarray(r.spectrum.flux, dtype=float) for r in self])
        return ModelGrid(axes, self.lam, spectra=nodes, device=self.engine.device)

    def set_mix(self, x, atm=None):
        """New compositions ``x`` (n, n_src, n_T, n_p) for the atmospheres ``atm`` (default
        all), re-mixed in place on the device (BatchEngine.set_mix); :meth:`rerun` then runs
        the batch again without a new context."""
        self.engine.set_mix(x, atm)

    def rerun(self):
        """Run the batch again with the arguments of the first run and replace the records."""
        if self.run_args is None:
            raise ValueError("this result holds no run to repeat")
        self[:] = k_records(self.engine, self.lam, self.weights, *self.run_args)
        self._cf = None
        return self


def k_records(eng, lam, weights, T_init, n_timesteps, n_zero_crossings, convergence_dT, alpha):
    """One run of a batch on k-columns with its post-processing -> the records, spectra
    collapsed onto ``lam``."""
    out = eng.run(T_init, n_timesteps, n_zero_crossings, convergence_dT, alpha, want_hist=True,
                  keep_dtaus=True)
    te = eng.post()
    flux = collapse_columns(out["spectra"], weights)
    return [BatchRecord(Spectrum(flux[m], lam), out["final_T"][m], int(out["n_iter"][m]),
                        out["temp_hist"][m], float(te["T_eff"][m]), float(te["T_milne"][m]),
                        float(te["T_planck"][m])) for m in range(eng.n_atm)]


def check_k_batch(grids):
    """The checks of :func:`batched_k_spectra`, all before any device use -> "library" (the
    grids share one KLibrary, each with its own mix) or "shared" (one opacity dict)."""
    grids = list(grids)
    if not grids:
        raise ValueError("batched_k_spectra needs at least one KGrid")
    for k, gr in enumerate(grids):
        if not isinstance(gr, KGrid):
            raise ValueError(f"grid {k} is not a KGrid: batched_emission_spectra runs Grids")
        if gr.opacities is None:
            raise ValueError(f"grid {k} has no opacities: call load_opacities first")
        if gr.chemistry is not None:
            raise ValueError(f"grid {k} steps a chemistry provider: a batch cannot")
    g0 = grids[0]
    for k, gr in enumerate(grids[1:], 1):
        for name in ("wl_bins", "g", "weights", "pressures"):
            if not np.array_equal(getattr(gr, name), getattr(g0, name)):
                raise ValueError(f"grid {k} does not share grid 0's {name}")
        if gr.planet.alpha != g0.planet.alpha or gr.planet.m_bar != g0.planet.m_bar:
            raise ValueError(f"grid {k} does not share grid 0's alpha and m_bar")
        if gr.device != g0.device:
            raise ValueError(f"grid {k} lives on another device than grid 0")
    if all(gr.opacities is g0.opacities for gr in grids):
        return "shared"
    mixed = [isinstance(gr.opacities.get("mix"), MixedKTable) and len(gr.opacities) == 1
             for gr in grids]
    if all(mixed):
        for k, gr in enumerate(grids[1:], 1):
            if gr.klibrary is not g0.klibrary:
                raise ValueError(f"grid {k} does not share grid 0's klibrary object: load every "
                                 "grid with load_opacities(klibrary=lib, mix=...)")
        return "library"
    raise ValueError("batched KGrids must share one klibrary object (each with its own mix) or "
                     "one opacity dict (a KTable or a premix)")


def batched_k_spectra(grids, n_timesteps=1, n_zero_crossings=2, convergence_dT=3.0, device=0,
                      post=False):
    """KGrid.emission_spectrum for a list of :class:`KGrid` as one batched device run (K20).
    The grids share ``wl_bins``, ``g``, ``weights``, pressures, ``alpha`` and ``m_bar``, and
    either (a) one ``klibrary`` object, each grid with its own ``mix`` — every atmosphere then
    gets its own random-overlap mixture, mixed on the device into the batch's per-atmosphere
    tables — or (b) one opacity dict (a :class:`KTable` or a premix), the shared-table batch on
    the columns.  Anything else is a ValueError naming the condition.  Returns
    [(Spectrum, final_T, n_iter)] in the order of ``grids``, the spectra collapsed onto ``lam``;
    with ``post=True`` a :class:`KBatchResult`."""
    from .batch import grid_mixing_ratios
    grids = list(grids)
    route = check_k_batch(grids)
    g0, pl = grids[0], grids[0].planet
    if g0.device != device:
        raise ValueError(f"the grids live on device {g0.device}, not device {device}")
    if route == "library":
        x = np.array([gr.opacities["mix"].x.transpose(0, 2, 1) for gr in grids])
        opacities, mmr = {"mix": g0.klibrary.tables(x)}, None
    else:
        opacities, mmr = g0.opacities, grid_mixing_ratios(grids, list(g0.opacities))
    ft = np.array([np.repeat(F_TOA(g0.lam, T_star=gr.planet.T_star, a_rstar=gr.planet.a_rstar,
                                   F_star=getattr(gr.planet, "stellar_spectrum", None)), g0.n_g)
                   for gr in grids])
    if all(np.array_equal(f, ft[0]) for f in ft[1:]):
        ft = ft[0]
    eng = BatchEngine(g0.col_lam, g0.pressures, opacities, [gr.planet.g for gr in grids],
                      mmr=mmr, m_bar=pl.m_bar, F_toa=ft, device=device,
                      quad_weights=g0.col_weights, k_weights=g0.weights)
    args = (np.array([gr.init_temperatures for gr in grids]), n_timesteps, n_zero_crossings,
            scalar(convergence_dT, "K"), pl.alpha)
    if post:
        try:
            records = k_records(eng, g0.lam, g0.weights, *args)
        except BaseException:
            eng.close()
            raise
        return KBatchResult(records, eng, [gr.planet for gr in grids], g0.lam, g0.weights, args)
    try:
        out = eng.run(*args)
    finally:
        eng.close()
    flux = collapse_columns(out["spectra"], g0.weights)
    return [(Spectrum(flux[m], g0.lam), out["final_T"][m], int(out["n_iter"][m]))
            for m in range(len(grids))]
