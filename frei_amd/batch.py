"""Batched atmospheres on one GPU (BASELINE config C5: grid sweeps).

The reference has no batch API: a grid sweep is a loop over independent ``Grid`` objects,
each running ``emission_spectrum`` (core.py:109-338).  :class:`BatchEngine` runs such a loop
as one device context (``frei_ctx_create_batch``): the atmospheres share the wavelength and
pressure grids and the opacity tables; each has its own temperatures, gravity and mixing
ratios.  Every sweep is one launch over (wavelength block, atmosphere); the per-atmosphere
species contraction is one dense product per layer on fp64 MFMA (K7).  Across GPUs the
atmospheres are sharded with no exchange.
"""
import collections
import ctypes

import numpy as np

from . import _native as N
from .binning import MixedKTables
from .chemistry import ChemistryTable, chemistry
from .constants import BAR, C, H, K_B, M_BAR_DEFAULT, SIGMA_SB, UM
from .emergent import emergent_call, pick
from .engine import EMIT, ContextBase, f_toa, planck_prefactor, quadrature_weights
from .opacity import sigma_scattering
from .transit import default_radius, level_radii, transit_call
from .units import scalar, value

__all__ = ["BatchEngine", "BatchRecord", "BatchResult", "batched_emission_spectra"]


def chemistry_tables(mmr, n_atm):
    """``mmr`` as chemistry tables of a batch: None when it holds no :class:`ChemistryTable`,
    else ``(tables, atm_tab)`` — the distinct tables (by identity, in order of first use) and
    the table index of every atmosphere.  One table serves every atmosphere; a sequence names
    one per atmosphere.  Tables and arrays cannot be mixed."""
    if isinstance(mmr, ChemistryTable):
        return [mmr], np.zeros(n_atm, dtype=np.int32)
    if not isinstance(mmr, (list, tuple)) or not any(isinstance(x, ChemistryTable) for x in mmr):
        return None
    if not all(isinstance(x, ChemistryTable) for x in mmr):
        raise ValueError("a batch takes ChemistryTables or mixing-ratio arrays, not a mix of both")
    if len(mmr) != n_atm:
        raise ValueError(f"{len(mmr)} chemistry tables for {n_atm} atmospheres")
    tables, atm_tab = [], np.empty(n_atm, dtype=np.int32)
    for m, t in enumerate(mmr):
        k = next((i for i, u in enumerate(tables) if u is t), len(tables))
        if k == len(tables):
            tables.append(t)
        atm_tab[m] = k
    return tables, atm_tab


def check_chemistry_nodes(tables):
    """ValueError unless the chemistry tables share their nodes: a batch interpolates every
    table on one (T, p) grid."""
    t0 = tables[0]
    for t in tables[1:]:
        if not (np.array_equal(t.temperature, t0.temperature) and
                np.array_equal(t.pressure, t0.pressure)):
            raise ValueError("the chemistry tables of a batch must share their temperature and "
                             "pressure nodes")


def stack_chemistry(tables, names):
    """values [n_tab][n_species][n_T][n_p] of chemistry tables on shared nodes."""
    check_chemistry_nodes(tables)
    return N.f64(np.array([t.array(names) for t in tables]))


def check_kmix(opacities, mmr, n_atm, n_lam, n_layers, device):
    """The :class:`~frei_amd.binning.MixedKTables` of a k-mix batch (K20), or None when
    ``opacities`` holds none; every misuse is a ValueError before any device call."""
    mixed = [k for k, t in opacities.items() if isinstance(t, MixedKTables)]
    if not mixed:
        return None
    if len(opacities) != 1:
        others = [k for k in opacities if k not in mixed]
        raise ValueError(f"a k-mix batch has the one species {mixed[0]!r}: the k(g) of several "
                         f"species do not add, so {others or mixed[1:]} cannot stand beside it "
                         "(put every species into the KLibrary)")
    tabs = opacities[mixed[0]]
    if tabs.n_comp != n_atm:
        raise ValueError(f"{tabs.n_comp} compositions for n_atm = {n_atm} atmospheres")
    if tabs.wavelength.size != n_lam:
        raise ValueError("k-table columns (n_bins * n_g) must match the grid's columns")
    if tabs.device != device:
        raise ValueError(f"the k-table library lives on device {tabs.device}, the engine on "
                         f"device {device}")
    if mmr is not None:
        if isinstance(mmr, (ChemistryTable, list, tuple)) and chemistry_tables(mmr, n_atm):
            raise ValueError("a k-mix batch takes no chemistry tables: the compositions hold "
                             "the mixing ratios")
        m = np.asarray(mmr, dtype=float)
        try:
            np.broadcast_to(m, (n_atm, 1, n_layers))
        except ValueError:
            raise ValueError(f"mmr of shape {m.shape} does not broadcast to (n_atm, 1, "
                             "n_layers)") from None
        if not np.all(m == 1.0):
            raise ValueError("mmr of a k-mix batch must be None or all ones: the compositions "
                             "hold the mixing ratios")
    return tabs


class BatchEngine(ContextBase):
    """``n_atm`` atmospheres on ``device``: ``g`` [n_atm] (cm s^-2), ``mmr``
    [n_atm][n_species][n_layers], ``F_toa`` [n_lam] shared or [n_atm][n_lam] per atmosphere;
    wavelengths, pressures (bar, descending), opacities and m_bar are shared (as in a grid of
    Planets that differ in T, g, metallicity and irradiation).

    ``mmr`` may also be T-dependent chemistry: one :class:`~frei_amd.chemistry.ChemistryTable`
    for every atmosphere, or a sequence of ``n_atm`` of them on shared nodes (a metallicity axis:
    one equilibrium table per [M/H]; the same object may serve several atmospheres and is
    uploaded once).  The device re-interpolates each atmosphere's table at its own layer
    temperatures every sweep (frei_set_chemistry_batch) and the species sum stays in the sweep.
    Consecutive atmospheres in the same T brackets share table rows in the tiled sweep
    (``FREI_ATM_TILE``), so order such a batch by temperature.

    ``quad_weights`` (cm, one per column) replaces the trapezoid weights of the bolometric sums, as
    in :class:`~frei_amd.engine.Engine` (a k-distribution's columns, ``KGrid.col_weights``).

    A k-mix batch (K20): ``opacities = {"mix": MixedKTables}`` (``KLibrary.tables(x)``, one
    composition per atmosphere) and nothing beside it; ``mmr`` is None or all ones.  The k(g) of
    several species do not add, so each atmosphere's table is its own random-overlap mixture,
    mixed on the device into the per-atmosphere tables the sweeps read
    (frei_set_table_kmix_batch).  :meth:`set_mix` re-mixes all or some atmospheres in place and
    :meth:`table` reads one atmosphere's table back.

    ``k_weights`` (the quadrature weights w_q of a k-distribution whose columns ``b * n_g + q``
    the engine runs on, ``KGrid.weights``) makes :meth:`post` finish on the bins: the Milne
    pressure of bin b is ``sum_q w_q p_milne[b n_g + q]`` and the Milne mean weights the bins by
    ``lam_b F_b`` of the collapsed spectrum (``frei_amd.core.milne_on_columns``)."""

    def __init__(self, lam_um, p_bar, opacities, g, mmr=None, m_bar=M_BAR_DEFAULT, F_toa=None,
                 device=0, quad_weights=None, k_weights=None):
        lib = N.lib()
        self.lam_um = np.asarray(value(lam_um, "um"), dtype=float)
        self.p_bar = np.asarray(value(p_bar, "bar"), dtype=float)
        self.g = N.f64(np.atleast_1d(np.asarray(g, dtype=float)))
        self.n_atm = self.g.size
        self.k_weights = None if k_weights is None else N.f64(np.atleast_1d(k_weights))
        if self.k_weights is not None and (self.k_weights.ndim != 1 or
                                           self.lam_um.size % self.k_weights.size):
            raise ValueError(f"{self.lam_um.size} columns are no whole number of bins of "
                             f"{self.k_weights.size} quadrature points")
        self.kmix = check_kmix(opacities, mmr, self.n_atm, self.lam_um.size, self.p_bar.size,
                               device)
        self.m_bar = scalar(m_bar, "g")
        self.names = list(opacities)
        self.n_layers = self.p_bar.size
        self.n_lam = self.lam_um.size
        self.device = device
        lam_cm = self.lam_um * UM
        c1 = N.f64(planck_prefactor(lam_cm))
        lk = N.f64(lam_cm * K_B)
        sig = N.f64(sigma_scattering(self.lam_um, self.m_bar))
        ft = N.f64(f_toa(self.lam_um) if F_toa is None else value(F_toa, "erg / (s cm3)"))
        ft_atm = None
        if ft.ndim == 2:     # one F_TOA per atmosphere (planets around different stars)
            ft_atm = N.f64(np.broadcast_to(ft, (self.n_atm, self.n_lam)))
            ft = N.f64(ft_atm[0])
        wtr = N.f64(quadrature_weights(lam_cm, quad_weights))
        p_cgs = N.f64(self.p_bar * BAR)
        ctx = ctypes.c_void_p()
        N.check(lib.frei_ctx_create_batch(ctypes.byref(ctx), device, self.n_layers, self.n_lam,
                                          len(self.names), self.n_atm))
        self._ctx = ctx
        N.check(lib.frei_set_grid(ctx, N.dptr(c1), N.dptr(lk), N.dptr(sig), N.dptr(ft),
                                  N.dptr(wtr), N.dptr(p_cgs), float(self.g[0]), self.m_bar))
        if self.n_atm > 1:
            N.check(lib.frei_set_gravity(ctx, N.dptr(self.g)))
            if ft_atm is not None:
                N.check(lib.frei_set_ftoa_batch(ctx, N.dptr(ft_atm)))
        self.lo = 0  # the whole wavelength grid
        # tables: the single-atmosphere engine's upload paths (shared by every atmosphere)
        try:
            if self.kmix is not None:   # one mixed table per atmosphere (K20)
                N.check(lib.frei_set_table_kmix_batch(ctx, self.kmix.library.handle(),
                                                      N.dptr(self.kmix.x), self.lo))
            else:
                for s, name in enumerate(self.names):
                    self._set_table(s, opacities[name], slice(0, self.n_lam))
        except BaseException:
            self.close()
            raise
        try:
            chem = chemistry_tables(mmr, self.n_atm)
            if self.kmix is not None:
                mmr = np.ones((1, self.n_layers))
            elif mmr is None or chem is not None:
                T0 = np.full(self.n_layers, 1000.0)
                mm = chemistry(T0, self.p_bar, self.names, m_bar=self.m_bar)
                mmr = np.array([mm[nm] for nm in self.names])
            self.mmr = N.f64(np.broadcast_to(np.asarray(mmr, dtype=float),
                                             (self.n_atm, len(self.names), self.n_layers)))
            N.check(lib.frei_set_mmr(ctx, N.dptr(self.mmr)))
            self.chemistry = None
            if chem is not None:   # T-dependent chemistry, re-evaluated on the device every sweep
                self.set_chemistry(*chem)
        except BaseException:
            self.close()
            raise

    def set_chemistry(self, tables, atm_tab=None):
        """Chemistry tables of the batch (frei_set_chemistry_batch): ``tables`` a list of
        :class:`~frei_amd.chemistry.ChemistryTable` on shared nodes, atmosphere m reads
        ``tables[atm_tab[m]]`` (default: table 0).  ``tables=None`` returns to the fixed
        mixing ratios and the contracted path."""
        lib = N.lib()
        if tables is None:
            N.check(lib.frei_set_chemistry_batch(self._ctx, None, 0, None, None, 0, None, 0))
            self.chemistry = None
            return
        tables = list(tables)
        atm = np.ascontiguousarray(np.zeros(self.n_atm) if atm_tab is None else atm_tab,
                                   dtype=np.int32)
        if atm.shape != (self.n_atm,):
            raise ValueError(f"atm_tab must have {self.n_atm} entries")
        v = stack_chemistry(tables, self.names)
        t0 = tables[0]
        N.check(lib.frei_set_chemistry_batch(
            self._ctx, N.dptr(v), len(tables), atm.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            N.dptr(N.f64(t0.temperature)), t0.temperature.size, N.dptr(N.f64(t0.pressure * BAR)),
            t0.pressure.size))
        self.chemistry = (tables, atm)

    def set_mix(self, x, atm=None):
        """New compositions of a k-mix batch, re-mixed in place on the device
        (frei_kmix_batch_update; no new context, no metadata rebuild): ``x`` (n, n_src, n_T,
        n_p) for the atmospheres ``atm`` (indices, in any order; default all ``n_atm``).  The
        other atmospheres' tables keep their bits."""
        if self.kmix is None:
            raise ValueError("set_mix needs a k-mix batch: BatchEngine(..., {'mix': "
                             "KLibrary.tables(x)}, ...)")
        atm = np.arange(self.n_atm) if atm is None else np.atleast_1d(np.asarray(atm, dtype=int))
        new = MixedKTables(self.kmix.library, x)
        if atm.ndim != 1 or new.n_comp != atm.size:
            raise ValueError(f"{new.n_comp} compositions for {atm.size} atmospheres")
        bad = atm[(atm < 0) | (atm >= self.n_atm)]
        if bad.size:
            raise ValueError(f"atmosphere {bad[0]} lies outside [0, n_atm = {self.n_atm})")
        lib = N.lib()
        k = 0
        while k < atm.size:            # one call per run of consecutive atmospheres
            e = k + 1
            while e < atm.size and atm[e] == atm[e - 1] + 1:
                e += 1
            N.check(lib.frei_kmix_batch_update(self._ctx, int(atm[k]), e - k,
                                               N.dptr(N.f64(new.x[k:e]))))
            self.kmix.x[atm[k:e]] = new.x[k:e]
            k = e

    def table(self, m):
        """Atmosphere ``m``'s table of a k-mix batch as the sweeps read it, (n_p, n_T, n_lam) on
        the library's nodes in their own order (frei_get_table_batch)."""
        if self.kmix is None:
            raise ValueError("table needs a k-mix batch: BatchEngine(..., {'mix': "
                             "KLibrary.tables(x)}, ...)")
        nd = self.kmix
        out = np.empty((nd.pressure.size, nd.temperature.size, self.n_lam))
        N.check(N.lib().frei_get_table_batch(self._ctx, int(m), N.dptr(out)))
        return out

    def run(self, T_init, n_timesteps=1, n_zero_crossings=2, convergence_dT=3.0, alpha=1.0,
            want_hist=False, keep_dtaus=False):
        """Every atmosphere's emission_spectrum (core.py:233-338) -> dict(spectra [n_atm]
        [n_lam], final_T [n_atm][n_layers], n_iter [n_atm]).  ``want_hist`` adds ``temp_hist``:
        a list of n_atm arrays, the m-th (n_layers, 2 * n_iter[m]) as Grid.emission_spectrum
        returns it.  ``keep_dtaus`` leaves every atmosphere's final-emit dtaus on the device
        for :meth:`get_dtaus` and :meth:`post` (n_atm * n_layers * n_lam doubles, allocated at
        the first request)."""
        T = N.f64(np.broadcast_to(np.asarray(T_init, dtype=float), (self.n_atm, self.n_layers)))
        n_iter = (ctypes.c_int * self.n_atm)()
        T_final = np.empty((self.n_atm, self.n_layers))
        spectra = np.empty((self.n_atm, self.n_lam))
        self._last_spectra = spectra
        if not (want_hist or keep_dtaus):
            N.check(N.lib().frei_run_batch(self._ctx, N.dptr(T), int(n_timesteps),
                                           int(n_zero_crossings), float(convergence_dT),
                                           float(alpha), n_iter, N.dptr(T_final),
                                           N.dptr(spectra)))
            return dict(spectra=spectra, final_T=T_final, n_iter=np.array(list(n_iter)))
        hist = (np.empty((self.n_atm, self.n_layers, 2 * int(n_timesteps)))
                if want_hist else None)
        N.check(N.lib().frei_run_batch_ex(self._ctx, N.dptr(T), int(n_timesteps),
                                          int(n_zero_crossings), float(convergence_dT),
                                          float(alpha), n_iter, N.dptr(T_final),
                                          N.dptr(spectra), N.dptr(hist), 1 if keep_dtaus else 0))
        out = dict(spectra=spectra, final_T=T_final, n_iter=np.array(list(n_iter)))
        if want_hist:
            out["temp_hist"] = [hist[m][:, :2 * int(out["n_iter"][m])].copy()
                                for m in range(self.n_atm)]
        return out

    def get_dtaus(self, m):
        """Atmosphere ``m``'s dtaus (n_layers, n_lam) of the last ``run(keep_dtaus=True)``;
        row 0 is the ones placeholder (Q12)."""
        out = np.empty((self.n_layers, self.n_lam))
        N.check(N.lib().frei_get_dtaus_batch(self._ctx, int(m), 1, N.dptr(out)))
        return out

    def get_temperatures(self):
        T = np.empty((self.n_atm, self.n_layers))
        N.check(N.lib().frei_get_temperatures(self._ctx, N.dptr(T)))
        return T

    def post(self, dtaus=None, spectra=None, T=None, want_p_milne=False, want_cf=False):
        """effective_temperature (core.py:386-439) of every atmosphere, and on request the
        per-wavelength Milne pressures and the contribution functions (plot.py:63-79), in one
        device launch (frei_post_batch).  ``dtaus`` [n_atm][n_layers][n_lam], ``spectra``
        [n_atm][n_lam] and ``T`` [n_atm][n_layers] are host arrays, or None for the state the
        last ``run(keep_dtaus=True)`` left on the device.  Returns dict(T_milne, T_planck, T_eff
        [n_atm] each; p_milne [n_atm][n_lam] and cf [n_atm][n_layers][n_lam], rows bottom-first,
        when asked; sums [n_atm][3] = the device's (sum p_milne w, sum w, sum F trapz_w)).
        The device returns the three wavelength sums per atmosphere; the scalar
        finish is the host's, as in frei_amd.core for one atmosphere."""
        A, nL, n = self.n_atm, self.n_layers, self.n_lam

        def arr(x, shape, name):
            if x is None:
                return None
            x = N.f64(x)
            if x.shape != shape:
                raise ValueError(f"{name} must have shape {shape}, not {x.shape}")
            return x
        d = arr(dtaus, (A, nL, n), "dtaus")
        sp = arr(spectra, (A, n), "spectra")
        Th = arr(T, (A, nL), "T")
        p = np.asarray(self.p_bar, dtype=float)
        lam_cm = N.f64(self.lam_um * UM)
        nu = ratio = cf = None
        if want_cf:     # formed as Engine.contribution forms them
            dlogP = (np.log10(p.max()) - np.log10(p.min())) / (len(p) - 1)
            k = 10 ** -dlogP
            ratio = N.f64(p / ((1 - k) * p))
            nu = N.f64(1.0 / (self.lam_um * UM))
            cf = np.empty((A, nL, n))
        pm = np.empty((A, n)) if want_p_milne or self.k_weights is not None else None
        sums = np.empty((A, 3))
        N.check(N.lib().frei_post_batch(self._ctx, N.dptr(d), N.dptr(sp), N.dptr(Th),
                                        N.dptr(N.f64(p)), N.dptr(lam_cm), N.dptr(nu),
                                        N.dptr(ratio), H * C / K_B, N.dptr(sums), N.dptr(pm),
                                        N.dptr(cf)))
        if Th is None:
            Th = self.get_temperatures()
        if self.k_weights is not None:   # k-columns: the host finishes on the bins
            from .core import collapse_columns, milne_on_columns, planck_temperature
            if sp is None:
                sp = getattr(self, "_last_spectra", None)
            if sp is None:
                raise ValueError("post on k-columns needs spectra= or a run before it")
            w = self.k_weights
            lam_b = self.lam_um[::w.size]
            flux = collapse_columns(sp, w)
            T_milne = np.array([milne_on_columns(pm[m], flux[m], lam_b, w, p, Th[m])
                                for m in range(A)])
            T_planck = np.array([planck_temperature(lam_b, flux[m]) for m in range(A)])
        else:
            T_milne = np.array([np.interp(sums[m, 0] / sums[m, 1], p[::-1], Th[m][::-1])
                                for m in range(A)])
            T_planck = (sums[:, 2] / SIGMA_SB) ** 0.25
        T_eff = np.array([float(np.mean([T_milne[m], T_planck[m]])) for m in range(A)])
        out = dict(T_milne=T_milne, T_planck=T_planck, T_eff=T_eff, sums=sums)
        if want_p_milne:
            out["p_milne"] = pm
        if want_cf:
            out["cf"] = cf
        return out

    def transit(self, radii, R_star, dtaus=None, want_tau=False):
        """Every atmosphere's transit depth (R_eff / R_star)^2 per wavelength, [n_atm][n_lam],
        in one device launch (frei_transit): ``radii`` [n_atm][n_layers] (cm, each row from
        :func:`frei_amd.transit.level_radii`), ``dtaus`` [n_atm][n_layers][n_lam] a host array,
        or None for the dtaus the last ``run(keep_dtaus=True)`` left on the device.  Row m is
        bitwise ``Engine.transit`` of atmosphere m.  ``want_tau`` also returns the slant optical
        depths [n_atm][n_layers - 1][n_lam]: (depth, tau_slant)."""
        depth, tau = transit_call(self, self.n_atm, radii, R_star, dtaus, want_tau)
        return (depth, tau) if want_tau else depth

    def emergent(self, T, mu=None, weights=None, dtaus=None, want_intensity=False):
        """Every atmosphere's ray-traced emergent flux [n_atm][n_lam] in one device launch
        (frei_emergent; pure absorption): ``T`` [n_atm][n_layers], ``dtaus``
        [n_atm][n_layers][n_lam] a host array, or None for the dtaus the last
        ``run(keep_dtaus=True)`` left on the device; ``mu``, ``weights`` and the return as
        ``Engine.emergent``, intensities [n_atm][n_mu][n_lam].  Row m is bitwise
        ``Engine.emergent`` of atmosphere m."""
        return pick(*emergent_call(self, self.n_atm, T, mu, weights, dtaus, want_intensity))

    def phase_curve(self, pc, T, dtaus=None, keep=False):
        """The atmospheres as the cells of a planet's surface, integrated over the visible disk
        at every orbital phase of ``pc`` (:class:`~frei_amd.phasecurve.PhaseCurve`, K16) ->
        [n_phase][n_lam]: ``T`` and ``dtaus`` as :meth:`emergent`.  ``keep=True`` leaves the
        result on the device (:class:`~frei_amd.phasecurve.PhaseSpectra`)."""
        return pc.integrate(self, T, dtaus=dtaus, keep=keep)

    # fixed-work driver pieces (benchmarks)
    def state_init(self, T_init):
        T = N.f64(np.broadcast_to(np.asarray(T_init, dtype=float), (self.n_atm, self.n_layers)))
        N.check(N.lib().frei_state_init(self._ctx, N.dptr(T)))

    def get_fluxes(self):
        up = np.empty((self.n_atm, self.n_layers, self.n_lam))
        down = np.empty_like(up)
        N.check(N.lib().frei_get_fluxes(self._ctx, N.dptr(up), N.dptr(down)))
        return up, down


BatchRecord = collections.namedtuple(
    "BatchRecord", "spectrum final_T n_iter temp_hist T_eff T_milne T_planck")
BatchRecord.__doc__ = """One atmosphere of ``batched_emission_spectra(..., post=True)``: what
Grid.emission_spectrum returns (spectrum, final_T, temp_hist; core.py:335-338) with its iteration
count, and effective_temperature's three values (core.py:386-439), K."""


class BatchResult(list):
    """The :class:`BatchRecord` list of ``batched_emission_spectra(..., post=True)``.  It keeps
    the batched engine (``engine``, with every atmosphere's dtaus on the device) until
    :meth:`close`, so per-atmosphere arrays are fetched only when asked for."""

    def __init__(self, records, engine, planets=None):
        super().__init__(records)
        self.engine = engine
        self.planets = planets     # the grids' Planets, in the order of the records
        self._cf = None

    def dtaus(self, m):
        """Atmosphere ``m``'s dtaus (n_layers, n_lam), as Grid.emission_spectrum returns them."""
        return self.engine.get_dtaus(m)

    def contribution(self, m):
        """Atmosphere ``m``'s contribution function (plot.py:63-79), rows bottom-first.  The
        first call computes every atmosphere's in one launch and keeps them on the host."""
        if self._cf is None:
            self._cf = self.engine.post(want_cf=True)["cf"]
        return self._cf[m]

    def transmission(self, R_p=None, R_star=None, P_ref=None):
        """Every atmosphere's transit depth (R_eff / R_star)^2 per wavelength, [n_atm][n_lam],
        from the dtaus the run left on the device, in one launch (BatchEngine.transit).  ``R_p``
        and ``R_star`` (cm or Quantities; scalars or one per atmosphere) default to each
        Planet's; ``P_ref`` (bar) is the pressure R_p refers to (level 1 by default)."""
        eng, A = self.engine, len(self)
        planets = self.planets if self.planets is not None else [None] * A

        def per_atm(x):
            return [None] * A if x is None else list(np.broadcast_to(value(x, "cm"), (A,)))
        Rp = [default_radius(x, pl, "R_p", "the planet's radius")
              for x, pl in zip(per_atm(R_p), planets)]
        Rs = [default_radius(x, pl, "R_star", "the star's radius")
              for x, pl in zip(per_atm(R_star), planets)]
        radii = np.array([level_radii(self[m].final_T, eng.p_bar, float(eng.g[m]), eng.m_bar,
                                      Rp[m], P_ref) for m in range(A)])
        if len(set(Rs)) == 1:
            return eng.transit(radii, Rs[0])
        # stars of different radii: the depth scales with 1 / R_star^2 (one division per value,
        # as the device forms it)
        area = eng.transit(radii, 1.0)
        return np.array([area[m] / (Rs[m] * Rs[m]) for m in range(A)])

    def final_temperatures(self):
        """[n_atm][n_layers]: each record's ``final_T``, K."""
        return np.array([np.asarray(value(r.final_T, "K"), dtype=float) for r in self])

    def emergent(self, mu=None, weights=None, want_intensity=False):
        """Every atmosphere's ray-traced emergent flux [n_atm][n_lam] from each record's
        ``final_T`` and the dtaus the run left on the device, in one launch
        (BatchEngine.emergent: angles, weights and the return as there)."""
        return self.engine.emergent(self.final_temperatures(), mu=mu, weights=weights,
                                    want_intensity=want_intensity)

    def phase_curve(self, pc, keep=False):
        """The phase spectra [n_phase][n_lam] of ``pc``
        (:class:`~frei_amd.phasecurve.PhaseCurve`, K16) from each record's ``final_T`` and the
        dtaus the run left on the device (BatchEngine.phase_curve): atmosphere ``m`` of the run
        is row ``m`` of ``pc.select``."""
        return self.engine.phase_curve(pc, self.final_temperatures(), keep=keep)

    def observe(self, instrument, kind="eclipse", depth=None, weighting=None, data=None,
                sigma=None, R_p=None, R_star=None, broadening=None):
        """Every atmosphere through ``instrument`` (:class:`~frei_amd.observe.Instrument`, K10)
        -> obs [n_atm][K], or (obs, chi2 [n_atm]) with ``data`` and ``sigma`` [K].  ``kind``:
        "flux" the channel means of the emergent flux, "eclipse" the secondary-eclipse depths
        (band integral of F_p / band integral of F_star) (R_p / R_star)^2 — both read the
        spectra where the run left them on the device — and "transit" the band-averaged transit
        depths of ``depth`` [n_atm][n_lam] (default: :meth:`transmission` with these radii),
        ``weighting`` "stellar" (the default with Planets) or "flat".  Stars are the Planets':
        ``stellar_spectrum``, else ``pi * B_star(T_star)``, distinct ones uploaded once; the radii
        (cm or Quantities, scalars or one per atmosphere) default to each Planet's.
        ``broadening`` (:class:`~frei_amd.broaden.Broadening`, K13) broadens the spectra on the
        device first."""
        from .observe import observe
        A = len(self)
        planets = self.planets if self.planets is not None else [None] * A
        x = None
        if kind == "transit":
            x = self.transmission(R_p=R_p, R_star=R_star) if depth is None else depth
        return observe(instrument, kind, planets, self.engine.lam_um, x=x,
                       engine=None if kind == "transit" else self.engine, weighting=weighting,
                       data=data, sigma=sigma, R_p=R_p, R_star=R_star, broadening=broadening)

    def cross_correlate(self, cc, kind="eclipse", depth=None, R_p=None, R_star=None,
                        offset=None, broadening=None, keep=False, **kw):
        """Every atmosphere against high-resolution data over a grid of trial velocities
        (``cc``: :class:`~frei_amd.crosscorr.CrossCorrelator`, K12) ->
        :class:`~frei_amd.crosscorr.CrossCorrelation`.  ``kind``: "flux" takes the emergent
        spectra as templates, "eclipse" the planet-to-star flux ratio F_p / F_star
        (R_p / R_star)^2 — both read the spectra where the run left them on the device — and
        "transit" minus ``depth`` [n_atm][n_lam] (default: :meth:`transmission` with these
        radii).  Stars and radii as in :meth:`observe`; ``offset`` (a number per atmosphere) is
        subtracted from each template.  ``broadening``
        (:class:`~frei_amd.broaden.Broadening`, K13) broadens the spectra (for "transit" minus
        the depth) on the device first: resident to resident, then the pre-pass.  ``keep=True``
        (and any further keyword, ``want=`` or ``form=``) goes to
        :meth:`~frei_amd.crosscorr.CrossCorrelator.correlate`: the sums stay on the device for
        :meth:`~frei_amd.stack.OrbitStack.stack` (K14)."""
        from .crosscorr import cross_correlate
        A = len(self)
        planets = self.planets if self.planets is not None else [None] * A
        x = None
        if kind == "transit":
            x = self.transmission(R_p=R_p, R_star=R_star) if depth is None else depth
        return cross_correlate(cc, kind, planets, self.engine.lam_um, x=x,
                               engine=None if kind == "transit" else self.engine, R_p=R_p,
                               R_star=R_star, offset=offset, broadening=broadening, keep=keep,
                               **kw)

    def model_grid(self, axes, broadening=None):
        """A :class:`~frei_amd.modelgrid.ModelGrid` (K15) whose nodes are the spectra the run
        left on the device, copied device to device without a host copy: ``axes`` are the
        sweep's parameter axes (1 to 4 strictly ascending arrays whose lengths multiply to the
        number of atmospheres), atmosphere ``m`` the node of C-order index ``m`` over them (the
        last axis fastest).  With ``broadening`` (:class:`~frei_amd.broaden.Broadening`, K13) the
        nodes are broadened first, resident to resident.  Interpolation is linear and its weights
        do not depend on wavelength, so broadening the nodes once equals broadening every
        interpolated query (up to rounding).  The grid owns its copy: it outlives :meth:`close`."""
        from .modelgrid import ModelGrid
        eng = self.engine
        if broadening is not None:
            kept = broadening.apply(engine=eng, keep=True)
            return ModelGrid(axes, eng.lam_um, spectra=kept, device=eng.device)
        return ModelGrid(axes, eng.lam_um, engine=eng, device=eng.device)

    def close(self):
        self.engine.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def grid_mixing_ratios(grids, names):
    """The ``mmr`` argument of :class:`BatchEngine` for a list of Grids: the list of their
    ChemistryTables when every grid carries one, else the array [n_atm][n_species][n_layers] of
    their fixed mixing ratios (the mock where a grid has none).  A grid with a chemistry
    provider, or tables on some grids and arrays on others, is a ValueError."""
    for gr in grids:
        if getattr(gr, "chemistry", None) is not None:
            raise ValueError("a batch cannot step a chemistry provider: tabulate it as a "
                             "ChemistryTable on (T, p) nodes and load it with mmr=")
    is_tab = [isinstance(gr.mmr, ChemistryTable) for gr in grids]
    if all(is_tab):
        check_chemistry_nodes(chemistry_tables([gr.mmr for gr in grids], len(grids))[0])
        return [gr.mmr for gr in grids]
    if any(is_tab):
        raise ValueError("batched grids must all carry ChemistryTables or all carry fixed "
                         "mixing ratios, not a mix of both")
    mmrs = []
    for gr in grids:
        if gr.mmr is not None:
            mmrs.append(np.broadcast_to(np.asarray(gr.mmr, dtype=float),
                                        (len(names), gr.pressures.size)))
        else:
            mm = chemistry(np.full(gr.pressures.size, 1000.0), gr.pressures, names,
                           m_bar=gr.planet.m_bar)
            mmrs.append(np.array([mm[n] for n in names]))
    return np.array(mmrs)


def batched_emission_spectra(grids, n_timesteps=1, n_zero_crossings=2, convergence_dT=3.0,
                             device=0, post=False):
    """Grid.emission_spectrum for a list of Grids that share wavelengths, pressures and
    opacity tables (a grid sweep over T, g and metallicity), as one batched device run.
    Returns [(Spectrum, final_T, n_iter)] in the order of ``grids``; with ``post=True`` a
    :class:`BatchResult` of :class:`BatchRecord` (spectrum, final_T, n_iter, temp_hist, T_eff,
    T_milne, T_planck) that keeps the engine for ``contribution(m)`` and ``dtaus(m)``."""
    from .core import F_TOA, Spectrum
    if any(hasattr(gr, "col_weights") for gr in grids):
        raise NotImplementedError(
            "batched_emission_spectra given KGrids: it would sum the columns of a k-distribution "
            "with trapezoid weights, not quad_weights=col_weights; use batched_k_spectra")
    g0 = grids[0]
    for gr in grids[1:]:
        if not (np.array_equal(gr.lam, g0.lam) and np.array_equal(gr.pressures, g0.pressures)):
            raise ValueError("batched grids must share wavelengths and pressures")
        if gr.opacities is not g0.opacities:
            raise ValueError("batched grids must share one opacity dict")
        if gr.planet.alpha != g0.planet.alpha or gr.planet.m_bar != g0.planet.m_bar:
            raise ValueError("batched grids must share alpha and m_bar")
    names = list(g0.opacities)
    mmr = grid_mixing_ratios(grids, names)
    pl = g0.planet
    # each planet's own irradiation (core.py:262): one F_TOA per atmosphere when they differ
    ft = np.array([F_TOA(g0.lam, T_star=gr.planet.T_star, a_rstar=gr.planet.a_rstar,
                         F_star=getattr(gr.planet, "stellar_spectrum", None))
                   for gr in grids])
    if all(np.array_equal(f, ft[0]) for f in ft[1:]):
        ft = ft[0]
    eng = BatchEngine(g0.lam, g0.pressures, g0.opacities, [gr.planet.g for gr in grids],
                      mmr=mmr, m_bar=pl.m_bar, F_toa=ft, device=device)
    T_init = np.array([gr.init_temperatures for gr in grids])
    if post:
        try:
            out = eng.run(T_init, n_timesteps, n_zero_crossings, scalar(convergence_dT, "K"),
                          pl.alpha, want_hist=True, keep_dtaus=True)
            te = eng.post()
        except BaseException:
            eng.close()
            raise
        return BatchResult(
            [BatchRecord(Spectrum(out["spectra"][m], g0.lam), out["final_T"][m],
                         int(out["n_iter"][m]), out["temp_hist"][m], float(te["T_eff"][m]),
                         float(te["T_milne"][m]), float(te["T_planck"][m]))
             for m in range(len(grids))], eng, [gr.planet for gr in grids])
    try:
        out = eng.run(T_init, n_timesteps, n_zero_crossings, scalar(convergence_dT, "K"),
                      pl.alpha)
    finally:
        eng.close()
    return [(Spectrum(out["spectra"][m], g0.lam), out["final_T"][m], int(out["n_iter"][m]))
            for m in range(len(grids))]
