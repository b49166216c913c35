/*
 * frei_hip.h — C ABI of the MI355X (gfx950) two-stream radiative-transfer engine.
 *
 * Drop-in boundary for bmorris3/frei's hot path.  The reference
 * has no FFI: its seam is a set of Python functions, and each entry point below
 * replaces one of them (file:line in /root/reference):
 *
 *   frei_propagate_fluxes   frei/twostream.py:97-177   propagate_fluxes(...)
 *   frei_kappa              frei/opacity.py:203-269    kappa(opacities, T, p, lam, m_bar)
 *   frei_sweep              frei/twostream.py:290-421  emit(..., n_timesteps=1)
 *                           frei/twostream.py:424-550  absorb(..., n_timesteps=1)
 *   frei_run                frei/core.py:233-338       Grid.emission_spectrum(...)
 *   frei_set_table*         frei/core.py:198-231       Grid.load_opacities(opacities=...)
 *   frei_set_grid           frei/core.py:113-188,48-55 Grid(...) + F_TOA(...)
 *   frei_xsec_bin           frei/opacity.py:66-170     binned_opacity(...) (one species)
 *                           frei/interp.py:156-307     groupby_bins_agg / AggregateTrapz
 *   frei_set_table_binned   frei/core.py:198-231       Grid.load_opacities(species, path)
 *   frei_sspec_bin          frei/phoenix.py:13-17,43-52 get_binned_phoenix_spectrum(...) after
 *                                                      the download
 *
 * Conventions (all plain pointers and sizes, no framework types):
 *   - Units are cgs: wavelength cm, pressure dyn cm^-2, T K, flux erg s^-1 cm^-3,
 *     opacity cm^2 g^-1, g cm s^-2, masses g.  Layer index 0 = bottom of atmosphere.
 *   - Every function returns 0 on success, < 0 on error; frei_last_error() then holds
 *     a message (thread-local).  The Python layer raises RuntimeError with it.
 *   - Host buffers are caller-owned and copied in/out; device buffers belong to the
 *     context.  One context per GPU; a context is not thread-safe.
 *   - A context owns the contiguous wavelength slice [lam_offset, lam_offset+n_lam)
 *     of a global grid; with nranks > 1 the per-sweep bolometric partial sums are
 *     all-gathered over RCCL (frei_comm_init) and summed in rank order, so every rank
 *     computes bitwise-identical temperatures.
 */
#ifndef FREI_HIP_H
#define FREI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct frei_ctx frei_ctx;

enum { FREI_EMIT = 0, FREI_ABSORB = 1 };

/* Library/ABI version (major*10000 + minor*100 + patch); 2.0.0. */
int frei_version(void);
/* Message of the last failing call on this thread ("" if none). */
const char* frei_last_error(void);
/* Number of visible HIP devices. */
int frei_device_count(int* n);
/*
 * What this process's handles hold right now: device buffers, pinned host buffers, streams
 * and events (a null pointer skips that figure).  Every handle type owns its resources
 * through the same counted types, so the figures return to their earlier values when a handle
 * is destroyed and a call's temporaries do not outlive the call.  Needs no device and no handle.
 */
int frei_live_resources(int64_t* device_buffers, int64_t* pinned_buffers, int64_t* streams,
                        int64_t* events);

/* Context for n_layers x n_lam (local slice) x n_species on `device`. */
int frei_ctx_create(frei_ctx** out, int device, int n_layers, int64_t n_lam, int n_species);
/*
 * Batched context (§8(f) #2, grid sweeps such as C5): n_atm independent atmospheres share the
 * wavelength and pressure grids and the opacity tables; each has its own temperatures,
 * gravity (frei_set_gravity) and mixing ratios (frei_set_mmr takes [n_atm][n_species]
 * [n_layers]).  The reference has no batch API: each atmosphere is the reference's
 * Grid.emission_spectrum (core.py:233-338) run independently.  Needs tables on shared
 * on-node p/T nodes without NaN; the per-atmosphere species contraction runs on fp64 MFMA
 * (K7).  State accessors (set/get fluxes and temperatures) take n_atm blocks; frei_sweep,
 * frei_run, frei_kappa and the rank exchange are single-atmosphere only (batched runs shard
 * atmospheres across ranks with no exchange).  Post-processing of every atmosphere of a
 * batched run is frei_run_batch_ex(keep_dtaus) + frei_post_batch below; frei_milne_pressure
 * and frei_contribution stay the single-context calls.
 */
int frei_ctx_create_batch(frei_ctx** out, int device, int n_layers, int64_t n_lam,
                          int n_species, int n_atm);
int frei_set_gravity(frei_ctx* ctx, const double* g);
/* Batched: one F_TOA per atmosphere, f_toa[n_atm][n_lam] (core.py:48-55 with each planet's
 * T_star and a/R_star; replaces frei_set_grid's shared F_TOA until the next frei_set_grid). */
int frei_set_ftoa_batch(frei_ctx* ctx, const double* f_toa);
/* Every atmosphere iterates to its own convergence (core.py:273-318), then the final emit;
 * n_iter[n_atm], T_final[n_atm][n_layers] and spectra[n_atm][n_lam] (F_up[n_layers-1]). */
int frei_run_batch(frei_ctx* ctx, const double* T_init, int n_timesteps, int n_zero_crossings,
                   double convergence_dT, double alpha, int* n_iter, double* T_final,
                   double* spectra);
/*
 * frei_run_batch with the rest of what the reference's Grid.emission_spectrum returns per
 * atmosphere (core.py:335-338: spectrum, final temperatures, temperature history, dtaus);
 * frei_run_batch is this call with temp_hist = NULL, keep_dtaus = 0.
 *   temp_hist[n_atm][n_layers][2*n_timesteps] (may be NULL): atmosphere m's first
 *     2*n_iter[m] columns are its absorb history (core.py:303-307, 320-321; transposed as in
 *     frei_run), the rest are zero.
 *   keep_dtaus != 0: the final emit (core.py:323-333) writes every atmosphere's dtaus into a
 *     device buffer [n_atm][n_layers][n_lam], row 0 of every atmosphere = 1 (Q12), allocated
 *     at the first request only; if that allocation fails the call returns an error naming
 *     the size and the context stays usable.  The kept dtaus feed frei_get_dtaus_batch and
 *     frei_post_batch until the next frei_state_init, frei_iterate or run without keep_dtaus.
 */
int frei_run_batch_ex(frei_ctx* ctx, const double* T_init, int n_timesteps,
                      int n_zero_crossings, double convergence_dT, double alpha, int* n_iter,
                      double* T_final, double* spectra, double* temp_hist, int keep_dtaus);
/* The kept dtaus of atmospheres [atm_lo, atm_lo + n): out[n][n_layers][n_lam]. */
int frei_get_dtaus_batch(frei_ctx* ctx, int atm_lo, int n, double* out);
int frei_ctx_destroy(frei_ctx* ctx);

/*
 * Grid and per-wavelength constants (frei/core.py:113-188, 48-55; twostream.py:46-67).
 *   c1[n_lam]     2 h c^2 / lam^5                (Planck prefactor, BB)
 *   lk[n_lam]     lam * k_B   (BB exponent h c / (lk T), formed as (h c / lk) * (1 / T))
 *   sigma[n_lam]  Rayleigh H2 + He, cm^2 g^-1    (opacity.py:173-200, 233)
 *   f_toa[n_lam]  stellar flux at TOA            (core.py:48-55)
 *   trapz_w[n_lam] per-point trapezoid weights of the GLOBAL grid (cm), sliced
 *   p[n_layers]   layer pressures, dyn cm^-2, descending (tp.py:10-33)
 *   g, m_bar      planet gravity and mean molecular mass (core.py:65-106)
 */
int frei_set_grid(frei_ctx* ctx, const double* c1, const double* lk, const double* sigma,
                  const double* f_toa, const double* trapz_w, const double* p,
                  double g, double m_bar);

/*
 * Opacity table of species s (Grid.load_opacities(opacities=...), core.py:198-231):
 * values[n_p][n_T][n_lam] (row-major, this context's wavelength slice), cm^2 g^-1,
 * on nodes p_nodes[n_p] (dyn cm^-2) x T_nodes[n_T] (K), any order.  Linear
 * interpolation with fill 0 outside the node hull (opacity.py:241-263); a table with
 * one unique T is interpolated in pressure only (opacity.py:256-259).
 */
int frei_set_table(frei_ctx* ctx, int s, const double* values, const double* p_nodes, int n_p,
                   const double* T_nodes, int n_T);
/*
 * Same, but the table is generated on the device (no host copy of n_p*n_T*n_lam values):
 * values[p][t][l] = min(max((fp[p] * fT[t]) * base[l], lo), hi).  Synthetic separable
 * tables for benchmarks and parity tests.
 */
int frei_set_table_separable(frei_ctx* ctx, int s, const double* base, const double* fp,
                             const double* fT, double lo, double hi, const double* p_nodes,
                             int n_p, const double* T_nodes, int n_T);
/* Per-species, per-layer mass mixing ratios mmr[n_species][n_layers] (chemistry.py:114-205;
 * the reference's mock gives a constant VMR).  CIA-like tables take their weights here. */
int frei_set_mmr(frei_ctx* ctx, const double* mmr);

/*
 * Temperature-dependent chemistry (chemistry(T, p) inside every kappa call,
 * opacity.py:246-248; chemistry.py:114-205): mass mixing ratios values[n_species][n_T][n_p]
 * on ascending T_nodes (K) x p_nodes (dyn cm^-2).  At every sweep step the layer's mmr is
 * interpolated at its current (T_i, p_i) — linear in T and in log10 p, clamped to the nodes —
 * when the update kernel writes the next sweep's step table; the species sum then stays in
 * the sweep (no K3 contraction).  values = NULL returns to frei_set_mmr's fixed arrays.
 * Single-atmosphere contexts (batched ones: frei_set_chemistry_batch); call after frei_set_grid.
 */
int frei_set_chemistry(frei_ctx* ctx, const double* values, const double* T_nodes, int n_T,
                       const double* p_nodes, int n_p);
/* Batched contexts: n_tab chemistry tables values[n_tab][n_species][n_T][n_p] on shared
 * ascending T_nodes (K) x p_nodes (dyn cm^-2); atmosphere m uses table atm_tab[m].
 * Interpolation exactly as frei_set_chemistry (chem_mmr_at).  values = NULL: back to
 * frei_set_mmr's fixed arrays and the contracted path.
 * With chemistry on, the context builds and allocates no contracted table (frei_ctx_path reports
 * contracted = 0): every atmosphere's sweep sums the species from the shared tables, which must
 * be on shared on-node p/T nodes without NaN as for any batched context.  Consecutive
 * atmospheres that sit in the same T brackets share table rows in the tiled sweep (option
 * "atm_tile"), so order a grid sweep by temperature.  frei_run_batch(_ex), frei_state_init /
 * frei_iterate, frei_get_dtaus_batch, frei_post_batch, frei_set_gravity and
 * frei_set_ftoa_batch work unchanged.  Errors: a context from frei_ctx_create (use
 * frei_set_chemistry), n_tab < 1, an atm_tab entry outside [0, n_tab), nodes that do not
 * ascend.  Call after frei_set_grid. */
int frei_set_chemistry_batch(frei_ctx* ctx, const double* values, int n_tab,
                             const int32_t* atm_tab, const double* T_nodes, int n_T,
                             const double* p_nodes, int n_p);

/* Flux state [n_layers][n_lam] (this slice), caller layout row-major. */
int frei_set_fluxes(frei_ctx* ctx, const double* up, const double* down);
int frei_get_fluxes(frei_ctx* ctx, double* up, double* down);
/* The emergent spectrum F_up[n_layers - 1] of this slice (n_lam values): the row the reference's
 * Grid returns as Spectrum1D(flux=fluxes_up[-1]) (frei/core.py:335-338), without reading back
 * the whole flux state. */
int frei_get_spectrum(frei_ctx* ctx, double* spectrum);
int frei_set_temperatures(frei_ctx* ctx, const double* T);
int frei_get_temperatures(frei_ctx* ctx, double* T);

/*
 * One sweep with the current temperatures (emit: twostream.py:351-407, absorb: 486-536),
 * in place on the flux state, then T <- T - dT (Q11).  alpha = mixing-length parameter.
 * Optional outputs (NULL to skip): dT[n_layers], bol[n_layers][4] = bolometric
 * (F_2_up, F_2_down, F_1_up, F_1_down) per sweep step, dtaus[n_layers][n_lam] (row 0 = 1,
 * row k = k-th step of the sweep, Q12).
 */
int frei_sweep(frei_ctx* ctx, int direction, double alpha, double* dT, double* bol,
               double* dtaus);

/*
 * Grid.emission_spectrum (core.py:233-338): zero fluxes, T = T_init, up to n_timesteps
 * (emit, absorb) iterations with the reference convergence test (sign flips of the
 * absorb temperature history > n_zero_crossings, or |dT| < convergence_dT, for all
 * layers), then a final emit with alpha = 1.  The loop stays on the device; the host
 * polls the convergence flag once per chunk of iterations.
 * Outputs: *n_iter; T_final[n_layers]; temp_hist[n_layers][2*n_iter] (may be NULL; caller
 * sizes it for n_timesteps); dtaus[n_layers][n_lam] (may be NULL); spectrum[n_lam]
 * = F_up[n_layers-1] (may be NULL).
 */
int frei_run(frei_ctx* ctx, const double* T_init, int n_timesteps, int n_zero_crossings,
             double convergence_dT, double alpha, int* n_iter, double* T_final,
             double* temp_hist, double* dtaus, double* spectrum);

/* Benchmark/driver pieces of frei_run (all asynchronous on the context's stream). */
int frei_state_init(frei_ctx* ctx, const double* T_init);
/* n T-P iterations; convergence is tracked but never stops the work when
 * n_zero_crossings < 0 (fixed-work benchmark steps). */
int frei_iterate(frei_ctx* ctx, int n, int n_zero_crossings, double convergence_dT,
                 double alpha);
int frei_synchronize(frei_ctx* ctx);

/* kappa (opacity.py:203-269) at one (T, p) on this slice: k[n_lam] (includes sigma, Q1),
 * sigma[n_lam] (may be NULL). */
int frei_kappa(frei_ctx* ctx, double T, double p, double* k, double* sigma);

/* propagate_fluxes (twostream.py:97-177), elementwise on n points; g_0[n] is the scattering
 * asymmetry factor (NULL: g_0 = 0, as at the emit/absorb call sites twostream.py:389, 518). */
int frei_propagate_fluxes(int device, int64_t n, const double* c1, const double* lk,
                          const double* F_1_up, const double* F_2_down, double T_1,
                          double T_2, const double* delta_tau, const double* omega_0,
                          const double* g_0, double* F_2_up, double* F_1_down);

/* Multi-GPU: 128-byte RCCL unique id (rank 0 creates, others receive it out of band),
 * then every rank joins.  Per sweep: one ncclAllGather of n_layers*4 doubles. */
int frei_comm_unique_id(void* id128);
int frei_comm_init(frei_ctx* ctx, int nranks, int rank, const void* id128);

/*
 * P2P exchange over xGMI without RCCL or the host: each rank allocates a
 * mailbox in uncached device memory and exports its 64-byte IPC handle
 * (frei_comm_p2p_handle); after the handles are all-gathered out of band (rank order),
 * frei_comm_p2p_open maps every rank's mailbox and runs a bounded handshake.  Per sweep the
 * update kernel pushes this rank's n_layers*4 partial sums into every mailbox with a
 * sequence flag per value and waits for every rank's flags (a rank that never publishes is
 * reported as an error after FREI_P2P_TIMEOUT_S seconds, default 30).
 * Ranks may share one GPU (processes on the same device).
 */
int frei_comm_p2p_handle(frei_ctx* ctx, int nranks, int rank, void* handle64);
int frei_comm_p2p_open(frei_ctx* ctx, const void* handles);

/* Alternative exchange for testing and for hosts without RCCL peers (e.g. several ranks
 * sharing one GPU): per sweep the n partial sums are copied to the host and
 * fn(send[n], recv[nranks*n], n, user) must all-gather them in rank order (returns 0). */
typedef int (*frei_allgather_fn)(const double* send, double* recv, int64_t n, void* user);
int frei_comm_init_host(frei_ctx* ctx, int nranks, int rank, frei_allgather_fn fn, void* user);

/*
 * Post-processing of a converged atmosphere (§8(f) #3), per wavelength on this slice.
 * dtaus[n_layers][n_lam] is the host array frei_run returned, or NULL to use the copy the
 * last frei_run left on the device.
 *   frei_milne_pressure  core.py:392-395  p_milne[j] = np.interp(2/3, exp(-dtaus[:, j]),
 *                        p_bar) (numpy's search, unsorted transmissions included); the
 *                        weighted mean and final interpolation (core.py:397-405) stay on
 *                        the host.
 *   frei_contribution    plot.py:63-79  cf[n_layers][n_lam], rows bottom-first (cf[::-1]),
 *                        from nu[n_lam] (cm^-1), ratio[n_layers] = p / dP, T[n_layers] and
 *                        hcperk = h c / k_B (cm K).
 */
int frei_milne_pressure(frei_ctx* ctx, const double* dtaus, const double* p_bar,
                        double* p_milne);
int frei_contribution(frei_ctx* ctx, const double* dtaus, const double* nu,
                      const double* ratio, const double* T, double hcperk, double* cf);
/*
 * The same post-processing for every atmosphere of a batched context (n_atm >= 1, from
 * frei_ctx_create_batch) in one launch over (wavelength block, atmosphere); the reference
 * calls effective_temperature (core.py:386-439) and the dashboard's contribution function
 * (plot.py:63-79) once per Grid.
 * Inputs dtaus[n_atm][n_layers][n_lam], spectra[n_atm][n_lam], T[n_atm][n_layers] are host
 * arrays to upload, or NULL for the device state the last frei_run_batch_ex(keep_dtaus) left
 * (the kept dtaus, the rows F_up[n_layers-1], the final temperatures); p_bar[n_layers],
 * lam_cm[n_lam] (the array spectrum * lam_cm is formed with, core.py:397-399), and for cf
 * nu[n_lam], ratio[n_layers], hcperk as in frei_contribution.
 * Outputs:
 *   sums[n_atm][3]  A = sum_j p_milne[j] w[j], B = sum_j w[j] with w[j] = spectrum[j] *
 *                   lam_cm[j] (core.py:397-403: np.average(p_milne, weights=w) = A / B), and
 *                   C = sum_j spectrum[j] * trapz_w[j] with frei_set_grid's weights
 *                   (core.py:408-414: np.trapz(flux, lam)).  Summed in a fixed order without
 *                   atomics: bitwise the same from run to run.  The final interpolation and
 *                   the fourth root stay on the host.
 *   p_milne[n_atm][n_lam] (may be NULL): bitwise frei_milne_pressure's on the same dtaus.
 *   cf[n_atm][n_layers][n_lam] (may be NULL: nothing is computed or allocated for it; T, nu
 *                   and ratio are then unused): bitwise frei_contribution's.
 * Fails with "no device dtaus" when an input is NULL and no kept dtaus are valid, and on a
 * context from frei_ctx_create (use frei_milne_pressure / frei_contribution there).
 */
int frei_post_batch(frei_ctx* ctx, const double* dtaus, const double* spectra, const double* T,
                    const double* p_bar, const double* lam_cm, const double* nu,
                    const double* ratio, double hcperk, double* sums, double* p_milne,
                    double* cf);
/*
 * Transmission (transit-depth) spectrum of every atmosphere of the context, (R_eff / R_star)^2
 * per wavelength, from the final emit's vertical optical depths (K9, one launch over
 * (wavelength block, atmosphere)).  The reference has no counterpart; this is the definition.
 * Layer 0 is the bottom, g and m_bar are constant, levels l = 1 .. n_layers - 1 sit at the
 * pressures p_l and the virtual top level n_layers at p_{nL-1} p_{nL-2} / p_{nL-3} (Q3).
 *   Shell l (1 <= l <= n_layers - 1) lies between levels l and l + 1; its vertical optical depth
 *   is row l of dtaus (emit order, as frei_run returns them; under hydrostatic equilibrium
 *   kappa rho dz of the shell).  Row 0 (the ones placeholder, Q12) is never read: layer 0 lies
 *   below the opaque base.
 *   radii[n_atm][n_layers], cm, radii[m][k] = r_{k+1}: the level radii, strictly ascending
 *   (frei_amd.transit.level_radii forms them from T, p, g, m_bar, R_p and a reference pressure).
 *   Chord weights, 1 <= i <= j <= n_layers - 1, built on the host once per call and atmosphere:
 *     s(i, k) = sqrt((r_k - r_i) * (r_k + r_i)),
 *     G[i][j] = 2 * (r_{j+1} + r_j) / (s(i, j+1) + s(i, j))     (= 2 ds_ij / dz_j, no cancellation)
 *   tau_i   = sum_{j=i}^{nL-1} G[i][j] * dtaus[j], added in ascending j from the j = i term;
 *   f_i     = -expm1(-tau_i), f_nL = 0;
 *   A       = r_1 r_1 + sum_{i=1}^{nL-1} (f_i r_i + f_{i+1} r_{i+1}) * (r_{i+1} - r_i), ascending i;
 *   depth   = A / (r_star * r_star).
 * dtaus[n_atm][n_layers][n_lam] is a host array to upload, or NULL for the device copy the last
 * frei_run / frei_run_batch_ex(keep_dtaus) left ("no device dtaus" when there is none).
 * Outputs depth[n_atm][n_lam] and, unless NULL (nothing is allocated or written for it then),
 * tau_slant[n_atm][n_layers - 1][n_lam], row k = tangent level k + 1.  n_atm = 1 on a context
 * from frei_ctx_create; a wavelength-slice context gives its own columns (every column is
 * independent).  NaN or inf in a column stays in that column; nothing is checked.  Results are
 * bitwise reproducible and the same from a single and a batched context.  Errors: null radii or
 * depth, radii not strictly ascending, r_star <= 0.
 */
int frei_transit(frei_ctx* ctx, const double* dtaus, const double* radii, double r_star,
                 double* depth, double* tau_slant);
/*
 * Emergent specific intensities I(mu) at the top of every atmosphere of the context at a set of
 * viewing angles, and their quadrature over the disk: the formal solution along rays through
 * the final emit's vertical optical depths (K11, one launch over (wavelength block,
 * atmosphere)).  The reference has no counterpart; this is the definition.
 * Layer 0 is the bottom.  Levels l = 1 .. nL-1 (nL = n_layers) carry the temperatures
 * T_l = T[l]; the virtual top level nL has T_nL = T_{nL-1} (emit's rule for its last step).
 *   Shell l (1 <= l <= nL-1) lies between levels l and l + 1; its vertical optical depth is row
 *   l of dtaus (emit order, as frei_run returns them).  Row 0 (the ones placeholder) is never
 *   read; T[0] is never read.
 *   The dtaus are absorption optical depths (twostream.py:371-373 forms them from k, not from
 *   k + sigma): this is the pure-absorption formal solution.  Scattering enters neither as
 *   extinction nor as source.
 * Per wavelength j, atmosphere m and angle k with 0 < mu[k] <= 1:
 *   B_l   = c1[j] / expm1((h c / lk[j]) * (1 / T_l))    the context's own Planck constants
 *                                                       (frei_set_grid)
 *   I     = B_1                                         opaque base at level 1 (as frei_transit)
 *   for l = 1 .. nL-1, ascending:
 *       x  = dtaus[l][j] / mu[k]
 *       e  = exp(-x);  em = -expm1(-x)
 *       v  = 1 - em / x    (v(0) = 0, v(inf) = 1)
 *       u  = em - v
 *       I  = I * e + (B_l * u + B_{l+1} * v)
 *   intensity[m][k][j] = I
 *   flux[m][j] = 2 pi * sum_k c_k * intensity[m][k][j],  c_k = weights[k] * mu[k] formed on the
 *                host, added in ascending k starting from the k = 0 term
 * This is the exact integral of a source function linear in tau across each shell (the
 * two-stream's Bprime makes the same assumption).  e, u and v are non-negative and
 * e + u + v = 1: every step is a convex combination.  v cancels for small x and is evaluated
 * there from the series x/2 - x^2/6 + x^3/24 - ...; e is never formed as 1 - em (a hot base
 * under a cold opaque top would lose the answer), and I * e underflows smoothly.  x = 0 leaves
 * I unchanged; x = inf gives B_{l+1}.  NaN or inf in a column stays in that column; nothing in
 * the input columns is checked.
 * dtaus[n_atm][n_layers][n_lam] is a host array to upload, or NULL for the device copy the last
 * frei_run / frei_run_batch_ex(keep_dtaus) left ("no device dtaus" when there is none).
 * T[n_atm][n_layers] is a host array, always given: the temperatures that belong to the kept
 * dtaus are the caller's business, as the radii are for frei_transit.  mu[n_mu], 1 <= n_mu <= 64;
 * weights[n_mu] is NULL exactly when flux is NULL.
 * Outputs intensity[n_atm][n_mu][n_lam] and flux[n_atm][n_lam]; either may be NULL, not both,
 * and nothing is allocated or written for an absent one.  n_atm = 1 on a context from
 * frei_ctx_create; a wavelength-slice context gives its own columns.  intensity[m][k] is bitwise
 * the same whatever else is in the call (other angles, n_mu, with or without flux, single or
 * batched context).  Errors (return codes; the context stays usable): null T or mu, both
 * outputs null, weights and flux not both present or both absent, n_mu out of range, a mu that
 * is not finite, <= 0 or > 1, a non-finite weight, a T[m][l], l >= 1, not finite and positive.
 */
int frei_emergent(frei_ctx* ctx, const double* dtaus, const double* T, const double* mu,
                  const double* weights, int n_mu, double* intensity, double* flux);
/* HIP-event milliseconds of the kernels of the last frei_milne_pressure, frei_contribution,
 * frei_post_batch, frei_transit or frei_emergent call on this context (uploads and read-backs
 * excluded); 0 before any. */
int frei_post_timing(frei_ctx* ctx, double* ms);

/* Which sweep implementation the context's current tables select (after metadata build):
 * bit 0 fast path (on-node pressures, >= 2 T nodes, S <= 8), bit 1 step table staged in
 * LDS (shared brackets, small slices), bit 2 species-contracted table (K3), bit 3 tables
 * hold NaN (per-species nansum variant), bit 4 / bit 5 grouped-lane sweep with two / four
 * lanes per wavelength (small slices), bits 6-8: consumer waves per block of the
 * producer/consumer sweep (1, 2 or 4; 0 = not used), bit 9 two wavelengths per lane in the
 * contracted one-lane sweep (large slices: option "lam2"), bit 10 the producer/consumer sweep
 * runs its update as trailing workgroups of its own launch (option "tail"; loops without
 * per-sweep events), bit 11 lazy K3: the setup contracted no row, the two-wavelength sweeps
 * contract the rows their records reach first (option "lazy_k3"), bits 12-14: atmospheres per
 * block of a chemistry batch's per-species sweep (frei_set_chemistry_batch: 1 the one-lane sweep
 * over (wavelength block, atmosphere), 2 or 4 the atmosphere-tiled sweep; 0 otherwise). */
int frei_ctx_path(frei_ctx* ctx, int* flags);

/* Tuning knobs (also FREI_<NAME> in the environment at context creation): "precontract"
 * (K3 species contraction: 1 on when it applies / 0 off / -1 automatic), "group_q" (lanes per
 * wavelength 1, 2, 4 or 0 = automatic), "shared" (LDS step table 1/0/-1), "prefetch_depth",
 * "shared_max_blocks", "pair_max_blocks", "quad_max_blocks", "depth4_max_blocks",
 * "red_rows", "red_stage" (take effect at the next metadata build), "fused_update" (1: one
 * launch for the partial-sum reduction and the T update when the exchange is local or P2P;
 * 0: two kernels; bitwise identical results; takes effect at the next sweep), "graph" (1:
 * replay T-P iterations from a captured hipGraph; 0, the default: launch kernel by kernel),
 * "tail" (1, the default: the producer/consumer sweep's fused update runs as trailing
 * workgroups of the sweep's launch, layer by layer as the sweep publishes; 0: a launch of its
 * own after the sweep; bitwise identical results), "lazy_k3" (1, the default: with the
 * two-wavelength sweep, K3 contracts no row at setup — each sweep contracts the (pressure row,
 * T node) rows its records reach for the first time, for its own wavelengths, with K3's sum;
 * 0: every row at setup; bitwise identical results), "atm_tile" (atmospheres per block of a
 * chemistry batch's sweep, frei_set_chemistry_batch: 1 one block per (wavelength block,
 * atmosphere), 2 or 4 consecutive atmospheres in lockstep, loading the table rows they share
 * once; -1, the default: the widest of them that leaves the launch four blocks per CU; bitwise
 * identical results). */
int frei_set_option(frei_ctx* ctx, const char* name, int value);
/* With the "graph" option on (default off), T-P iterations (frei_iterate, frei_run) are
 * replayed from a captured hipGraph of a few iterations when one rank runs with timing off:
 * the number of captures and of graph launches so far. */
int frei_graph_info(frei_ctx* ctx, int* captures, int* replays);
/* Chained sweep launches so far (FREI_CHAIN / option "chain": a sweep launch whose leading
 * workgroups run the previous sweep's deferred fused update).  Never while per-sweep HIP events
 * are on (frei_timing) or when P2P ranks share this device. */
int frei_chain_info(frei_ctx* ctx, int64_t* chained);
/* Trailing-update launches so far (FREI_TAIL / option "tail", round 6): producer/consumer sweeps
 * whose launch also ran their own fused update, layer by layer as the sweep published each
 * layer's partial sums (twostream.py:396-407: a layer's dT needs only its own four bolometric
 * sums), instead of a separate update kernel after the sweep.  Never while per-sweep HIP events
 * are on, when chained, or when ranks share this device; bitwise the separate launches. */
int frei_tail_info(frei_ctx* ctx, int64_t* launches);
/* Ranks of this communicator share the context's GPU (shared != 0): no chained launches (a
 * chained launch's sweep blocks spin on update workgroups that wait for every rank's sums, and
 * could hold the CUs another rank's kernels need).  frei_amd sets it when two ranks report the
 * same host and PCI bus id (frei_device_pci_bus_id). */
int frei_comm_shared_device(frei_ctx* ctx, int shared);
/* The PCI bus id string of a device ("0000:05:00.0"), len >= 16. */
int frei_device_pci_bus_id(int device, char* buf, int len);
/* Host wall-clock milliseconds of the last metadata build (the one-time setup before the
 * first sweep after tables/mmr change), by phase: [0] per-(species, layer) brackets on the
 * host, [1] metadata uploads, [2] contracted-table allocation, [3] its zero fill, [4] the K3
 * contraction kernel. */
int frei_setup_timing(frei_ctx* ctx, double* ms5);
/* The last species-contraction launch (K3 for one atmosphere, K7 on fp64 MFMA for a batched
 * context; part of the metadata build): its duration by HIP events on the context stream, ms,
 * and its algorithmic HBM bytes (the S tables' used pressure rows read once, one contracted
 * table per atmosphere written).  0 / 0 before any contraction.  (No reference counterpart:
 * the reference sums species inside every kappa call, opacity.py:250-268.) */
int frei_contract_timing(frei_ctx* ctx, double* ms, double* bytes);

/* Timing of the sweep kernel (HIP events on the context stream around every sweep
 * launch while enabled): total milliseconds and number of timed launches. */
int frei_timing_enable(frei_ctx* ctx, int on);
int frei_timing_read(frei_ctx* ctx, double* total_ms, int* n_launches);
/* While timing is enabled, also HIP events around each sweep's rank exchange (the RCCL
 * all-gather of the bolometric partials, or the host hook): total ms and number of calls.
 * With the P2P exchange: the time the update kernels spent waiting for peers' sums. */
int frei_timing_read_exchange(frei_ctx* ctx, double* total_ms, int* n_calls);

/*
 * Opacity binning (opacity.py:66-170).  A frei_xsec is one species' high-resolution
 * cross-section resident in HBM, in the opacity_dir_to_netcdf layout (opacity.py:395-483):
 * values[n_T][n_p][n_hi] float32 on nodes T_nodes (K) x p_nodes (bar), wavelengths
 * wl_hi[n_hi] (µm, strictly ascending).
 */
typedef struct frei_xsec frei_xsec;
enum { FREI_BIN_GROUPIES = 0, FREI_BIN_EXACT = 1 };

int frei_xsec_create(frei_xsec** out, int device, const float* values, int n_T, int n_p,
                     int64_t n_hi, const double* T_nodes, const double* p_nodes,
                     const double* wl_hi);
/* Synthetic line forest generated on the device (benchmarks; no host copy). */
int frei_xsec_create_synthetic(frei_xsec** out, int device, int n_T, int n_p, int64_t n_hi,
                               const double* T_nodes, const double* p_nodes,
                               const double* wl_hi, uint64_t seed);
int frei_xsec_destroy(frei_xsec* x);
/*
 * K17: the cross-section computed line by line from a line list on the device (no reference
 * counterpart: the reference downloads this table, opacity.py:345-372, 493-540).
 *
 * Inputs: n_line lines of nondecreasing position, each with nu0 (cm^-1), S_ref (cm molecule^-1 at
 * T_ref), E_low (cm^-1), gamma_ref (Lorentz HWHM, cm^-1 per bar at T_ref) and n_exp (its
 * temperature exponent); mass_amu, T_ref (K), cutoff (cm^-1); q_ratio[n_T] = Q(T_ref) / Q(T_t);
 * nodes T_nodes[n_T] (K), p_nodes[n_p] (bar); axis wl_hi[n_hi] (µm, strictly ascending).
 * Constants: c2 = H C / K_B, m = mass_amu AMU (frei_amd/constants.py).  nu_i = 1e4 / wl_hi[i] is
 * formed on the host and uploaded.
 *
 * Per (T node t, line l), on the host in the C++ runtime (fp64, in this order):
 *   S     = ((S_ref q_ratio[t]) exp(-(c2 E_low) (1/T - 1/T_ref)))
 *           (expm1(-(c2 nu0) / T) / expm1(-(c2 nu0) / T_ref))
 *   alpha = nu0 sqrt(((2 K_B) T) / m) / C                 (Doppler 1/e half-width)
 *   gT    = gamma_ref exp(n_exp ln(T_ref / T))            (ln(T_ref / T) once per node)
 *   A = S / (alpha sqrt(pi)),  1 / alpha,  gT / alpha
 * Per pressure node: y = (gT / alpha) p.  Per axis point: x = |nu_i - nu0| (1 / alpha),
 * K(x, y) = Re w(x + iy) (Faddeeva; relative error <= 2^-26 for x in [0, 1e6], y in [1e-8, 1e5];
 * the algorithm is in frei_amd/csrc/frei_lines.hip) and
 *   values[t][p][i] = float32((1 / m) sum_l A_l K(x, y))        (cm^2 g^-1, as kappa reads tables)
 * over exactly the lines with |nu_i - nu0_l| <= cutoff (compared in fp64 on the uploaded nu_i),
 * in ascending line index, accumulated in fp64 and rounded once: the result does not depend on
 * how the axis, the nodes or the lines are blocked.  A point no line reaches is exactly 0.
 *
 * Not modelled: pressure shift, self-broadening, sub-Lorentzian wings, line mixing, continua,
 * renormalisation of the truncated wing, and y = 0 (gamma_ref and p must be positive).
 *
 * Every argument error is found on the host before any device call and names the first
 * offending index: null pointers, n_line < 1, unsorted nu0, non-finite values, S_ref < 0,
 * gamma_ref <= 0, nu0 <= 0, mass_amu <= 0, T_ref <= 0, cutoff <= 0, q_ratio <= 0, T <= 0, p <= 0,
 * a non-ascending axis.  *kernel_ms (may be NULL) receives the HIP-event time of the main kernel.
 */
int frei_xsec_create_lines(frei_xsec** out, int device, int64_t n_line, const double* nu0,
                           const double* S_ref, const double* E_low, const double* gamma_ref,
                           const double* n_exp, double mass_amu, double T_ref, double cutoff,
                           const double* q_ratio, int n_T, int n_p, int64_t n_hi,
                           const double* T_nodes, const double* p_nodes, const double* wl_hi,
                           double* kernel_ms);
/* Reads back points [lo, lo + n) of row (t, p) of any cross-section (uploaded, synthetic or
 * from lines) into out[n]. */
int frei_xsec_values(frei_xsec* x, int t, int p, int64_t lo, int64_t n, float* out);
/*
 * binned_opacity for this species onto a grid: bins wl_bins[n_bins+1] (µm, ascending) with
 * centres lam[n_bins] (µm).  Target nodes T_nodes[n_T] (K) x p_nodes[n_p] (bar) each take
 * the nearest source node (xarray interp 'nearest', extrapolating; opacity.py:26-29).
 *   mode FREI_BIN_GROUPIES (binned_opacity default, opacity.py:126-146): per bin the
 *     reference's float32 unit-step trapezoid (interp.py:176-194) x bin width x 1e-3;
 *   mode FREI_BIN_EXACT (Grid.load_opacities default, opacity.py:148-167): per non-empty
 *     bin the trapezoid integral / bin span (NaN for single-point bins) at the bin's mean
 *     wavelength, then linear interpolation/extrapolation onto lam.
 * out[n_p][n_T][n_bins] float64 on the host (NULL: leave the result on the device, for
 * timing).
 */
int frei_xsec_bin(frei_xsec* x, int mode, const double* wl_bins, const double* lam,
                  int64_t n_bins, const double* T_nodes, int n_T, const double* p_nodes,
                  int n_p, double* out);
/* HIP-event timing of the binning kernels: returns the accumulated milliseconds and calls
 * since the last reset; on = 1/0 enables/disables and resets, on = -1 only reads. */
int frei_xsec_timing(frei_xsec* x, int on, double* total_ms, int* n_calls);
/*
 * Same binning, written straight into species s of a context (no host round trip): the
 * context's wavelength slice is [lam_lo, lam_lo + n_lam) of the global grid
 * (wl_bins[n_bins+1], lam[n_bins]); the table gets nodes p_nodes (bar) x T_nodes (K).
 */
int frei_set_table_binned(frei_ctx* ctx, int s, frei_xsec* x, int mode, const double* wl_bins,
                          const double* lam, int64_t n_bins, int64_t lam_lo,
                          const double* T_nodes, int n_T, const double* p_nodes, int n_p);

/*
 * K18: correlated-k tables (no reference counterpart; HELIOS-K gives its line-by-line calculator
 * this second output for HELIOS).
 *
 * Premix.  out = a new cross-section on the sources' device, nodes and axis with
 *   out[t][p][i] = float32(acc),  acc = +0.0, then for s = 0 .. n_src - 1 in this order
 *   acc = acc + weight[s][t][p] * double(src_s[t][p][i])       (the product rounded, then the sum)
 * weight[n_src][n_T][n_p] are the mass mixing ratios at the sources' own nodes.  The result is an
 * ordinary frei_xsec: K6 bins it, frei_xsec_values reads it back, frei_xsec_destroy frees it; the
 * sources stay as they are.  Correlated-k needs it: adding the k(g) of several species at equal g
 * would treat their lines as perfectly correlated, so the mixture is sorted, not the species.
 * Errors, all found on the host before any device call, each naming the first offender:
 * n_src < 1, a null source, sources on different devices, sources whose T_nodes, p_nodes or wl_hi
 * are not element for element equal, a weight that is not finite or is negative.  *kernel_ms (may
 * be NULL) receives the HIP-event time of the kernel.
 */
int frei_xsec_mix(frei_xsec** out, int n_src, frei_xsec* const* src, const double* weight,
                  double* kernel_ms);
/*
 * The k-distribution of x on bins wl_bins[n_bins + 1] (µm, strictly ascending) at the quadrature
 * points g[n_g] (each finite and in (0, 1), any order; 1 <= n_g <= 64), for target nodes
 * T_nodes[n_T] (K) x p_nodes[n_p] (bar).  out[n_p][n_T][n_bins][n_g] float64 on the host (NULL:
 * leave the result on the device, for timing); counts[n_bins] (may be NULL) receives the points
 * per bin.
 *
 * Bin membership is K6's: bin k holds the points wl_bins[k] < wl <= wl_bins[k + 1], the last bin
 * wl < wl_bins[n_bins] (pandas.cut right-closed on the cropped axis).  Every target node takes
 * its nearest source node as in frei_xsec_bin, and target nodes that select one source row get
 * the same values.  Per (source row, bin) with n points:
 *   the float32 values, with -0 made +0 and every NaN the canonical quiet NaN, are sorted
 *   ascending with NaN last (np.sort's order): s_0 ... s_{n-1};
 *   per g_q the plan, on the host in the C++ runtime in fp64:
 *     t = g_q n - 0.5,  j = clamp(floor(t), 0, n - 2),  f = clamp(t - j, 0, 1);
 *   k = double(s_j) + f (double(s_{j+1}) - double(s_j)), unfused;
 *   n = 1: k = double(s_0);  n = 0: k = NaN.
 * A bin of more than 32768 points is an error that names the bin and its count, and nothing is
 * launched: a bin's keys are sorted in LDS (32768 float32 keys are 128 KiB of the 160 KiB); a
 * merge pass for wider bins is out of scope.  Every argument error is found before any device
 * call.  Two kernel forms, chosen by bin size, give the same bits (frei_kdist.hip;
 * FREI_KDIST_FORM = auto, block or wave selects one for diagnostics).  Timing: frei_xsec_timing.
 */
int frei_xsec_kdist(frei_xsec* x, const double* wl_bins, int64_t n_bins, int n_g, const double* g,
                    const double* T_nodes, int n_T, const double* p_nodes, int n_p, double* out,
                    int64_t* counts);
/*
 * The same k-distribution written straight into species s of a context, as
 * frei_set_table_binned does: the context's n_lam columns are [col_lo, col_lo + n_lam) of the
 * n_bins * n_g columns (column b * n_g + q is bin b at g_q); the table gets nodes p_nodes (bar) x
 * T_nodes (K).
 */
int frei_set_table_kdist(frei_ctx* ctx, int s, frei_xsec* x, const double* wl_bins, int64_t n_bins,
                         int n_g, const double* g, const double* T_nodes, int n_T,
                         const double* p_nodes, int n_p, int64_t col_lo);

/*
 * K19: a mixture's k-table from the species' k-tables by random overlap with resort-and-rebin
 * (no reference counterpart; the method of Lacis & Oinas 1991 as every correlated-k code uses it).
 *
 * A frei_klib holds n_src k-tables K_s[n_p][n_T][n_bins][n_g] (float64) resident on one device.
 * All share the nodes p_nodes[n_p] (bar) x T_nodes[n_T] (K), the bins wl_bins[n_bins + 1] (µm,
 * strictly ascending) and one quadrature: g[n_g] strictly ascending in (0, 1), w[n_g] finite and
 * positive, 1 <= n_g <= 64.
 *
 * Fixed-point weights.  W_q = llrint(w_q 2^30) in uint64, on the host; every W_q >= 1 and
 * Wt = sum W_q <= 2^31, anything else is an argument error naming q.  The pair weights W_i W_j
 * and their prefix sums stay below 2^62 in uint64: they are exact, so the result cannot depend
 * on the order of the scan.  The interval of g-point q is [E_q, E_{q+1}) with
 * E_q = Wt sum_{q' < q} W_q', in units of Wt^2.
 *
 * Mixing.  A composition is x[n_src][n_p][n_T], finite and >= 0: the mass mixing ratios at the
 * table's nodes.  Per (composition, node, bin) start from a[q] = x_0 K_0[q]; then for
 * s = 1 .. n_src - 1, in this order:
 *   1. b[r] = x_s K_s[r].  Pair e = q n_g + r has the value v_e = a[q] + b[r] (the products
 *      rounded, then the sum, unfused) and the weight u_e = W_q W_r.
 *   2. The pairs are ordered by (v, e) ascending; v is compared as K18 compares: -0 as +0, every
 *      NaN the canonical quiet NaN and last.  Ties go to the smaller e, so the order is total
 *      whatever network sorts it.  Neither a nor b is assumed monotone.
 *   3. C_e is the exact exclusive prefix sum of u in that order: pair e covers [C_e, C_e + u_e).
 *   4. Per q, over the pairs that overlap q's interval, in sorted order: acc = +0.0, then
 *      acc = acc + double(ov_e) log(v_e), ov_e the exact integer overlap (> 0);
 *      a'[q] = exp(acc / double(W_q Wt)) — the weight-averaged geometric mean of k over the
 *      interval.  log(0) = -inf gives 0; a negative or NaN value gives NaN in exactly the
 *      intervals it overlaps.
 *   5. a = a'.
 * The result is out[n_p][n_T][n_bins][n_g] = a; with n_src = 1 it is x_0 K_0, with no log or exp.
 *
 * frei_klib_set copies a host table into slot s; frei_klib_set_kdist writes K18's k-distribution
 * of a resident cross-section (frei_xsec_kdist at the library's nodes, bins and g) straight into
 * slot s.  frei_klib_mix mixes n_comp compositions x[n_comp][n_src][n_p][n_T] into
 * out[n_comp][n_p][n_T][n_bins][n_g] on the host (NULL: leave the result on the device, for
 * timing).  form: 0 automatic (the wave form for n_g <= 2, the block form above, as measured),
 * 1 the wave form (n_g <= 8 only: one pair per lane), 2 the block form; both give the same bits
 * (frei_kmix.hip).  With form = 0, FREI_KMIX_FORM = auto, wave or block selects one
 * for diagnostics.  *kernel_ms (may be NULL)
 * receives the HIP-event time of the kernel.
 *
 * Every argument error is found on the host before any device call and names the first offender:
 * a null pointer, a size below 1, n_g > 64, g not ascending in (0, 1), a bad weight, a slot out of
 * range or not set, an x that is not finite or is negative, a device mismatch.
 */
typedef struct frei_klib frei_klib;
int frei_klib_create(frei_klib** out, int device, int n_src, int n_p, int n_T, int64_t n_bins,
                     int n_g, const double* wl_bins, const double* g, const double* w,
                     const double* p_nodes, const double* T_nodes);
int frei_klib_destroy(frei_klib* lib);
int frei_klib_set(frei_klib* lib, int s, const double* k);
int frei_klib_set_kdist(frei_klib* lib, int s, frei_xsec* x);
int frei_klib_mix(frei_klib* lib, int n_comp, const double* x, double* out, int form,
                  double* kernel_ms);
/*
 * One composition's mixture (x[n_src][n_p][n_T]) written straight into species s of a context,
 * as frei_set_table_kdist writes a k-distribution: the context's n_lam columns are
 * [col_lo, col_lo + n_lam) of the library's n_bins * n_g; the table gets the library's nodes.
 * The mix runs on the context's stream (the library's tables are complete when frei_klib_set and
 * frei_klib_set_kdist return) and the call returns when the table is complete.
 */
int frei_set_table_kmix(frei_ctx* ctx, int s, frei_klib* lib, const double* x, int64_t col_lo);

/*
 * K20: a batch of correlated-k atmospheres, one composition each.  A batched context shares its
 * species tables between atmospheres and forms each atmosphere's table as the linear species sum
 * K7; the k(g) of several species do not add, so a k-mix batch keeps one mixed table per
 * atmosphere instead, in the slot K7 writes ([n_atm][n_p][n_T][pitch], the only table the batched
 * sweeps read), filled by K19's kernels.
 *
 * frei_set_table_kmix_batch: ctx comes from frei_ctx_create_batch with n_species = 1, after
 * frei_set_grid; x is [n_atm][n_src][n_p][n_T], frei_klib_mix's layout.  Species 0 gets the
 * library's nodes and composition 0's mixture (as frei_set_table_kmix writes it), the context
 * records the library and a copy of x, and every mixing ratio becomes 1.  Each time the context
 * builds its per-atmosphere tables (in this call, and after any call that rebuilds the metadata),
 * atmosphere m's table is the random-overlap mixture of x[m] on the library's nodes, columns
 * [col_lo, col_lo + n_lam): bitwise what frei_klib_mix returns for that composition, written
 * straight into the table (K7 is not launched).  As for K7 only the pressure rows some layer sits
 * on are mixed; the other rows, the column padding up to the pitch and each atmosphere's
 * 64-element tail are zero.  A context with n_atm = 1 sweeps species 0's table: composition 0.
 * Everything that runs on a batched context runs unchanged afterwards.  The library must outlive
 * the context's use of it (the context keeps the pointer, not the library).
 *
 * frei_kmix_batch_update: new compositions x[n][n_src][n_p][n_T] for the atmospheres
 * [atm_lo, atm_lo + n).  Only their rows are mixed again, in place, on the context's stream: no
 * metadata rebuild, no allocation of a table; the other atmospheres' tables keep their bits.  The
 * step a retrieval loop repeats.
 *
 * frei_get_table_batch: out[n_p][n_T][n_lam] is atmosphere atm's table as the sweeps read it
 * (tests, diagnostics).  On a k-mix batch T is in the library's node order; on any other batched
 * context with a per-atmosphere table it is ascending, as the table is stored.
 *
 * Every argument error is found on the host before any device call and names the first offender:
 * a null argument; a context not made by frei_ctx_create_batch, or with n_species != 1;
 * frei_set_grid not yet called; columns outside the library's n_bins * n_g; a device mismatch; a
 * slot that holds no table; an x that is not finite or is negative, named x[m][s][p][t] (m counts
 * from the first composition passed); atm_lo / n or atm out of range; an update on a context that
 * holds no k-mix batch.  frei_set_chemistry_batch on a k-mix batch and frei_set_table_kmix_batch
 * on a chemistry batch are refused, and so is a frei_set_mmr with any value other than 1 ("the
 * compositions hold the mixing ratios").  After mixing, a NaN in a row that a layer uses fails
 * the call that mixed and names the atmosphere, as batched contexts refuse NaN tables.  Any
 * frei_set_table* call on the context ends the k-mix batch.
 */
int frei_set_table_kmix_batch(frei_ctx* ctx, frei_klib* lib, const double* x, int64_t col_lo);
int frei_kmix_batch_update(frei_ctx* ctx, int atm_lo, int n, const double* x);
int frei_get_table_batch(frei_ctx* ctx, int atm, double* out);

/*
 * Stellar spectrum binning (phoenix.py:13-17, 43-52).  A frei_sspec is a library of model
 * spectra on one shared wavelength axis: flux[n_spec][n_hi] float64 resident in HBM on
 * wl_hi[n_hi] (um, strictly ascending).
 */
typedef struct frei_sspec frei_sspec;
int frei_sspec_create(frei_sspec** out, int device, const double* flux, int n_spec,
                      int64_t n_hi, const double* wl_hi);
/*
 * Bin every spectrum onto wl_bins[n_bins+1] (um, strictly ascending).  Bin k holds the points
 * wl_bins[k] < wl <= wl_bins[k+1] (pandas.cut, right-closed, the last bin too); its value is
 * the trapezoid integral over its points divided by their span (max - min).
 * out[n_spec][n_bins] is aligned with the bins (NaN: bins of < 2 points); NULL leaves it on
 * the device.  counts[n_bins] receives the points per bin (may be NULL).  form: 0 automatic
 * (by mean points per non-empty bin), 1 one lane per bin, 2 one wave per bin (a group of 4 to
 * 32 lanes per bin where the bins hold fewer points than a wave has lanes); *form_used and
 * *kernel_ms (HIP events around the kernel only) may be NULL.
 */
int frei_sspec_bin(frei_sspec* s, const double* wl_bins, int64_t n_bins, int form,
                   double* out, int64_t* counts, int* form_used, double* kernel_ms);
int frei_sspec_destroy(frei_sspec* s);

/*
 * Synthetic observations (K10): native-resolution spectra taken to the channels of an
 * instrument and scored against data.  The reference has no counterpart; this is the definition.
 * An instrument is n_chan channels on a native wavelength axis of n_lam points.  Channel k covers
 * the contiguous native indices first[k] .. first[k] + count[k] - 1 and has one weight per
 * covered index, stored back to back: weights[off_k + t], off_k the prefix sum of the counts.
 * Channels may overlap, come in any order and hold zero weights.  Required (frei_obs_create
 * checks it on the host before it touches a device, naming the channel): count[k] >= 1,
 * 0 <= first[k], first[k] + count[k] <= n_lam, every weight finite and >= 0, every channel's
 * weight sum > 0.  Plan and weights stay resident on `device` with the handle.
 */
typedef struct frei_obs frei_obs;
int frei_obs_create(frei_obs** out, int device, int64_t n_lam, int64_t n_chan,
                    const int64_t* first, const int64_t* count, const double* weights);
/*
 * Apply the instrument to x[n_atm][n_lam].  Optional libraries num[n_lib][n_lam] and
 * den[n_lib][n_lam]; select[n_atm] is the library row of atmosphere m (NULL: row 0 for all;
 * ignored without num and den); scale[n_atm] (NULL: 1).  With w = weights + off_k, i = first[k] + t:
 *   N_mk = sum_t (w[t] * x[m][i]) * num[select_m][i]        (without num: w[t] * x[m][i])
 *   D_mk = sum_t  w[t] * den[select_m][i]                    (without den: sum_t w[t])
 *   obs[m][k] = scale_m * (N_mk / D_mk)
 * and, with data[n_chan], sigma[n_chan] and chi2 given,
 *   chi2[m] = sum_k ((obs[m][k] - data[k]) / sigma[k])^2;
 * sigma[k] = +inf makes channel k contribute exactly 0, sigma[k] <= 0 or NaN is an error.
 * x is a host array (uploaded for the call), or NULL with a context: the source is then the
 * emergent row F_up[n_layers - 1] of every atmosphere, in place in the flux state (what
 * frei_post_batch reads with spectra = NULL); that needs n_atm == the context's atmosphere
 * count, n_lam == its n_lam and the same device.  (A context of a wavelength slice therefore
 * does not fit an instrument on the whole axis: a channel may straddle slices.)
 * form: 0 automatic (by the mean points per channel), 1 one lane per channel (its points in
 * ascending t), 2 one group of 4 to 64 lanes per channel (lane l of G sums t = l, l + G, ... in
 * order, the G sums combine in the xor butterfly G/2, ..., 1; G follows from the mean points per
 * channel).  chi2: lane l of 64 sums k = l, l + 64, ..., then the butterfly 32, ..., 1.  No
 * atomics and no contraction of products: every result is bitwise the same from call to call,
 * and row m of a batched call is bitwise the call on that row alone.  NaN or inf in x reaches
 * exactly the channels that cover it; nothing in x, num or den is checked.
 * Outputs obs[n_atm][n_chan]; chi2[n_atm], *form_used and *kernel_ms (HIP events around the
 * kernels only) may be NULL.  Errors (handle and context stay usable): null handle or obs, x and
 * ctx both null, a select entry outside [0, n_lib), chi2 without data or sigma, bad sigma, a
 * context of another shape or device.
 */
int frei_obs_apply(frei_obs* o, frei_ctx* ctx, const double* x, int n_atm, const double* num,
                   const double* den, int n_lib, const int32_t* select, const double* scale,
                   const double* data, const double* sigma, int form, double* obs, double* chi2,
                   int* form_used, double* kernel_ms);
int frei_obs_destroy(frei_obs* o);

/*
 * Doppler cross-correlation (K12): batched templates against high-resolution data over a grid
 * of trial velocities.  The reference has no counterpart; this is the definition.
 * A correlator holds, resident on `device` with the handle: a native axis of n_lam >= 2 points,
 * n_pix >= 1 data pixels, n_vel >= 1 trial velocities, n_exp >= 1 exposures; the plan
 * idx[n_vel][n_pix] (0 <= idx <= n_lam - 2) and frac[n_vel][n_pix] (finite, in [0, 1]): the
 * native bracket and the weight of its upper point at which pixel p samples a template shifted
 * by velocity v; the weighted data a[n_exp][n_pix] (finite, any sign) and the pixel weights
 * w[n_pix] (finite, >= 0, sum > 0).  frei_ccf_create checks all of it on the host before it
 * touches a device and names the first offending index.
 */
typedef struct frei_ccf frei_ccf;
int frei_ccf_create(frei_ccf** out, int device, int64_t n_lam, int64_t n_pix, int n_vel,
                    const int32_t* idx, const double* frac, int n_exp, const double* a,
                    const double* w);
/*
 * Template pre-pass, once per call over [n_atm][n_lam]:
 *   y[m][j] = scale_m * (x[m][j] / den[select_m][j]) - offset_m
 * den[n_lib][n_lam] with select[n_atm] (NULL: row 0 for all; ignored without den), scale[n_atm]
 * and offset[n_atm] are each optional; an absent one drops its operation (it is not replaced
 * by a multiplication by 1 or a subtraction of 0).  x is a host array [n_atm][n_lam] (uploaded
 * for the call), or NULL with a context: the source is then the emergent row F_up[n_layers - 1]
 * of every atmosphere, in place in the flux state, under the rules of frei_obs_apply (n_atm ==
 * the context's atmosphere count, n_lam == its n_lam, the same device; a context of a
 * wavelength slice does not fit: a pixel's bracket may straddle slices).
 * Sums: for atmosphere m, velocity v, pixel p, with j = idx[v][p] and t = frac[v][p],
 *   g = y[m][j] + t * (y[m][j+1] - y[m][j])            (three operations, never contracted)
 *   S_fg[m][e][v] = sum_p a[e][p] * g
 *   S_g[m][v]     = sum_p w[p] * g
 *   S_gg[m][v]    = sum_p (w[p] * g) * g
 * Order: the pixels are taken in chunks of 4096 and the chunk sums are added in ascending chunk
 * order; every term enters by one fused multiply-add (a * g, w * g, and (w * g) rounded then
 * times g).  Within a chunk starting at p0,
 *   form 1 (VALU): lane l of 64 accumulates the pixels p0 + l, p0 + l + 64, ... in order and
 *     the 64 lane sums combine in the xor butterfly 32, 16, ..., 1;
 *   form 2 (fp64 MFMA, v_mfma_f64_16x16x4_f64): the chunk goes in groups of 16 pixels; step s
 *     = 0 .. 3 of the group at q adds the pixels q + s, q + 4 + s, q + 8 + s, q + 12 + s to S_fg
 *     in the matrix unit (A = 16 velocities x 4 pixels of g, B = 4 pixels x 16 exposures of a),
 *     groups and steps ascending, the last group padded with g = 0, a = 0; S_g and S_gg
 *     accumulate beside it on the VALU, lane k of 4 taking the pixels q + 4 k + s, s = 0 .. 3, of
 *     every group in order, combined as (k0 + k1) + (k2 + k3).
 * For a given form the order depends on n_pix alone and there are no atomics: every result is
 * bitwise the same from call to call, row m of a batched call is bitwise the call on that row
 * alone, an output is bitwise unchanged when other exposures or velocities are added to or
 * removed from the handle, and when other outputs are or are not asked for.  A NaN or inf in y
 * reaches exactly the outputs whose pixels touch it (with t = 0, 0 * NaN also touches); nothing
 * in x or den is checked.
 * form: 0 automatic (form 2 from 9 exposures, form 1 below: the measured crossover), 1 or 2 as
 * above; *form_used receives the form that ran.
 * Outputs sfg[n_atm][n_exp][n_vel], sg[n_atm][n_vel], sgg[n_atm][n_vel]: any may be NULL, not all
 * three (but see keep mode, frei_ccf_keep below); nothing is computed or allocated for an absent
 * one.  *form_used and *kernel_ms (HIP
 * events around the kernels only) may be NULL.  Errors (handle and context stay usable): null
 * handle, all outputs null, x and ctx both null, a select entry outside [0, n_lib), a context
 * of another shape or device.
 */
int frei_ccf_apply(frei_ccf* c, frei_ctx* ctx, const double* x, int n_atm, const double* den,
                   int n_lib, const int32_t* select, const double* scale, const double* offset,
                   int form, double* sfg, double* sg, double* sgg, int* form_used,
                   double* kernel_ms);
int frei_ccf_destroy(frei_ccf* c);

/*
 * Broadening (K13): batched native-resolution spectra convolved with a kernel tabulated in
 * velocity (a planet's rotation, an instrument's line-spread function, or both).  The reference
 * has no counterpart; this is the definition.
 * A broadener on a native axis lam[n_lam] (strictly ascending, n_lam >= 2) holds, resident on
 * `device` with the handle:
 *   u[j] = c ln(lam[j]), c = 299792.458 km/s, formed on the host and passed in (never recomputed
 *     on the device);
 *   tw[j], the trapezoid weights of the axis in u: half the neighbouring gaps, one-sided at the
 *     ends;
 *   the kernel table tab[n_tab], n_tab odd and >= 3, h = (n_tab - 1) / 2, every value finite and
 *     >= 0, sampled at the velocities (k - h) dv, dv > 0: its half-width is H = h * dv;
 *   the window of every output i, first[i] and count[i]: the contiguous run of j with
 *     |u[j] - u[i]| <= H, decided with that very subtraction in fp64.  It contains i and is
 *     truncated at the ends of the axis (no padding, no wrap);
 *   norm[i], below.
 * The weight of input j in output i, by exactly these IEEE operations (never contracted):
 *   d = u[j] - u[i];  q = d * inv_dv + h;  k = clamp(floor(q), 0, n_tab - 2);  f = q - k
 *   K = tab[k] + f * (tab[k+1] - tab[k]);  w_ij = tw[j] * K
 * with inv_dv = 1 / dv formed once on the host and passed in.
 *   norm[i] = sum_j w_ij over the window, ascending j, plain additions; frei_brd_create forms it
 *     on the host and uploads it (frei_brd_norm reads it back).
 *   out[m][i] = (sum_j w_ij * x[m][j]) / norm[i]: every term enters by one fused multiply-add,
 *     one division at the end.  Renormalising over the truncated window is the edge rule.
 * frei_brd_create checks on the host, before it touches a device, naming the first offending
 * index: u finite and strictly ascending, tw finite and >= 0, dv and inv_dv > 0, n_tab odd and
 * >= 3, the table finite and >= 0, every window on the axis, holding its own point, agreeing
 * with the criterion above (its two ends within H, the points just outside not) and of at most
 * FREI_BRD_MAX_COUNT points, every norm[i] finite and > 0.
 */
#define FREI_BRD_MAX_COUNT 4096
typedef struct frei_brd frei_brd;
int frei_brd_create(frei_brd** out, int device, int64_t n_lam, const double* u, const double* tw,
                    const int32_t* first, const int32_t* count, int n_tab, double dv,
                    double inv_dv, const double* tab);
/* norm[n_lam] as frei_brd_create formed it. */
int frei_brd_norm(frei_brd* b, double* norm);
/*
 * Broaden x[n_atm][n_lam], a host array (uploaded for the call), or NULL with a context: the
 * source is then the emergent row F_up[n_layers - 1] of every atmosphere, in place in the flux
 * state on the context's stream, under the rules of frei_obs_apply and frei_ccf_apply (n_atm ==
 * the context's atmosphere count, n_lam == its n_lam, the same device; a context of a wavelength
 * slice does not fit: a window may straddle slices).
 * out[n_atm][n_lam] receives the result; it may be NULL when keep is set.  With keep != 0 the
 * result also stays in a device buffer the handle owns until the next frei_brd_apply (kept or
 * not, successful or not once its arguments are accepted) or frei_brd_destroy;
 * frei_ccf_apply_brd and frei_obs_apply_brd read it there.
 * Order of summation:
 *   form 1 (VALU): one lane per output i; the taps j = first[i] .. first[i] + count[i] - 1 in
 *     ascending order, acc = fma(w_ij, x[m][j], acc) from acc = 0.
 *   form 2 (fp64 MFMA, v_mfma_f64_16x16x4_f64): tiles of the 16 consecutive outputs i0 .. i0 +
 *     15 (i0 a multiple of 16) x 16 atmospheres.  The tile's span is jlo = first[i0] to jhi =
 *     first[il] + count[il], il = min(i0 + 15, n_lam - 1): the union of its windows.  Step s = 0,
 *     1, ... while jlo + 4 s < jhi, ascending, adds the points jlo + 4 s + (0 .. 3) in the matrix
 *     unit: A = 16 outputs x 4 points of weights, each lane forming its own w_ij, exactly 0 where
 *     j lies outside that output's own window (and for outputs past the axis); B = 4 points x 16
 *     atmospheres of x, 0 for points at or past jhi and for atmospheres at or past n_atm.  x
 *     reaches B through LDS in chunks of 64 points from jlo (read in rows of consecutive points);
 *     the trailing steps of a chunk that begin at or past jhi are not taken.
 *   form 0 picks form 2 from 5 atmospheres on where the windows hold 21 points or more on
 *     average (sum of count / n_lam) and from 2 atmospheres on where they hold 81 or more, form
 *     1 otherwise: the measured crossover
 *     (tools/broaden_probe.py, profiles/r12/broaden/README.md); *form_used receives the form
 *     that ran.
 * No atomics; for a given form and handle the order of every sum is fixed: results are bitwise
 * the same from call to call, and row m of a batched call is bitwise the call on that row alone.
 * Form 1 returns a spectrum that is constant at 1 or any other power of two exactly: numerator
 * and norm are then the same sum (scaled exactly).  Non-finite input: form 1 carries a NaN or inf
 * in x[m][j] to exactly the outputs i of row m whose window holds j.  Form 2 carries it to those
 * and, because 0 * NaN enters the product (B is not masked), to every other output of a 16-output
 * tile whose span [jlo, jhi) holds j — of row m alone; other rows and tiles are untouched.
 * Nothing in x is checked.
 * *form_used and *kernel_ms (HIP events around the kernel only) may be NULL.  Errors (handle and
 * context stay usable): null handle, x and ctx both null, out null without keep, a context of
 * another shape or device.
 */
int frei_brd_apply(frei_brd* b, frei_ctx* ctx, const double* x, int n_atm, int form,
                   double* out, int keep, int* form_used, double* kernel_ms);
int frei_brd_destroy(frei_brd* b);
/*
 * frei_ccf_apply and frei_obs_apply with the result `src` kept (frei_brd_apply with keep) as
 * their x: a third source beside the host array and the context, read where it lies.  The other
 * arguments and the results are those of frei_ccf_apply / frei_obs_apply, bitwise what they give
 * for a host copy of the same numbers.  Errors: a null broadener, one with nothing kept, or one
 * of another n_lam, n_atm or device.
 */
int frei_ccf_apply_brd(frei_ccf* c, frei_brd* src, int n_atm, const double* den, int n_lib,
                       const int32_t* select, const double* scale, const double* offset,
                       int form, double* sfg, double* sg, double* sgg, int* form_used,
                       double* kernel_ms);
int frei_obs_apply_brd(frei_obs* o, frei_brd* src, int n_atm, const double* num,
                       const double* den, int n_lib, const int32_t* select, const double* scale,
                       const double* data, const double* sigma, int form, double* obs,
                       double* chi2, int* form_used, double* kernel_ms);

/*
 * Keep mode of a correlator.  frei_ccf_keep(c, 1) switches it on: every later successful
 * frei_ccf_apply / frei_ccf_apply_brd then also leaves the sums it computed in device buffers
 * the handle owns, complete, until the next apply (successful or not once its arguments are
 * accepted), frei_ccf_keep(c, 0) or frei_ccf_destroy; frei_stack_apply reads them there.  The
 * sums computed are those whose host pointer is given; in keep mode all three host pointers may
 * be NULL, and all three sums are then computed and kept and none is copied back.  What is copied
 * back is bitwise what is kept.  frei_ccf_keep(c, 0) frees the buffers and restores the default:
 * with keep off "sfg, sg and sgg are all null" stays an error and nothing else changes.
 * Error: a null handle.
 */
int frei_ccf_keep(frei_ccf* c, int on);

/*
 * Orbital stack (K14): a detection statistic formed from the sums of frei_ccf_apply and summed
 * over the exposures along trial orbits, one K_p-V_sys map per atmosphere.  The reference has no
 * counterpart; this is the definition.
 * A stacker holds the n_vel >= 2 trial velocities vel[n_vel] of the values (finite, strictly
 * ascending; not assumed uniform), n_exp >= 1 exposures, n_kp >= 1 trial orbits with
 * dv[n_kp][n_exp], the planet's line-of-sight velocity of trial k at exposure e (finite; formed
 * by the caller, K_p[k] sin(2 pi phase_e) for a circular orbit, and never recomputed on the
 * device), v_obs[n_exp] (finite) and n_vsys >= 1 systemic velocities vsys[n_vsys] (finite, any
 * order).  frei_stack_create checks all of it on the host, naming the first offending index, and
 * touches no device: the arrays are uploaded by the first frei_stack_apply and stay resident on
 * `device` with the handle from then on.
 *
 * Statistic, per atmosphere m, exposure e and velocity v, by exactly these IEEE operations in
 * this order, never contracted (frei_amd.crosscorr.CrossCorrelation._moments, .ccf, .loglike):
 *   gbar = sg[m][v] / W
 *   C_fg = sfg[m][e][v] - gbar * S_wf[e]
 *   V_g  = sgg[m][v] - sg[m][v] * gbar
 *   V_f  = S_wff[e] - (S_wf[e] * S_wf[e]) / W                        (formed on the host)
 *   statistic 1 (ccf):     values = C_fg / sqrt(V_f * V_g)
 *   statistic 2 (loglike): values = (-(n_eff / 2)) * log(((V_f - 2 * C_fg) + V_g) / W)
 * Division and square root are the correctly rounded ones; log is the device library's.  With
 * statistic 0 sfg already holds the values [n_atm][n_exp][n_vel]; sg, sgg, W, S_wf, S_wff and
 * n_eff are ignored and may be NULL or 0.  Nothing is checked for sign: a non-positive variance
 * gives the NaN or inf of the host methods.
 *
 * Stack, per atmosphere m, trial k and systemic velocity s, with f = values[m][e][:]:
 *   u = (vsys[s] + dv[k][e]) + v_obs[e]                              (two additions, this order)
 *   u clamped to [vel[0], vel[n_vel-1]]
 *   j = the largest index with vel[j] <= u, limited to n_vel - 2     (a binary search)
 *   t = (u - vel[j]) / (vel[j+1] - vel[j])
 *   val = f[j] + t * (f[j+1] - f[j])                                 (three operations)
 *   map[m][k][s] = sum of val over e = 0 .. n_exp - 1, ascending, one accumulator from 0, plain
 *     additions.
 * Beyond the ends of vel the end value holds (j = 0, t = 0 below; j = n_vel - 2, t = 1 above).
 * A NaN or inf in values[m][e][i] reaches exactly the outputs (m, k, s) whose bracket at exposure
 * e is j = i or j = i - 1, whatever t is (0 * NaN also touches).  One lane owns one (k, s) and a
 * tile of 8 atmospheres: bracket and t are formed once for the tile.
 * form 1 searches a copy of vel in LDS (n_vel <= FREI_STACK_LDS_VEL), form 2 searches vel in
 * global memory (any n_vel); form 0 takes form 1 where it fits.  The forms give the same bits.
 * No atomics; the order of summation depends on n_exp alone: results are bitwise the same from
 * call to call and between the forms, row m of a batched call is bitwise the call on that row
 * alone, an output (k, s) is bitwise unchanged when other trials or systemic velocities are added
 * to or dropped from the handle, and the map of statistic 1 or 2 is bitwise the map of statistic
 * 0 fed with the `values` the same call returned.
 *
 * Source of the sums: host arrays sfg[n_atm][n_exp][n_vel], sg and sgg [n_atm][n_vel] (uploaded
 * for the call; statistic 0 needs sfg alone), or all three NULL with `kept`: a correlator in keep
 * mode, whose last apply's sums are read where they lie (statistic 0 stacks its kept sfg).
 * map[n_atm][n_kp][n_vsys] is required; values[n_atm][n_exp][n_vel] (what was stacked) may be
 * NULL.  *form_used and *kernel_ms (HIP events around the statistic and stack kernels only) may
 * be NULL.  Errors, all found before any device call (handles stay usable): a null handle or a
 * null map; n_atm < 1; a statistic outside 0 .. 2 or a form outside 0 .. 2; form 1 with n_vel
 * beyond FREI_STACK_LDS_VEL; neither host sums nor a kept source; host sums without sfg, or
 * without sg or sgg for statistic 1 or 2; statistic 1 or 2 without S_wf, S_wff or with W = 0; a
 * correlator that holds nothing kept, or lacks a kept sum the statistic needs; kept sums whose
 * n_atm, n_exp or n_vel differ from the call's or the stacker's; different devices; n_kp or
 * n_atm / 8 beyond the launch grid (65535).
 */
#define FREI_STACK_LDS_VEL 2048
typedef struct frei_stack frei_stack;
int frei_stack_create(frei_stack** out, int device, int n_exp, int n_vel, const double* vel,
                      int n_kp, const double* dv, const double* v_obs, int n_vsys,
                      const double* vsys);
int frei_stack_apply(frei_stack* s, frei_ccf* kept, int n_atm, const double* sfg,
                     const double* sg, const double* sgg, int statistic, double W,
                     const double* S_wf, const double* S_wff, double n_eff, double* map,
                     double* values, int form, int* form_used, double* kernel_ms);
int frei_stack_destroy(frei_stack* s);

/*
 * Model-grid interpolation (K15): spectra at arbitrary points between the node spectra of a
 * grid sweep, as weighted sums of a few nodes each, formed and kept on the device.  The
 * reference has no counterpart; this is the definition.
 * An interpolator on `device` holds a library of node spectra X[n_node][n_lam] in a buffer of its
 * own.  frei_itp_create checks n_lam >= 1, n_node >= 1 and n_lam / 512 <= 65535 (the launch grid)
 * and touches no device; the buffer is allocated by the first frei_itp_set_nodes.
 */
#define FREI_ITP_MAX_CORNERS 16
typedef struct frei_itp frei_itp;
int frei_itp_create(frei_itp** out, int device, int64_t n_lam, int n_node);
/*
 * Fill the library from one of the three sources of spectra: x, a host array [n_node][n_lam]; or
 * x NULL with ctx, the emergent row F_up[n_layers - 1] of every atmosphere of the context, copied
 * where it lies on the context's stream behind the work that wrote it, honouring the row stride
 * of the flux state; or x and ctx NULL with brd, what frei_brd_apply kept.  The context or the
 * broadener must hold n_node rows of n_lam points on the interpolator's device.  The rows are
 * copied: the source may be reused or closed once the call returns.  Setting nodes again replaces
 * the library; whatever frei_itp_apply kept ends with any frei_itp_set_nodes whose arguments are
 * accepted, successful or not, and after a failed one no nodes are set.
 * Errors: a null handle, all three sources null, a source of another shape or device, a broadener
 * with nothing kept.
 */
int frei_itp_set_nodes(frei_itp* itp, frei_ctx* ctx, frei_brd* brd, const double* x);
/*
 * Interpolate n_query spectra from the plan idx[n_query][n_corner] (int32, 0 <= idx < n_node)
 * and w[n_query][n_corner] (fp64), 1 <= n_corner <= FREI_ITP_MAX_CORNERS.  Per query q and
 * wavelength i, by exactly these IEEE operations, the corners in ascending c, one multiply and
 * one add per term, never contracted (NumPy's acc + w * x):
 *   acc = w[q][0] * X[idx[q][0]][i]
 *   acc = acc + w[q][c] * X[idx[q][c]][i]            for c = 1 .. n_corner - 1
 *   out[q][i] = acc
 * The device normalises, clamps and transforms nothing: what the weights mean (multilinear
 * corners, simplices, a barycentric scheme) is the caller's business.  A node may appear in
 * several corners of a query.  Nothing in w or X is checked.
 * out[n_query][n_lam] receives the result; it may be NULL when keep is set.  The result is formed
 * in a device buffer the handle owns, reused from call to call and grown when a call needs more.
 * With keep != 0 the result stays valid there until the next frei_itp_apply (kept or
 * not, successful or not once its arguments are accepted), frei_itp_set_nodes (likewise) or
 * frei_itp_destroy; frei_ccf_apply_itp, frei_obs_apply_itp and frei_brd_apply_itp read it there.
 * Two forms give the same bits (the operations per output above do not depend on the form):
 *   form 1 (gather): one lane owns two consecutive outputs (q, i), (q, i + 1) and reads its
 *     corners' node values from global memory 16 bytes at a time (the library's rows are padded
 *     to a 16-byte-aligned pitch).  The blocks of one tile of 512 wavelengths, over all queries,
 *     are consecutive in the grid, so the tile's slab of X (n_node x 4 KiB) is read from L2.
 *     Traffic at L2: n_corner reads per output.
 *   form 2 (LDS-staged): one workgroup of FREI_ITP_LDS_WAVES waves owns a tile of T consecutive
 *     wavelengths, stages X[0 .. n_node)[tile] in LDS once and runs over every query, wave v
 *     taking the queries v, v + FREI_ITP_LDS_WAVES, ...: idx and w of a query are uniform in
 *     its wave, lane l reads the LDS doubles at l + 64 k of a node's row (consecutive 8-byte
 *     addresses, conflict-free) and a row of out is written in runs of a whole tile.  HBM
 *     traffic: the library once plus the output once, whatever n_corner is.  A query's corners
 *     alone are multiplied in: a node it does not list never enters its sum.
 *     Tile-width rule: T is the widest of 256, 128 and 64 with n_node * T * 8 bytes <=
 *     FREI_ITP_LDS_BYTES (the CU's whole LDS, one workgroup per CU beyond half of it): 256 up to
 *     80 nodes, 128 up to 160, 64 up to FREI_ITP_LDS_MAX_NODES = 320.  A taller library is an
 *     error for form 2.
 *   form 0 takes form 2 where it fits, the axis gives at least 256 tiles (one workgroup per CU;
 *     fewer leave CUs idle whatever the query count), n_query >= FREI_ITP_LDS_FROM_QUERIES = 32
 *     and n_corner >= FREI_ITP_LDS_FROM_CORNERS = 12, form 1 otherwise: the crossover measured
 *     on MI355X at 256 nodes x 100k wavelengths (tools/interp_probe.py,
 *     profiles/r15/interp/README.md): at 16 corners form 2 wins from 64 queries on, at 8 the
 *     forms tie within the run-to-run spread, at 2 corners and for a single query form 1 wins;
 *     the thresholds are the midpoints of the timed neighbours (8 and 16 corners, 1 and 64
 *     queries).  *form_used receives the form that ran.
 * No atomics: results are bitwise the same from call to call and between the forms, row q of a
 * call is bitwise the call on that query alone, and an output does not change when other queries
 * or unused nodes are added.  A NaN or inf in X[n][i] reaches exactly the outputs (q, i) of the
 * queries that list node n in any corner, whatever its weight (0 * NaN also counts), and no other
 * wavelength or query, in both forms.
 * *form_used and *kernel_ms (HIP events around the kernel only) may be NULL.  Errors, all found on
 * the host before any device call, naming the first offending index (the handle stays usable): a
 * null handle; n_query < 1; n_corner outside its range; idx or w null; out null without keep; a
 * form outside 0 .. 2; an idx outside [0, n_node); form 2 with a library too tall; no nodes set.
 */
#define FREI_ITP_LDS_BYTES 163840
#define FREI_ITP_LDS_WAVES 16
#define FREI_ITP_LDS_MAX_NODES 320
#define FREI_ITP_LDS_FROM_QUERIES 32
#define FREI_ITP_LDS_FROM_CORNERS 12
int frei_itp_apply(frei_itp* itp, int n_query, int n_corner, const int32_t* idx, const double* w,
                   int form, double* out, int keep, int* form_used, double* kernel_ms);
int frei_itp_destroy(frei_itp* itp);
/*
 * frei_ccf_apply, frei_obs_apply and frei_brd_apply with the result `src` kept (frei_itp_apply
 * with keep) as their x: a fourth source beside the host array, the context and the broadener,
 * read where it lies.  The queries play the role of the atmospheres (n_atm = n_query): select,
 * scale, offset and den are per query.  The other arguments and the results are those of the
 * plain calls, bitwise what they give for a host copy of the same numbers.  Errors: a null
 * interpolator, one with nothing kept, or one of another n_lam, n_query or device.
 */
int frei_ccf_apply_itp(frei_ccf* c, frei_itp* src, int n_atm, const double* den, int n_lib,
                       const int32_t* select, const double* scale, const double* offset,
                       int form, double* sfg, double* sg, double* sgg, int* form_used,
                       double* kernel_ms);
int frei_obs_apply_itp(frei_obs* o, frei_itp* src, int n_atm, const double* num,
                       const double* den, int n_lib, const int32_t* select, const double* scale,
                       const double* data, const double* sigma, int form, double* obs,
                       double* chi2, int* form_used, double* kernel_ms);
int frei_brd_apply_itp(frei_brd* b, frei_itp* src, int n_atm, int form, double* out, int keep,
                       int* form_used, double* kernel_ms);

/*
 * Phase curves (K16): the columns of a context seen as the cells of a planet's surface and
 * integrated over the visible disk at every orbital phase, formed and kept on the device.  The
 * reference has no counterpart; this is the definition.
 * A phase integrator on `device` holds a geometry of n_cell >= 1 cells at n_phase >= 1 phases:
 *   select[n_cell]       the atmosphere (row of the context) of each cell, >= 0; several cells
 *                        may name the same row
 *   mu[n_phase][n_cell]  the cosine of the angle between the cell's normal and the observer at
 *                        that phase, finite and <= 1
 *   coef[n_phase][n_cell] the cell's weight in the disk integral, its solid angle times mu, formed
 *                        by the caller and never recomputed on the device
 * A pair (p, c) is visible exactly when mu[p][c] > 0.  Pairs with mu <= 0 are skipped: they are
 * not multiplied by zero and their coef is never read (it may be anything).  For a visible pair
 * imu = 1.0 / mu is formed here in fp64, as frei_emergent forms it, and must be finite; coef must
 * be finite and >= 0.  frei_phs_create checks all of it on the host, naming the first offending
 * index, and touches no device: the plan is uploaded by the first frei_phs_apply and stays
 * resident on `device` with the handle from then on.
 */
typedef struct frei_phs frei_phs;
int frei_phs_create(frei_phs** out, int device, int n_cell, int n_phase, const int32_t* select,
                    const double* mu, const double* coef);
/*
 * Integrate.  ctx, dtaus and T are those of frei_emergent: dtaus[n_atm][n_layers][n_lam] is a host
 * array to upload, or NULL for the device copy the last frei_run / frei_run_batch_ex(keep_dtaus)
 * left; T[n_atm][n_layers] is a host array, always given; a wavelength-slice context gives its
 * own columns.  Per phase p and wavelength j:
 *   I_pc      = the intensity frei_emergent defines for atmosphere select[c] at the angle
 *               mu[p][c], by that function's own operations: bitwise its intensity[select[c]][k][j]
 *               for mu[k] = mu[p][c]
 *   out[p][j] = sum over the visible cells c, ascending, of coef[p][c] * I_pc: the first visible
 *               term starts the sum, every later one enters by one multiply and one add, never
 *               contracted (frei_emergent's flux order; NumPy's acc + w * x)
 *   a phase with no visible cell gives exactly 0.0
 * There is no 2 pi factor: with coef = solid angle x mu a uniform planet gives the flux of
 * frei_emergent in the same unit (the sum of coef over the visible hemisphere is pi).
 * out[n_phase][n_lam] receives the result; it may be NULL when keep is set.  The result is formed
 * in a device buffer the handle owns, reused from call to call and grown when a call needs more.
 * With keep != 0 it stays valid there until the next frei_phs_apply (kept or not, successful or
 * not once its arguments are accepted) or frei_phs_destroy; frei_obs_apply_phs,
 * frei_brd_apply_phs and frei_ccf_apply_phs read it there.
 * Kernel: one lane per wavelength; a block owns 256 wavelengths and a tile of 8 consecutive phases
 * whose sums live in registers, and walks the cells in ascending order.  Per tile the list of
 * cells to visit (those visible at one of its phases or more) and, per visit, the phases that see
 * the cell are built on the host at create: a cell's column is loaded once per tile, B_{l+1} is
 * formed once per shell for all the tile's rays through the cell, an invisible pair costs nothing.
 * There is one form: form 0 (automatic) and form 1 name it, *form_used receives 1.
 * Guarantees.  No atomics.  Results are bitwise the same from call to call; row p is bitwise the
 * row of a handle that holds phase p alone; an output does not change when other phases are
 * added, permuted or dropped, or when cells invisible at p are added; two cells on one row give
 * the bits of the same data in two rows; a single context gives the bits of a one-atmosphere
 * batch.  (A pair of cells with the same row and the same mu may be evaluated once and reused —
 * the north/south symmetry at 90 degrees inclination; the bits would be the same.  It is allowed,
 * not required, and not done.)  A NaN or inf in a column of atmosphere m at wavelength j reaches
 * exactly the outputs (p, j) at which some cell with select = m is visible, and no other
 * wavelength or phase; nothing in the columns is checked.
 * *form_used and *kernel_ms (HIP events around the kernel only) may be NULL.  Errors (return
 * codes; handle and context stay usable): a null handle, context or T; out null without keep; a
 * form outside 0 .. 1; a context on another device; a select entry >= n_atm (the message names the
 * cell); a T[m][l], l >= 1, not finite and positive in an atmosphere some visible cell uses (the
 * other atmospheres' temperatures are not read); no device dtaus; n_phase / 8 beyond the launch
 * grid (65535).
 */
int frei_phs_apply(frei_phs* phs, frei_ctx* ctx, const double* dtaus, const double* T,
                   double* out, int keep, int form, int* form_used, double* kernel_ms);
int frei_phs_destroy(frei_phs* phs);
/*
 * frei_ccf_apply, frei_obs_apply and frei_brd_apply with the result `src` kept (frei_phs_apply
 * with keep) as their x: a fifth source, read where it lies.  The phases play the role of the
 * atmospheres (n_atm = n_phase): select, scale, offset and den are per phase.  The other
 * arguments and the results are those of the plain calls, bitwise what they give for a host copy
 * of the same numbers.  Errors: a null phase integrator, one with nothing kept, or one of another
 * n_lam, n_phase or device.
 */
int frei_ccf_apply_phs(frei_ccf* c, frei_phs* src, int n_atm, const double* den, int n_lib,
                       const int32_t* select, const double* scale, const double* offset,
                       int form, double* sfg, double* sg, double* sgg, int* form_used,
                       double* kernel_ms);
int frei_obs_apply_phs(frei_obs* o, frei_phs* src, int n_atm, const double* num,
                       const double* den, int n_lib, const int32_t* select, const double* scale,
                       const double* data, const double* sigma, int form, double* obs,
                       double* chi2, int* form_used, double* kernel_ms);
int frei_brd_apply_phs(frei_brd* b, frei_phs* src, int n_atm, int form, double* out, int keep,
                       int* form_used, double* kernel_ms);

#ifdef __cplusplus
}
#endif

#endif /* FREI_HIP_H */
