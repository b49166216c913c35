"""NumPy restatement of K18 (include/frei_hip.h: frei_xsec_mix, frei_xsec_kdist), in the
header's operation order, and the seeded line-forest case the k-distribution's physics is held
to (tests/test_kdist_host.py through the oracle alone, tests/test_gpu_kdist.py on the device).
"""
import numpy as np

from oracle import frei_oracle as O


def mix_ref(sources, weights):
    """out[t][p][i] = float32(acc): acc = +0.0, then acc = acc + weights[s][t][p] *
    float64(sources[s][t][p][i]) for s ascending (product rounded, then the sum)."""
    sources = [np.asarray(s, dtype=np.float32) for s in sources]
    w = np.broadcast_to(np.asarray(weights, dtype=np.float64),
                        (len(sources),) + sources[0].shape[:2])
    acc = np.zeros(sources[0].shape, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s, x in enumerate(sources):
            acc = acc + w[s][:, :, None] * x.astype(np.float64)
        return acc.astype(np.float32)


def kdist_plan(n, g):
    """(j, f) per g_q for a bin of n points: t = g n - 0.5, j = clamp(floor(t), 0, n - 2),
    f = clamp(t - j, 0, 1), in float64."""
    t = np.asarray(g, dtype=np.float64) * float(n) - 0.5
    j = np.minimum(np.maximum(np.floor(t), 0.0), float(max(n - 2, 0)))
    return j.astype(np.int64), np.minimum(np.maximum(t - j, 0.0), 1.0)


def canonical(v):
    """float32 values as the sort sees them: -0 -> +0, every NaN the canonical quiet NaN."""
    v = np.array(v, dtype=np.float32)
    v[v == 0] = np.float32(0.0)
    v[np.isnan(v)] = np.float32(np.nan)
    return v


def kdist_rows(rows, start, end, g):
    """k[row][bin][g] (float64) of float32 ``rows`` [R][n_hi] for the bins [start_k, end_k)."""
    rows = np.asarray(rows, dtype=np.float32)
    g = np.asarray(g, dtype=np.float64)
    out = np.full((rows.shape[0], len(start), g.size), np.nan)
    for k, (a, b) in enumerate(zip(start, end)):
        n = int(b - a)
        if n == 0:
            continue
        s = np.sort(canonical(rows[:, a:b]), axis=-1).astype(np.float64)   # NaN last
        if n == 1:
            out[:, k, :] = s[:, :1]
            continue
        j, f = kdist_plan(n, g)
        with np.errstate(invalid="ignore", over="ignore"):
            out[:, k, :] = s[:, j] + f * (s[:, j + 1] - s[:, j])
    return out


def kdist_ref(xsec, src_T, src_p, wl_hi, wl_bins, g, T_nodes, p_nodes):
    """-> (k[n_p][n_T][n_bins][n_g] float64, counts[n_bins]) of the float32 cross-section
    ``xsec`` [n_T_src][n_p_src][n_hi]: K6's bin membership and nearest source node, then per
    (distinct source row, bin) sort, plan and sample; every target that selects the row gets
    the same values."""
    xsec = np.asarray(xsec, dtype=np.float32)
    start, end = O.bin_ranges(wl_hi, wl_bins)
    ti = O.nearest_index(src_T, np.atleast_1d(T_nodes))
    pi = O.nearest_index(src_p, np.atleast_1d(p_nodes))
    pairs = sorted({(int(a), int(b)) for a in ti for b in pi})
    k = kdist_rows(np.stack([xsec[a, b] for a, b in pairs]), start, end, g)
    at = {pr: u for u, pr in enumerate(pairs)}
    out = np.empty((len(pi), len(ti), len(start), np.size(g)))
    for kp, b in enumerate(pi):
        for kt, a in enumerate(ti):
            out[kp, kt] = k[at[(int(a), int(b))]]
    return out, (end - start).astype(np.int64)


# ----------------------------------------------------------------- the seeded forest case
N_BINS, N_HI, N_LAYERS = 8, 4096, 12
N_SAMPLED = 16


def forest_case():
    """8 bins x 512 native points over 2.5-3 µm, 12 layers, 120 lines whose strengths and widths
    move with T and p; the cross-section on T nodes 800 .. 2000 K x the layers' pressures."""
    rng = np.random.default_rng(11)
    wl_bins = np.linspace(2.5, 3.0, N_BINS + 1)
    wl = 2.5 + (np.arange(N_HI) + 0.5) * 0.5 / N_HI
    p = np.logspace(1, -5, N_LAYERS)
    T = np.linspace(1800.0, 900.0, N_LAYERS)
    T_nodes = np.array([800.0, 1200.0, 1600.0, 2000.0])
    c = rng.uniform(2.5, 3.0, 120)
    S = rng.lognormal(0.0, 2.0, 120)
    E = rng.uniform(0.0, 4000.0, 120)
    g0 = 2e-4 * rng.uniform(0.5, 1.5, 120)
    x = np.empty((T_nodes.size, p.size, N_HI), dtype=np.float32)
    for a, Tn in enumerate(T_nodes):
        s = S * np.exp(-1.4388 * E * (1.0 / Tn - 1.0 / 1200.0))
        for b, pn in enumerate(p):
            w = g0 * pn * (1200.0 / Tn) ** 0.5 + 3e-5 * (Tn / 1200.0) ** 0.5
            prof = s[:, None] * w[:, None] / np.pi / ((wl[None, :] - c[:, None]) ** 2 +
                                                      w[:, None] ** 2)
            x[a, b] = (1e-4 + 1e-3 * prof.sum(axis=0)).astype(np.float32)
    x.setflags(write=False)
    return dict(wl_bins=wl_bins, wl=wl, p=p, T=T, T_nodes=T_nodes, xsec=x)


def native_table(case):
    """The run on the native axis: the cross-section itself, [p][T][n_hi] float64."""
    return np.ascontiguousarray(case["xsec"].transpose(1, 0, 2), dtype=np.float64)


def sampled_columns():
    """16 native points per bin: the middle point of each run of 32."""
    per = N_HI // N_BINS
    step = per // N_SAMPLED
    return (np.arange(N_BINS)[:, None] * per + step // 2 + step * np.arange(N_SAMPLED)).ravel()


def mean_table(case):
    """The mean opacity of each bin, [p][T][n_bins] float64."""
    t = native_table(case)
    return t.reshape(t.shape[:2] + (N_BINS, N_HI // N_BINS)).mean(axis=-1)


def band_mean(x, n_bins=N_BINS):
    """[..., n] -> [..., n_bins]: the mean over each bin's equally spaced points."""
    x = np.asarray(x)
    return x.reshape(x.shape[:-1] + (n_bins, x.shape[-1] // n_bins)).mean(axis=-1)


def oracle_top_flux(table, lam_um, case, planet):
    """F_up[top] per column after emit -> absorb -> emit at the case's fixed T, through the
    oracle alone: one species of mixing ratio 1 with ``table`` [p][T][n_col] on the case's
    nodes."""
    tabs = {"x": O.Table(table, case["p"], case["T_nodes"])}
    lam_um = np.asarray(lam_um, dtype=float)
    ft = O.F_TOA(lam_um, T_star=planet["T_star"], a_rstar=planet["a_rstar"])
    mmr = np.ones((1, N_LAYERS))
    kw = dict(g=planet["g"], m_bar=planet["m_bar"], alpha=1, mmr=mmr)
    with np.errstate(all="ignore"):   # repeated wavelengths: the oracle's own trapz dT is unused
        Fu, Fd, *_ = O.emit(tabs, case["T"], case["p"], lam_um, ft, **kw)
        Fu, Fd, *_ = O.absorb(tabs, case["T"], case["p"], lam_um, ft, fluxes_up=Fu,
                              fluxes_down=Fd, **kw)
        Fu, Fd, *_ = O.emit(tabs, case["T"], case["p"], lam_um, ft, fluxes_up=Fu,
                            fluxes_down=Fd, **kw)
    return Fu[-1].copy()
