"""Fixtures of the chemistry-batch edge tests (test infrastructure, like tests/parity.py): the
inputs that tests/test_gpu_batch_chemistry.py's one benign fixture leaves out, built once per
process from ``oracle.frei_oracle`` and, where a ``frei_amd`` handle is given, the engine's
twins of the same tables.  tests/test_batch_chemistry_edges_host.py proves on the CPU that each
fixture has the property it exists for; tests/test_gpu_batch_chemistry_edges.py runs them.

All of them keep the base fixture's five atmospheres (T_REF, G, ATM_TAB), three species, two
chemistry tables at +0.0 and +0.5 dex, 20 layers and 700 wavelengths (two full 256-blocks and one
of 188 lanes):

H   high albedo, well conditioned: 0.3-3 um, weak tables (base 1e-4..1, the default clip
    [1e-4, 1e3] that never binds above), top of the atmosphere at 1e-2 bar.
H6  H with the top at 1e-6 bar: optically thin layers meet the same branch.
R   H with opacity and chemistry T nodes narrower than the layer temperatures: layers above
    and below both ranges (opacity 0 outside its range, so w0 = 1/2 for every lane; the
    chemistry table clamps).
P   the base fixture itself (0.5-10 um, tables clipped to [10, 1e3], seed 30), whose
    convergence run stops after 13, 14, 13, 13, 12 iterations, with the atmospheres reordered
    so that a tile sees every shape of run mask.
"""
import numpy as np

from oracle import frei_oracle as O
from tests.parity import grid_floor, perturbed_exp, rel

M_BAR = 4.0142926168559996e-24
NAMES = ["1H2-16O", "12C-16O", "12C-1H4"]
T_REF = [1500.0, 1500.0, 1540.0, 2100.0, 2100.0]
G = np.array([1200.0, 2478.65, 4000.0, 900.0, 3000.0])
ATM_TAB = [0, 1, 0, 1, 1]
N_ATM, N_LAYERS, N_LAM = 5, 20, 700

# three fixed iterations (H, H6, R) and the convergence run (P)
KW_FIXED = dict(n_timesteps=3, n_zero_crossings=10 ** 6, convergence_dT=-1.0)
KW_CONV = dict(n_timesteps=30, n_zero_crossings=2, convergence_dT=10.0)

# R: opacity T nodes and the chemistry table's T range, chosen on the CPU so that every
# atmosphere keeps at least two layers on either side of both at T0 and at the final T
R_OPACITY_T = np.linspace(1850.0, 2900.0, 6)
R_CHEM_T = (2000.0, 2750.0)

# P: oracle iteration counts in natural order, and the orders of the run-mask table
P_COUNTS = [13, 14, 13, 13, 12]
P_ORDERS = {
    "gap": [1, 4, 0, 2, 3],
    "leader": [4, 1, 0, 2, 3],
    "last_slot_converged": [0, 2, 3, 4, 1],
    "only_last_slot": [0, 4, 2, 1, 3],
}


def chem_values(names, T_lo=300.0, T_hi=4000.0, n_T=14, n_p=9):
    """tests/test_gpu_batch_chemistry.py::_chem_values, with the T range as a parameter."""
    T = np.linspace(T_lo, T_hi, n_T)
    p = np.logspace(-7, 3, n_p)
    x = np.tanh((T[:, None] - 1500.0) / 400.0) + 0.05 * np.log10(p)[None, :]
    base = O.mock_mmr(names, M_BAR)
    vals = []
    for s, n in enumerate(names):
        sign = -1.0 if s % 2 == 0 else 1.0
        vals.append(base[s] * 10 ** (0.8 * sign * x))
    return np.array(vals), T, p


def chem_pair(fa, names, **kw):
    """Two chemistry tables on shared nodes, at +0.0 and +0.5 dex: (engine's, oracle's); the
    engine's are None without a ``frei_amd`` handle."""
    vals, cT, cp = chem_values(names, **kw)
    f, o = [], []
    for dex in (0.0, 0.5):
        v = vals * 10 ** dex
        f.append(fa.ChemistryTable({n: v[s] for s, n in enumerate(names)}, cT, cp)
                 if fa is not None else None)
        o.append(O.ChemistryTable(v, cT, cp))
    return f, o


def separable_tables(fa, rng, names, lam, p, Tn, dex, clip=None):
    """One separable table per species, base = 10 ** uniform(*dex): (oracle's, engine's)."""
    tabs_o, tabs_f = {}, {}
    kw = {} if clip is None else dict(lo=clip[0], hi=clip[1])
    for n in names:
        base = 10 ** rng.uniform(dex[0], dex[1], lam.size)
        fp, fT = (p / 1.0) ** 0.1, (Tn / 1000.0) ** 0.5
        tabs_o[n] = O.Table(O.separable_table(base, fp, fT, **kw), p, Tn)
        if fa is not None:
            tabs_f[n] = fa.SeparableTable(base, fp, fT, p, Tn, **kw)
    return tabs_o, tabs_f


_CACHE = {}


def fixture(kind, fa=None):
    """The fixture ``kind`` (H, H6, R or P) as a dict: lam, p, Tn, tabs_o / tabs_f (oracle's and
    engine's opacity tables), chem_o / chem_f (the two chemistry tables), chem_T (their T nodes),
    T0 [5][20], Ft, and ``cache`` (oracle runs, shared by every test of the process).  Built once
    per (kind, with or without the engine's objects)."""
    key = (kind, fa is not None)
    if key in _CACHE:
        return _CACHE[key]
    if kind == "P":
        rng = np.random.default_rng(30)
        lam, _, _ = O.wavelength_grid(0.5, 10, N_LAM)
        p = O.pressure_grid(N_LAYERS, -6, np.log10(200))
        Tn = np.linspace(400.0, 5000.0, 12)
        tabs_o, tabs_f = separable_tables(fa, rng, NAMES, lam, p, Tn, (0, 4.5), (10.0, 1e3))
        chem_kw = {}
    else:
        rng = np.random.default_rng(41)
        lam, _, _ = O.wavelength_grid(0.3, 3, N_LAM)
        p = O.pressure_grid(N_LAYERS, -6 if kind == "H6" else -2, np.log10(200))
        Tn = R_OPACITY_T if kind == "R" else np.linspace(400.0, 5000.0, 12)
        tabs_o, tabs_f = separable_tables(fa, rng, NAMES, lam, p, Tn, (-4, 0))
        chem_kw = dict(T_lo=R_CHEM_T[0], T_hi=R_CHEM_T[1]) if kind == "R" else {}
    chem_f, chem_o = chem_pair(fa, NAMES, **chem_kw)
    T0 = np.array([O.temperature_grid(p, t, 0.1, 0.1) for t in T_REF])
    # oracle runs are shared between the fixture with and without the engine's objects
    cache = _CACHE.setdefault(("oracle", kind), {})
    fx = dict(kind=kind, lam=lam, p=p, Tn=Tn, tabs_o=tabs_o, tabs_f=tabs_f, chem_o=chem_o,
              chem_f=chem_f, chem_T=chem_o[0].T, T0=T0, Ft=O.F_TOA(lam), cache=cache)
    _CACHE[key] = fx
    return fx


def fixed_mmr():
    """The mock mixing ratios [3][20] of the fixed-mmr (contracted) runs."""
    return O.mock_mmr(NAMES, M_BAR)[:, None] * np.ones(N_LAYERS)


def _mmr_of(fx, m, chem):
    return fx["chem_o"][ATM_TAB[m]] if chem else fixed_mmr()


def oracle(fx, m, chem=True, **kw):
    """Oracle emission_spectrum of atmosphere m (computed once per process and left unchanged):
    (spectrum, final_T, temp_hist, dtaus, F_up, F_down, n_iter).  ``chem=False``: the fixed
    mock mixing ratios instead of the atmosphere's chemistry table."""
    k = ("run", m, chem, tuple(sorted(kw.items())))
    if k not in fx["cache"]:
        fx["cache"][k] = O.emission_spectrum(
            fx["tabs_o"], fx["T0"][m], fx["p"], fx["lam"], fx["Ft"], G[m], M_BAR, 1,
            mmr=_mmr_of(fx, m, chem), **kw)
    return fx["cache"][k]


def floors(fx, m, chem=True, **kw):
    """The oracle's own one-ulp floor of atmosphere m (tests/parity.py: perturbed_exp,
    grid_floor): ((spectrum, F_up, F_down), T)."""
    k = ("floor", m, chem, tuple(sorted(kw.items())))
    if k not in fx["cache"]:
        osp, oT, _, _, ou, od, _ = oracle(fx, m, chem, **kw)
        with perturbed_exp():
            psp, pT, _, _, pu, pd, _ = O.emission_spectrum(
                fx["tabs_o"], fx["T0"][m], fx["p"], fx["lam"], fx["Ft"], G[m], M_BAR, 1,
                mmr=_mmr_of(fx, m, chem), **kw)
        fx["cache"][k] = (grid_floor(osp, ou, od, psp, pu, pd), rel(pT, oT))
    return fx["cache"][k]


def albedo(fx, m, T, layer, chem=True):
    """w0 = sigma / (sigma + kappa) of atmosphere m's ``layer`` at the temperatures T [20], as
    the sweep forms it (kappa includes sigma)."""
    mm = _mmr_of(fx, m, chem)
    mmr = mm(T[layer], fx["p"][layer]) if callable(mm) else mm[:, layer]
    k, sig = O.kappa(fx["tabs_o"], T[layer], fx["p"][layer], fx["lam"], M_BAR, mmr=mmr)
    return sig / (sig + k)


def mixed_waves(w0):
    """Fraction of the 64-lane waves (of the 256-lane blocks) that hold lanes on both sides of
    w0 > 0.1: the waves in which the wave-uniform branch runs both heads."""
    hi = w0 > 0.1
    return float(np.mean([0 < hi[i:i + 64].mean() < 1 for i in range(0, hi.size, 64)]))


def outside(T, nodes):
    """(layers above nodes[-1], layers below nodes[0]) of a temperature profile."""
    return int(np.count_nonzero(T > nodes[-1])), int(np.count_nonzero(T < nodes[0]))


def run_masks(counts, tile):
    """masks[n - 1][b]: the run mask of tile b during T-P iteration n (1-based) for atmospheres
    with these iteration counts: an atmosphere that stopped after c iterations runs iterations
    1..c, slots past the batch never run (the last tile may be partial)."""
    out = []
    for n in range(1, max(counts) + 1):
        row = []
        for b in range(0, len(counts), tile):
            row.append([int(b + t < len(counts) and counts[b + t] >= n) for t in range(tile)])
        out.append(row)
    return out


# atm_tile_width's two size rules (frei_runtime.hip, frei_kernels.hip) with kBlock = 256 (four
# waves), kStageRow = 72 and sizeof(FastStepS) = 120; ns = layers - 1
def staged_sums_fit(ns):
    """staged_sums_fit: the per-wave partial sums, two stage tiles per wave and the step table
    within 48 KiB."""
    return (4 * ns * 4 + 4 * 2 * 4 * 72) * 8 + ns * 120 <= 48 * 1024


def tile_lds_bytes(at, ns):
    """tile_lds_bytes: one partial-sum block per atmosphere of the tile and one stage tile per
    wave."""
    return (at * 4 * ns * 4 + 4 * 4 * 72) * 8
