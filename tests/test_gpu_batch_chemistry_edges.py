"""The atmosphere-tiled chemistry sweep (sweep_tile_kernel<DIR, S, AT>, atm_tile_width) at its
branches and edges: what tests/test_gpu_batch_chemistry.py's one strongly absorbing fixture
leaves out.  Fixtures and their CPU-proved properties: tests/chem_batch_fixtures.py and
tests/test_batch_chemistry_edges_host.py.

E1  every S instantiation (2..8) at tile 2 and 4, both directions, bitwise the tile-1 run.
E2  lanes with w0 > 0.1 mixed inside most waves (the kernel's own coef_head_general branch):
    oracle parity per atmosphere and bitwise single contexts; with optically thin layers (H6,
    floor rule); and the contracted fixed-mmr batch on the same inputs.
E3  layers outside the opacity tables' and the chemistry tables' T ranges.
E4  run masks with a gap, a converged leader, a converged last slot, a lone last slot.
E5  the smallest shapes: four layers (the fewest the engine takes), a block of one lane, one wave.
E6  the width rules of atm_tile_width: every fallback to 1, and the halving at 64 KiB of LDS.

Tolerances: 1e-10 outright where the oracle's CPU-measured one-ulp floor is below 1e-11,
max(1e-10, 2 x floor) elsewhere (tests/parity.py), bitwise between two engine paths."""
import numpy as np
import pytest

from oracle import frei_oracle as O
from tests import chem_batch_fixtures as F
from tests.parity import assert_grid_parity, rel

pytestmark = pytest.mark.gpu

TILES = [1, 2, 4]
_REFS = {}   # engine reference runs shared between the cases of a test (left unchanged)


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


def _batch(fa, fx, tile, monkeypatch, order=range(F.N_ATM)):
    monkeypatch.setenv("FREI_ATM_TILE", str(tile))
    order = list(order)
    return fa.BatchEngine(fx["lam"], fx["p"], fx["tabs_f"], g=F.G[order],
                          mmr=[fx["chem_f"][F.ATM_TAB[m]] for m in order], F_toa=fx["Ft"])


def _iterate(eng, T0, n):
    eng.state_init(T0)
    eng.iterate(n)
    eng.synchronize()
    up, down = eng.get_fluxes()
    return eng.get_temperatures(), up, down


def _assert_bitwise(got, want, what):
    for a, b, name in zip(got, want, ("T", "F_up", "F_down")):
        assert np.array_equal(a, b), f"{what}: {name} differs by {rel(a, b):.3e}"


def _small_batch(fa, monkeypatch, names, n_lam, n_layers, n_atm, tile, seed, env=(), p_toa=-6):
    """A strongly absorbing batch of the base fixture's kind at a small shape: (engine, T0)."""
    rng = np.random.default_rng(seed)
    lam, _, _ = O.wavelength_grid(0.5, 10, n_lam)
    p = O.pressure_grid(n_layers, p_toa, np.log10(200))
    Tn = np.linspace(400.0, 5000.0, 12)
    _, tabs_f = F.separable_tables(fa, rng, names, lam, p, Tn, (0, 4.5), (10.0, 1e3))
    chem_f, _ = F.chem_pair(fa, names)
    T0 = np.array([O.temperature_grid(p, t, 0.1, 0.1) for t in F.T_REF[:n_atm]])
    monkeypatch.setenv("FREI_ATM_TILE", str(tile))
    for k, v in env:
        monkeypatch.setenv(k, v)
    eng = fa.BatchEngine(lam, p, tabs_f, g=F.G[:n_atm],
                         mmr=[chem_f[k] for k in F.ATM_TAB[:n_atm]])
    return eng, T0


def _tiles_against_tile_1(fa, monkeypatch, names, n_lam, n_layers, n_atm, seed, want=None,
                          env=(), tiles=(1, 2, 4), p_toa=-6):
    """Two T-P iterations (both sweep directions twice) at every requested tile width: the
    width the engine reports is ``want[tile]`` (default: the requested one), the tile-1 run is
    finite and positive, and every other run is bitwise the tile-1 run."""
    out = {}
    for tile in tiles:
        eng, T0 = _small_batch(fa, monkeypatch, names, n_lam, n_layers, n_atm, tile, seed, env,
                               p_toa)
        try:
            path = eng.path()
            assert not path["contracted"], path
            assert path["atm_tile"] == (want or {}).get(tile, tile), (tile, path)
            out[tile] = _iterate(eng, T0, 2)
        finally:
            eng.close()
    T, up, down = out[1]
    assert all(np.all(np.isfinite(x)) for x in out[1])
    assert np.all(T > 0) and np.all(up[:, -1] > 0)
    assert not np.array_equal(T, T0)
    for tile in tiles[1:]:
        _assert_bitwise(out[tile], out[1], f"requested tile {tile} against tile 1")


# ------------------------------------------------------------------ E1: every instantiation
@pytest.mark.parametrize("S", [2, 3, 4, 5, 6, 7, 8])
def test_every_species_count_at_both_tile_widths(fa, monkeypatch, S):
    """E1: sweep_tile_kernel<emit / absorb, S, 2 / 4> for every S it is instantiated for, on the
    first S of C3_SPECIES: 300 wavelengths (one full block and 44 lanes), 8 layers, 5 atmospheres
    (tile 2: two full tiles and a remainder; tile 4: one full and one of a single atmosphere),
    two chemistry tables."""
    from frei_amd.workloads import C3_SPECIES
    names = list(C3_SPECIES)[:S]
    assert len(names) == S
    _tiles_against_tile_1(fa, monkeypatch, names, 300, 8, 5, seed=50 + S)


# ------------------------------------------------------------------ E2 / E3: oracle parity
def _singles(fa, fx):
    """Every atmosphere as a single-context Engine with its own table and gravity (once)."""
    key = ("single", fx["kind"])
    if key not in _REFS:
        ref = []
        for m in range(F.N_ATM):
            single = fa.Engine(fx["lam"], fx["p"], fx["tabs_f"], g=F.G[m],
                               mmr=fx["chem_f"][F.ATM_TAB[m]], F_toa=fx["Ft"])
            try:
                assert not single.path()["contracted"]
                r = single.run(fx["T0"][m], alpha=1.0, **F.KW_FIXED)
                up, down = single.get_fluxes()
            finally:
                single.close()
            ref.append((r["final_T"], r["spectrum"], up, down))
        _REFS[key] = ref
    return _REFS[key]


def _oracle_and_singles(fa, monkeypatch, kind, tile, outright):
    """Three fixed iterations of fixture ``kind`` at ``tile``: every atmosphere against the
    oracle (spectrum, F_up, F_down, T) — 1e-10 outright, or the floor rule with the floors
    measured on the CPU — and bitwise against its single context; all outputs finite."""
    fx = F.fixture(kind, fa)
    eng = _batch(fa, fx, tile, monkeypatch)
    try:
        path = eng.path()
        assert not path["contracted"] and path["atm_tile"] == tile, path
        out = eng.run(fx["T0"], alpha=1.0, **F.KW_FIXED)
        ups, downs = eng.get_fluxes()
    finally:
        eng.close()
    assert all(np.all(np.isfinite(x)) for x in (out["spectra"], out["final_T"], ups, downs))
    assert list(out["n_iter"]) == [3] * F.N_ATM
    for m in range(F.N_ATM):
        osp, oT, _, _, ou, od, _ = F.oracle(fx, m, **F.KW_FIXED)
        flux, T_floor = F.floors(fx, m, **F.KW_FIXED)
        print(f"{kind} atmosphere {m}: oracle one-ulp floors {flux} T {T_floor:.2e}")
        what = f"fixture {kind}, tile {tile}, atmosphere {m}"
        if outright:
            assert max(flux) < 1e-11 and T_floor < 1e-11
            e = assert_grid_parity(out["spectra"][m], osp, ups[m], ou, downs[m], od,
                                   what + " (outright)", T=out["final_T"][m], ref_T=oT)
            assert e["within_1e-10"], e
        else:
            assert max(flux) < 1e-10 and T_floor < 1e-10
            e = assert_grid_parity(out["spectra"][m], osp, ups[m], ou, downs[m], od, what,
                                   floor=flux, T=out["final_T"][m], ref_T=oT, T_floor=T_floor)
        print({k: v for k, v in e.items() if k.endswith(("wise", "norm")) or k == "rule"})
    for m, (Ts, ss, su, sd) in enumerate(_singles(fa, fx)):
        what = f"fixture {kind}, tile {tile}, atmosphere {m} against its single context"
        _assert_bitwise((out["final_T"][m], ups[m], downs[m]), (Ts, su, sd), what)
        assert np.array_equal(out["spectra"][m], ss), what + ": spectrum"


@pytest.mark.parametrize("tile", TILES)
def test_high_albedo_tiles_match_oracle_outright(fa, monkeypatch, tile):
    """E2, fixture H: 10 to 27 % of every atmosphere's lanes have w0 > 0.1, mixed inside more
    than half of the waves, no optically thin layer (floors <= 4.6e-13 fluxes, 2.2e-16 T):
    1e-10 outright against the oracle, bitwise against single contexts."""
    _oracle_and_singles(fa, monkeypatch, "H", tile, outright=True)


@pytest.mark.parametrize("tile", TILES)
def test_high_albedo_thin_layers_tiles_match_oracle(fa, monkeypatch, tile):
    """E2, fixture H6: H with the top of the atmosphere at 1e-6 bar, so that optically thin
    layers meet the branch.  CPU-measured floors (spectrum / F_up / F_down / T) up to 4.2e-11 /
    1.0e-11 / 5.5e-11 / 9.7e-12: the floor rule, max(1e-10, 2 x floor) per atmosphere
    (test_high_albedo_tiles_match_oracle_outright is the outright twin)."""
    _oracle_and_singles(fa, monkeypatch, "H6", tile, outright=False)


def test_high_albedo_fixed_mmr_batch_matches_oracle_outright(fa):
    """E2, fixture H through the contracted path: a fixed-mmr BatchEngine with the mock mixing
    ratios against the oracle with mmr= that array, 1e-10 outright (floors <= 1.2e-12 fluxes,
    2.2e-16 T; 16 to 33 % of the lanes have w0 > 0.1)."""
    fx = F.fixture("H", fa)
    eng = fa.BatchEngine(fx["lam"], fx["p"], fx["tabs_f"], g=F.G, mmr=F.fixed_mmr(),
                         F_toa=fx["Ft"])
    try:
        path = eng.path()
        assert path["contracted"] and path["atm_tile"] == 0, path
        out = eng.run(fx["T0"], alpha=1.0, **F.KW_FIXED)
        ups, downs = eng.get_fluxes()
    finally:
        eng.close()
    for m in range(F.N_ATM):
        osp, oT, _, _, ou, od, _ = F.oracle(fx, m, chem=False, **F.KW_FIXED)
        flux, T_floor = F.floors(fx, m, chem=False, **F.KW_FIXED)
        assert max(flux) < 1e-11 and T_floor < 1e-11
        e = assert_grid_parity(out["spectra"][m], osp, ups[m], ou, downs[m], od,
                               f"fixture H, fixed mmr, atmosphere {m} (outright)",
                               T=out["final_T"][m], ref_T=oT)
        print({k: v for k, v in e.items() if k.endswith(("wise", "norm"))})
        assert e["within_1e-10"], e


@pytest.mark.parametrize("tile", TILES)
def test_layers_outside_the_table_ranges_match_oracle(fa, monkeypatch, tile):
    """E3, fixture R: every atmosphere has layers above and below the opacity tables' T range
    (opacity 0, w0 = 1/2 in every lane) and the chemistry tables' (clamped), at T0 and at the
    final T.  CPU-measured floors (spectrum / F_up / F_down / T) per atmosphere: 7.3e-12 /
    1.1e-12 / 7.0e-12 / 1.2e-13; 1.5e-11 / 2.3e-12 / 1.0e-11 / 5.1e-13; 2.6e-11 / 3.1e-12 /
    2.1e-11 / 1.2e-12; 5.2e-12 / 3.1e-13 / 5.3e-12 / 2.1e-14; 3.2e-11 / 7.1e-13 / 1.6e-11 /
    2.2e-13: above 1e-11, so the floor rule, max(1e-10, 2 x floor) = 1e-10 here
    (test_high_albedo_tiles_match_oracle_outright is the outright twin)."""
    _oracle_and_singles(fa, monkeypatch, "R", tile, outright=False)


# ------------------------------------------------------------------ E4: run masks
def _natural_order_run(fa, fx, monkeypatch):
    if "P" not in _REFS:
        eng = _batch(fa, fx, 1, monkeypatch)
        try:
            assert eng.path()["atm_tile"] == 1
            _REFS["P"] = eng.run(fx["T0"], alpha=1.0, want_hist=True, **F.KW_CONV)
        finally:
            eng.close()
    return _REFS["P"]


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("name", list(F.P_ORDERS))
def test_run_mask_shapes(fa, monkeypatch, name, tile):
    """E4: the convergence run of the base fixture (oracle counts 13, 14, 13, 13, 12) with the
    atmospheres reordered so that block 0 of a tile of 4 sweeps with a gap in its run mask, a
    converged leader, a converged last slot and a lone last slot (and a tile of 2 with [1, 0]
    and [0, 1]).  Counts are the permuted oracle counts; T, spectrum and T history of every
    atmosphere are bitwise those of the tile-1 run in natural order and within 1e-10 of the
    oracle."""
    fx = F.fixture("P", fa)
    order = F.P_ORDERS[name]
    ref = _natural_order_run(fa, fx, monkeypatch)
    eng = _batch(fa, fx, tile, monkeypatch, order)
    try:
        assert eng.path()["atm_tile"] == tile
        out = eng.run(fx["T0"][order], alpha=1.0, want_hist=True, **F.KW_CONV)
    finally:
        eng.close()
    ora = [F.oracle(fx, m, **F.KW_CONV) for m in range(F.N_ATM)]
    assert [o[6] for o in ora] == F.P_COUNTS
    print(name, order, "iterations", list(out["n_iter"]))
    assert list(out["n_iter"]) == [F.P_COUNTS[m] for m in order]
    assert list(ref["n_iter"]) == F.P_COUNTS
    for slot, m in enumerate(order):
        what = f"order {name}, tile {tile}, slot {slot} (atmosphere {m})"
        assert np.array_equal(out["final_T"][slot], ref["final_T"][m]), what + ": T"
        assert np.array_equal(out["spectra"][slot], ref["spectra"][m]), what + ": spectrum"
        assert np.array_equal(out["temp_hist"][slot], ref["temp_hist"][m]), what + ": T history"
        osp, oT, oth = ora[m][:3]
        assert out["temp_hist"][slot].shape == oth.shape
        errs = (rel(out["final_T"][slot], oT), rel(out["spectra"][slot], osp),
                rel(out["temp_hist"][slot], oth))
        print(f"{what}: T {errs[0]:.2e} spectrum {errs[1]:.2e} history {errs[2]:.2e}")
        assert max(errs) <= 1e-10, (what, errs)


# ------------------------------------------------------------------ E5: smallest shapes
@pytest.mark.parametrize("n_lam,n_layers", [(3, 4), (257, 5), (64, 4)])
def test_smallest_shapes(fa, monkeypatch, n_lam, n_layers):
    """E5: 3 wavelengths x 4 layers (three steps, the fewest the engine takes: it refuses fewer
    than 4 layers, "the emit top layer uses p[-3]"; 253 inactive lanes read j = n_lam - 1);
    257 x 5 (a second block of one active lane); 64 x 4 (exactly one wave).  3 species,
    5 atmospheres, two iterations."""
    _tiles_against_tile_1(fa, monkeypatch, F.NAMES, n_lam, n_layers, 5, seed=60 + n_layers)


# ------------------------------------------------------------------ E6: width rules
# atm_tile_width (frei_runtime.hip) with kBlock = 256 (4 waves), kStageRow = 72 and
# sizeof(FastStepS) = 120 (five doubles, one int64, two int32, eight mmr doubles), ns = layers - 1:
#   staged_sums_fit(ns): (4 * ns * 4 + 4 * 2 * 4 * 72) * 8 + 120 ns = 248 ns + 18432 <= 49152,
#       i.e. ns <= 123: up to 124 layers
#   tile_lds_bytes(AT, ns) = (AT * 4 * ns * 4 + 4 * 4 * 72) * 8 = 128 AT ns + 9216 <= 65536:
#       AT = 4 up to ns = 110 (111 layers: exactly 64 KiB), AT = 2 up to ns = 219
# so a requested width of 4 becomes 2 from 112 to 124 layers and 1 from 125 layers on
# (tests/chem_batch_fixtures.py mirrors the two formulas; the host test checks these counts).
@pytest.mark.parametrize("case,names,n_layers,env,width", [
    ("one species", F.NAMES[:1], 8, (), 1),
    ("no staged sums", F.NAMES, 8, (("FREI_RED_STAGE", "0"),), 1),
    ("prefetch depth 1", F.NAMES, 8, (("FREI_PREFETCH_DEPTH", "1"),), 1),
    ("prefetch depth 4", F.NAMES, 8, (("FREI_PREFETCH_DEPTH", "4"),), 1),
    ("staged sums do not fit", F.NAMES, 125, (), 1),
    ("64 KiB of LDS halves the tile", F.NAMES, 120, (), 2),
    ("deepest tile of 4 that fits", F.NAMES, 111, (), 4),
])
def test_requested_width_4_follows_the_width_rules(fa, monkeypatch, case, names, n_layers, env,
                                                   width):
    """E6: FREI_ATM_TILE=4 on 300 wavelengths x 3 atmospheres; path()["atm_tile"] is what
    atm_tile_width derives (see the arithmetic above), and two iterations are bitwise the
    FREI_ATM_TILE=1 run under the same knobs.  The top of the atmosphere is at 1e-2 bar: with
    more than a hundred layers down to 1e-6 bar the reference algorithm's own T update turns
    temperatures negative within two iterations (the oracle gives NaN there too).  120 layers
    at width 2 (39680 bytes) and 111 layers at width 4 (exactly 64 KiB) are the kernel's
    largest-LDS launches."""
    ns = n_layers - 1
    fits = len(names) >= 2 and not env and F.staged_sums_fit(ns)
    derived = 1 if not fits else next(t for t in (4, 2, 1) if t == 1 or
                                      F.tile_lds_bytes(t, ns) <= 64 * 1024)
    assert derived == width, (case, derived)
    _tiles_against_tile_1(fa, monkeypatch, names, 300, n_layers, 3, seed=70, want={4: width},
                          env=env, tiles=(1, 4), p_toa=-2)
