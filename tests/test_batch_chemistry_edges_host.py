"""The fixtures of tests/chem_batch_fixtures.py have the properties they exist for, proved on
the CPU with the oracle alone (no GPU, no engine objects): tests/test_gpu_batch_chemistry_edges.py
then runs the atmosphere-tiled sweep on inputs that really take its high-albedo branch, leave the
tables' T ranges, and present every shape of run mask.  The figures in the docstrings are the
measured ones (printed by each test)."""
import numpy as np
import pytest

from tests import chem_batch_fixtures as F

LAYERS = (0, 5, 10, 19)


@pytest.mark.parametrize("kind", ["H", "H6"])
def test_high_albedo_fixtures_mix_both_branches_in_most_waves(kind):
    """H / H6: per atmosphere a share of the lanes has w0 > 0.1 at layers 0, 5, 10 and 19 of the
    oracle's final T, and most 64-lane waves hold lanes on both sides at layer 5 of T0, so the
    wave-uniform branch `!__all(!(w0 > 0.1))` is taken with both heads live in one wave.

    Measured: H lane fractions 0.097..0.273 (per atmosphere, min..max over the four layers:
    0.187..0.269, 0.110..0.174, 0.187..0.273, 0.097..0.200, 0.097..0.200), mixed waves at layer 5
    of T0 0.73, 0.55, 0.73, 0.55, 0.55; H6 lane fractions 0.097..0.314, mixed 0.82, 0.55, 0.82,
    0.55, 0.55.  One-ulp floors (spectrum / F_up / F_down / T), largest over the atmospheres:
    H 2.7e-13 / 6.4e-14 / 4.6e-13 / 2.2e-16, below 1e-11: 1e-10 outright; H6 4.2e-11 / 1.0e-11 /
    5.5e-11 / 9.7e-12: the floor rule, max(1e-10, 2 x floor), with H as its outright twin."""
    fx = F.fixture(kind)
    worst = np.zeros(4)
    for m in range(F.N_ATM):
        oT = F.oracle(fx, m, **F.KW_FIXED)[1]
        frac = [float((F.albedo(fx, m, oT, l) > 0.1).mean()) for l in LAYERS]
        mixed = F.mixed_waves(F.albedo(fx, m, fx["T0"][m], 5))
        flux, T_floor = F.floors(fx, m, **F.KW_FIXED)
        worst = np.maximum(worst, list(flux) + [T_floor])
        print(f"{kind} atmosphere {m}: w0 > 0.1 lane fraction {np.round(frac, 3)}, mixed waves "
              f"at layer 5 of T0 {mixed:.2f}, floors {flux} T {T_floor:.2e}")
        assert all(0.05 < f < 0.6 for f in frac), (m, frac)
        assert mixed >= 0.5, (m, mixed)
        if kind == "H":
            assert max(flux) < 1e-11 and T_floor < 1e-11, (m, flux, T_floor)
        else:
            assert max(flux) < 1e-10 and T_floor < 1e-10, (m, flux, T_floor)
    print(f"{kind}: largest floors spectrum / F_up / F_down / T", worst)
    if kind == "H6":   # it exists for the floor rule: its thin layers lift the floor
        assert worst[:3].max() > 1e-11


def test_high_albedo_fixture_with_fixed_mixing_ratios():
    """H through the contracted path (fixed mock mixing ratios): the same albedo mix, floors
    below 1e-11, so that run is held to 1e-10 outright too.

    Measured: lane fractions 0.164..0.326; floors at most 2.7e-13 / 8.4e-14 / 1.2e-12 /
    2.2e-16 (spectrum / F_up / F_down / T)."""
    fx = F.fixture("H")
    for m in range(F.N_ATM):
        oT = F.oracle(fx, m, chem=False, **F.KW_FIXED)[1]
        frac = [float((F.albedo(fx, m, oT, l, chem=False) > 0.1).mean()) for l in LAYERS]
        mixed = F.mixed_waves(F.albedo(fx, m, fx["T0"][m], 5, chem=False))
        flux, T_floor = F.floors(fx, m, chem=False, **F.KW_FIXED)
        print(f"H fixed mmr, atmosphere {m}: lane fraction {np.round(frac, 3)}, mixed {mixed:.2f}, "
              f"floors {flux} T {T_floor:.2e}")
        assert all(0.05 < f < 0.6 for f in frac) and mixed >= 0.5, (m, frac, mixed)
        assert max(flux) < 1e-11 and T_floor < 1e-11, (m, flux, T_floor)


def test_out_of_range_fixture_has_layers_on_both_sides_of_both_tables():
    """R: opacity T nodes linspace(1850, 2900, 6), chemistry T nodes in [2000, 2750].  At T0 and
    at the oracle's final T every atmosphere has at least two layers above and two below the
    opacity range (there the opacity is 0 and w0 is exactly 1/2 for the whole wave) and the
    chemistry range (the table clamps); the in-range layers still mix both branches inside
    their waves; the oracle's outputs are finite.

    Measured (above, below), T0 then final T — opacity: (2, 9), (2, 9), (3, 8) -> (3, 9),
    (9, 2), (9, 2); chemistry: (3, 10) -> (3, 11), (3, 10) -> (3, 11), (4, 10), (10, 4),
    (10, 4).  Mixed waves of the in-range layers 0.55..0.82.  Floors (spectrum / F_up / F_down /
    T) per atmosphere: 7.3e-12 / 1.1e-12 / 7.0e-12 / 1.2e-13; 1.5e-11 / 2.3e-12 / 1.0e-11 /
    5.1e-13; 2.6e-11 / 3.1e-12 / 2.1e-11 / 1.2e-12; 5.2e-12 / 3.1e-13 / 5.3e-12 / 2.1e-14;
    3.2e-11 / 7.1e-13 / 1.6e-11 / 2.2e-13 — below 1e-10, above 1e-11: the floor rule."""
    fx = F.fixture("R")
    for m in range(F.N_ATM):
        osp, oT, _, _, ou, od, _ = F.oracle(fx, m, **F.KW_FIXED)
        for T, when in ((fx["T0"][m], "T0"), (oT, "final T")):
            for nodes, what in ((fx["Tn"], "opacity"), (fx["chem_T"], "chemistry")):
                above, below = F.outside(T, nodes)
                print(f"R atmosphere {m}, {when}, {what}: {above} layers above, {below} below")
                assert above >= 2 and below >= 2, (m, when, what, above, below)
            # outside the opacity range the oracle's opacity is 0: w0 is exactly 1/2
            out = [l for l in range(F.N_LAYERS) if not fx["Tn"][0] <= T[l] <= fx["Tn"][-1]]
            assert all(np.all(F.albedo(fx, m, T, l) == 0.5) for l in out)
        inside = [l for l in range(F.N_LAYERS) if fx["Tn"][0] <= oT[l] <= fx["Tn"][-1]]
        mixed = [F.mixed_waves(F.albedo(fx, m, oT, l)) for l in inside]
        print(f"R atmosphere {m}: in-range layers {inside}, mixed waves {np.round(mixed, 2)}")
        assert len(inside) >= 2 and min(mixed) >= 0.5, (m, inside, mixed)
        assert all(np.all(np.isfinite(x)) for x in (osp, oT, ou, od))
        flux, T_floor = F.floors(fx, m, **F.KW_FIXED)
        print(f"R atmosphere {m}: floors {flux} T {T_floor:.2e}")
        assert max(flux) < 1e-10 and T_floor < 1e-10, (m, flux, T_floor)


def test_permuted_orders_present_every_run_mask_shape():
    """P: the oracle's counts are 13, 14, 13, 13, 12 in natural order; atmospheres are
    independent, so a reordered batch carries them along.  Block 0 of a tile of 4 then sees,
    in iterations 13 and 14: a converged atmosphere between two running ones, a converged leader
    with followers, a converged last slot (and a block that retires while the partial tile's
    block still runs), and a lone running last slot; a tile of 2 sees [1, 0] and [0, 1]."""
    fx = F.fixture("P")
    counts = [F.oracle(fx, m, **F.KW_CONV)[6] for m in range(F.N_ATM)]
    print("oracle iteration counts", counts)
    assert counts == F.P_COUNTS
    want = {"gap": ([14, 12, 13, 13, 13], [1, 0, 1, 1], [1, 0, 0, 0]),
            "leader": ([12, 14, 13, 13, 13], [0, 1, 1, 1], [0, 1, 0, 0]),
            "last_slot_converged": ([13, 13, 13, 12, 14], [1, 1, 1, 0], [0, 0, 0, 0]),
            "only_last_slot": ([13, 12, 13, 14, 13], [1, 0, 1, 1], [0, 0, 0, 1])}
    assert set(want) == set(F.P_ORDERS)
    pair_masks = set()
    for name, order in F.P_ORDERS.items():
        assert sorted(order) == list(range(F.N_ATM))
        permuted = [counts[m] for m in order]
        masks4 = F.run_masks(permuted, 4)
        print(name, order, permuted, "tile 4, block 0:", masks4[12][0], masks4[13][0],
              "block 1:", masks4[12][1], masks4[13][1])
        assert (permuted, masks4[12][0], masks4[13][0]) == want[name]
        # until iteration 12 every slot of the batch runs
        assert all(masks4[n][0] == [1, 1, 1, 1] and masks4[n][1] == [1, 0, 0, 0]
                   for n in range(12))
        for row in F.run_masks(permuted, 2):
            pair_masks.update(tuple(mask) for mask in row[:2])   # the two full tiles
    # the whole block retires while the partial tile's block still runs
    last = F.run_masks([counts[m] for m in F.P_ORDERS["last_slot_converged"]], 4)[13]
    assert last == [[0, 0, 0, 0], [1, 0, 0, 0]]
    assert (1, 0) in pair_masks and (0, 1) in pair_masks, pair_masks


def test_layer_counts_of_the_width_rules():
    """The layer counts of the GPU width cases, from atm_tile_width's formulas with
    sizeof(FastStepS) = 120 (read off frei_device.h: five doubles, one int64, two int32 and
    kMaxFastS = 8 mmr doubles) and kStageRow = 72: a tile of 4 fits 64 KiB of LDS up to 111
    layers (exactly 65536 bytes), the staged sums fit up to 124 layers, so a requested width of 4
    becomes 2 from 112 to 124 layers (120: 39680 bytes) and 1 from 125 on."""
    import pathlib
    import re
    root = pathlib.Path(__file__).resolve().parents[1]
    dev = (root / "frei_amd/csrc/frei_device.h").read_text()
    ker = (root / "frei_amd/csrc/frei_kernels.hip").read_text()
    assert re.search(r"constexpr int kBlock = 256;", dev)
    assert re.search(r"constexpr int kMaxFastS = 8;", dev)
    assert re.search(r"constexpr int kStageRow = 72;", ker)
    body = re.search(r"struct FastStepS \{(.*?)\};", dev, re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    size = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind, names = decl.split(None, 1)
        n = sum(8 if "[kMaxFastS]" in v else 1 for v in names.split(","))
        size += n * {"double": 8, "int64_t": 8, "int32_t": 4}[kind]
    assert size == 120, size
    assert F.tile_lds_bytes(4, 110) == 65536 < F.tile_lds_bytes(4, 111)
    assert F.staged_sums_fit(123) and not F.staged_sums_fit(124)
    assert F.tile_lds_bytes(4, 119) > 65536 >= F.tile_lds_bytes(2, 119) == 39680
    assert F.staged_sums_fit(119)
