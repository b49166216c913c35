"""Chemistry tables for batched runs (frei_set_chemistry_batch) without a GPU: the symbol and
knob exist, the Python layer de-duplicates tables into (n_tab, atm_tab), refuses mismatched
nodes, a table/array mix and a chemistry provider, and the entry point validates its context
before it touches a device."""
import ctypes
import types

import numpy as np
import pytest


def _table(fa, scale=1.0, T=(500.0, 1500.0, 3000.0), p=(1e-6, 1e-2, 1e2), S=2):
    v = scale * np.arange(1, S * len(T) * len(p) + 1, dtype=float).reshape(S, len(T), len(p))
    return fa.ChemistryTable(v, np.array(T), np.array(p))


def test_entry_point_and_knob_exist():
    from frei_amd import _native as N
    lib = N.lib()
    assert "frei_set_chemistry_batch" in N.SIGNATURES and hasattr(lib, "frei_set_chemistry_batch")
    assert lib.frei_version() == 20000
    assert lib.frei_set_chemistry_batch(None, None, 1, None, None, 0, None, 0) < 0
    assert b"null" in lib.frei_last_error()
    import pathlib
    root = pathlib.Path(__file__).resolve().parents[1]
    assert '"atm_tile"' in (root / "frei_amd/csrc/frei_runtime.hip").read_text()
    assert "`FREI_ATM_TILE`" in (root / "README.md").read_text()


def test_tables_are_deduplicated_by_identity():
    import frei_amd as fa
    from frei_amd.batch import chemistry_tables, stack_chemistry
    a, b = _table(fa), _table(fa, 3.0)
    tables, atm_tab = chemistry_tables([a, b, a, b, b], 5)
    assert len(tables) == 2 and tables[0] is a and tables[1] is b
    assert atm_tab.dtype == np.int32 and atm_tab.tolist() == [0, 1, 0, 1, 1]
    # equal values in two objects stay two tables: identity, not equality
    c = _table(fa)
    tables, atm_tab = chemistry_tables((a, c), 2)
    assert len(tables) == 2 and atm_tab.tolist() == [0, 1]
    # one table serves every atmosphere
    tables, atm_tab = chemistry_tables(a, 4)
    assert tables == [a] and atm_tab.tolist() == [0, 0, 0, 0]
    # fixed mixing ratios are not chemistry tables
    assert chemistry_tables(None, 3) is None
    assert chemistry_tables(np.ones((3, 2, 5)), 3) is None
    assert chemistry_tables([np.ones((2, 5))] * 3, 3) is None
    v = stack_chemistry([a, b], ["x", "y"])
    assert v.shape == (2, 2, 3, 3) and v.flags["C_CONTIGUOUS"]
    assert np.array_equal(v[1], 3.0 * v[0])
    with pytest.raises(ValueError, match="3 chemistry tables for 2 atmospheres"):
        chemistry_tables([a, b, a], 2)


def test_node_mismatch_is_refused():
    import frei_amd as fa
    from frei_amd.batch import stack_chemistry
    a = _table(fa)
    for other in (_table(fa, T=(500.0, 1600.0, 3000.0)), _table(fa, p=(1e-6, 1e-3, 1e2)),
                  _table(fa, T=(500.0, 3000.0))):
        with pytest.raises(ValueError, match="share their temperature and pressure nodes"):
            stack_chemistry([a, other], ["x", "y"])


def test_table_and_array_mix_is_refused():
    import frei_amd as fa
    from frei_amd.batch import chemistry_tables
    a = _table(fa)
    with pytest.raises(ValueError, match="not a mix"):
        chemistry_tables([a, np.ones((2, 5))], 2)


def _grid(mmr=None, chemistry=None):
    """What batched_emission_spectra reads of a Grid before it creates an engine."""
    lam = np.linspace(1.0, 2.0, 8)
    p = np.geomspace(10.0, 1e-4, 5)
    planet = types.SimpleNamespace(alpha=1.0, m_bar=4.0e-24, g=1000.0, T_star=5800.0,
                                   a_rstar=6.0)
    return types.SimpleNamespace(lam=lam, pressures=p, opacities=_OPACITIES, planet=planet,
                                 mmr=mmr, chemistry=chemistry, init_temperatures=np.full(5, 1e3))


_OPACITIES = {"1H2-16O": None, "12C-16O": None}


def test_grids_with_a_provider_or_a_mix_are_refused_before_any_device_work():
    import frei_amd as fa
    from frei_amd.batch import grid_mixing_ratios
    a, b = _table(fa), _table(fa, 2.0)

    def provider(T, p, species, m_bar=None):
        return {s: np.full(np.shape(T), 1e-3) for s in species}

    with pytest.raises(ValueError, match="tabulate it as a ChemistryTable"):
        fa.batched_emission_spectra([_grid(mmr=None), _grid(chemistry=provider)])
    with pytest.raises(ValueError, match="not a mix"):
        fa.batched_emission_spectra([_grid(mmr=a), _grid(mmr=np.ones((2, 5)))])
    with pytest.raises(ValueError, match="not a mix"):
        fa.batched_emission_spectra([_grid(mmr=a), _grid(mmr=None)])
    with pytest.raises(ValueError, match="share their temperature and pressure nodes"):
        fa.batched_emission_spectra([_grid(mmr=a), _grid(mmr=_table(fa, T=(1.0, 2.0, 3.0)))])
    names = list(_OPACITIES)
    out = grid_mixing_ratios([_grid(mmr=a), _grid(mmr=b), _grid(mmr=a)], names)
    assert len(out) == 3 and out[0] is a and out[1] is b and out[2] is a
    fixed = grid_mixing_ratios([_grid(), _grid(mmr=np.full((2, 5), 2e-3))], names)
    assert fixed.shape == (2, 2, 5) and np.all(fixed[1] == 2e-3)


def test_single_context_is_refused_before_a_device_call():
    """The message names frei_set_chemistry; the check precedes every device call, so a context
    is not needed to see the NULL-context refusal, and the header documents the rest."""
    import pathlib
    hdr = (pathlib.Path(__file__).resolve().parents[1] / "include/frei_hip.h").read_text()
    assert "int frei_set_chemistry_batch(frei_ctx* ctx, const double* values, int n_tab," in hdr
    from frei_amd import _native as N
    res, args = N.SIGNATURES["frei_set_chemistry_batch"]
    assert res is ctypes.c_int and len(args) == 8
    assert args[3] == ctypes.POINTER(ctypes.c_int32)
