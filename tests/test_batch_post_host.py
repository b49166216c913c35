"""Batched post-processing (frei_run_batch_ex, frei_get_dtaus_batch, frei_post_batch,
frei_post_timing) without a GPU: the symbols and keywords exist and every new entry point
validates its arguments before it touches a device."""
import ctypes
import inspect

import numpy as np


def test_new_names_are_exported():
    import frei_amd as fa
    from frei_amd import _native as N
    for name in ("BatchEngine", "BatchRecord", "BatchResult", "batched_emission_spectra"):
        assert name in fa.__all__ and hasattr(fa, name), name
    assert fa.BatchRecord._fields == ("spectrum", "final_T", "n_iter", "temp_hist", "T_eff",
                                      "T_milne", "T_planck")
    lib = N.lib()
    for sym in ("frei_run_batch_ex", "frei_get_dtaus_batch", "frei_post_batch",
                "frei_post_timing"):
        assert sym in N.SIGNATURES and hasattr(lib, sym), sym
    assert lib.frei_version() == 20000


def test_defaults_of_the_batched_surface_are_unchanged():
    import frei_amd as fa
    run = inspect.signature(fa.BatchEngine.run).parameters
    assert [k for k in run][:6] == ["self", "T_init", "n_timesteps", "n_zero_crossings",
                                    "convergence_dT", "alpha"]
    assert run["want_hist"].default is False and run["keep_dtaus"].default is False
    bes = inspect.signature(fa.batched_emission_spectra).parameters
    assert bes["post"].default is False
    post = inspect.signature(fa.BatchEngine.post).parameters
    assert [post[k].default for k in ("dtaus", "spectra", "T")] == [None, None, None]
    assert post["want_p_milne"].default is False and post["want_cf"].default is False
    assert callable(fa.BatchEngine.get_dtaus)


def test_new_entry_points_reject_null_arguments_without_a_device():
    from frei_amd import _native as N
    lib = N.lib()
    T = np.full((2, 4), 1000.0)
    n_iter = (ctypes.c_int * 2)()
    buf = np.zeros(8)
    # a NULL context: every call fails with a message, before any device call
    calls = [
        lambda: lib.frei_run_batch_ex(None, N.dptr(T), 1, 2, 3.0, 1.0, n_iter, None, None, None,
                                      1),
        lambda: lib.frei_run_batch_ex(None, None, 1, 2, 3.0, 1.0, None, None, None, None, 0),
        lambda: lib.frei_get_dtaus_batch(None, 0, 1, N.dptr(buf)),
        lambda: lib.frei_get_dtaus_batch(None, 0, 1, None),
        lambda: lib.frei_post_batch(None, None, None, None, N.dptr(buf), N.dptr(buf), None, None,
                                    1.0, N.dptr(buf), None, None),
        lambda: lib.frei_post_batch(None, None, None, None, None, None, None, None, 1.0, None,
                                    None, None),
        lambda: lib.frei_post_timing(None, None),
    ]
    for k, call in enumerate(calls):
        assert call() < 0, k
        assert lib.frei_last_error() != b"", k
    ms = ctypes.c_double(-1.0)
    assert lib.frei_post_timing(None, ctypes.byref(ms)) < 0
    assert b"null" in lib.frei_last_error()
