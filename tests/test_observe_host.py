"""Host-side tests of the synthetic observations (K10): the Instrument constructors against the
explicit loops of tests/observe_ref.py, the plan validation of frei_obs_create (it runs before
any device call) and the argument checks of the user-level calls.  No GPU."""
import ctypes

import numpy as np
import pytest

from tests import observe_ref as R

WTOL = 4 * 2.0 ** -53


def _same(inst, ref):
    first, count, weights = ref
    assert inst.first.tolist() == list(first)
    assert inst.count.tolist() == list(count)
    w = np.array(weights)
    assert inst.weights.shape == w.shape
    assert np.all(np.abs(inst.weights - w) <= WTOL * np.abs(w))


def _lam(n=400):
    return np.logspace(np.log10(0.5), 1.0, n)


def test_top_hat_matches_the_loops():
    import frei_amd as fa
    lam = _lam()
    # edges exactly on grid points (both included), a channel of one point, overlapping bands
    # out of wavelength order, a band reaching past either end of the axis
    lo = np.array([lam[10], lam[50], 2.0, lam[7], 0.1, 8.0])
    hi = np.array([lam[20], lam[50], 4.0, lam[15], 0.6, 50.0])
    inst = fa.Instrument.top_hat(lam, lo, hi)
    _same(inst, R.top_hat(lam, lo, hi))
    assert inst.n_channels == 6
    assert (inst.first[0], inst.count[0]) == (10, 11)
    assert (inst.first[1], inst.count[1]) == (50, 1)
    assert inst.first[4] == 0 and inst.first[5] + inst.count[5] == lam.size


def test_top_hat_names_an_empty_channel():
    import frei_amd as fa
    lam = _lam()
    between = 0.5 * (lam[30] + lam[31])
    with pytest.raises(ValueError, match="channel 1"):
        fa.Instrument.top_hat(lam, [1.0, between - 1e-6], [2.0, between + 1e-6])
    with pytest.raises(ValueError, match="channel 1"):
        R.top_hat(lam, [1.0, between - 1e-6], [2.0, between + 1e-6])


def test_throughput_matches_the_loops():
    import frei_amd as fa
    lam = _lam()
    curves = [
        (np.array([1.0, 1.2, 1.8, 2.0]), np.array([0.0, 0.9, 0.8, 0.0])),
        # interior zeros: one contiguous support, zeros kept inside
        (np.array([3.0, 3.2, 3.3, 3.9, 4.0, 4.4]), np.array([0.0, 0.5, 0.0, 0.0, 0.7, 0.0])),
        # running off both ends of the axis
        (np.array([0.1, 0.7]), np.array([1.0, 1.0])),
        (np.array([9.0, 20.0]), np.array([0.3, 0.4])),
    ]
    inst = fa.Instrument.from_throughput(lam, curves)
    ref = R.from_throughput(lam, curves)
    _same(inst, ref)
    off = int(inst.count[0])
    w1 = inst.weights[off:off + int(inst.count[1])]
    assert np.any(w1 == 0.0) and w1[0] > 0.0 and w1[-1] > 0.0
    assert inst.first[2] == 0 and inst.first[3] + inst.count[3] == lam.size
    with pytest.raises(ValueError, match="channel 0"):
        fa.Instrument.from_throughput(lam, [(np.array([20.0, 30.0]), np.array([1.0, 1.0]))])


def test_gaussian_matches_the_loops():
    import frei_amd as fa
    lam = _lam()
    # clipped at either end of the axis, and interior channels
    centres = np.array([lam[0], 1.0, 3.0, lam[-1]])
    inst = fa.Instrument.gaussian(lam, centres, resolving_power=20.0)
    _same(inst, R.gaussian(lam, centres, resolving_power=20.0))
    assert inst.first[0] == 0 and inst.first[3] + inst.count[3] == lam.size
    fw = np.array([0.02, 0.05, 0.3, 1.0])
    inst = fa.Instrument.gaussian(lam, centres, fwhm=fw, n_sigma=3.0)
    _same(inst, R.gaussian(lam, centres, fwhm=fw, n_sigma=3.0))
    one = fa.Instrument.gaussian(lam, [lam[100]], fwhm=1e-6)      # a channel of one point
    assert (one.first[0], one.count[0]) == (100, 1)
    with pytest.raises(ValueError, match="channel 1"):
        fa.Instrument.gaussian(lam, [lam[100], 0.5 * (lam[200] + lam[201])], fwhm=1e-6)
    with pytest.raises(ValueError, match="fwhm or resolving_power"):
        fa.Instrument.gaussian(lam, [1.0])


def test_raw_instrument_checks_its_shapes():
    import frei_amd as fa
    lam = _lam(10)
    inst = fa.Instrument(lam, [0, 3], [2, 4], np.ones(6))
    assert inst.n_channels == 2 and inst.form_used is None and inst.timing() == (0.0, 0)
    inst.release()
    with pytest.raises(ValueError, match="weights"):
        fa.Instrument(lam, [0, 3], [2, 4], np.ones(5))
    with pytest.raises(ValueError, match="n_lam"):
        inst.apply(np.ones(9))
    with pytest.raises(ValueError, match="engine"):
        inst.apply(None)


def test_names_and_abi():
    import frei_amd as fa
    from frei_amd import _native as N
    assert "Instrument" in fa.__all__ and fa.Instrument is not None
    lib = N.lib()
    for name in ("frei_obs_create", "frei_obs_apply", "frei_obs_destroy"):
        assert name in N.SIGNATURES
        assert hasattr(lib, name)
    assert lib.frei_version() == 20000


def _create(n_lam, first, count, weights):
    from frei_amd import _native as N
    lib = N.lib()
    h = ctypes.c_void_p()
    f = np.ascontiguousarray(first, dtype=np.int64)
    c = np.ascontiguousarray(count, dtype=np.int64)
    w = N.f64(weights)
    p = ctypes.POINTER(ctypes.c_int64)
    rc = lib.frei_obs_create(ctypes.byref(h), 0, n_lam, f.size, f.ctypes.data_as(p),
                             c.ctypes.data_as(p), N.dptr(w))
    return rc, lib.frei_last_error().decode(), h


@pytest.mark.parametrize("first,count,weights,msg", [
    ([0, 2], [2, 0], [1.0, 1.0], "channel 1 has count < 1"),
    ([0, 8], [2, 3], [1.0] * 5, "channel 1 has a range outside the axis"),
    ([-1], [2], [1.0, 1.0], "channel 0 has a range outside the axis"),
    ([0, 2, 4], [2, 2, 2], [1.0, 1.0, 1.0, 1.0, -1.0, 2.0],
     "channel 2 has a negative or non-finite weight"),
    ([0, 2], [2, 2], [1.0, 1.0, np.nan, 1.0], "channel 1 has a negative or non-finite weight"),
    ([0, 2], [2, 2], [1.0, np.inf, 1.0, 1.0], "channel 0 has a negative or non-finite weight"),
    ([0, 2], [2, 2], [1.0, 1.0, 0.0, 0.0], "channel 1 has a zero weight sum"),
])
def test_plan_errors_are_named_without_a_device(first, count, weights, msg):
    rc, err, h = _create(10, first, count, weights)
    assert rc != 0 and msg in err, err
    assert not h.value


def test_apply_refuses_a_null_handle():
    from frei_amd import _native as N
    lib = N.lib()
    obs = np.empty(1)
    assert lib.frei_obs_apply(None, None, None, 1, None, None, 0, None, None, None, None, 0,
                              N.dptr(obs), None, None, None) < 0
    assert b"null handle" in lib.frei_last_error()
    assert lib.frei_obs_destroy(None) == 0


def test_eclipse_without_radii_is_refused_before_any_device_work():
    import frei_amd as fa
    from frei_amd.batch import BatchRecord, BatchResult
    lam = _lam(50)
    inst = fa.Instrument.top_hat(lam, [1.0], [2.0])
    pl = fa.Planet(a_rstar=6.45, m_bar=4.0e-24, g=2478.0, T_star=5800.0, alpha=1)
    grid = fa.Grid(pl, lam=lam, n_layers=10)
    spec = fa.Spectrum(np.ones(50), lam)
    with pytest.raises(ValueError, match="R_p"):
        grid.observe(inst, spec, kind="eclipse")
    with pytest.raises(ValueError, match="R_star"):
        grid.observe(inst, spec, kind="eclipse", R_p=7e9)
    with pytest.raises(ValueError, match="kind"):
        grid.observe(inst, spec, kind="phase curve")
    assert grid._engine is None and inst._handle is None

    class NoDevice:            # any use of the engine is an AttributeError
        lam_um = lam
    rec = BatchRecord(spec, np.ones(10), 1, None, 0.0, 0.0, 0.0)
    res = BatchResult([rec, rec], NoDevice(), [pl, pl])
    with pytest.raises(ValueError, match="R_p"):
        res.observe(inst, kind="eclipse")
    with pytest.raises(ValueError, match="R_p"):
        res.observe(inst)
    assert inst._handle is None
