"""Host tests of the Doppler cross-correlation (frei_amd.crosscorr) that need no GPU: the plan
against the loop restatement (tests/crosscorr_ref.py) bitwise, the statistics and the K_p-V_sys
map against loops to 1e-12 relative (a handful of NumPy operations on the same inputs), and
frei_ccf_create's validation, which happens before any device call."""
import ctypes

import numpy as np
import pytest

from tests import crosscorr_ref as R


def _axis(n=33):
    return np.exp(np.linspace(np.log(1.0), np.log(2.0), n))


def test_plan_is_bitwise_the_restatement():
    from frei_amd.crosscorr import CrossCorrelator
    lam = _axis()
    rng = np.random.default_rng(1)
    wl = rng.uniform(1.05, 1.9, 40)                 # unsorted
    wl[3], wl[17] = lam[5], lam[20]                 # exact hits at v = 0
    wl[8] = lam[-1]                                 # the axis' last point at v = 0
    wl[0], wl[11] = 0.9, 0.999                      # below the axis at every velocity here
    wl[30] = 2.5                                    # above it
    vel = np.array([-3000.0, -40.0, 0.0, 14.0, 6000.0])
    cc = CrossCorrelator(lam, wl, rng.normal(1.0, 0.1, (2, 40)), vel)
    idx, frac, n_clamped = R.plan(lam, wl, vel)
    assert cc.idx.dtype == np.int32 and cc.idx.shape == (5, 40) and cc.frac.shape == (5, 40)
    assert np.array_equal(cc.idx, idx)
    assert np.array_equal(cc.frac, frac), "frac must be bitwise the restatement's"
    assert np.array_equal(cc.n_clamped, n_clamped)
    v0 = 2                                          # d_v = 1 exactly
    assert (cc.idx[v0, 3], cc.frac[v0, 3]) == (5, 0.0)
    assert (cc.idx[v0, 17], cc.frac[v0, 17]) == (20, 0.0)
    assert (cc.idx[v0, 8], cc.frac[v0, 8]) == (lam.size - 2, 1.0)
    for v in range(5):                              # clamped pixels sit on the axis' ends
        assert (cc.idx[v, 0], cc.frac[v, 0]) == (0, 0.0)
        assert (cc.idx[v, 30], cc.frac[v, 30]) == (lam.size - 2, 1.0)
    assert cc.n_clamped[v0] == 3
    # at -3000 km/s the pixel at 0.999 um samples the axis and the one at lam[-1] leaves it
    assert cc.n_clamped[0] == 3 and cc.frac[0, 11] > 0.0 and cc.idx[0, 11] == 0
    for v in range(5):
        s = wl * (1.0 / (1.0 + vel[v] / R.C_KMS))
        assert cc.n_clamped[v] == np.count_nonzero((s < lam[0]) | (s > lam[-1]))
    assert np.all((cc.idx >= 0) & (cc.idx <= lam.size - 2))
    assert np.all((cc.frac >= 0.0) & (cc.frac <= 1.0))


def test_constructor_arguments():
    from frei_amd.crosscorr import CrossCorrelator
    lam = _axis()
    with pytest.raises(ValueError, match="ascending"):
        CrossCorrelator(lam[::-1], [1.5], [1.0], [0.0])
    with pytest.raises(ValueError, match="n_pix"):
        CrossCorrelator(lam, [1.5, 1.6], [[1.0, 2.0, 3.0]], [0.0])
    with pytest.raises(ValueError, match="weights"):
        CrossCorrelator(lam, [1.5, 1.6], [1.0, 2.0], [0.0], weights=[1.0])
    cc = CrossCorrelator(lam, [1.5, 1.6], [1.0, 2.0], 10.0)
    assert (cc.n_exp, cc.n_pix, cc.n_vel, cc.n_lam) == (1, 2, 1, 33)
    assert np.array_equal(cc.weights, [1.0, 1.0]) and np.array_equal(cc.a, [[1.0, 2.0]])


def _small():
    """2 atmospheres, 3 exposures, 7 velocities, 30 pixels on 40 points: the sums of the
    restatement, for the statistics."""
    rng = np.random.default_rng(2)
    lam = _axis(40)
    wl = rng.uniform(1.1, 1.8, 30)
    vel = np.linspace(-60.0, 60.0, 7)
    y = 1e-3 * (1.0 + 0.3 * rng.uniform(-1, 1, (2, 40)))
    flux = 1e-3 * (1.0 + 0.3 * rng.uniform(-1, 1, (3, 30)))
    w = rng.uniform(0.5, 1.5, 30)
    return lam, wl, vel, y, flux, w


def test_statistics_against_loops():
    from frei_amd.crosscorr import CrossCorrelation, CrossCorrelator
    lam, wl, vel, y, flux, w = _small()
    cc = CrossCorrelator(lam, wl, flux, vel, weights=w)
    W, S_wf, S_wff = R.host_sums(flux, w)
    assert abs(cc.W - W) <= 1e-12 * W
    assert np.all(np.abs(cc.S_wf - S_wf) <= 1e-12 * np.abs(S_wf))
    assert np.all(np.abs(cc.S_wff - S_wff) <= 1e-12 * np.abs(S_wff))
    assert np.array_equal(cc.a, w * flux)
    sfg, sg, sgg = R.sums(y, cc.idx, cc.frac, cc.a, w)
    res = CrossCorrelation(sfg, sg, sgg, vel, cc.W, cc.S_wf, cc.S_wff, cc.n_pix)
    ref = R.ccf(sfg, sg, sgg, cc.W, cc.S_wf, cc.S_wff)
    got = res.ccf()
    assert got.shape == (2, 3, 7) and np.all(np.abs(ref) <= 1.0)
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref))
    ref = R.loglike(sfg, sg, sgg, cc.W, cc.S_wf, cc.S_wff, cc.n_pix)
    got = res.loglike()
    assert got.shape == (2, 3, 7) and np.all(np.isfinite(ref))
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref))
    # a single template: no atmosphere axis
    one = CrossCorrelation(sfg[1], sg[1], sgg[1], vel, cc.W, cc.S_wf, cc.S_wff, cc.n_pix)
    assert one.ccf().shape == (3, 7) and np.array_equal(one.ccf(), res.ccf()[1])
    assert np.array_equal(one.loglike(), res.loglike()[1])
    with pytest.raises(ValueError, match="all three"):
        CrossCorrelation(sfg, None, sgg, vel, cc.W, cc.S_wf, cc.S_wff, cc.n_pix).ccf()


def test_a_template_correlates_perfectly_with_itself():
    """Data that are a template sampled at one of the trial velocities: CCF = 1 there, for any
    weights, and below 1 elsewhere."""
    from frei_amd.crosscorr import CrossCorrelation, CrossCorrelator
    lam, wl, vel, y, _, w = _small()
    probe = CrossCorrelator(lam, wl, np.zeros(30), vel, weights=w)
    j, t = probe.idx[4], probe.frac[4]
    flux = y[0][j] + t * (y[0][j + 1] - y[0][j])
    cc = CrossCorrelator(lam, wl, flux, vel, weights=w)
    sfg, sg, sgg = R.sums(y, cc.idx, cc.frac, cc.a, w)
    c = CrossCorrelation(sfg, sg, sgg, vel, cc.W, cc.S_wf, cc.S_wff, 30).ccf()
    assert abs(c[0, 0, 4] - 1.0) <= 1e-9
    assert np.all(c[0, 0, [0, 1, 2, 3, 5, 6]] < 1.0 - 1e-6) and np.all(c[1] < 1.0 - 1e-6)


def test_kp_vsys_map_against_loops():
    from frei_amd.crosscorr import kp_vsys_map
    rng = np.random.default_rng(3)
    vel = np.linspace(-100.0, 100.0, 41)
    values = rng.uniform(1.0, 2.0, (2, 4, 41))
    phases = np.array([0.30, 0.35, 0.42, 0.61])
    Kp, Vsys = np.linspace(0.0, 200.0, 5), np.linspace(-30.0, 30.0, 7)
    v_obs = np.array([1.0, 0.5, -0.5, -1.0])
    ref = R.kp_vsys_map(values, vel, phases, Kp, Vsys, v_obs)
    got = kp_vsys_map(values, vel, phases, Kp, Vsys, v_obs=v_obs)
    assert got.shape == (2, 5, 7)
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref))
    assert np.any(Kp[-1] * np.sin(2 * np.pi * phases) + Vsys[0] < vel[0]), "the ends are used"
    # no leading axis, a scalar v_obs
    flat = kp_vsys_map(values[1], vel, phases, Kp, Vsys)
    ref0 = R.kp_vsys_map(values[1:], vel, phases, Kp, Vsys, np.zeros(4))[0]
    assert flat.shape == (5, 7) and np.all(np.abs(flat - ref0) <= 1e-12 * np.abs(ref0))
    # a delta at (Kp, Vsys): each exposure's CCF peaks on the planet's trail
    trail = np.zeros((4, 41))
    for e in range(4):
        trail[e, 20 + round((10.0 + 60.0 * np.sin(2 * np.pi * phases[e])) / 5.0)] = 1.0
    m = kp_vsys_map(trail, vel, phases, [30.0, 60.0, 90.0], [0.0, 10.0, 20.0])
    assert np.unravel_index(np.argmax(m), m.shape) == (1, 1)
    with pytest.raises(ValueError, match="values"):
        kp_vsys_map(values[:, :3], vel, phases, Kp, Vsys)


def _correlator(**tamper):
    from frei_amd.crosscorr import CrossCorrelator
    lam, wl, vel, _, flux, w = _small()
    cc = CrossCorrelator(lam, wl, flux, vel, weights=w)
    for name, (where, v) in tamper.items():
        getattr(cc, name)[where] = v
    return cc


@pytest.mark.parametrize("tamper, message", [
    (dict(idx=((1, 2), 39)), r"idx\[1\]\[2\] = 39"),          # n_lam - 1
    (dict(idx=((6, 29), -1)), r"idx\[6\]\[29\] = -1"),
    (dict(frac=((0, 5), 1.0000001)), r"frac\[0\]\[5\]"),
    (dict(frac=((3, 0), np.nan)), r"frac\[3\]\[0\]"),
    (dict(a=((2, 7), np.nan)), r"a\[2\]\[7\]"),
    (dict(weights=(4, -0.5)), r"w\[4\]"),
    (dict(weights=(slice(None), 0.0)), "sum to zero"),
])
def test_create_rejects_bad_plans_before_touching_a_device(tamper, message):
    cc = _correlator(**tamper)
    with pytest.raises(RuntimeError, match=message):
        cc.handle()
    assert cc._handle is None


def test_create_rejects_a_one_point_axis():
    from frei_amd import _native as N
    h = ctypes.c_void_p()
    idx, one = np.zeros(1, dtype=np.int32), np.ones(1)
    rc = N.lib().frei_ccf_create(ctypes.byref(h), 0, 1, 1, 1,
                                 idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                 N.dptr(one), 1, N.dptr(one), N.dptr(one))
    assert rc != 0 and b"n_lam must be >= 2" in N.lib().frei_last_error()
    assert not h.value
    assert N.lib().frei_ccf_apply(None, None, None, 1, None, 0, None, None, None, 0, None, None,
                                  None, None, None) != 0
    assert N.lib().frei_ccf_destroy(None) == 0


def test_exports():
    import frei_amd
    from frei_amd import crosscorr
    assert 1 in crosscorr.FORMS and 0 not in crosscorr.FORMS
    assert crosscorr.PIXEL_CHUNK >= 64 and crosscorr.PIXEL_CHUNK % 64 == 0
    assert frei_amd.CrossCorrelator is crosscorr.CrossCorrelator
    assert frei_amd.kp_vsys_map is crosscorr.kp_vsys_map
