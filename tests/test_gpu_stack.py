"""GPU tests of the orbital stack (K14, frei_stack_apply): OrbitStack.stack against
tests/stack_ref.py, the plain restatement of the definition (the reference has no counterpart),
the bitwise guarantees of the header, the statistic against its bounded high-precision
reference, NaN containment, the correlator's keep mode, and a small injection end to end.

Tolerances, derived rather than measured (stack_ref.py):
  stack of given values    u and j are identical in exact arithmetic and the sums run in the same
      order; only t's division and knock-on roundings could differ:
      |map - ref| <= (n_exp + 4) 2^-53 sum_e (|f_j| + |f_{j+1}|).  The device's fp64 division is
      the correctly rounded one, so bitwise equality with the restatement is asserted as well.
  statistic    |values - ref| <= 2 x the first-order bound of the 60-digit reference (0.5 ulp for
      + - * / sqrt, 2 ulp for log; the factor 2 covers the second order, the convention of
      test_gpu_update_exact.py).  The cases are built so that the bound stays below 1e-9 |value|
      for every element (asserted on the CPU); no element is skipped.
  statistic then stack    the stack's bound on the reference values plus sum_e (B_j + B_{j+1}),
      B the statistic's tolerance: a linear interpolation with t in [0, 1] moves by no more than
      the errors of its two points together (stack_ref.stacked_statistic_bound).
  end to end against the host path    kp_vsys_map(res.loglike()) and the device map are each
      within that last bound of the stack of the reference values (np.interp's slope form obeys
      the stack's bound, tests/test_stack_host.py), so they differ by at most twice it.
Each test prints its measured maximum of |got - ref| / bound (pytest -s).

Measured on MI355X (maximum of |got - ref| / bound): stack of given values 0 — every map of the
base shape (forms 1, 2 and 0) and of the 24 edge shapes is bitwise the restatement's; statistic
0.155 (ccf; its bound at most 1.7e-13 |value|) and 0.122 (loglike; 2.0e-14 |value|) of twice the
first-order bound; statistic then stack 0.033 (ccf) and 0.029 (loglike); end to end against
kp_vsys_map(res.loglike()) 0.0077, the injected atmosphere's maximum 32515.2 at the injected
(K_p, V_sys) against 13611.7 and 12950.0 for the two others.
"""
import ctypes
import functools

import numpy as np
import pytest

from tests import crosscorr_ref as R
from tests import stack_ref as S

pytestmark = pytest.mark.gpu

BASE = dict(n_atm=3, n_exp=3, n_vel=7, n_kp=3, n_vsys=5)


def _tile():
    from frei_amd.stack import ATM_TILE
    return ATM_TILE


def _lds():
    from frei_amd.stack import LDS_VELOCITIES
    return LDS_VELOCITIES


def _edge_shapes():
    """One axis at a time at its edges, the others at base."""
    T = _tile()
    shapes = []
    for key, values in (("n_vsys", (1, 63, 64, 65, 257)), ("n_exp", (1, 2, 17)),
                        ("n_vel", (2, 3, 65, 513, _lds(), _lds() + 1)), ("n_kp", (1, 4)),
                        ("n_atm", (1, 2, T - 1, T, T + 1))):
        for v in values:
            s = tuple(dict(BASE, **{key: v}).values())
            if s not in shapes and s != tuple(BASE.values()):
                shapes.append(s)
    return shapes


def pytest_generate_tests(metafunc):
    if "shape" in metafunc.fixturenames:
        metafunc.parametrize("shape", _edge_shapes(),
                             ids=lambda s: "atm%d-exp%d-vel%d-kp%d-vsys%d" % s)
    if "form" in metafunc.fixturenames:
        from frei_amd.stack import FORMS
        metafunc.parametrize("form", (*FORMS, 0))


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    from frei_amd import _native as N
    assert N.device_count() >= 1, "no HIP device visible"
    return frei_amd


# ------------------------------------------------------------------ cases
def _grid(n_vel):
    """Non-uniform, ascending, dyadic: sums with the dyadic shifts below are exact."""
    steps = np.array([0.5, 1.0, 1.5, 2.0, 0.75, 1.25])[np.arange(n_vel - 1) % 6]
    return np.concatenate([[-4.0], -4.0 + np.cumsum(steps)])


@functools.lru_cache(maxsize=None)
def _case(n_atm, n_exp, n_vel, n_kp, n_vsys):
    """shifts dv (multiples of 1/4, dv[0][0] = 0), v_obs (multiples of 1/8, v_obs[0] = 0) and an
    unsorted vsys whose first entries put (k, e) = (0, 0) exactly on an interior node, above the
    last node, on the first node, below the first and on the last; the rest spread over the grid
    and a little beyond.  Signed values."""
    rng = np.random.default_rng([n_atm, n_exp, n_vel, n_kp, n_vsys])
    vel = _grid(n_vel)
    dv = rng.integers(-12, 13, (n_kp, n_exp)) / 4.0
    v_obs = rng.integers(-8, 9, n_exp) / 8.0
    dv[0, 0] = v_obs[0] = 0.0
    special = [vel[n_vel // 2], vel[-1] + 10.0, vel[0], vel[0] - 10.0, vel[-1]]
    vsys = rng.uniform(vel[0] - 3.0, vel[-1] + 3.0, n_vsys)
    vsys[:min(5, n_vsys)] = special[:n_vsys]
    values = rng.normal(0.0, 1.0, (n_atm, n_exp, n_vel))
    for a in (vel, dv, v_obs, vsys, values):
        a.setflags(write=False)
    return dict(vel=vel, dv=dv, v_obs=v_obs, vsys=vsys, values=values)


@functools.lru_cache(maxsize=None)
def _reference(*shape):
    """(j, t, outside, map, bound) of the restatement for _case; computed once, left unchanged."""
    c = _case(*shape)
    j, t, outside = S.brackets(c["vel"], c["dv"], c["v_obs"], c["vsys"])
    ref, bound = S.stack(c["values"], j, t), S.stack_bound(c["values"], j)
    for a in (j, t, outside, ref, bound):
        a.setflags(write=False)
    return j, t, outside, ref, bound


def _stacker(fa, c, kp=slice(None), vs=slice(None)):
    return fa.OrbitStack(c["vel"], np.zeros(c["dv"].shape[0])[kp], c["vsys"][vs],
                         shifts=c["dv"][kp], v_obs=c["v_obs"])


def _ratio(got, ref, bound):
    d = np.abs(np.asarray(got) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.max(np.where(d == 0.0, 0.0, d / bound)))


# ------------------------------------------------------------------ 1: parity
def test_base_shape_against_restatement(fa, form):
    """Measured on MI355X: exactly the restatement's numbers, for every form."""
    shape = tuple(BASE.values())
    c = _case(*shape)
    j, t, outside, ref, bound = _reference(*shape)
    n = BASE["n_vel"]
    # (k, e) = (0, 0): an interior node, above, the first node, below, the last node
    assert [(j[0, 0, s], t[0, 0, s], bool(outside[0, 0, s])) for s in range(5)] == [
        (n // 2, 0.0, False), (n - 2, 1.0, True), (0, 0.0, False), (0, 0.0, True),
        (n - 2, 1.0, False)]
    assert np.any(np.diff(c["vsys"]) < 0) and np.any(np.diff(c["vsys"]) > 0), "unsorted"
    st = _stacker(fa, c)
    try:
        assert np.array_equal(st.n_outside, outside.sum(axis=(1, 2)))
        got = st.stack(c["values"], form=form)
        assert st.form_used == (form or 1) and st.timing()[1] == 1
        one = st.stack(c["values"][1], form=form)
    finally:
        st.release()
    r = _ratio(got, ref, bound)
    print(f"base shape, form {form}: max |map - ref| / bound = {r:.3g}")
    assert got.shape == (3, 3, 5) and np.all(np.abs(got - ref) <= bound)
    assert np.array_equal(got, ref), "the division is correctly rounded: the restatement's bits"
    assert one.shape == (3, 5) and np.array_equal(one, got[1])


def test_axis_edges_against_restatement(fa, shape):
    """Measured on MI355X: exactly the restatement's numbers for every shape, and form 2
    bitwise form 1."""
    c = _case(*shape)
    _, _, _, ref, bound = _reference(*shape)
    st = _stacker(fa, c)
    try:
        got = st.stack(c["values"])
        assert st.form_used == (1 if shape[2] <= _lds() else 2)
        other = st.stack(c["values"], form=2) if st.form_used == 1 else None
    finally:
        st.release()
    r = _ratio(got, ref, bound)
    print(f"shape {shape}: max |map - ref| / bound = {r:.3g}")
    assert got.shape == ref.shape and np.all(np.abs(got - ref) <= bound)
    assert np.array_equal(got, ref)
    assert other is None or np.array_equal(other, got), "the forms give the same bits"


# ------------------------------------------------------------------ 2: bitwise properties
def test_bitwise_repeat_rows_and_subsets(fa):
    T = _tile()
    shape = (T + 1, 3, 7, 4, 65)
    c = _case(*shape)
    st = _stacker(fa, c)
    try:
        full = st.stack(c["values"])
        again = st.stack(c["values"])
        rows = {m: st.stack(c["values"][m]) for m in (0, T - 1, T)}
        pair = st.stack(c["values"][T - 1:])
    finally:
        st.release()
    assert np.array_equal(full, again), "a repeated call"
    for m, one in rows.items():
        assert np.array_equal(one, full[m]), f"row {m} alone"
    assert np.array_equal(pair, full[T - 1:])
    kp, vs = np.array([2, 0]), np.array([64, 3, 17, 0])
    sub = _stacker(fa, c, kp=kp, vs=vs)
    try:
        part = sub.stack(c["values"])
    finally:
        sub.release()
    assert part.shape == (T + 1, 2, 4)
    assert np.array_equal(part, full[:, kp][:, :, vs]), "a K_p / V_sys subset of the handle"


# ------------------------------------------------------------------ 3: statistic
@functools.lru_cache(maxsize=None)
def _sums_case():
    """Sums of the K12 restatement for 3 offset-subtracted templates against 3 exposures of noisy
    data (atmosphere 0's template plus noise), 7 velocities, 60 weighted pixels: V_f, V_g and
    the log's argument are positive."""
    from frei_amd.crosscorr import doppler_plan
    rng = np.random.default_rng(140)
    lam = np.exp(np.linspace(np.log(1.0), np.log(1.01), 200))
    wl = np.sort(rng.uniform(1.002, 1.008, 60))
    vel = np.array([-30.0, -19.0, -11.0, -2.0, 4.0, 13.0, 31.0])        # non-uniform
    y = rng.normal(0.0, 0.1, (3, 200))
    y -= y.mean(axis=1, keepdims=True)
    idx, frac, _ = doppler_plan(lam, wl, vel)
    flux = 1.0 + y[0][idx[3]] + frac[3] * (y[0][idx[3] + 1] - y[0][idx[3]]) + \
        rng.normal(0.0, 0.05, (3, 60))
    w = rng.uniform(0.5, 1.5, 60)
    sfg, sg, sgg = R.sums(y, idx, frac, w * flux, w)
    W, S_wf, S_wff = R.host_sums(flux, w)
    out = dict(vel=vel, sfg=sfg, sg=sg, sgg=sgg, W=W, S_wf=S_wf, S_wff=S_wff, n_pix=60)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _statistic_reference(which):
    q = _sums_case()
    ref, bound = S.statistic_ref(which, q["sfg"], q["sg"], q["sgg"], q["W"], q["S_wf"],
                                 q["S_wff"], q["n_pix"])
    assert np.all(np.isfinite(ref)) and np.all(bound <= 1e-9 * np.abs(ref)), "the case is tame"
    return ref, bound


def _orbit(vel, n_exp):
    """Kp, Vsys (both unsorted), phases and v_obs for n_exp exposures."""
    phases = np.linspace(0.31, 0.44, n_exp)
    return dict(Kp=np.array([0.0, 8.0, 20.0, 3.0]), Vsys=np.array([5.0, -12.0, 0.0, 9.5, -3.0]),
                phases=phases, v_obs=np.linspace(-0.5, 0.5, n_exp))


@pytest.mark.parametrize("statistic", ["ccf", "loglike"])
def test_statistic_against_bounded_reference(fa, statistic):
    """Measured on MI355X: values 0.155 (ccf) and 0.122 (loglike) of twice the bound; the maps
    0.033 and 0.029 of theirs."""
    q = _sums_case()
    which = S.CCF if statistic == "ccf" else S.LOGLIKE
    ref, bound = _statistic_reference(which)
    res = fa.CrossCorrelation(q["sfg"], q["sg"], q["sgg"], q["vel"], q["W"], q["S_wf"],
                              q["S_wff"], q["n_pix"])
    st = fa.OrbitStack(q["vel"], **_orbit(q["vel"], 3))
    try:
        got, values = st.stack(res, statistic, want_values=True)
        plain = st.stack(values)
        only = st.stack(res, statistic)
    finally:
        st.release()
    r = _ratio(values, ref, 2 * bound)
    print(f"{statistic}: max |values - ref| / (2 bound) = {r:.3g}; "
          f"max bound / |value| = {float(np.max(bound / np.abs(ref))):.2g}")
    assert values.shape == (3, 3, 7) and np.all(np.abs(values - ref) <= 2 * bound)
    host = res.ccf() if statistic == "ccf" else res.loglike()
    assert np.all(np.abs(host - ref) <= 2 * bound), "the host method, the second yardstick"
    assert np.array_equal(got, plain), "statistic 1/2 is statistic 0 on the returned values"
    assert np.array_equal(got, only)
    j, t, _ = S.brackets(q["vel"], st.dv, st.v_obs, st.Vsys)
    mb = S.stacked_statistic_bound(ref, 2 * bound, j)
    mref = S.stack(ref, j, t)
    r = _ratio(got, mref, mb)
    print(f"{statistic} then stack: max |map - ref| / bound = {r:.3g}")
    assert np.all(np.abs(got - mref) <= mb)
    assert np.array_equal(got, S.stack(values, j, t))


# ------------------------------------------------------------------ 4: NaN containment
def test_nan_reaches_exactly_the_brackets_that_touch_it(fa):
    shape = (3, 3, 7, 3, 65)
    c = _case(*shape)
    j, t, _, _, _ = _reference(*shape)
    # t = 0 at the upper point: (k, e, s) = (0, 0, 0) sits on node 3, so a NaN in node 4 of
    # exposure 0 must reach it (0 * NaN)
    assert (j[0, 0, 0], t[0, 0, 0]) == (3, 0.0)
    st = _stacker(fa, c)
    try:
        clean = st.stack(c["values"])
        for m, e, i in ((1, 2, 3), (0, 0, 0), (2, 1, 6), (1, 0, 4)):
            bad = c["values"].copy()
            bad[m, e, i] = np.nan
            got = st.stack(bad)
            touched = (j[:, e, :] == i) | (j[:, e, :] == i - 1)        # [n_kp][n_vsys]
            assert touched.any() and not touched.all()
            assert np.all(np.isnan(got[m][touched])), (m, e, i)
            got[m][touched] = clean[m][touched]
            assert np.array_equal(got, clean), "every other output is bitwise unchanged"
    finally:
        st.release()


# ------------------------------------------------------------------ 5: keep mode
@functools.lru_cache(maxsize=None)
def _keep_case():
    rng = np.random.default_rng(141)
    lam = np.exp(np.linspace(np.log(1.0), np.log(1.01), 300))
    wl = rng.uniform(1.002, 1.008, 70)
    vel = np.linspace(-30.0, 30.0, 9)
    x = rng.normal(0.0, 0.1, (3, 300))
    flux = 1.0 + rng.normal(0.0, 0.05, (17, 70))          # 17 exposures: the MFMA form
    for a in (lam, wl, vel, x, flux):
        a.setflags(write=False)
    return lam, wl, vel, x, flux


def test_keep_mode(fa):
    from frei_amd import _native as N
    lam, wl, vel, x, flux = _keep_case()
    cc = fa.CrossCorrelator(lam, wl, flux, vel)
    st = fa.OrbitStack(vel, **_orbit(vel, 17))
    try:
        host = cc.correlate(x)                                   # keep off: today's path
        assert host.kept is None
        kept = cc.correlate(x, keep=True, want=())
        assert kept.sfg is None and kept.sg is None and kept.sgg is None
        assert kept.kept.names == ("sfg", "sg", "sgg") and kept.kept.n_atm == 3
        for statistic in ("ccf", "loglike"):
            a, va = st.stack(kept, statistic, want_values=True)
            b, vb = st.stack(host, statistic, want_values=True)
            assert np.array_equal(a, b) and np.array_equal(va, vb), "kept sums are the host's"
            assert np.all(np.isfinite(a)) and a.shape == (3, 4, 5)
        both = cc.correlate(x, keep=True)                        # kept and downloaded
        for k in ("sfg", "sg", "sgg"):
            assert np.array_equal(getattr(both, k), getattr(host, k)), k
        with pytest.raises(RuntimeError, match="stale kept sums"):
            st.stack(kept, "ccf")
        assert np.array_equal(st.stack(both, "loglike"), b)
        # a kept sum missing for the statistic; statistic 0 stacks the kept S_fg
        part = cc.correlate(x, keep=True, want=("sfg",))
        with pytest.raises(RuntimeError, match="a kept sum is missing"):
            st.stack(part, "ccf")
        used = ctypes.c_int(0)
        out = np.empty((3, 4, 5))
        N.check(N.lib().frei_stack_apply(st.handle(), part.kept.handle(), 3, None, None, None,
                                         0, 0.0, None, None, 0.0, N.dptr(out), None, 0,
                                         ctypes.byref(used), None))
        assert np.array_equal(out, st.stack(host.sfg))
        # another atmosphere count, another stacker
        rc = N.lib().frei_stack_apply(st.handle(), part.kept.handle(), 2, None, None, None, 0,
                                      0.0, None, None, 0.0, N.dptr(out), None, 0, None, None)
        assert rc != 0 and b"keeps 3 atmospheres, not n_atm = 2" in N.lib().frei_last_error()
        short = fa.OrbitStack(vel[:-1], **_orbit(vel, 17))
        try:
            rc = N.lib().frei_stack_apply(short.handle(), part.kept.handle(), 3, None, None,
                                          None, 0, 0.0, None, None, 0.0, N.dptr(out), None, 0,
                                          None, None)
            assert rc != 0 and b"n_vel = 9 is not the stacker's 8" in N.lib().frei_last_error()
        finally:
            short.release()
        # keep off again: the buffers are freed, and all outputs null is the error it was
        after = cc.correlate(x, want=("sg",))
        assert after.kept is None and np.array_equal(after.sg, host.sg)
        rc = N.lib().frei_stack_apply(st.handle(), cc.handle(), 3, None, None, None, 0, 0.0,
                                      None, None, 0.0, N.dptr(out), None, 0, None, None)
        assert rc != 0 and b"holds nothing kept" in N.lib().frei_last_error()
        with pytest.raises(RuntimeError, match="all null"):
            cc.correlate(x, want=())
        rc = N.lib().frei_ccf_apply(cc.handle(), None, N.dptr(np.ascontiguousarray(x)), 3, None,
                                    0, None, None, None, 0, None, None, None, None, None)
        assert rc != 0 and b"sfg, sg and sgg are all null" in N.lib().frei_last_error()
    finally:
        st.release()
        cc.release()


# ------------------------------------------------------------------ 6: end to end
@functools.lru_cache(maxsize=None)
def _injection():
    """3 atmospheres with distinct line lists on 2048 native points; 9 exposures of atmosphere
    1's broadened template shifted to (K_p, V_sys) = (100, 5) km/s, plus seeded noise."""
    rng = np.random.default_rng(142)
    n = 2048
    lam = np.exp(np.linspace(np.log(1.0), np.log(1.02), n))
    x = np.ones((3, n))
    for m in range(3):
        for c0, depth in zip(rng.uniform(1.001, 1.019, 60), rng.uniform(0.05, 0.4, 60)):
            x[m] -= depth * np.exp(-0.5 * ((lam - c0) / 2.5e-5) ** 2)
    wl = np.linspace(1.003, 1.017, 700)
    phases = np.linspace(0.32, 0.68, 9)
    v_obs = np.linspace(-1.0, 1.0, 9)
    Kp = np.arange(0.0, 151.0, 10.0)
    Vsys = np.arange(-30.0, 30.1, 2.5)
    vel = np.arange(-180.0, 180.1, 2.0)
    for a in (lam, x, wl, phases, v_obs, Kp, Vsys, vel):
        a.setflags(write=False)
    return dict(lam=lam, x=x, wl=wl, phases=phases, v_obs=v_obs, Kp=Kp, Vsys=Vsys, vel=vel,
                truth=(10, 14), noise=rng.normal(0.0, 2e-3, (9, 700)))


def test_injection_end_to_end(fa):
    """Measured on MI355X: 0.0077 of the bound against the host path; maxima 32515.2 (injected
    atmosphere, at the injected K_p and V_sys) against 13611.7 and 12950.0."""
    q = _injection()
    k0, s0 = q["truth"]
    assert (q["Kp"][k0], q["Vsys"][s0]) == (100.0, 5.0)
    b = fa.Broadening(q["lam"], fa.BroadeningKernel.gaussian(fwhm_kms=5.0))
    st = fa.OrbitStack(q["vel"], q["Kp"], q["Vsys"], phases=q["phases"], v_obs=q["v_obs"])
    cc = None
    try:
        xb = b.apply(q["x"])                               # the broadened templates, on the host
        v_e = (q["Vsys"][s0] + st.dv[k0]) + q["v_obs"]
        flux = np.array([np.interp(q["wl"] / (1.0 + v / R.C_KMS), q["lam"], xb[1])
                         for v in v_e]) + q["noise"]
        cc = fa.CrossCorrelator(q["lam"], q["wl"], flux, q["vel"])
        assert np.all(cc.n_clamped == 0)
        offset = xb.mean(axis=1)
        res = cc.correlate(b.apply(q["x"], keep=True), offset=offset, keep=True)
        got = st.stack(res, "loglike")
        ms, calls = st.timing()
    finally:
        b.release()
        st.release()
        if cc is not None:
            cc.release()
    assert got.shape == (3, 16, 25) and np.all(np.isfinite(got)) and calls == 1 and ms > 0.0
    peak = [np.unravel_index(np.argmax(got[m]), got[m].shape) for m in range(3)]
    assert peak[1] == (k0, s0), peak
    assert got[1].max() > got[0].max() and got[1].max() > got[2].max()
    # against the host path from the downloaded sums
    ref, bound = S.statistic_ref(S.LOGLIKE, res.sfg, res.sg, res.sgg, res.W, res.S_wf,
                                 res.S_wff, res.n_pix)
    assert np.all(bound <= 1e-9 * np.abs(ref))
    host = fa.kp_vsys_map(res.loglike(), q["vel"], q["phases"], q["Kp"], q["Vsys"],
                          v_obs=q["v_obs"])
    j = np.empty((16, 9, 25), dtype=int)
    u = np.clip((q["Vsys"][None, None, :] + st.dv[:, :, None]) + q["v_obs"][None, :, None],
                q["vel"][0], q["vel"][-1])
    j[...] = np.minimum(np.searchsorted(q["vel"], u, "right") - 1, q["vel"].size - 2)
    mb = 2 * S.stacked_statistic_bound(ref, 2 * bound, j)
    r = _ratio(got, host, mb)
    print(f"end to end: device map against kp_vsys_map(loglike()): max |diff| / bound = {r:.3g}; "
          f"peak {got[1].max():.6g} against {got[0].max():.6g} and {got[2].max():.6g}")
    assert np.all(np.abs(got - host) <= mb)


# ------------------------------------------------------------------ 7: keep= passes through
def test_batch_result_and_grid_pass_keep_through(fa):
    """BatchResult.cross_correlate and Grid.cross_correlate with keep=True: the maps from the
    kept sums are bitwise those from the sums the same calls return without keep."""
    lam, _, _ = fa.wavelength_grid(0.5, 10, 500)
    grids, op = [], None
    for T_ref, g in [(2300, 2478.6519476149147), (1400, 1500.0)]:
        pl = fa.Planet.from_hot_jupiter()
        pl.g = g
        gr = fa.Grid(pl, lam=lam, n_layers=30, T_ref=T_ref)
        if op is None:
            op = fa.load_example_opacity(gr)
        gr.load_opacities(opacities=op)
        grids.append(gr)
    lam = np.asarray(grids[0].lam, dtype=float)
    rng = np.random.default_rng(143)
    vel = np.linspace(-4000.0, 4000.0, 9)
    cc = fa.CrossCorrelator(lam, rng.uniform(1.0, 4.0, 300), rng.normal(1.0, 0.1, (3, 300)), vel)
    st = fa.OrbitStack(vel, [0.0, 900.0, 2500.0], [-300.0, 0.0, 450.0, 100.0],
                       phases=[0.2, 0.3, 0.4])
    try:
        with fa.batched_emission_spectra(grids, n_timesteps=1, post=True) as res:
            host = res.cross_correlate(cc, kind="eclipse")
            kept = res.cross_correlate(cc, kind="eclipse", keep=True, want=())
            assert kept.sfg is None and kept.kept.n_atm == 2 and host.kept is None
            a = st.stack(kept, "ccf")
        assert a.shape == (2, 3, 4) and np.array_equal(a, st.stack(host, "ccf"), equal_nan=True)
        spec, _, _, _ = grids[0].emission_spectrum(n_timesteps=1)
        one = grids[0].cross_correlate(cc, spec, kind="eclipse", keep=True)
        assert one.kept.single and one.sfg.shape == (3, 9)
        b = st.stack(one, "ccf")
        plain = fa.CrossCorrelation(one.sfg, one.sg, one.sgg, vel, cc.W, cc.S_wf, cc.S_wff,
                                    cc.n_pix)
        assert b.shape == (3, 4) and np.array_equal(b, st.stack(plain, "ccf"), equal_nan=True)
    finally:
        grids[0]._close_engine()
        st.release()
        cc.release()
