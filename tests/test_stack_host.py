"""Host tests of the orbital stack (frei_amd.stack, K14) that need no GPU: the restatement
(tests/stack_ref.py) against the np.interp form of tests/crosscorr_ref.kp_vsys_map, the host
side of OrbitStack (dv, n_outside, argument checks), the validation of frei_stack_create,
frei_stack_apply and frei_ccf_keep — all of it happens before any device call — and the stale
token of kept sums in pure Python.

Tolerance of the first: the restatement forms f_j + t (f_{j+1} - f_j) with t = (u - v_j) / (v_{j+1}
- v_j), np.interp forms slope (u - v_j) + f_j with slope = (f_{j+1} - f_j) / (v_{j+1} - v_j): the
same u, j and differences, three roundings each on a term of at most |f_j| + |f_{j+1}|, then the
same n_exp additions: |map - ref| <= (n_exp + 4) 2^-53 sum_e (|f_j| + |f_{j+1}|)
(stack_ref.stack_bound).  Measured: 0.11 of the bound at most.
"""
import ctypes

import numpy as np
import pytest

from tests import crosscorr_ref as R
from tests import stack_ref as S


def _grid(n_vel=9):
    """A non-uniform ascending grid of dyadic numbers: sums with dyadic shifts are exact."""
    steps = np.array([0.5, 1.0, 1.5, 2.0, 0.75, 1.25])[np.arange(n_vel - 1) % 6]
    return np.concatenate([[-4.0], -4.0 + np.cumsum(steps)])


def test_restatement_agrees_with_np_interp_form():
    rng = np.random.default_rng(14)
    vel = _grid(9)
    phases = np.array([0.05, 0.31, 0.58, 0.77])
    Kp = np.array([0.0, 2.5, 6.0])
    v_obs = np.array([0.25, -0.5, 0.0, 0.125])
    # with Kp = 0 and v_obs as above: on the first node, an interior node and the last node,
    # below the first and above the last, and in between
    Vsys = np.array([vel[3] - 0.25, vel[-1] + 3.0, vel[0] - 0.25, vel[0] - 7.0, vel[-1] - 0.25,
                     0.3, 1.7])
    values = rng.normal(0.0, 1.0, (2, 4, 9))
    dv = Kp[:, None] * np.sin(2.0 * np.pi * phases)[None, :]
    j, t, outside = S.brackets(vel, dv, v_obs, Vsys)
    assert (j[0, 0, 0], t[0, 0, 0]) == (3, 0.0)                       # interior node
    assert (j[0, 0, 2], t[0, 0, 2], outside[0, 0, 2]) == (0, 0.0, False)   # first node
    assert (j[0, 0, 4], t[0, 0, 4], outside[0, 0, 4]) == (7, 1.0, False)   # last node
    assert (j[0, 0, 3], t[0, 0, 3], outside[0, 0, 3]) == (0, 0.0, True)    # below
    assert (j[0, 0, 1], t[0, 0, 1], outside[0, 0, 1]) == (7, 1.0, True)    # above
    got = S.stack(values, j, t)
    ref = R.kp_vsys_map(values, vel, phases, Kp, Vsys, v_obs)
    bound = S.stack_bound(values, j)
    ratio = float(np.max(np.abs(got - ref) / bound))
    print(f"restatement against np.interp form: max |map - ref| / bound = {ratio:.3f}")
    assert got.shape == (2, 3, 7) and np.all(np.abs(got - ref) <= bound)
    # and the library's own host path
    from frei_amd.crosscorr import kp_vsys_map
    host = kp_vsys_map(values, vel, phases, Kp, Vsys, v_obs=v_obs)
    assert np.all(np.abs(got - host) <= bound)


def test_statistic_restatement_against_host_methods():
    """The restatement's doubles are the host methods' (the same IEEE operations in the same
    order; numpy's log may differ from math.log by an ulp), and within the reference's bound."""
    from frei_amd.crosscorr import CrossCorrelation
    rng = np.random.default_rng(15)
    n_pix, W = 50, 47.5
    sg = rng.normal(0.0, 0.3, (2, 5))
    sgg = rng.uniform(2.0, 3.0, (2, 5))
    sfg = rng.normal(0.0, 0.5, (2, 3, 5))
    S_wf = rng.uniform(45.0, 50.0, 3)
    S_wff = S_wf * S_wf / W + rng.uniform(1.0, 2.0, 3)
    res = CrossCorrelation(sfg, sg, sgg, np.arange(5.0), W, S_wf, S_wff, n_pix)
    for which, host in ((S.CCF, res.ccf()), (S.LOGLIKE, res.loglike())):
        got = S.statistic(which, sfg, sg, sgg, W, S_wf, S_wff, n_pix)
        ref, bound = S.statistic_ref(which, sfg, sg, sgg, W, S_wf, S_wff, n_pix)
        assert np.all(np.abs(got - host) <= 4 * np.spacing(np.abs(host)))
        if which == S.CCF:
            assert np.array_equal(got, host)
        assert np.all(bound <= 1e-9 * np.abs(ref))
        assert np.all(np.abs(got - ref) <= 2 * bound)


def test_orbit_stack_host_side():
    from frei_amd import OrbitStack
    vel = _grid(9)
    phases = np.array([0.05, 0.31, 0.58, 0.77])
    Kp = np.array([0.0, 2.5, 60.0])
    Vsys = np.array([1.0, vel[0] - 0.25, -1.0, vel[-1]])
    v_obs = np.array([0.25, -0.5, 0.0, 0.125])
    st = OrbitStack(vel, Kp, Vsys, phases=phases, v_obs=v_obs)
    assert (st.n_vel, st.n_exp, st.n_kp, st.n_vsys) == (9, 4, 3, 4)
    assert np.array_equal(st.dv, Kp[:, None] * np.sin(2 * np.pi * phases)[None, :])
    _, _, outside = S.brackets(vel, st.dv, v_obs, Vsys)
    assert np.array_equal(st.n_outside, outside.sum(axis=(1, 2)))
    assert st.n_outside[0] < st.n_outside[2] <= 16
    shifts = np.arange(12.0).reshape(3, 4)
    sh = OrbitStack(vel, Kp, Vsys, shifts=shifts)
    assert np.array_equal(sh.dv, shifts) and np.all(sh.v_obs == 0.0)
    assert sh.n_exp == 4 and sh.form_used is None and sh.timing() == (0.0, 0)
    with pytest.raises(ValueError, match="exactly one"):
        OrbitStack(vel, Kp, Vsys)
    with pytest.raises(ValueError, match="exactly one"):
        OrbitStack(vel, Kp, Vsys, phases=phases, shifts=shifts)
    with pytest.raises(ValueError, match="ascending"):
        OrbitStack(vel[::-1], Kp, Vsys, phases=phases)
    with pytest.raises(ValueError, match="at least 2"):
        OrbitStack([1.0], Kp, Vsys, phases=phases)
    with pytest.raises(ValueError, match="shifts"):
        OrbitStack(vel, Kp, Vsys, shifts=np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r"values must be \[n_exp\]\[n_vel\]"):
        st.stack(np.zeros((4, 8)))
    with pytest.raises(ValueError, match="statistic"):
        st.stack(np.zeros((4, 9)), statistic="ccf")
    assert st._handle is None


def test_n_outside_first_row():
    """Kp = 0: u = Vsys + v_obs alone."""
    from frei_amd import OrbitStack
    vel = _grid(9)
    st = OrbitStack(vel, [0.0], [vel[0], vel[-1], vel[0] - 1.0], phases=[0.1, 0.2],
                    v_obs=[0.0, 0.5])
    # exposure 0: one below; exposure 1: vel[-1] + 0.5 above, vel[0] - 0.5 below
    assert list(st.n_outside) == [3]


def _create(n_exp=2, vel=(0.0, 1.0, 3.0), dv=((0.0, 1.0), (2.0, 3.0)), v_obs=(0.0, 0.0),
            vsys=(0.5, -0.5, 0.0), n_vel=None, n_kp=None, n_vsys=None):
    from frei_amd import _native as N
    vel, dv, v_obs, vsys = (N.f64(a) for a in (vel, dv, v_obs, vsys))
    h = ctypes.c_void_p()
    rc = N.lib().frei_stack_create(
        ctypes.byref(h), 0, n_exp, vel.size if n_vel is None else n_vel, N.dptr(vel),
        dv.shape[0] if n_kp is None else n_kp, N.dptr(dv), N.dptr(v_obs),
        vsys.size if n_vsys is None else n_vsys, N.dptr(vsys))
    return rc, h, N.lib().frei_last_error().decode()


@pytest.mark.parametrize("kw, message", [
    (dict(vel=(0.0, 1.0, 1.0)), r"vel\[2\] is not above vel\[1\]"),
    (dict(vel=(0.0, np.inf, 3.0)), r"vel\[1\] is not finite"),
    (dict(vel=(0.0,)), "n_vel must be >= 2"),
    (dict(dv=((0.0, 1.0), (np.nan, 3.0))), r"dv\[1\]\[0\] is not finite"),
    (dict(v_obs=(0.0, -np.inf)), r"v_obs\[1\] is not finite"),
    (dict(vsys=(0.5, -0.5, np.nan)), r"vsys\[2\] is not finite"),
    (dict(n_exp=0), "n_exp must be >= 1"),
    (dict(n_kp=0), "n_kp must be >= 1"),
    (dict(n_vsys=0), "n_vsys must be >= 1"),
])
def test_create_rejects_bad_arguments(kw, message):
    import re
    rc, h, err = _create(**kw)
    assert rc != 0 and not h.value
    assert re.search(message, err), err


def test_create_touches_no_device_and_apply_validates_first():
    """A valid stacker exists without a GPU (its arrays are uploaded by the first apply), so
    every argument error of frei_stack_apply is reached here."""
    from frei_amd import _native as N
    lib = N.lib()
    rc, h, err = _create()                      # unsorted vsys, unsorted dv rows: accepted
    assert rc == 0 and h.value, err
    vals = np.zeros((1, 2, 3))
    row = np.zeros((1, 3))
    out = np.zeros((1, 2, 3))
    two = np.ones(2)

    def apply(handle=h, kept=None, n_atm=1, sfg=vals, sg=None, sgg=None, statistic=0, W=0.0,
              S_wf=None, S_wff=None, n_eff=0.0, map_=out, form=0):
        rc = lib.frei_stack_apply(handle, kept, n_atm, N.dptr(sfg), N.dptr(sg), N.dptr(sgg),
                                  statistic, W, N.dptr(S_wf), N.dptr(S_wff), n_eff,
                                  N.dptr(map_), None, form, None, None)
        return rc, lib.frei_last_error().decode()

    for kw, message in [
            (dict(handle=None), "null handle"),
            (dict(map_=None), "map is null"),
            (dict(n_atm=0), "n_atm must be >= 1"),
            (dict(statistic=3), "statistic must be 0"),
            (dict(statistic=-1), "statistic must be 0"),
            (dict(form=3), "form must be 0"),
            (dict(sfg=None), "neither host sums nor a kept source"),
            (dict(sfg=None, sg=row, sgg=row), "lack sfg"),
            (dict(statistic=1, W=3.0, S_wf=two, S_wff=two), "needs sfg, sg and sgg"),
            (dict(statistic=2, sg=row, sgg=row, W=3.0, S_wf=two), "needs W, S_wf and S_wff"),
            (dict(statistic=2, sg=row, sgg=row, W=0.0, S_wf=two, S_wff=two),
             "needs W, S_wf and S_wff")]:
        rc, err = apply(**kw)
        assert rc != 0 and message in err, (kw, err)
    assert lib.frei_stack_destroy(h) == 0
    assert lib.frei_stack_destroy(None) == 0
    # form 1 beyond the LDS copy of the velocities
    from frei_amd.stack import LDS_VELOCITIES
    n = LDS_VELOCITIES + 1
    rc, h, err = _create(vel=np.arange(float(n)))
    assert rc == 0, err
    big = np.zeros((1, 2, n))
    rc = lib.frei_stack_apply(h, None, 1, N.dptr(big), None, None, 0, 0.0, None, None, 0.0,
                              N.dptr(out), None, 1, None, None)
    assert rc != 0 and f"at most {LDS_VELOCITIES} velocities" in lib.frei_last_error().decode()
    assert lib.frei_stack_destroy(h) == 0


def test_ccf_keep_rejects_a_null_handle():
    from frei_amd import _native as N
    assert N.lib().frei_ccf_keep(None, 1) != 0
    assert b"frei_ccf_keep: null handle" in N.lib().frei_last_error()
    # a null correlator as the kept source is no source
    rc, h, _ = _create()
    out, vals = np.zeros((1, 2, 3)), None
    assert N.lib().frei_stack_apply(h, None, 1, None, None, None, 0, 0.0, None, None, 0.0,
                                    N.dptr(out), vals, 0, None, None) != 0
    assert b"neither host sums nor a kept source" in N.lib().frei_last_error()
    assert N.lib().frei_stack_destroy(h) == 0


def test_stale_kept_sums_raise():
    """The token of correlate(keep=True) in pure Python: (owner, serial), stale at the owner's
    next correlate or release."""
    from frei_amd.crosscorr import CrossCorrelation, CrossCorrelator, KeptSums
    from frei_amd import OrbitStack
    lam = np.exp(np.linspace(0.0, 0.1, 20))
    vel = np.array([-10.0, 0.0, 10.0])
    cc = CrossCorrelator(lam, [1.02, 1.05], [[1.0, 2.0], [2.0, 1.0]], vel)
    assert cc._serial == 0
    cc._handle = ctypes.c_void_p(1)              # a stand-in: no library call is made with it
    try:
        cc._serial += 1                          # what correlate does before its apply
        tok = KeptSums(cc, cc._serial, 2, False, ("sfg", "sg", "sgg"))
        assert tok.handle() is cc._handle and tok.names == ("sfg", "sg", "sgg")
        cc._serial += 1                          # the next correlate
        with pytest.raises(RuntimeError, match="stale kept sums"):
            tok.handle()
        res = CrossCorrelation(None, None, None, vel, cc.W, cc.S_wf, cc.S_wff, cc.n_pix,
                               kept=tok)
        st = OrbitStack(vel, [0.0, 1.0], [0.0], phases=[0.1, 0.2])
        with pytest.raises(RuntimeError, match="stale kept sums"):
            st.stack(res, "loglike")
        assert st._handle is None
        fresh = KeptSums(cc, cc._serial, 2, False, ("sfg",))
        assert fresh.handle() is cc._handle
    finally:
        cc._handle = None                        # nothing to destroy
    with pytest.raises(RuntimeError, match="stale kept sums"):
        fresh.handle()                           # released: no handle
    cc.release()
    assert cc._serial == 3
    # a correlation without kept sums and without host sums cannot be stacked
    bare = CrossCorrelation(None, None, None, vel, cc.W, cc.S_wf, cc.S_wff, cc.n_pix)
    assert bare.kept is None
    with pytest.raises(ValueError, match="all three sums"):
        OrbitStack(vel, [0.0], [0.0], phases=[0.1, 0.2]).stack(bare, "ccf")


def test_exports():
    import frei_amd
    from frei_amd import stack
    assert frei_amd.OrbitStack is stack.OrbitStack
    assert stack.FORMS == (1, 2) and stack.STATISTICS == {"values": 0, "ccf": 1, "loglike": 2}
    assert stack.ATM_TILE >= 1 and stack.LDS_VELOCITIES >= 2
    from frei_amd import build as B
    src = open(B.HERE + "/csrc/frei_stack.hip").read()
    assert f"kAT = {stack.ATM_TILE};" in src
    hdr = open(B.ROOT + "/include/frei_hip.h").read()
    assert f"#define FREI_STACK_LDS_VEL {stack.LDS_VELOCITIES}\n" in hdr
