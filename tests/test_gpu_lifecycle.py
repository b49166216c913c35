"""Ownership of device buffers, pinned buffers, streams and events (frei_live_resources).

Every handle type owns its resources through the counted types of csrc/frei_host.h, so the four
process-wide figures are exact: they return to their earlier values when a handle is destroyed,
a call's temporaries (DeviceCall) never outlive the call, and a failing call leaves nothing
behind.  The figures are the library's own, not the runtime's free memory, which other processes
on the device move.

What each handle documents as kept, and the tests below assert count by count:
  frei_sspec   the plan and the result of the last bin (2 device buffers, grow-only)
  frei_xsec    the scratch result (1), the plan slots (6 after a groupies bin, 12 after an exact
               one), the exact mode's half-widths (1) and one pinned staging buffer
  frei_klib    the result of frei_klib_mix (1)
  frei_obs     nothing
  frei_ccf     the sums asked for in keep mode (up to 3), nothing otherwise
  frei_brd     the kept rows (1) after apply(keep), nothing otherwise
  frei_stack   its stream and four arrays from the first apply on
  frei_itp     its stream and the node library from set_nodes on, the result buffer (1, grow-only)
  frei_phs     the plan (2) and the result buffer (1, grow-only) from the first apply on
A context's buffers are compared call against call (a repeated call adds nothing) and against
the baseline after destroy.

A batched context takes no rank exchange, so the "fully dressed" context is two: a
single-atmosphere one with the P2P communicator, timing, the lazy contraction and the trailing
update, and a batched one with chemistry tables, per-atmosphere F_TOA and keep_dtaus.

Shapes are the smallest the constructors take or the neighbouring files use; the dressed
single-atmosphere context takes tests/test_gpu_lazy_k3.py's and tests/test_gpu_tail.py's
arrangements, whose sweep forms need their sizes."""
import contextlib
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import frei_amd as fa
from frei_amd import _native as N
from frei_amd import constants as K
from frei_amd.binning import KLibrary
from frei_amd.broaden import BroadenedSpectra
from frei_amd.kdist import gauss_g
from frei_amd.lines import LineList
from oracle import frei_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = np.linspace(1.0, 2.0, 256)
NL = 6


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@contextlib.contextmanager
def adds(device=0, pinned=0, streams=0, events=0):
    """The block changes the live figures by exactly this much."""
    before = N.live_resources()
    yield
    want = tuple(b + d for b, d in zip(before, (device, pinned, streams, events)))
    assert N.live_resources() == want, (before, N.live_resources(), want)


def spectra(n_atm, n_lam=LAM.size, seed=0):
    return np.random.default_rng(40 + seed).uniform(1.0, 2.0, (n_atm, n_lam))


# ------------------------------------------------------------------------------ small makers
def make_batch(n_atm, n_lam=128, n_layers=NL):
    lam = np.logspace(np.log10(0.5), 1.0, n_lam)
    p = np.logspace(np.log10(200.0), -6, n_layers)
    tabs = {"1H2-16O": fa.OpacityTable(np.ones((n_layers, 2, n_lam)), p, [1000.0, 2000.0])}
    return fa.BatchEngine(lam, p, tabs, g=np.linspace(900.0, 5200.0, n_atm))


def ramp(n_atm, n_layers=NL):
    return np.array([np.linspace(1900.0 - 100.0 * m, 1100.0, n_layers) for m in range(n_atm)])


def make_xsec():
    rng = np.random.default_rng(3)
    vals = 10 ** rng.uniform(-24, -20, (2, 3, 400))
    return fa.CrossSection(vals, [500.0, 900.0], [0.1, 1.0, 10.0], np.linspace(1.0, 2.0, 400))


def bins(n):
    edges = np.linspace(1.05, 1.95, n + 1)
    return edges, (edges[:-1] + edges[1:]) / 2


def make_lines():
    rng = np.random.default_rng(5)
    n = 40
    ll = LineList(nu0=rng.uniform(5100.0, 9900.0, n), S=10.0 ** rng.uniform(-25.0, -19.0, n),
                  E_low=rng.uniform(0.0, 3000.0, n), gamma=rng.uniform(0.03, 0.1, n),
                  n_exp=rng.uniform(0.4, 0.8, n), mass=28.0,
                  partition=(np.array([200.0, 3000.0]), np.array([50.0, 900.0])))
    return ll.cross_section([500.0, 900.0], [0.1, 1.0], np.linspace(1.0, 2.0, 400), cutoff=25.0)


def make_klib(n_g=4):
    rng = np.random.default_rng(11)
    T, p, wl = np.array([1000.0, 1500.0]), np.logspace(1, -4, 4), np.linspace(1.0, 3.0, 4)
    Ks = np.sort(rng.lognormal(0.0, 2.0, (2, 4, 2, 3, n_g)), axis=-1)
    g, w = gauss_g(n_g)
    return KLibrary({f"s{k}": t for k, t in enumerate(Ks)}, wl, g, w, T, p), Ks


def make_sspec():
    wl = np.linspace(0.9, 2.1, 2000)
    return fa.StellarSpectra(wl, np.random.default_rng(8).uniform(1.0, 2.0, (2, wl.size)))


def make_obs():
    return fa.Instrument.top_hat(LAM, [1.1, 1.5], [1.3, 1.9])


VEL = np.linspace(-60.0, 60.0, 9)


def make_ccf(n_exp=3):
    rng = np.random.default_rng(21)
    return fa.CrossCorrelator(LAM, rng.uniform(1.05, 1.95, 300), rng.normal(1.0, 0.1, (n_exp, 300)),
                              VEL)


def make_brd():
    return fa.Broadening(LAM, fa.BroadeningKernel.gaussian(fwhm_kms=3000.0))


def make_stack(n_exp=3):
    return fa.OrbitStack(VEL, [0.0, 20.0], [-10.0, 0.0, 10.0],
                         phases=np.linspace(-0.03, 0.03, n_exp))


def make_itp():
    return fa.ModelGrid([np.array([0.0, 1.0, 2.0])], LAM, spectra=spectra(3, seed=5))


def phase_plan(n_atm, n_cell=5, n_phase=3):
    rng = np.random.default_rng(77)
    mu = rng.uniform(-1.0, 1.0, (n_phase, n_cell))
    mu[0, 0] = 1.0
    coef = np.where(mu > 0, rng.uniform(0.0, 2.0, mu.shape), np.nan)
    return (np.arange(n_cell) % n_atm).astype(np.int32), mu, coef


def columns(n_atm, n_lam, n_layers=NL):
    rng = np.random.default_rng(n_lam)
    dt = 10 ** rng.uniform(-8, 3, (n_atm, n_layers, n_lam))
    dt[:, 0] = np.nan
    T = ramp(n_atm, n_layers)
    T[:, 0] = np.nan
    return dt, T


# ------------------------------------------------------------------------------ 2. balance
def test_single_context_balance():
    base = N.live_resources()
    lam = np.logspace(np.log10(0.5), 1.0, 128)
    p = np.logspace(np.log10(200.0), -6, NL)
    eng = fa.Engine(lam, p, {"1H2-16O": fa.OpacityTable(np.ones((NL, 2, 128)), p,
                                                         [1000.0, 2000.0])})
    try:
        assert N.live_resources()[2] == base[2] + 1
        first = eng.run(ramp(1)[0], n_timesteps=2)
        with adds():                                   # the same call again: nothing new
            again = eng.run(ramp(1)[0], n_timesteps=2)
        eng.run(ramp(1)[0], n_timesteps=9)             # a longer history
        assert same_bits(first["spectrum"], again["spectrum"])
    finally:
        eng.close()
    assert N.live_resources() == base


def test_batched_context_balance():
    base = N.live_resources()
    eng = make_batch(3)
    try:
        first = eng.run(ramp(3), n_timesteps=2)
        with adds():
            again = eng.run(ramp(3), n_timesteps=2)
        assert same_bits(first["spectra"], again["spectra"])
        eng.run(ramp(3), n_timesteps=3, want_hist=True, keep_dtaus=True)
        with adds():                                   # the same again: nothing new
            eng.run(ramp(3), n_timesteps=3, want_hist=True, keep_dtaus=True)
        with adds():                                   # a longer history: grown, not added
            eng.run(ramp(3), n_timesteps=7, want_hist=True, keep_dtaus=True)
        with adds():
            eng.get_dtaus(1)
    finally:
        eng.close()
    assert N.live_resources() == base


@pytest.mark.parametrize("kind", ["uploaded", "synthetic", "lines"])
def test_xsec_balance(kind):
    base = N.live_resources()
    make = dict(uploaded=make_xsec, lines=make_lines,
                synthetic=lambda: fa.CrossSection.synthetic(
                    [500.0, 900.0], [0.1, 1.0, 10.0], np.linspace(1.0, 2.0, 400), seed=4))[kind]
    with adds(device=1, streams=1):                    # the values; every temporary is gone
        xs = make()
        xs.handle()
    try:
        e8, l8 = bins(8)
        e16, l16 = bins(16)
        with adds(device=7, pinned=1):                 # scratch, 6 plan slots, the staging buffer
            xs.bin(e8, l8, [600.0], [1.0])
        with adds():                                   # more bins and nodes: grown in place
            xs.bin(e16, l16, [600.0, 800.0], [0.5, 1.0])
        with adds(device=7):                           # exact: 6 more plan slots, the half-widths
            xs.bin(e16, l16, [600.0, 800.0], [0.5, 1.0], groupies=False)
        with adds():
            xs.kdist(e16, gauss_g(4)[0], [600.0, 800.0], [0.5, 1.0])
        with adds():
            xs.kdist(e16, gauss_g(8)[0], [600.0, 800.0], [0.5, 1.0, 5.0])
    finally:
        xs.release()
    assert N.live_resources() == base


def test_klib_balance():
    base = N.live_resources()
    lib, _ = make_klib()
    rng = np.random.default_rng(2)
    try:
        with adds(device=3, streams=1):                # the tables and the two weight arrays
            lib.handle()
        with adds(device=1):                           # the result buffer
            lib.mix(rng.uniform(1e-3, 1e-1, (1, 2, 2, 4)))
        with adds():                                   # more compositions: grown
            lib.mix(rng.uniform(1e-3, 1e-1, (5, 2, 2, 4)))
    finally:
        lib.release()
    assert N.live_resources() == base


def test_sspec_balance():
    base = N.live_resources()
    s = make_sspec()
    try:
        with adds(device=2, streams=1):
            s.handle()
        with adds(device=2):                           # the plan and the result
            s.bin(np.linspace(1.0, 2.0, 9))
        with adds():
            s.bin(np.linspace(1.0, 2.0, 65))
    finally:
        s.release()
    assert N.live_resources() == base


def test_obs_balance():
    base = N.live_resources()
    o = make_obs()
    try:
        with adds(device=2, streams=1):
            o.handle()
        with adds():
            o.apply(spectra(1))
        with adds():
            o.apply(spectra(3), den=spectra(2, seed=1), select=[0, 1, 0], data=[1.0, 2.0],
                    sigma=[0.1, 0.2])
    finally:
        o.release()
    assert N.live_resources() == base


def test_ccf_balance():
    base = N.live_resources()
    c = make_ccf()
    try:
        with adds(device=5, streams=1):
            c.handle()
        with adds(device=3):                           # keep mode: the three sums stay
            c.correlate(spectra(2), keep=True)
        with adds():                                   # more atmospheres: replaced, not added
            c.correlate(spectra(3), keep=True, want=())
        with adds(device=-3):                          # keep off drops them
            c.correlate(spectra(3))
        with adds(device=1):
            c.correlate(spectra(1), keep=True, want=("sfg",), scale=2.0)
    finally:
        c.release()
    assert N.live_resources() == base


def test_brd_balance():
    base = N.live_resources()
    b = make_brd()
    try:
        with adds(device=6, streams=1):
            b.handle()
        with adds():
            b.apply(spectra(1))
        with adds(device=1):
            b.apply(spectra(2), keep=True)
        with adds():                                   # more atmospheres: replaced
            b.apply(spectra(5), keep=True)
        with adds(device=-1):
            b.apply(spectra(5))
    finally:
        b.release()
    assert N.live_resources() == base


def test_stack_balance():
    base = N.live_resources()
    s, c = make_stack(), make_ccf()
    try:
        with adds():                                   # no device before the first apply
            s.handle()
        with adds(device=4, streams=1):
            s.stack(spectra(1, 3 * VEL.size).reshape(3, VEL.size))
        with adds():
            s.stack(spectra(4, 3 * VEL.size).reshape(4, 3, VEL.size))
        kept = c.correlate(spectra(2), keep=True)
        with adds():
            s.stack(kept, "loglike")
    finally:
        s.release()
        c.release()
    assert N.live_resources() == base


def test_itp_balance():
    base = N.live_resources()
    g = make_itp()
    try:
        with adds(device=1, streams=1):                # the node library
            g.handle()
        with adds(device=1):                           # the result buffer
            g.interpolate(np.array([[0.5]]))
        with adds():
            g.interpolate(np.array([[0.1], [1.5], [1.9], [0.7]]), keep=True)
        with adds():
            g.set_nodes(spectra(3, seed=6))
            g.interpolate(np.array([[0.5]]))
    finally:
        g.release()
    assert N.live_resources() == base


def test_phs_balance():
    base = N.live_resources()
    select, mu, coef = phase_plan(2)
    pc = fa.PhaseCurve(mu=mu, coef=coef, select=select)
    small, large = make_batch(2, 128), make_batch(2, 256)
    try:
        with adds():                                   # no device before the first apply
            pc.handle()
        dt, T = columns(2, 128)
        with adds(device=3):                           # the plan (2) and the result buffer
            pc.integrate(small, T, dtaus=dt)
        dt, T = columns(2, 256)
        with adds():                                   # a wider axis: grown
            pc.integrate(large, T, dtaus=dt, keep=True)
    finally:
        pc.release()
        small.close()
        large.close()
    assert N.live_resources() == base


# ------------------------------------------------------------------------------ 3. dressed
def lazy_case(nL=40, n_lam=8192):
    """tests/test_gpu_lazy_k3.py's case with species 1 as a plain table: two setters."""
    rng = np.random.default_rng(5)
    lam, _, _ = O.wavelength_grid(0.5, 10, n_lam)
    p = O.pressure_grid(nL, -6, np.log10(200))
    T0 = O.temperature_grid(p, 1800.0, 0.1, 0.1)
    Tn = np.linspace(0.8 * T0.min(), 1.2 * T0.max(), 16)
    names = ["1H2-16O", "12C-16O", "12C-1H4"]
    fp, fT = (p / 1.0) ** 0.1, (Tn / 1000.0) ** 0.5
    tabs = {n: fa.SeparableTable(10 ** rng.uniform(-3, 1.5, lam.size), fp, fT, p, Tn)
            for n in names}
    base = 10 ** rng.uniform(-3, 1.5, lam.size)
    tabs["12C-16O"] = fa.OpacityTable(fp[:, None, None] * fT[None, :, None] * base, p, Tn)
    mmr = O.mock_mmr(names, K.M_BAR_HOT_JUPITER)[:, None] * np.ones(nL)
    return lam, p, T0, tabs, mmr


@pytest.mark.parametrize("rebuild", [False, True])
def test_dressed_single_context(rebuild):
    """Two setters, a one-rank P2P communicator, the lazy contraction, an option change that
    rebuilds the metadata (rebuild: twice more, back and forth), timing for one iteration (the
    event pools) and the trailing update."""
    from frei_amd.distributed import p2p_comm
    from frei_amd.rendezvous import Rendezvous
    base = N.live_resources()
    lam, p, T0, tabs, mmr = lazy_case()
    eng = fa.Engine(lam, p, tabs, mmr=mmr, comm=p2p_comm(Rendezvous(1, 0)))
    try:
        for k, v in (("group_q", 1), ("shared", 0), ("pipe", 0), ("lam2", 1)):
            eng.set_option(k, v)
        path = eng.path()
        print("lazy path", path)
        assert path["lazy_k3"] and path["contracted"], path
        eng.run(T0, n_timesteps=3, n_zero_crossings=10 ** 6, convergence_dT=-1.0)
        if rebuild:
            eng.set_option("lazy_k3", 0)
            eng.run(T0, n_timesteps=2, n_zero_crossings=10 ** 6, convergence_dT=-1.0)
            eng.set_option("lazy_k3", 1)
            eng.run(T0, n_timesteps=2, n_zero_crossings=10 ** 6, convergence_dT=-1.0)
        eng.state_init(T0)
        eng.timing(True)
        with adds(events=4):                           # two per sweep, pooled
            eng.iterate(1)
            eng.synchronize()
        eng.timing_read()
        eng.timing(True)                               # enabling again hands the pool back
        with adds():
            eng.iterate(1)
            eng.synchronize()
        eng.timing_read()
        eng.timing(False)
        # back to the default sweep choice, then tests/test_gpu_tail.py's arrangement
        for k, v in (("group_q", 0), ("shared", -1), ("lam2", -1), ("pipe", 4), ("tail", 1)):
            eng.set_option(k, v)
        n0 = eng.tail_count()
        eng.run(T0, n_timesteps=3, n_zero_crossings=10 ** 6, convergence_dT=-1.0)
        eng.state_init(T0)
        eng.iterate(3)
        eng.synchronize()
        print("tail path", eng.path(), "launches", eng.tail_count() - n0)
        assert eng.tail_count() > n0
    finally:
        eng.close()
    assert N.live_resources() == base


def test_dressed_batched_context():
    """Two setters, chemistry batch tables, per-atmosphere F_TOA, keep_dtaus; then the chemistry
    is taken off again, which rebuilds the metadata for the contracted path."""
    base = N.live_resources()
    rng = np.random.default_rng(30)
    n_lam, n_atm = 256, 3
    lam, _, _ = O.wavelength_grid(0.5, 10, n_lam)
    p = O.pressure_grid(8, -6, np.log10(200))
    Tn = np.linspace(400.0, 5000.0, 6)
    names = ["1H2-16O", "12C-16O"]
    fp, fT = (p / 1.0) ** 0.1, (Tn / 1000.0) ** 0.5
    b0, b1 = 10 ** rng.uniform(0, 3, (2, n_lam))
    tabs = {names[0]: fa.SeparableTable(b0, fp, fT, p, Tn, lo=10.0, hi=1e3),
            names[1]: fa.OpacityTable(np.clip(fp[:, None, None] * fT[None, :, None] * b1, 10.0,
                                              1e3), p, Tn)}
    cT, cp = np.linspace(300.0, 4000.0, 5), np.logspace(-7, 3, 4)
    x = np.tanh((cT[:, None] - 1500.0) / 400.0) + 0.05 * np.log10(cp)[None, :]
    chem = [fa.ChemistryTable({n: 1e-3 * 10 ** (0.5 * s * x + d) for s, n in enumerate(names)},
                              cT, cp) for d in (0.0, 0.3)]
    ftoa = O.F_TOA(lam)[None, :] * np.array([1.0, 0.5, 2.0])[:, None]
    T0 = np.array([O.temperature_grid(p, t, 0.1, 0.1) for t in (1500.0, 1800.0, 2100.0)])
    eng = fa.BatchEngine(lam, p, tabs, g=np.linspace(900.0, 3000.0, n_atm), mmr=chem[0],
                         F_toa=ftoa)
    try:
        eng.set_chemistry(chem, atm_tab=[0, 1, 0])
        eng.run(T0, n_timesteps=2)
        eng.run(T0, n_timesteps=4, want_hist=True, keep_dtaus=True)
        eng.set_chemistry(None)
        eng.run(T0, n_timesteps=2, keep_dtaus=True)
    finally:
        eng.close()
    assert N.live_resources() == base


# ------------------------------------------------------------------------------ 4. failing calls
def test_kmix_batch_nan_failure_leaves_nothing():
    """The failure of tests/test_gpu_kbatch.py: the mixed table holds a NaN, found after the
    kernels ran."""
    from tests.test_gpu_kbatch import P6, T3, USED, WL5, raw_context, small_case
    base = N.live_resources()
    c = small_case(4)
    lib, klib = N.lib(), c["lib"]
    g4, w4 = gauss_g(4)
    nan_lib = KLibrary({f"s{k}": t.copy() for k, t in enumerate(c["Ks"])}, WL5, g4, w4, T3, P6)
    nan_lib.sources["s1"][USED[1], 0, 2, 1] = -1.0
    x = klib.tables(c["x"]).x
    zero = x.copy()
    zero[:, 0] = 0.0
    _, ctx = raw_context(c["lam"], c["qw"], c["p"], 5)
    tab0, tab1 = np.empty((6, 3, c["lam"].size)), np.empty((6, 3, c["lam"].size))
    try:
        h, hn = klib.handle(), nan_lib.handle()
        N.check(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(x), 0))
        N.check(lib.frei_get_table_batch(ctx, 3, N.dptr(tab0)))
        with adds():
            assert lib.frei_set_table_kmix_batch(ctx, hn, N.dptr(zero), 0) != 0
            assert "holds a NaN" in lib.frei_last_error().decode()
        N.check(lib.frei_set_table_kmix_batch(ctx, h, N.dptr(x), 0))
        N.check(lib.frei_get_table_batch(ctx, 3, N.dptr(tab1)))
        assert same_bits(tab0, tab1) and np.all(np.isfinite(tab0[USED]))
    finally:
        lib.frei_ctx_destroy(ctx)
        nan_lib.release()
        klib.release()
    assert N.live_resources() == base


def test_obs_apply_brd_mismatch_leaves_nothing():
    base = N.live_resources()
    o, b = make_obs(), make_brd()
    try:
        kept = b.apply(spectra(3), keep=True)
        good = o.apply(kept)
        with adds():
            with pytest.raises(RuntimeError, match="keeps 3 atmospheres, not n_atm = 2"):
                o.apply(BroadenedSpectra(b, kept.serial, 2, False))
        assert same_bits(o.apply(kept), good)
    finally:
        o.release()
        b.release()
    assert N.live_resources() == base


def test_brd_apply_beyond_the_grid_leaves_nothing():
    """The call fails after the old kept rows were dropped: with rows kept, the failing call
    lowers the device figure by that one buffer; with none kept it changes nothing."""
    base = N.live_resources()
    b = make_brd()
    lib = N.lib()
    x, out = spectra(2), np.empty((2, LAM.size))
    used, ms = ctypes.c_int(0), ctypes.c_double(0.0)
    too_many = 8 * 65535 + 1                           # one lane tile beyond the grid's 65535

    def failing():
        rc = lib.frei_brd_apply(b.handle(), None, N.dptr(x), too_many, 1, N.dptr(out), 0,
                                ctypes.byref(used), ctypes.byref(ms))
        assert rc != 0 and "exceeds the launch grid" in lib.frei_last_error().decode()
    try:
        good = b.apply(x)
        with adds():
            failing()
        assert same_bits(b.apply(x), good)
        kept = b.apply(x, keep=True)
        with adds(device=-1):
            failing()
        o = make_obs()
        try:
            with pytest.raises(RuntimeError, match="holds nothing kept"):
                o.apply(kept)
        finally:
            o.release()
        assert same_bits(b.apply(x), good)
    finally:
        b.release()
    assert N.live_resources() == base


# ------------------------------------------------------------------------------ 5. filled
def fill_cases():
    """One small case per post-processing handle -> {name: sha256 of the result's bytes}."""
    out = {}

    def put(name, *arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        out[name] = h.hexdigest()

    s = make_sspec()
    put("sspec", s.bin(np.linspace(1.0, 2.0, 33)))
    s.release()
    xs = make_xsec()
    e, l = bins(16)
    put("xsec groupies", xs.bin(e, l, [600.0, 800.0], [0.5, 1.0]))
    put("xsec exact", xs.bin(e, l, [600.0, 800.0], [0.5, 1.0], groupies=False))
    put("kdist", *xs.kdist(e, gauss_g(4)[0], [600.0, 800.0], [0.5, 1.0]))
    xs.release()
    o = make_obs()
    put("obs", *o.apply(spectra(3), den=spectra(2, seed=1), select=[0, 1, 0], data=[1.0, 2.0],
                        sigma=[0.1, 0.2]))
    o.release()
    c = make_ccf()
    for form in (1, 2):
        r = c.correlate(spectra(3), form=form, scale=[1.0, 2.0, 0.5])
        put(f"ccf form {form}", r.sfg, r.sg, r.sgg)
    b = make_brd()
    for form in (1, 2):
        put(f"brd form {form}", b.apply(spectra(3), form=form))
    st = make_stack()
    kept = c.correlate(spectra(2), keep=True)
    put("stack", *st.stack(kept, "loglike", want_values=True))
    st.release()
    c.release()
    b.release()
    g = make_itp()
    put("itp", g.interpolate(np.array([[0.1], [1.5], [1.9], [0.7]])))
    g.release()
    select, mu, coef = phase_plan(2)
    pc, eng = fa.PhaseCurve(mu=mu, coef=coef, select=select), make_batch(2, 128)
    dt, T = columns(2, 128)
    put("phs", pc.integrate(eng, T, dtaus=dt))
    pc.release()
    eng.close()
    return out


def child_main():
    print("cases " + json.dumps(fill_cases()))


def test_filled_allocations_change_no_result(monkeypatch):
    """A process whose every new device buffer starts as 0xFF bytes computes the same bits: no
    handle reads memory the library never wrote."""
    monkeypatch.delenv("FREI_ALLOC_FILL", raising=False)
    want = fill_cases()
    r = subprocess.run([sys.executable, "-c",
                        "from tests.test_gpu_lifecycle import child_main; child_main()"],
                       cwd=ROOT, env=dict(os.environ, FREI_ALLOC_FILL="255"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.split("cases ")[-1])
    assert set(got) == set(want)
    differing = sorted(k for k in want if got[k] != want[k])
    assert not differing, differing
