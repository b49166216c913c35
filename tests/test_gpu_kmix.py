"""K19 on the GPU: frei_klib_mix against the NumPy restatement (tests/kmix_ref.py) to the rounding
bound of the definition, the two kernel forms and the other invariances bit for bit, K18's
k-distribution written into a slot, the device route into an Engine, KGrid(overlap="random") end
to end on the two-species forest, and the C-level argument errors (the properties of the
definition itself and the physics: tests/test_kmix_host.py).

The bound: per fold every value may differ from the restatement's by the relative
(n_g^2 + 4) 2^-52 max(1, max |ln v|) — one rounding per term of the interval's sum plus a log and
an exp on each side — compounded over the folds, with max |ln v| the item's own.
"""
import ctypes
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import frei_amd as fa
from frei_amd import _native as N
from frei_amd import constants as K
from frei_amd.binning import CrossSection, KLibrary
from frei_amd.engine import ABSORB, EMIT, Engine
from frei_amd.kdist import KGrid, gauss_g
from tests import kdist_ref as R
from tests import kmix_ref as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANET = dict(T_star=5800.0, a_rstar=K.A_RSTAR_HOT_JUPITER, g=K.G_JUPITER,
              m_bar=K.M_BAR_HOT_JUPITER)
WL3 = np.array([1.0, 1.5, 2.5, 3.0])
T2, P2 = np.array([1000.0, 2000.0]), np.array([1e-3, 1.0])


def same_bits(a, b):
    return (np.array_equal(a, b, equal_nan=True) and
            np.array_equal(np.signbit(a) & ~np.isnan(a), np.signbit(b) & ~np.isnan(b)))


def quad(n_g):
    return gauss_g(n_g) if n_g > 1 else (np.array([0.5]), np.array([1.0]))


def make_tables(n_src, n_g, n_bins=3, seed=0, special=False):
    """K[n_src][2][2][n_bins][n_g]: slot 0 ascending in g as a k-table is, the others in any
    order.  ``special`` (6 bins): ties in bin 0, a zero pair in bin 1, a -0 pair in bin 2, a NaN
    in bin 3, a negative value in bin 4, each at one node; bin 5 is ordinary."""
    rng = np.random.default_rng(1000 * n_g + 10 * n_src + seed)
    Ks = rng.lognormal(0.0, 3.0, (n_src, 2, 2, n_bins, n_g))
    Ks[0] = np.sort(Ks[0], axis=-1)
    if special:
        assert n_bins == 6
        Ks[:, :, :, 0, : (n_g + 1) // 2] = Ks[:, :, :, 0, :1]      # ties in a and in b
        Ks[:, 0, 0, 1, 0] = 0.0                                    # a[0] + b[0] = 0 in every fold
        Ks[:, 0, 1, 2, 0] = -0.0
        Ks[min(n_src, 2) - 1, 1, 0, 3, n_g // 2] = np.nan
        Ks[0, 1, 1, 4, 0] = -1e9                                   # every pair of a[0] negative
    return Ks


def library(Ks, n_g):
    g, w = quad(n_g)
    bins = np.linspace(1.0, 3.0, Ks.shape[3] + 1)
    return KLibrary({f"s{k}": t for k, t in enumerate(Ks)}, bins, g, w, T2, P2)


def composition(n_src, seed=0, n_comp=None):
    rng = np.random.default_rng(50 + n_src + seed)
    shape = (n_src, 2, 2) if n_comp is None else (n_comp, n_src, 2, 2)
    return rng.uniform(0.05, 1.0, shape)          # (.., n_src, n_T, n_p)


# ------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("n_src", [1, 2, 3])
@pytest.mark.parametrize("n_g", [1, 2, 8, 12, 16, 64])
def test_device_matches_restatement(n_g, n_src):
    Ks = make_tables(n_src, n_g, n_bins=6, special=True)
    x = composition(n_src)
    lib = library(Ks, n_g)
    got = lib.mix(x)
    want, lnmax = M.kmix_ref(Ks, x.transpose(0, 2, 1), quad(n_g)[1])
    assert got.shape == want.shape == (2, 2, 6, n_g)
    if n_src == 1:
        assert same_bits(got, want)            # x_0 K_0: no log, no exp
        assert np.isnan(got[1, 0, 3]).sum() == 1 and np.signbit(got[0, 1, 2, 0])
        return
    eps = np.array([[[M.step_bound(n_g, v) for v in r] for r in pl] for pl in lnmax])
    bound = ((1.0 + eps) ** (n_src - 1) - 1.0)[..., None]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(got == 0, want == 0) and not np.signbit(got[got == 0]).any()
    ok = np.isfinite(want) & (want != 0)
    assert np.all(np.isfinite(got[ok]))
    with np.errstate(all="ignore"):
        rel = np.where(ok, np.abs(got / want - 1.0), 0.0)
    print(f"n_g {n_g} n_src {n_src}: worst {rel.max():.3e} of bound "
          f"{(rel / np.broadcast_to(bound, rel.shape)).max():.3f}; tightest bound {bound.min():.3e}")
    assert np.all(rel <= bound)
    # the special values landed: the zero pair in interval 0 of its item, the -0 pair likewise, a
    # NaN in the last interval; after one fold the negative value is a NaN in the first interval
    # alone (a second fold sorts that NaN last)
    assert got[0, 0, 1, 0] == 0 and got[0, 1, 2, 0] == 0 and np.isnan(got[1, 0, 3, -1])
    assert np.isnan(got[1, 1, 4, 0 if n_src == 2 else -1])
    assert np.isnan(got[1, 1, 4]).sum() == 1 and np.isnan(got).sum() >= 2
    assert np.all(np.isfinite(got[:, :, 5])) and np.all(np.isfinite(got[:, :, 0]))
    lib.release()


# ------------------------------------------------------------------------------ invariances
def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def child_main(n_g, n_src):
    """What the child process of test_forms_give_the_same_bits runs: one automatic-form mix
    under the environment's FREI_KMIX_FORM, its bits as a digest."""
    Ks = make_tables(n_src, n_g, seed=3)
    print("digest", digest(library(Ks, n_g).mix(composition(n_src, n_comp=2))))


@pytest.mark.parametrize("n_g", [1, 5, 8])
def test_forms_give_the_same_bits(n_g, monkeypatch):
    """n_g <= 8, which both forms can take: through form=, and through FREI_KMIX_FORM in a fresh
    child process."""
    monkeypatch.delenv("FREI_KMIX_FORM", raising=False)
    n_src = 3
    Ks = make_tables(n_src, n_g, seed=3)
    x = composition(n_src, n_comp=2)
    lib = library(Ks, n_g)
    out = {form: lib.mix(x, form=form) for form in (0, 1, 2)}
    assert same_bits(out[1], out[2]) and same_bits(out[0], out[1])
    assert np.all(np.isfinite(out[0])) and np.ptp(out[0]) > 0
    if n_g != 8:
        return
    for form in ("wave", "block"):
        env = dict(os.environ, FREI_KMIX_FORM=form)
        r = subprocess.run([sys.executable, "-c",
                            f"from tests.test_gpu_kmix import child_main; child_main({n_g}, {n_src})"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        assert r.stdout.split("digest")[-1].strip() == digest(out[0]), form
    monkeypatch.setenv("FREI_KMIX_FORM", "sideways")
    with pytest.raises(RuntimeError, match="FREI_KMIX_FORM"):
        lib.mix(x)
    assert same_bits(lib.mix(x, form=2), out[0])       # an explicit form does not read it
    big = library(make_tables(2, 12), 12)
    monkeypatch.setenv("FREI_KMIX_FORM", "wave")
    with pytest.raises(RuntimeError, match=r"wave form takes n_g <= 8, not n_g = 12"):
        big.mix(composition(2))
    with pytest.raises(RuntimeError, match=r"wave form takes n_g <= 8"):
        big.mix(composition(2), form=1)
    monkeypatch.delenv("FREI_KMIX_FORM")
    assert np.all(np.isfinite(big.mix(composition(2))))


@pytest.mark.parametrize("n_g", [8, 12])
def test_compositions_are_independent_and_calls_repeat(n_g):
    n_src = 3
    lib = library(make_tables(n_src, n_g, seed=4), n_g)
    x = composition(n_src, n_comp=3)
    whole = lib.mix(x)
    assert whole.shape == (3, 2, 2, 3, n_g)
    for c in range(3):
        assert same_bits(lib.mix(x[c]), whole[c])
    assert not same_bits(whole[0], whole[1])
    assert same_bits(lib.mix(x), whole)
    assert lib.mix(x, out=False) is None and lib.kernel_ms > 0


def test_more_than_2_32_lanes_in_one_call():
    """2^22 + 12 items of the 1024-lane block form (n_g = 33, P = 2048) are more than 2^32 lanes:
    the call is split into launches, and every composition — the first, those around the split
    at item 2^21, the last — equals the call on it alone."""
    n_g, n_comp = 33, (1 << 20) + 3
    Ks = make_tables(2, n_g, n_bins=1, seed=5)
    lib = library(Ks, n_g)
    base = composition(2, n_comp=7)
    single = lib.mix(base)
    which = np.arange(n_comp) % 7
    whole = lib.mix(base[which])
    assert whole.shape == (n_comp, 2, 2, 1, n_g)
    half = 1 << 19
    look = np.concatenate([np.arange(8), np.arange(half - 8, half + 8),
                           np.arange(n_comp - 8, n_comp), np.arange(0, n_comp, 100003)])
    assert same_bits(whole[look], single[which[look]])
    assert np.all(np.isfinite(single)) and not same_bits(single[0], single[1])
    del whole
    lib.release()


def test_set_kdist_holds_the_k_distribution():
    """The slot holds exactly frei_xsec_kdist's values: compared through n_src = 1, x = 1."""
    rng = np.random.default_rng(31)
    counts = [3, 64, 65, 700]
    wl = np.concatenate([k + (np.arange(n) + 0.5) / n for k, n in enumerate(counts)])
    bins = np.arange(len(counts) + 1.0)
    x = rng.lognormal(0.0, 2.0, (2, 2, wl.size)).astype(np.float32)
    xs = CrossSection(x, T2, P2, wl)
    g, w = gauss_g(8)
    T_t, p_t = np.array([1900.0, 900.0, 1200.0]), np.array([2.0, 1e-3])
    lib = KLibrary({"x": xs}, bins, g, w, T_t, p_t)
    got = lib.mix(np.ones((1, 3, 2)))
    want, _ = xs.kdist(bins, g, T_t, p_t)
    assert got.shape == (2, 3, 4, 8) and same_bits(got, want)
    ref, _ = R.kdist_ref(x, T2, P2, wl, bins, g, T_t, p_t)
    assert same_bits(got, ref)


# ------------------------------------------------------------------------------ device route
def _sweeps(eng, T):
    for d in (EMIT, ABSORB, EMIT):
        eng.set_temperatures(T)
        eng.sweep(d, want_dtaus=False)
    return list(eng.get_fluxes())


@pytest.mark.parametrize("n_g", [8, 12])
def test_engine_route_matches_host_table(n_g):
    """3 bins x n_g points x 4 layers: an Engine given the MixedKTable (frei_set_table_kmix) and
    one given the host array of .mix(x) give the same bits after emit -> absorb -> emit; a column
    slice through col_lo / n_lam equals the full run's columns."""
    p_bar = np.logspace(0.5, -3, 4)
    T_nodes = np.array([2000.0, 1000.0, 1500.0])            # stored ascending by the engine
    T = np.linspace(1700.0, 1100.0, 4)
    rng = np.random.default_rng(41 + n_g)
    Ks = np.sort(rng.lognormal(0.0, 2.0, (2, 4, 3, 3, n_g)), axis=-1)
    g, w = gauss_g(n_g)
    lib = KLibrary({"a": Ks[0], "b": Ks[1]}, WL3, g, w, T_nodes, p_bar)
    x = rng.uniform(1e-4, 1e-2, (2, 3, 4))
    tab = lib.table(x)
    n_col = 3 * n_g
    lam = 1.0 + tab.wavelength / 10.0
    qw = np.full(n_col, 1e-6)
    mmr = np.ones((1, 4))
    dev = Engine(lam, p_bar, {"mix": tab}, mmr=mmr, quad_weights=qw)
    host_vals = lib.mix(x).reshape(4, 3, n_col)
    assert same_bits(tab.values, host_vals)
    host = Engine(lam, p_bar, {"mix": fa.OpacityTable(host_vals, p_bar, T_nodes, lam)}, mmr=mmr,
                  quad_weights=qw)
    a, b = _sweeps(dev, T), _sweeps(host, T)
    for u, v in zip(a, b):
        assert same_bits(u, v)
    assert np.all(np.isfinite(a[0][1:])) and np.ptp(a[0][-1]) > 0
    lo, hi = n_g - 3, 2 * n_g + 2                            # parts of bins 0 and 2, all of bin 1
    part = Engine(lam, p_bar, {"mix": tab}, mmr=mmr, quad_weights=qw, lam_slice=(lo, hi))
    fu, fd = _sweeps(part, T)
    assert same_bits(fu, a[0][:, lo:hi]) and same_bits(fd, a[1][:, lo:hi])
    with pytest.raises(ValueError, match="must match the grid's columns"):
        Engine(lam[:-1], p_bar, {"mix": tab}, mmr=mmr, quad_weights=qw[:-1])
    for e in (dev, host, part):
        e.close()


# ------------------------------------------------------------------------------ KGrid
def _device_top_flux(eng, T):
    for d in (EMIT, ABSORB, EMIT):
        eng.set_temperatures(T)
        eng.sweep(d, want_dtaus=False)
    return eng.get_fluxes()[0][-1].copy()


def test_kgrid_random_overlap_end_to_end():
    """The two-species forest through KGrid(overlap="random"), 16 Gauss points: F_up[top] after
    emit -> absorb -> emit equals the oracle's run on the restatement's table to the 1e-10 of
    test_gpu_kdist.py's forest, per column and collapsed; set_mix with the same mix reproduces
    the bits, with another mix it changes them."""
    case = M.forest_pair()
    planet = fa.Planet.from_hot_jupiter()
    assert (planet.g, planet.m_bar, planet.a_rstar) == (PLANET["g"], PLANET["m_bar"],
                                                        PLANET["a_rstar"])
    xs = {n: CrossSection(case[k], case["T_nodes"], case["p"], case["wl"], n)
          for n, k in (("one", "xsec1"), ("two", "xsec2"))}
    mix = np.array(M.FOREST_MIX)[:, None, None]
    for x in xs.values():
        x.timing(1)                       # count the sorts
    grid = KGrid(planet, case["wl_bins"], n_g=16, pressures=case["p"],
                 init_temperatures=case["T"])
    out = grid.load_opacities(cross_sections=xs, mix=mix, overlap="random")
    assert list(out) == ["mix"] and grid.klibrary.n_src == 2
    assert np.array_equal(out["mix"].temperature, case["T_nodes"])
    kflux = _device_top_flux(grid.engine(), case["T"])
    want, _ = M.kmix_ref(M.species_tables(case, grid.g), mix, grid.weights)
    o_k = R.oracle_top_flux(want.reshape(want.shape[:2] + (-1,)), grid.col_lam, case, PLANET)
    err_col = float(np.max(np.abs(kflux / o_k - 1.0)))
    err = float(np.max(np.abs(grid.collapse(kflux) / grid.collapse(o_k) - 1.0)))
    print("per column", err_col, "collapsed", err)
    assert err_col <= 1e-10 and err <= 1e-10
    sorts = [x.timing(-1)[1] for x in xs.values()]
    assert sorts == [1, 1]
    grid.set_mix(mix)
    assert grid._engine is None
    assert same_bits(_device_top_flux(grid.engine(), case["T"]), kflux)
    grid.set_mix(np.array([0.2, 0.8])[:, None, None])
    other = _device_top_flux(grid.engine(), case["T"])
    assert np.all(np.isfinite(other)) and not same_bits(other, kflux)
    assert float(np.max(np.abs(other / kflux - 1.0))) > 1e-3
    assert [x.timing(-1)[1] for x in xs.values()] == sorts     # nothing was sorted again


# ------------------------------------------------------------------------------ C-level errors
def _create(n_src=2, n_p=2, n_T=2, n_bins=3, n_g=4, g=None, w=None, out=True, wl=WL3):
    lib, h = N.lib(), ctypes.c_void_p()
    gq, wq = gauss_g(4)
    g = N.f64(gq if g is None else g)
    w = N.f64(wq if w is None else w)
    rc = lib.frei_klib_create(ctypes.byref(h) if out else None, 0, n_src, n_p, n_T, n_bins, n_g,
                              N.dptr(N.f64(wl)), N.dptr(g), N.dptr(w), N.dptr(P2), N.dptr(T2))
    return rc, h, lib.frei_last_error().decode()


def test_c_level_argument_errors():
    lib = N.lib()
    for kw, msg in ((dict(out=False), "null argument"),
                    (dict(n_src=0), "n_src < 1"),
                    (dict(n_p=0), "at least one"),
                    (dict(n_bins=0), "n_bins < 1"),
                    (dict(n_g=0), "n_g = 0"),
                    (dict(n_g=65), "n_g = 65 lies outside [1, 64]"),
                    (dict(wl=[1.0, 2.0, 2.0, 3.0]), "wl_bins"),
                    (dict(g=[0.1, 0.5, 0.4, 0.9]), "g[2]"),
                    (dict(g=[0.1, 0.5, 0.6, 1.0]), "g[3]"),
                    (dict(w=[0.5, np.nan, 0.2, 0.2]), "w[1]"),
                    (dict(w=[0.5, 0.3, -0.2, 0.2]), "w[2]"),
                    (dict(w=[0.5, 0.3, 0.2, 1e-10]), "w[3]"),
                    (dict(w=[0.9, 0.9, 0.9, 0.1]), "w[2]")):
        rc, h, err = _create(**kw)
        assert rc != 0 and msg in err and not h.value, (kw, err)
    rc, h, err = _create()
    assert rc == 0 and h.value, err
    tab = N.f64(np.ones((2, 2, 3, 4)))
    x = N.f64(np.ones((1, 2, 2, 2)))
    out = np.empty((1, 2, 2, 3, 4))

    def fails(rc, msg):
        err = lib.frei_last_error().decode()
        assert rc != 0 and msg in err, err

    fails(lib.frei_klib_set(h, 2, N.dptr(tab)), "slot 2 lies outside [0, n_src = 2)")
    fails(lib.frei_klib_set(h, -1, N.dptr(tab)), "slot -1")
    fails(lib.frei_klib_set(h, 0, None), "null argument")
    fails(lib.frei_klib_set(None, 0, N.dptr(tab)), "null argument")
    fails(lib.frei_klib_set_kdist(h, 0, None), "null argument")
    assert lib.frei_klib_set(h, 0, N.dptr(tab)) == 0
    fails(lib.frei_klib_mix(h, 1, N.dptr(x), N.dptr(out), 0, None), "slot 1 holds no table")
    assert lib.frei_klib_set(h, 1, N.dptr(tab)) == 0
    fails(lib.frei_klib_mix(None, 1, N.dptr(x), N.dptr(out), 0, None), "null library")
    fails(lib.frei_klib_mix(h, 1, None, N.dptr(out), 0, None), "null x")
    fails(lib.frei_klib_mix(h, 0, N.dptr(x), N.dptr(out), 0, None), "n_comp < 1")
    fails(lib.frei_klib_mix(h, 1, N.dptr(x), N.dptr(out), 3, None), "form must be")
    bad = x.copy()
    bad[0, 1, 0, 1] = -0.5
    fails(lib.frei_klib_mix(h, 1, N.dptr(bad), N.dptr(out), 0, None), "x[0][1][0][1] = -0.5")
    bad[0, 1, 0, 1] = np.inf
    fails(lib.frei_klib_mix(h, 1, N.dptr(bad), N.dptr(out), 0, None), "x[0][1][0][1]")
    bad[0, 0, 1, 0] = np.nan                                  # the first offender is named
    fails(lib.frei_klib_mix(h, 1, N.dptr(bad), N.dptr(out), 0, None), "x[0][0][1][0]")
    # into a context: columns outside the library's, a null, and the library goes on
    lam = np.linspace(1.0, 2.0, 12)
    eng = Engine(lam, np.logspace(0, -3, 4), {"x": fa.OpacityTable(np.ones((2, 2, 12)), P2, T2, lam)},
                 mmr=np.ones((1, 4)))
    fails(lib.frei_set_table_kmix(eng._ctx, 0, h, N.dptr(x), 1),
          "frei_set_table_kmix: columns [1, 13) lie outside the 12")
    fails(lib.frei_set_table_kmix(eng._ctx, 0, h, N.dptr(x), -1), "columns [-1, 11)")
    fails(lib.frei_set_table_kmix(eng._ctx, 0, None, N.dptr(x), 0), "null argument")
    fails(lib.frei_set_table_kmix(eng._ctx, 0, h, None, 0), "null argument")
    fails(lib.frei_set_table_kmix(eng._ctx, 0, h, N.dptr(bad), 0), "x[0][0][1][0]")
    fails(lib.frei_set_table_kmix(eng._ctx, 1, h, N.dptr(x), 0), "species index out of range")
    assert lib.frei_set_table_kmix(eng._ctx, 0, h, N.dptr(x), 0) == 0
    eng.close()
    assert lib.frei_klib_mix(h, 1, N.dptr(x), N.dptr(out), 0, None) == 0
    # two equal tables of ones at x = 1: every pair is 2
    assert np.allclose(out, 2.0, rtol=1e-14, atol=0)
    assert lib.frei_klib_destroy(h) == 0 and lib.frei_klib_destroy(None) == 0
