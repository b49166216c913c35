"""K17 on the GPU: frei_xsec_create_lines against the 50-digit fixture and the NumPy restatement
(tests/lines_ref.py), its bitwise properties, the result as an ordinary frei_xsec under K6, and
frei_xsec_values.  The bar is one float32 ulp (tests/test_lines_host.py says why); points no
line reaches are exactly 0.
"""
import ctypes
import os

import numpy as np
import pytest

import frei_amd as fa
from frei_amd import _native as N
from frei_amd.lines import LineList
from tests import lines_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "voigt_case.npz")
PART = (np.array([150.0, 296.0, 1000.0, 3000.0]), np.array([55.0, 108.0, 380.0, 2900.0]))
T_NODES = np.array([200.0, 800.0, 2500.0])
P_NODES = np.array([1e-6, 1e-3, 0.1, 1.0, 30.0])       # 5: no multiple of a tile of 2 or 4
CUTOFF = 2.0


def ulps32(a, b):
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def forest_lines(seed=5, n=700):
    rng = np.random.default_rng(seed)
    return dict(nu0=rng.uniform(1990.0, 2010.0, n), S=10.0 ** rng.uniform(-25.0, -19.0, n),
                E_low=rng.uniform(0.0, 3000.0, n), gamma=rng.uniform(0.03, 0.1, n),
                n_exp=rng.uniform(0.4, 0.8, n))


def forest_axis():
    """805 points, non-uniform (three blocks of 256 and a 37-point tail): the first block and the
    tail lie farther than the cutoff from every line (empty line ranges), the two blocks between
    see different line ranges, each longer than one staging chunk of 256 lines."""
    rng = np.random.default_rng(6)
    nu = np.concatenate([np.sort(rng.uniform(2012.5, 2015.0, 256))[::-1],
                         np.sort(rng.uniform(1988.5, 2012.4, 512))[::-1],
                         np.sort(rng.uniform(1985.0, 1987.9, 37))[::-1]])
    wl = 1e4 / nu
    assert wl.size == 805 and np.all(np.diff(wl) > 0)
    return wl


@pytest.fixture(scope="module")
def forest():
    lines = forest_lines()
    ll = LineList(mass=28.0, partition=PART, **lines)
    wl = forest_axis()
    xs = ll.cross_section(T_NODES, P_NODES, wl, cutoff=CUTOFF)
    full = xs.values()
    full.setflags(write=False)
    return dict(lines=lines, ll=ll, wl=wl, xs=xs, full=full)


def test_fixture_case():
    c = dict(np.load(GOLDEN))
    h = ctypes.c_void_p()
    nT, npn, nhi = c["T_nodes"].size, c["p_nodes"].size, c["wl_hi"].size
    ms = ctypes.c_double(-1.0)
    N.check(N.lib().frei_xsec_create_lines(
        ctypes.byref(h), 0, 1, N.dptr(c["nu0"]), N.dptr(c["S_ref"]), N.dptr(c["E_low"]),
        N.dptr(c["gamma_ref"]), N.dptr(c["n_exp"]), float(c["mass_amu"]), float(c["T_ref"]),
        float(c["cutoff"]), N.dptr(c["q_ratio"]), nT, npn, nhi, N.dptr(c["T_nodes"]),
        N.dptr(c["p_nodes"]), N.dptr(c["wl_hi"]), ctypes.byref(ms)))
    try:
        got = np.empty((nT, npn, nhi), dtype=np.float32)
        for t in range(nT):
            for p in range(npn):
                N.check(N.lib().frei_xsec_values(h, t, p, 0, nhi, N.fptr(got[t, p])))
    finally:
        N.lib().frei_xsec_destroy(h)
    assert ms.value > 0.0
    want = c["values"].astype(np.float32)
    assert np.all(got[..., ~c["inside"]] == 0.0)
    d = ulps32(got, want)
    print("device vs fixture: worst float32 ulps", d.max(), "differing", int((d > 0).sum()))
    assert d.max() <= 1


def test_forest_against_restatement(forest):
    ll, wl, got = forest["ll"], forest["wl"], forest["full"]
    want = R.cross_section(ll.nu0, ll.S, ll.E_low, ll.gamma, ll.n_exp, ll.mass, ll.T_ref, CUTOFF,
                           ll.q_ratio(T_NODES), T_NODES, P_NODES, wl)
    assert got.shape == want.shape == (3, 5, 805) and got.dtype == np.float32
    nu = R.wavenumbers(wl)
    reached = (np.abs(nu[:, None] - ll.nu0[None, :]) <= CUTOFF).any(axis=1)
    assert not reached[:256].any() and not reached[-37:].any() and reached[256:768].sum() > 400
    assert np.all(got[..., ~reached] == 0.0)
    assert np.all(got[..., reached] > 0.0)
    d = ulps32(got, want)
    print("device vs restatement: worst float32 ulps", d.max(), "differing", int((d > 0).sum()))
    assert d.max() <= 1


def test_two_calls_are_identical(forest):
    xs = forest["ll"].cross_section(T_NODES, P_NODES, forest["wl"], cutoff=CUTOFF)
    assert np.array_equal(xs.values(), forest["full"])
    assert xs.opacity is None and xs.kernel_ms > 0.0


@pytest.mark.parametrize("form", ["l1", "l2", "l4", "s1", "s2", "s4"])
def test_every_form_adds_the_same_bits(forest, form, monkeypatch):
    """LDS-staged or scalar-loaded line parameters, pressure tiles of 1, 2 and 4 nodes (5 nodes:
    the tile of 2 and of 4 both leave a rest of 1)."""
    monkeypatch.setenv("FREI_LINES_FORM", form)
    xs = forest["ll"].cross_section(T_NODES, P_NODES, forest["wl"], cutoff=CUTOFF)
    assert np.array_equal(xs.values(), forest["full"])
    monkeypatch.setenv("FREI_LINES_FORM", "x3")
    with pytest.raises(RuntimeError, match="FREI_LINES_FORM"):
        forest["ll"].cross_section(T_NODES, P_NODES, forest["wl"], cutoff=CUTOFF)


def test_axis_subrange_is_that_slice(forest):
    xs = forest["ll"].cross_section(T_NODES, P_NODES, forest["wl"][100:600], cutoff=CUTOFF)
    assert np.array_equal(xs.values(), forest["full"][..., 100:600])


def test_single_node_is_its_row(forest):
    xs = forest["ll"].cross_section(T_NODES[1], P_NODES[3], forest["wl"], cutoff=CUTOFF)
    assert np.array_equal(xs.values(t=0, p=0), forest["full"][1, 3])
    xs = forest["ll"].cross_section(T_NODES[2:], P_NODES[1:3], forest["wl"], cutoff=CUTOFF)
    assert np.array_equal(xs.values(t=0), forest["full"][2, 1:3])


def test_lines_beyond_the_cutoff_change_no_bit(forest):
    rng = np.random.default_rng(8)
    far = dict(nu0=np.concatenate([rng.uniform(1900.0, 1982.9, 25), rng.uniform(2017.1, 2100.0, 25)]),
               S=np.full(50, 1e-15), E_low=np.zeros(50), gamma=np.full(50, 0.1),
               n_exp=np.full(50, 0.5))
    lines = {k: np.concatenate([far[k], v]) for k, v in forest["lines"].items()}
    xs = LineList(mass=28.0, partition=PART, **lines).cross_section(T_NODES, P_NODES, forest["wl"],
                                                                  cutoff=CUTOFF)
    assert np.array_equal(xs.values(), forest["full"])


def test_shuffled_lines_equal_sorted(forest):
    lines = forest["lines"]
    assert np.unique(lines["nu0"]).size == lines["nu0"].size
    perm = np.random.default_rng(9).permutation(lines["nu0"].size)
    ll = LineList(mass=28.0, partition=PART, **{k: v[perm] for k, v in lines.items()})
    xs = ll.cross_section(T_NODES, P_NODES, forest["wl"], cutoff=CUTOFF)
    assert np.array_equal(xs.values(), forest["full"])


def test_it_is_a_real_xsec(forest):
    xs, wl = forest["xs"], forest["wl"]
    host = fa.CrossSection(forest["full"], T_NODES, P_NODES, wl)
    edges = np.linspace(4.965, 5.035, 22)
    lam = 0.5 * (edges[1:] + edges[:-1])
    T, p = np.array([300.0, 2000.0]), np.array([1e-4, 1.0, 10.0])
    for groupies in (True, False):
        a = xs.bin(edges, lam, T, p, groupies=groupies)
        b = host.bin(edges, lam, T, p, groupies=groupies)
        assert a.shape == (3, 2, 21) and np.all(np.isfinite(a)) and a.max() > 0
        assert np.array_equal(a, b)
    tabs = fa.binned_opacity(T, p, edges, lam, cross_sections={"12C-16O": xs})
    assert np.array_equal(tabs["12C-16O"].values, xs.bin(edges, lam, T, p))


def test_values_of_an_uploaded_cross_section():
    rng = np.random.default_rng(10)
    vals = rng.uniform(0.0, 1.0, (2, 3, 50)).astype(np.float32)
    xs = fa.CrossSection(vals, [500.0, 900.0], [0.1, 1.0, 10.0], np.linspace(1.0, 2.0, 50))
    assert np.array_equal(xs.values(), vals)
    assert np.array_equal(xs.values(t=1, p=2), vals[1, 2])
    assert np.array_equal(xs.values(p=0), vals[:, 0])
    part = np.full(20, -1.0, dtype=np.float32)
    N.check(N.lib().frei_xsec_values(xs.handle(0), 1, 2, 7, 20, N.fptr(part)))   # the last row
    assert np.array_equal(part, vals[1, 2, 7:27])
    assert N.lib().frei_xsec_values(xs.handle(0), 1, 2, 40, 11, N.fptr(part)) != 0
    assert N.lib().frei_xsec_values(xs.handle(0), 2, 0, 0, 1, N.fptr(part)) != 0
