"""K15 on the host: ModelGrid.plan against the plain restatement (tests/interp_ref.py), the
exactness of plan x sum on a dyadic case, the argument errors of the frei_itp_* entry points —
all reached before a device is touched —, the staleness of InterpolatedSpectra and the form-0
rule.  No GPU is needed."""
import ctypes

import numpy as np
import pytest

from tests import interp_ref as R


def _grid(axes, n_lam=5, **kw):
    from frei_amd.modelgrid import ModelGrid
    n = int(np.prod([len(a) for a in axes]))
    X = np.arange(n * n_lam, dtype=float).reshape(n, n_lam)
    return ModelGrid(axes, np.linspace(1.0, 2.0, n_lam), spectra=X, **kw)


AXES = {
    1: [np.array([1.0, 1.5, 4.0, 4.25])],
    2: [np.array([-2.0, 0.0, 0.3]), np.array([10.0, 11.0, 15.0, 15.5, 40.0])],
    3: [np.array([1000.0, 1400.0, 2300.0]), np.array([2.5, 3.0]), np.array([-1.0, 0.0, 0.7])],
    4: [np.array([0.0, 1.0]), np.array([0.0, 0.1, 0.7]), np.array([5.0, 6.0]),
        np.array([-3.0, -1.0, 0.0, 8.0])],
}


def _queries(axes, seed):
    """Seeded queries inside the grid, then the special ones: on a node, on the first and the
    last node of every axis, and beyond both ends."""
    rng = np.random.default_rng(seed)
    lo = np.array([g[0] for g in axes])
    hi = np.array([g[-1] for g in axes])
    inside = rng.uniform(lo, hi, size=(12, len(axes)))
    node = np.array([[g[min(1, g.size - 1)] for g in axes]])
    first, last = lo[None, :], hi[None, :]
    below, above = first - 1.5, last + 2.5
    mixed = np.where(np.arange(len(axes)) % 2 == 0, below, inside[:1])
    return np.concatenate([inside, node, first, last, below, above, mixed])


@pytest.mark.parametrize("d", [1, 2, 3, 4])
def test_plan_matches_the_restatement(d):
    axes = AXES[d]
    g = _grid(axes)
    theta = _queries(axes, d)
    idx, w, n_out = g.plan(theta)
    r_idx, r_w, r_out = R.plan(axes, theta)
    assert idx.dtype == np.int32 and w.dtype == np.float64
    assert idx.shape == w.shape == (theta.shape[0], 2 ** d)
    assert np.array_equal(idx, r_idx)
    assert R.same_bits(w, r_w)
    # beyond both ends: every coordinate of two queries, and every other one of the mixed query
    assert n_out == r_out == 2 * d + (d + 1) // 2
    assert np.all(w >= 0.0)
    ulp = np.finfo(float).eps
    assert np.all(np.abs(w.sum(axis=1) - 1.0) <= 2 ** d * ulp)


def test_query_on_a_node_and_at_the_ends():
    axes = AXES[2]
    g = _grid(axes)
    theta = np.array([[0.0, 15.0],       # on an inner node
                      [-2.0, 10.0],      # the first node of both axes
                      [0.3, 40.0],       # the last node of both axes
                      [-9.0, 99.0]])     # clamped to (first, last)
    idx, w, n_out = g.plan(theta)
    assert n_out == 2
    on = [(1, 2), (0, 0), (2, 4), (0, 4)]
    for q, (i, j) in enumerate(on):
        node = i * 5 + j
        hit = idx[q] == node
        assert hit.sum() == 1
        assert np.array_equal(w[q][hit], [1.0]) and np.array_equal(w[q][~hit], [0.0] * 3)
    # the last node is reached from the last cell with t = 1 exactly
    assert idx[2].tolist() == [1 * 5 + 3, 1 * 5 + 4, 2 * 5 + 3, 2 * 5 + 4]


def test_axis_of_one_node_takes_no_part():
    axes = [np.array([1.0, 2.0, 4.0]), np.array([7.0]), np.array([0.0, 8.0])]
    g = _grid(axes)
    assert g.n_corner == 4 and g.participating == [0, 2]
    theta = np.array([[1.5, 123.0, 2.0], [4.0, -5.0, 8.0]])
    idx, w, n_out = g.plan(theta)
    r_idx, r_w, r_out = R.plan(axes, theta)
    assert n_out == r_out == 0          # the coordinate on the single-node axis is not clamped
    assert np.array_equal(idx, r_idx) and R.same_bits(w, r_w)
    assert idx[0].tolist() == [0, 1, 2, 3] and w[0].tolist() == [0.375, 0.125, 0.375, 0.125]
    with pytest.raises(ValueError, match=r"theta\[1\]\[1\] is not finite"):
        g.plan(np.array([[1.5, 0.0, 2.0], [1.5, np.inf, 2.0]]))
    one = _grid([np.array([3.0])])
    idx, w, n_out = one.plan(np.array([[-40.0], [3.0]]))
    assert idx.tolist() == [[0], [0]] and w.tolist() == [[1.0], [1.0]] and n_out == 0


def test_plan_argument_errors():
    g = _grid(AXES[2])
    with pytest.raises(ValueError, match=r"theta\[1\]\[0\] is NaN"):
        g.plan(np.array([[0.0, 11.0], [np.nan, 11.0]]))
    with pytest.raises(ValueError, match="n_query"):
        g.plan(np.array([0.0, 11.0]))
    with pytest.raises(ValueError, match="n_query"):
        g.plan(np.zeros((3, 3)))
    from frei_amd.modelgrid import ModelGrid
    lam = np.linspace(1.0, 2.0, 5)
    with pytest.raises(ValueError, match="strictly ascending"):
        ModelGrid([np.array([1.0, 1.0])], lam, spectra=np.zeros((2, 5)))
    with pytest.raises(ValueError, match="1 to 4 axes"):
        ModelGrid([np.array([1.0, 2.0])] * 5, lam, spectra=np.zeros((32, 5)))
    with pytest.raises(ValueError, match="product of the axis lengths"):
        ModelGrid([np.array([1.0, 2.0]), np.array([1.0, 2.0, 3.0])], lam,
                  spectra=np.zeros((5, 5)))
    with pytest.raises(ValueError, match="pass x, or engine="):
        ModelGrid([np.array([1.0, 2.0])], lam)
    with pytest.raises(ValueError, match="theta, or idx= and w="):
        g.interpolate()
    with pytest.raises(ValueError, match="theta, or idx= and w="):
        g.interpolate(idx=np.zeros((1, 1), dtype=np.int32))


@pytest.mark.parametrize("shape", [(5,), (3, 4), (3, 2, 3), (2, 3, 2, 2), (3, 1, 2)])
def test_dyadic_multilinear_function_is_reproduced_exactly(shape):
    axes, X, theta, exact = R.dyadic_case(shape)
    g = _grid(axes)
    idx, w, n_out = g.plan(theta)
    assert n_out == 0
    assert R.same_bits(R.interpolate(X, idx, w), exact)


def test_argument_errors_without_gpu():
    """Every host-side check of frei_itp_create, _set_nodes and _apply comes before any device
    call: all of them are reached on a machine without a GPU."""
    from frei_amd import _native as N
    from frei_amd.modelgrid import LDS_MAX_NODES, MAX_CORNERS
    lib = N.lib()
    i32p = ctypes.POINTER(ctypes.c_int32)

    def err():
        return lib.frei_last_error().decode()

    h = ctypes.c_void_p()
    assert lib.frei_itp_create(None, 0, 10, 3) != 0 and "null argument" in err()
    assert lib.frei_itp_create(ctypes.byref(h), 0, 0, 3) != 0 and "n_lam must be >= 1" in err()
    assert lib.frei_itp_create(ctypes.byref(h), 0, 10, 0) != 0 and "n_node must be >= 1" in err()
    assert lib.frei_itp_create(ctypes.byref(h), -1, 10, 3) != 0 and "device" in err()
    assert lib.frei_itp_create(ctypes.byref(h), 0, 512 * 65535 + 1, 3) != 0
    assert "launch grid" in err()
    assert h.value is None
    tall = ctypes.c_void_p()
    assert lib.frei_itp_create(ctypes.byref(h), 0, 10, 3) == 0
    assert lib.frei_itp_create(ctypes.byref(tall), 0, 10, LDS_MAX_NODES + 1) == 0
    try:
        assert lib.frei_itp_set_nodes(None, None, None, None) != 0 and "null handle" in err()
        assert lib.frei_itp_set_nodes(h, None, None, None) != 0
        assert "x, ctx and brd are all null" in err()

        idx = np.array([[0, 1], [2, 3]], dtype=np.int32)
        w = np.array([[0.5, 0.5], [0.5, 0.5]])
        out = np.empty((2, 10))
        ip, wp, op = idx.ctypes.data_as(i32p), N.dptr(w), N.dptr(out)

        def apply(handle=h, n_query=2, n_corner=2, ip=ip, wp=wp, form=0, op=op, keep=0):
            return lib.frei_itp_apply(handle, n_query, n_corner, ip, wp, form, op, keep, None,
                                      None)
        assert apply(handle=None) != 0 and "null handle" in err()
        assert apply(n_query=0) != 0 and "n_query must be >= 1" in err()
        assert apply(n_corner=0) != 0 and "n_corner = 0 lies outside [1, 16]" in err()
        assert apply(n_corner=MAX_CORNERS + 1) != 0 and "n_corner = 17" in err()
        assert apply(ip=None) != 0 and "idx or w is null" in err()
        assert apply(wp=None) != 0 and "idx or w is null" in err()
        assert apply(op=None) != 0 and "out is null and keep is not set" in err()
        assert apply(form=3) != 0 and "form must be 0" in err()
        assert apply(form=-1) != 0 and "form must be 0" in err()
        assert apply() != 0 and "idx[1][1] = 3 lies outside [0, n_node = 3)" in err()
        idx[1, 1], idx[0, 1] = 2, -1
        assert apply() != 0 and "idx[0][1] = -1 lies outside" in err()
        idx[0, 1] = 1
        assert apply(handle=tall, form=2) != 0
        assert f"at most {LDS_MAX_NODES} nodes in LDS, not n_node = {LDS_MAX_NODES + 1}" in err()
        # everything accepted: the one thing missing is the library
        for form in (0, 1, 2):
            assert apply(form=form) != 0 and "no nodes set" in err()
        assert apply(op=None, keep=1) != 0 and "no nodes set" in err()
        assert apply(handle=tall) != 0 and "no nodes set" in err()

        # the consumers' fourth source
        assert lib.frei_ccf_apply_itp(None, None, 2, None, 0, None, None, None, 0, None, None,
                                      None, None, None) != 0
        assert "null interpolator" in err()
        assert lib.frei_obs_apply_itp(None, None, 2, None, None, 0, None, None, None, None, 0,
                                      None, None, None, None) != 0
        assert "null interpolator" in err()
        assert lib.frei_brd_apply_itp(None, None, 2, 0, None, 0, None, None) != 0
        assert "null interpolator" in err()
    finally:
        assert lib.frei_itp_destroy(h) == 0 and lib.frei_itp_destroy(tall) == 0
    assert lib.frei_itp_destroy(None) == 0


class _NoDevice:
    """frei_itp_apply and frei_itp_set_nodes stubbed: the staleness rules are the Python
    layer's and need no device."""

    def __init__(self, monkeypatch):
        from frei_amd import _native as N
        real = N.lib()

        class Lib:
            def __getattr__(self, name):
                return getattr(real, name)

            @staticmethod
            def frei_itp_set_nodes(*a):
                return 0

            @staticmethod
            def frei_itp_apply(*a):
                return 0
        monkeypatch.setattr(N, "_lib", Lib())


def test_interpolated_spectra_go_stale(monkeypatch):
    _NoDevice(monkeypatch)
    g = _grid(AXES[1])
    theta = np.array([[1.25], [4.0], [9.0]])
    kept = g.interpolate(theta, keep=True)
    assert kept.n_query == kept.n_atm == 3 and kept.n_lam == 5 and not kept.single
    assert g.n_outside == 1
    assert kept.handle() is g._handle
    again = g.interpolate(theta[:1], keep=True)            # the next interpolate
    with pytest.raises(RuntimeError, match="stale InterpolatedSpectra"):
        kept.handle()
    assert again.handle() is g._handle
    g.interpolate(theta[:1])                               # kept or not
    with pytest.raises(RuntimeError, match="stale"):
        again.handle()
    kept = g.interpolate(idx=np.array([[0, 3]]), w=np.array([[0.5, 0.5]]), keep=True)
    g.set_nodes(np.zeros((4, 5)))                          # new nodes
    with pytest.raises(RuntimeError, match="stale"):
        kept.handle()
    kept = g.interpolate(theta, keep=True)
    g.release()                                            # the handle is gone
    with pytest.raises(RuntimeError, match="stale"):
        kept.handle()
    # kept spectra are told apart by their suffix, and a model grid refuses them as nodes
    from frei_amd._device import kept_suffix
    from frei_amd.broaden import BroadenedSpectra
    assert kept_suffix(kept) == "_itp" and kept_suffix(np.zeros(3)) is None
    assert kept_suffix(BroadenedSpectra(None, 0, 1, False)) == "_brd"
    with pytest.raises(TypeError, match="cannot be a model grid's nodes"):
        g.set_nodes(kept)


def test_automatic_form():
    from frei_amd import modelgrid as M
    assert M.tile_width(1) == 256 and M.tile_width(80) == 256
    assert M.tile_width(81) == 128 and M.tile_width(160) == 128
    assert M.tile_width(161) == 64 and M.tile_width(M.LDS_MAX_NODES) == 64
    assert M.tile_width(M.LDS_MAX_NODES + 1) == 0
    assert M.LDS_MAX_NODES * 64 * 8 == M.LDS_BYTES and M.MAX_CORNERS == 16
    Q, C, T = M.LDS_FROM_QUERIES, M.LDS_FROM_CORNERS, M.LDS_FROM_TILES
    n_lam = 100000                       # 1563 tiles of 64, 391 of 256
    assert M.automatic_form(256, n_lam, Q, C) == 2
    assert M.automatic_form(256, n_lam, 4096, 16) == 2
    # the probe's shapes (profiles/r15/interp): the LDS form at 16 corners from 64 queries on
    assert [M.automatic_form(256, n_lam, q, c) for q, c in
            ((1, 8), (64, 8), (4096, 8), (4096, 2), (4096, 16), (64, 16), (512, 16))] == \
        [1, 1, 1, 1, 2, 2, 2]
    assert M.automatic_form(256, n_lam, Q - 1, 16) == 1
    assert M.automatic_form(256, n_lam, 4096, C - 1) == 1
    assert M.automatic_form(M.LDS_MAX_NODES + 1, n_lam, 4096, 16) == 1     # does not fit
    assert M.automatic_form(27, 256 * T, Q, C) == 2
    assert M.automatic_form(27, 256 * (T - 1), 4096, 16) == 1              # too few tiles
    # the header's constants are the module's
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "frei_hip.h")).read()
    defs = dict(re.findall(r"#define FREI_ITP_(\w+) (\d+)", text))
    assert {k: int(v) for k, v in defs.items()} == {
        "MAX_CORNERS": M.MAX_CORNERS, "LDS_BYTES": M.LDS_BYTES, "LDS_WAVES": M.LDS_WAVES,
        "LDS_MAX_NODES": M.LDS_MAX_NODES, "LDS_FROM_QUERIES": Q, "LDS_FROM_CORNERS": C}
