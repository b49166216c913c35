"""CPU restatement of the reference's stellar-spectrum binning (phoenix.py:13-17, 43-52), the
checker of the GPU binning tests.  ``test_stellar_host.py`` holds it to the reference-made
fixture ``golden/stellar_bin.npz`` bitwise.

Bin k holds the points ``wl_bins[k] < wl <= wl_bins[k+1]`` (pandas.cut, right-closed); its
value is xarray's ``integrate`` — ``np.sum(dx * 0.5 * (y[1:] + y[:-1]))``, numpy's pairwise
sum — over ``max - min`` of the group's wavelengths; a single-point bin is 0 / 0 = NaN.
"""
import numpy as np


def plan(wl, wl_bins):
    """Edge positions: bin k is the points [pos[k], pos[k+1])."""
    return np.searchsorted(np.asarray(wl), np.asarray(wl_bins), side="right")


def counts(wl, wl_bins):
    return np.diff(plan(wl, wl_bins)).astype(np.int64)


def bin_aligned(wl, flux, wl_bins):
    """(values, scale): values[n_spec][n_bins] aligned with the bins, NaN for bins of fewer
    than two points; scale = sum_i |term_i| / span of each (spectrum, bin), what the summation
    error bound is relative to (0 where the value is NaN)."""
    wl = np.asarray(wl, dtype=float)
    flux = np.atleast_2d(np.asarray(flux, dtype=float))
    pos = plan(wl, wl_bins)
    nb = len(pos) - 1
    val = np.full((flux.shape[0], nb), np.nan)
    scale = np.zeros((flux.shape[0], nb))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(nb):
            s, e = pos[k], pos[k + 1]
            if e - s < 1:
                continue
            x = wl[s:e]
            span = x.max() - x.min()
            dx = x[1:] - x[:-1]
            for m in range(flux.shape[0]):
                y = flux[m, s:e]
                term = dx * 0.5 * (y[1:] + y[:-1])
                val[m, k] = np.sum(term) / span
                if e - s >= 2:
                    scale[m, k] = np.sum(np.abs(term)) / span
    return val, scale


def compact_padded(aligned, n_points, n_lam):
    """The reference's output (phoenix.py:47-51): the non-empty bins' values in bin order,
    zero-padded at the end to n_lam."""
    aligned = np.asarray(aligned)
    vals = aligned[..., np.asarray(n_points) > 0]
    pad = [(0, 0)] * (vals.ndim - 1) + [(0, n_lam - vals.shape[-1])]
    return np.pad(vals, pad)


def bound(n_points, scale):
    """|x - ref| <= 2 max(n_k, 4) eps sum_i |term_i| / span: both sides form the same terms, so
    only the order of at most n_k additions differs (each side's sum is within
    (n_k - 1) eps sum|term| of the exact one to first order, whatever its order)."""
    n = np.maximum(np.asarray(n_points), 4)
    return 2.0 * n * np.finfo(float).eps * scale


def assert_binned(got, ref, tol, what=""):
    """The NaN pattern of ``got`` is ``ref``'s exactly and |got - ref| <= tol elsewhere; prints
    the largest |err| / tol before asserting."""
    got, ref = np.atleast_2d(got), np.atleast_2d(ref)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = np.broadcast_to(tol, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(ref)
    err = np.abs(np.where(ok, got - ref, 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / tol, 0.0)
    worst = float(np.max(ratio, initial=0.0))
    print(f"{what}: max |err| / bound = {worst:.3g}")
    assert np.all(err <= np.where(ok, tol, 0.0)), f"{what}: max |err| / bound = {worst:.3g}"
