"""Plain numpy restatement of the broadening (K13): the definition in the header comment of
frei_brd_apply (include/frei_hip.h), written for reading, not for speed.  The weights are formed
by the operations of the definition, one rounding each, so they are bitwise the device's; the
sums here are numpy's, in whatever order it takes."""
import numpy as np

C_KMS = 299792.458


def axis(lam):
    """(u, tw): u = c ln(lam) and its trapezoid weights, half the neighbouring gaps, one-sided
    at the ends."""
    u = C_KMS * np.log(np.asarray(lam, dtype=float))
    tw = np.empty_like(u)
    for j in range(u.size):
        lo, hi = max(j - 1, 0), min(j + 1, u.size - 1)
        tw[j] = 0.5 * (u[hi] - u[lo])
    return u, tw


def plan(u, n_tab, dv):
    """(first, count) by brute force: the run of j with |u[j] - u[i]| <= H = h dv."""
    H = float((n_tab - 1) // 2) * dv
    first, count = np.empty(u.size, np.int32), np.empty(u.size, np.int32)
    for i in range(u.size):
        inside = np.nonzero(np.abs(u - u[i]) <= H)[0]
        assert np.array_equal(inside, np.arange(inside[0], inside[-1] + 1))
        first[i], count[i] = inside[0], inside.size
    return first, count


def weights(u, tw, i, first, count, inv_dv, tab):
    """w_ij for j = first .. first + count - 1."""
    h = float((tab.size - 1) // 2)
    j = np.arange(first, first + count)
    d = u[j] - u[i]
    q = d * inv_dv + h
    k = np.clip(np.floor(q), 0, tab.size - 2)
    f = q - k
    k = k.astype(int)
    K = tab[k] + f * (tab[k + 1] - tab[k])
    return tw[j] * K


def norm(u, tw, first, count, inv_dv, tab):
    """norm[i]: the weights added in ascending j, one plain addition each."""
    out = np.empty(u.size)
    for i in range(u.size):
        s = 0.0
        for w in weights(u, tw, i, first[i], count[i], inv_dv, tab):
            s = s + float(w)
        out[i] = s
    return out


def apply(x, u, tw, first, count, inv_dv, tab):
    """(out, bound) [n_atm][n_lam]: out = (sum_j w_ij x[m][j]) / norm[i] and the bound on
    |device - out|, (2 count_i + 8) 2^-53 sum_j |w_ij x[m][j]| / norm[i]."""
    x = np.atleast_2d(np.asarray(x, dtype=float))
    nm = norm(u, tw, first, count, inv_dv, tab)
    out, bound = np.empty(x.shape), np.empty(x.shape)
    for i in range(u.size):
        w = weights(u, tw, i, first[i], count[i], inv_dv, tab)
        seg = x[:, first[i]:first[i] + count[i]]
        out[:, i] = (seg * w).sum(axis=1) / nm[i]
        bound[:, i] = (2 * count[i] + 8) * 2.0 ** -53 * np.abs(seg * w).sum(axis=1) / nm[i]
    return out, bound


def covers(first, count, j):
    """The outputs whose window holds the input j, [n_lam] bool."""
    return (first <= j) & (j < first + count)


def tile_spans(first, count):
    """(jlo, jhi) per output: the span of its 16-output tile, the union of the tile's
    windows."""
    n = first.size
    jlo, jhi = np.empty(n, int), np.empty(n, int)
    for i0 in range(0, n, 16):
        il = min(i0 + 15, n - 1)
        jlo[i0:i0 + 16] = first[i0]
        jhi[i0:i0 + 16] = first[il] + count[il]
    return jlo, jhi
