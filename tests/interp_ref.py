"""Plain NumPy restatement of K15's two definitions (include/frei_hip.h, frei_itp_apply, and
frei_amd.modelgrid.ModelGrid.plan): the multilinear plan, one query and one axis at a time, and
the weighted sum, one corner at a time.  Device results are compared with these bit for bit:
both sides run the same IEEE multiplies and adds in the same order (NumPy fuses nothing)."""
import numpy as np


def plan(axes, theta):
    """(idx int32 [n_query][2^d_eff], w float64 [n_query][2^d_eff], n_outside) of the queries
    ``theta`` [n_query][d] on the ascending ``axes``; axes of one node take no part."""
    axes = [np.asarray(g, dtype=np.float64) for g in axes]
    theta = np.asarray(theta, dtype=np.float64)
    if np.any(np.isnan(theta)):
        raise ValueError("NaN coordinate")
    part = [a for a, g in enumerate(axes) if g.size > 1]
    d_eff = len(part)
    stride = [1] * len(axes)
    for a in range(len(axes) - 2, -1, -1):
        stride[a] = stride[a + 1] * axes[a + 1].size
    Q = theta.shape[0]
    idx = np.zeros((Q, 1 << d_eff), dtype=np.int32)
    w = np.zeros((Q, 1 << d_eff), dtype=np.float64)
    n_outside = 0
    for q in range(Q):
        j, t = {}, {}
        for a in part:
            g = axes[a]
            th = theta[q, a]
            if th < g[0] or th > g[-1]:
                n_outside += 1
            th = min(max(th, g[0]), g[-1])
            k = 0
            while k + 1 < g.size and g[k + 1] <= th:
                k += 1
            k = min(k, g.size - 2)
            j[a] = k
            t[a] = (th - g[k]) / (g[k + 1] - g[k])
        for c in range(1 << d_eff):
            node, weight = 0, None
            for pos, a in enumerate(part):
                up = (c >> (d_eff - 1 - pos)) & 1
                node += (j[a] + up) * stride[a]
                f = t[a] if up else np.float64(1.0) - t[a]
                weight = f if weight is None else weight * f
            idx[q, c] = node
            w[q, c] = 1.0 if weight is None else weight
    return idx, w, n_outside


def interpolate(X, idx, w):
    """out[q][i] = sum_c w[q][c] X[idx[q][c]][i]: the corners ascending, acc + w * x."""
    X = np.asarray(X, dtype=np.float64)
    out = np.empty((idx.shape[0], X.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for q in range(idx.shape[0]):
            acc = w[q, 0] * X[idx[q, 0]]
            for c in range(1, idx.shape[1]):
                acc = acc + w[q, c] * X[idx[q, c]]
            out[q] = acc
    return out


def same_bits(a, b):
    """True when the float64 arrays agree bit for bit, NaNs matching NaNs of any payload."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a)
    if not np.array_equal(nan, np.isnan(b)):
        return False
    return np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


def dyadic_case(shape, n_lam=70, seed=15):
    """A function multilinear in theta on a dyadic grid, built from dyadic numbers so that every
    operation of plan and sum is exact: axes of integers, coefficients k / 8 with |k| <= 16,
    queries at multiples of 1/4 -> (axes, X [n_node][n_lam], theta [n_query][d], exact
    [n_query][n_lam])."""
    rng = np.random.default_rng(seed)
    d = len(shape)
    axes = [np.cumsum(rng.choice([1.0, 2.0, 4.0], size=n)) for n in shape]
    # f(theta)[i] = sum over subsets S of the axes of coef[S][i] prod_{a in S} theta_a
    coef = rng.integers(-16, 17, size=(1 << d, n_lam)) / 8.0

    def f(pts):
        out = np.zeros((pts.shape[0], n_lam))
        for s in range(1 << d):
            mono = np.ones(pts.shape[0])
            for a in range(d):
                if (s >> a) & 1:
                    mono = mono * pts[:, a]
            out += mono[:, None] * coef[s][None, :]
        return out
    nodes = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, d)
    theta = np.stack([rng.integers(int(g[0]) * 4, int(g[-1]) * 4 + 1, size=9) / 4.0
                      for g in axes], axis=1)
    return axes, f(nodes), theta, f(theta)
