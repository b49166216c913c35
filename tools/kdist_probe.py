"""Time the premix and the k-distribution kernels (K18: frei_xsec_mix, frei_xsec_kdist).

Workload: a device-generated cross-section on --points (1.5 M) log-spaced points over 2.5-5 um at
--n-T (16) x --n-p (10) nodes, every node a target.  The premix of two such sources, then the
k-distribution at n_g = 16 on three bin grids: R ~ 100 (about 21 600 points per bin), R ~ 1000, and
a fine grid of 32-point bins, each through every kernel form that can take it (FREI_KDIST_FORM,
read by the library at every call).  Per configuration one warm-up, then --reps calls; the time is
HIP events around the kernels only, the result stays on the device.

Yardstick: the least traffic — the premix reads n_src and writes one float32 per point; the
k-distribution reads the selected source rows once at 4 B per point and writes the table once at
8 B per value — against the rate of a device-to-device copy measured here on the same device
(tools/broaden_probe.py hbm_rate).  There is no rate bar: the sort is LDS work, not a stream.

Beside them the path the kernels replace, on a shape small enough to measure (--host-rows nodes of
the same axis at R ~ 1000): CrossSection.values() and np.sort per bin on the host, wall clock,
against the wall clock of CrossSection.kdist with its read-back.  Prints one JSON line per record.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def log_edges(lo, hi, R):
    n = max(int(round(np.log(hi / lo) * R)), 1)
    return np.exp(np.linspace(np.log(lo), np.log(hi), n + 1))


def host_kdist(rows, wl, edges, g):
    """np.sort per bin and the sample, on the host (bins by searchsorted)."""
    start = np.searchsorted(wl, edges[:-1], side="right")
    end = np.searchsorted(wl, edges[1:], side="right")
    out = np.full((rows.shape[0], len(start), g.size), np.nan)
    for k, (a, b) in enumerate(zip(start, end)):
        n = b - a
        if n < 2:
            continue
        s = np.sort(rows[:, a:b], axis=-1).astype(np.float64)
        t = g * n - 0.5
        j = np.clip(np.floor(t), 0, n - 2).astype(np.int64)
        out[:, k] = s[:, j] + np.clip(t - j, 0, 1) * (s[:, j + 1] - s[:, j])
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=1500000)
    ap.add_argument("--n-T", type=int, default=16)
    ap.add_argument("--n-p", type=int, default=10)
    ap.add_argument("--n-g", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    from broaden_probe import hbm_rate
    hbm, rec = hbm_rate()
    emit(rec)

    from frei_amd.binning import CrossSection
    from frei_amd.kdist import gauss_g
    T = np.linspace(500.0, 3000.0, a.n_T)
    p = np.logspace(-6, 2, a.n_p)
    wl = np.exp(np.linspace(np.log(2.5), np.log(5.0), a.points + 2)[1:-1])
    g = gauss_g(a.n_g)[0]
    rows = a.n_T * a.n_p
    srcs = [CrossSection.synthetic(T, p, wl, seed=s) for s in (1, 2)]

    # ---- premix
    w = np.random.default_rng(1).uniform(1e-4, 1e-2, (2, a.n_T, a.n_p))
    ms = []
    for _ in range(a.reps + 1):
        mixed = CrossSection.mix(srcs, w)
        ms.append(mixed.kernel_ms)
        if len(ms) <= a.reps:
            mixed.release()
    ms = ms[1:]
    nbytes = 3 * 4.0 * rows * a.points
    med = float(np.median(ms))
    emit(dict(what="mix", n_src=2, rows=rows, points=a.points,
              kernel_ms=dict(median=med, min=min(ms), max=max(ms)), least_bytes=nbytes,
              bytes_per_s=nbytes / (med * 1e-3),
              fraction_of_measured_copy_rate=nbytes / (med * 1e-3) / hbm))
    for s in srcs:
        s.release()

    # ---- k-distribution
    grids = [("R100", log_edges(2.5, 5.0, 100), ("auto",)),
             ("R1000", log_edges(2.5, 5.0, 1000), ("auto",)),
             ("fine32", np.concatenate([[2.5], (wl[31:-1:32] + wl[32::32]) / 2]),
              ("wave", "block"))]
    for name, edges, forms in grids:
        for form in forms:
            os.environ["FREI_KDIST_FORM"] = form
            _, counts = mixed.kdist(edges, g, T, p, out=False)
            mixed.timing(1)
            for _ in range(a.reps):
                mixed.kdist(edges, g, T, p, out=False)
            tot, n = mixed.timing(0)
            ms_call = tot / n
            n_bins = edges.size - 1
            nbytes = 4.0 * rows * float(counts.sum()) + 8.0 * rows * n_bins * a.n_g
            emit(dict(what="kdist", grid=name, form=form, n_bins=n_bins, n_g=a.n_g, rows=rows,
                      points_per_bin=dict(mean=float(counts.mean()), min=int(counts.min()),
                                          max=int(counts.max())),
                      kernel_ms_mean=ms_call, least_bytes=nbytes,
                      bytes_per_s=nbytes / (ms_call * 1e-3),
                      fraction_of_measured_copy_rate=nbytes / (ms_call * 1e-3) / hbm,
                      keys_per_s=rows * float(counts.sum()) / (ms_call * 1e-3)))
    os.environ.pop("FREI_KDIST_FORM", None)
    mixed.release()

    # ---- the host path it replaces, small
    nT = max(a.host_rows // 2, 1)
    small = CrossSection.synthetic(T[:nT], p[:2], wl, seed=3)
    edges = log_edges(2.5, 5.0, 1000)
    small.kdist(edges, g, T[:nT], p[:2])
    t0 = time.perf_counter()
    dev, _ = small.kdist(edges, g, T[:nT], p[:2])
    t_dev = time.perf_counter() - t0
    t0 = time.perf_counter()
    v = small.values()
    t_read = time.perf_counter() - t0
    t0 = time.perf_counter()
    host = host_kdist(v.reshape(-1, wl.size), wl, edges, g)
    t_sort = time.perf_counter() - t0
    same = bool(np.array_equal(host.reshape(nT, 2, -1, a.n_g).transpose(1, 0, 2, 3)[:, :, :-1],
                               dev[:, :, :-1], equal_nan=True))
    emit(dict(what="host_path", rows=2 * nT, points=a.points, n_bins=edges.size - 1, n_g=a.n_g,
              device_wall_ms=1e3 * t_dev, host_values_wall_ms=1e3 * t_read,
              host_sort_wall_ms=1e3 * t_sort, host_over_device=(t_read + t_sort) / t_dev,
              same_values=same))
    small.release()


if __name__ == "__main__":
    main()
