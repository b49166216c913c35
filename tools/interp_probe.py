"""Time the model-grid interpolation kernels (K15, frei_itp_apply), both forms, find the form-0
crossover, and time the host path the kept chain replaces.

Workload: a library of --nodes (256) random spectra of --lam (100k) points; plans of random
nodes and weights for (queries, corners) = (1, 8), (64, 8), (4096, 8), (4096, 2), (4096, 16),
and (64, 16) and (512, 16) for the query count from which the many-corner rule holds.
Per shape every form is warmed once, then the forms take turns for --reps rounds; the time is
HIP events around the kernel only (the plan is uploaded anew for every call; the result is kept
on the device, so there is no read-back).  `spread` is (max - min) / median of a form's calls:
the run-to-run spread the form-0 choice is judged against.

Yardstick, measured here on the same device: the least traffic, 8 n_lam (n_node + n_query)
bytes (the library read once, the output written once), against the HBM rate of a
device-to-device copy of 1 GiB (torch, events, median of 9; 2 bytes moved per byte copied).

Then, in the same process, one sampler step of --path-queries (4096) queries of 8 corners both
ways: on the host NumPy forms the same plan's spectra (acc + w * x per corner) and
Instrument.apply uploads them and returns chi-squares, against ModelGrid.interpolate(keep=True)
followed by Instrument.apply on what was kept.  Wall-clock times of the whole calls.  Prints one
JSON line per record.
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

SHAPES = "1x8,64x8,4096x8,4096x2,4096x16,64x16,512x16"


def stats(v):
    med = float(np.median(v))
    return dict(median=med, min=float(min(v)), max=float(max(v)),
                spread=float((max(v) - min(v)) / med) if med > 0 else 0.0)


def host_interpolate(X, idx, w):
    """The restatement's operations, one corner at a time over all queries."""
    acc = w[:, 0, None] * X[idx[:, 0]]
    for c in range(1, idx.shape[1]):
        acc = acc + w[:, c, None] * X[idx[:, c]]
    return acc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lam", type=int, default=100000)
    ap.add_argument("--nodes", type=int, default=256)
    ap.add_argument("--shapes", default=SHAPES, help="queries x corners, comma-separated")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--path-queries", type=int, default=4096)
    ap.add_argument("--path-reps", type=int, default=2)
    ap.add_argument("--channels", type=int, default=200)
    ap.add_argument("--no-path", action="store_true")
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

    import frei_amd as fa
    from frei_amd.modelgrid import FORMS, automatic_form, tile_width
    forms = (*FORMS, 0)
    rng = np.random.default_rng(15)
    lam = np.exp(np.linspace(np.log(0.5), np.log(10.0), a.lam))
    X = 10 ** rng.uniform(3, 4, (a.nodes, a.lam))
    g = fa.ModelGrid([np.arange(a.nodes, dtype=float)], lam, spectra=X)
    try:
        for shape in [s for s in a.shapes.split(",") if s]:
            Q, C = (int(v) for v in shape.split("x"))
            idx = np.ascontiguousarray(rng.integers(0, a.nodes, (Q, C)), dtype=np.int32)
            w = rng.uniform(0.0, 1.0, (Q, C))
            used, ms = {}, {f: [] for f in forms}
            for f in forms:
                g.interpolate(idx=idx, w=w, form=f, keep=True)
                used[f] = g.form_used
            for _ in range(a.reps):
                for f in forms:
                    g.timing(reset=True)
                    g.interpolate(idx=idx, w=w, form=f, keep=True)
                    ms[f].append(g.timing()[0])
            least = 8.0 * a.lam * (a.nodes + Q)
            med = {f: float(np.median(ms[f])) for f in forms}
            for f in forms:
                emit(dict(what="scan", n_node=a.nodes, n_lam=a.lam, n_query=Q, n_corner=C,
                          form=f, form_used=used[f], tile=tile_width(a.nodes),
                          kernel_ms=stats(ms[f]), least_bytes=least,
                          bytes_per_s=least / (med[f] * 1e-3),
                          fraction_of_measured_copy_rate=least / (med[f] * 1e-3) / hbm))
            fast = min(FORMS, key=lambda f: med[f])
            emit(dict(what="choice", n_query=Q, n_corner=C, faster_form=fast,
                      ratio_slower_over_faster=max(med[f] for f in FORMS) / med[fast],
                      form0_takes=used[0], automatic_form=automatic_form(a.nodes, a.lam, Q, C),
                      form0_over_faster=med[0] / med[fast],
                      spread=max(stats(ms[f])["spread"] for f in forms)))

        if not a.no_path:
            Q, C = a.path_queries, 8
            idx = np.ascontiguousarray(rng.integers(0, a.nodes, (Q, C)), dtype=np.int32)
            w = rng.uniform(0.0, 1.0, (Q, C))
            w /= w.sum(axis=1, keepdims=True)
            edges = np.exp(np.linspace(np.log(0.6), np.log(9.0), a.channels + 1))
            inst = fa.Instrument.top_hat(lam, edges[:-1], edges[1:])
            data = inst.apply(X[0])
            sigma = 0.01 * data
            try:
                kept = g.interpolate(idx=idx, w=w, keep=True)
                _, chi2_dev = inst.apply(kept, data=data, sigma=sigma)
                wall = {k: [] for k in ("host_interpolate", "host_apply_with_upload",
                                        "device_interpolate_keep", "device_apply_kept")}
                for _ in range(a.path_reps):
                    t0 = time.perf_counter()
                    rows = host_interpolate(X, idx, w)
                    t1 = time.perf_counter()
                    _, chi2_host = inst.apply(rows, data=data, sigma=sigma)
                    t2 = time.perf_counter()
                    kept = g.interpolate(idx=idx, w=w, keep=True)
                    t3 = time.perf_counter()
                    _, chi2_dev = inst.apply(kept, data=data, sigma=sigma)
                    t4 = time.perf_counter()
                    del rows          # 3.3 GB returned to the system outside the timed spans
                    for k, v in zip(wall, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                        wall[k].append(1e3 * v)
                med = {k: float(np.median(v)) for k, v in wall.items()}
                host = med["host_interpolate"] + med["host_apply_with_upload"]
                dev = med["device_interpolate_keep"] + med["device_apply_kept"]
                emit(dict(what="path", n_node=a.nodes, n_lam=a.lam, n_query=Q, n_corner=C,
                          n_channels=a.channels, upload_bytes=8 * Q * a.lam,
                          interpolate_form_used=g.form_used,
                          wall_ms={k: stats(v) for k, v in wall.items()},
                          host_path_ms=host, kept_chain_ms=dev, gain=host / dev,
                          upload_and_apply_over_kept_chain=med["host_apply_with_upload"] / dev,
                          chi2_bitwise_equal=bool(np.array_equal(chi2_host, chi2_dev))))
            finally:
                inst.release()
    finally:
        g.release()


if __name__ == "__main__":
    main()
