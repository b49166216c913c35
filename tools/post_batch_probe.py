"""Time batched post-processing (frei_post_batch) against the per-atmosphere route.

Shape: the per-GPU share of config C5, 32 atmospheres x 60 layers x 100k wavelengths (change it
with --atm / --layers / --lam).  Both routes get the same dtaus arrays from the host and are
timed the same way: HIP events around their kernels on the context's stream (frei_post_timing;
uploads and read-backs excluded) and, beside it, the wall clock of the whole calls.

  batched   one frei_post_batch call: Milne pressures, the three T_eff sums and, with cf, the
            contribution functions of all atmospheres in one launch + the partial-sum launch
  loop      the route without it: one single-atmosphere context, frei_milne_pressure (+
            frei_contribution) once per atmosphere; the weighted means then cost the host
            O(n_atm n_lam) more, which is not counted

Algorithmic bytes of the batched call: dtaus read once, one F_up row and the T rows per
atmosphere, p_milne written, cf written when asked.  Peak HBM bandwidth taken as 8 TB/s.
Prints one JSON line per (route, cf) with the median, minimum and maximum over --repeats runs
after --warmup runs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12


def stats(xs):
    xs = np.asarray(xs, dtype=float)
    return dict(median=float(np.median(xs)), min=float(xs.min()), max=float(xs.max()))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--atm", type=int, default=32)
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--lam", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import frei_amd as fa
    A, nL, n = a.atm, a.layers, a.lam
    rng = np.random.default_rng(11)
    lam = np.logspace(np.log10(0.5), np.log10(10), n)
    p = fa.pressure_grid(n_layers=nL, P_toa=-6, P_boa=np.log10(200))
    Tn = np.array([1000.0, 2000.0])
    tabs = {"1H2-16O": fa.SeparableTable(np.ones(n), np.ones(nL), np.ones(2), p, Tn)}
    # optical depths that grow with pressure, scaled per (atmosphere, wavelength): ascending
    # transmissions whose 2/3 crossing moves from lane to lane (numpy's bisection diverges)
    prof = 10 ** np.linspace(2.0, -6.0, nL)
    dt = (prof[None, :, None] * 10 ** rng.uniform(-1, 1, (A, 1, n))) * \
        rng.uniform(0.5, 1.5, (A, nL, n))
    dt[:, 0, :] = 1.0
    spectra = rng.uniform(1e10, 1e13, (A, n))
    T = rng.uniform(500.0, 3000.0, (A, nL))

    lines = []

    def report(route, cf, ker_ms, wall_ms, nbytes):
        k = stats(ker_ms)
        rec = dict(route=route, cf=bool(cf), n_atm=A, n_layers=nL, n_lam=n,
                   kernel_ms=k, wall_ms=stats(wall_ms), algorithmic_bytes=nbytes,
                   fraction_of_8TBps=nbytes / (k["median"] * 1e-3) / PEAK)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for cf in (False, True):
        nbytes = 8.0 * (A * nL * n + A * (n + nL) + A * n + (A * nL * n if cf else 0))
        # ---- batched
        eng = fa.BatchEngine(lam, p, tabs, g=np.full(A, 1000.0))
        ker, wall = [], []
        for it in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            out = eng.post(dt, spectra, T, want_p_milne=True, want_cf=cf)
            t1 = time.perf_counter()
            if it >= a.warmup:
                ker.append(eng.post_timing())
                wall.append((t1 - t0) * 1e3)
        pm_b = out["p_milne"]
        cf_b0 = out["cf"][0].copy() if cf else None
        del out
        eng.close()
        report("batched", cf, ker, wall, nbytes)
        # ---- the loop over a single-atmosphere context
        single = fa.Engine(lam, p, tabs)
        ker, wall = [], []
        for it in range(a.warmup + a.repeats):
            k_ms = 0.0
            t0 = time.perf_counter()
            for m in range(A):
                pm = single.milne_pressure(p, dt[m])
                k_ms += single.post_timing()
                if cf:
                    c = single.contribution(p, T[m], dt[m])
                    k_ms += single.post_timing()
                if it == 0:   # the two routes compute the same thing
                    assert np.array_equal(pm, pm_b[m])
                    assert not cf or m > 0 or np.array_equal(c, cf_b0)
            t1 = time.perf_counter()
            if it >= a.warmup:
                ker.append(k_ms)
                wall.append((t1 - t0) * 1e3)
        single.close()
        report("loop", cf, ker, wall, nbytes)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
