"""Time the synthetic-observation kernel (K10, frei_obs_apply) and find its form crossover.

Workload: --atm (64) atmospheres x 100k and x 500k wavelengths of positive random spectra;
instruments of back-to-back channels of 4, 32, 300 and 3000 points covering the axis, with and
without a one-row `den` library (the eclipse depth against the flux mean), each with form 1 (one
lane per channel) and form 2 (one group of lanes per channel).  Then the crossover scan: channels
of --scan points (2 .. 8) at the smaller size, both forms.  Per configuration every form is
warmed once, then the forms take turns for --reps rounds; the time is HIP events around the
kernels only (uploads and the read-back excluded; x is uploaded anew for every call, so no call
finds it in a cache).

Algorithmic bytes: every covered element of x, num and den once, the weights and the plan once
per tile of 4 atmospheres, obs written once.  Peak HBM bandwidth taken as 8 TB/s.  Prints one
JSON line per configuration with the median, minimum and maximum kernel milliseconds.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BW = 8e12
TILE = 4


def measure(inst, x, den, forms, reps):
    """Kernel milliseconds per form, the forms taking turns call by call (so a drift of the
    machine falls on all of them alike) after one warm-up call each."""
    used, xs = {}, {f: [] for f in forms}
    for f in forms:
        inst.apply(x, den=den, form=f)
        used[f] = inst.form_used
    for _ in range(reps):
        for f in forms:
            inst.timing(reset=True)
            inst.apply(x, den=den, form=f)
            xs[f].append(inst.timing()[0])
    return used, xs


def record(what, n_atm, n_lam, points, with_den, form, used, xs):
    K = n_lam // points
    cov = K * points
    tiles = -(-n_atm // TILE)
    nbytes = 8.0 * (n_atm * cov + (cov if with_den else 0) + tiles * (cov + 3 * K) + n_atm * K)
    med = float(np.median(xs))
    return dict(what=what, n_atm=n_atm, n_lam=n_lam, points_per_channel=points, channels=K,
                den=bool(with_den), form=form, form_used=used,
                kernel_ms=dict(median=med, min=float(min(xs)), max=float(max(xs))),
                algorithmic_bytes=nbytes, fraction_of_8TBps=nbytes / (med * 1e-3) / PEAK_BW)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--atm", type=int, default=64)
    ap.add_argument("--lam", default="100000,500000")
    ap.add_argument("--points", default="4,32,300,3000")
    ap.add_argument("--scan", default="2,3,4,5,6,8")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import frei_amd as fa
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def instrument(lam, points):
        K = lam.size // points
        first = np.arange(K, dtype=np.int64) * points
        w = np.random.default_rng(points).uniform(0.1, 1.0, K * points)
        return fa.Instrument(lam, first, np.full(K, points), w)

    sizes = [int(v) for v in a.lam.split(",") if v]
    rng = np.random.default_rng(10)
    for i, n_lam in enumerate(sizes):
        lam = np.linspace(0.5, 10.0, n_lam)
        x = 10 ** rng.uniform(3, 5, (a.atm, n_lam))
        star = 10 ** rng.uniform(5, 7, n_lam)
        plan = [("rate", int(p)) for p in a.points.split(",") if p]
        if i == 0:
            plan += [("scan", int(p)) for p in a.scan.split(",") if p]
        for what, points in plan:
            inst = instrument(lam, points)
            try:
                # a lane walking thousands of points is not a candidate
                forms = (2, 0) if points > 300 else (1, 2, 0)
                for with_den in ((False, True) if what == "rate" else (False,)):
                    used, xs = measure(inst, x, star if with_den else None, forms, a.reps)
                    for form in forms:
                        emit(record(what, a.atm, n_lam, points, with_den, form, used[form],
                                    xs[form]))
            finally:
                inst.release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
