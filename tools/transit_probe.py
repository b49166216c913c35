"""Time the transmission-spectrum kernel (K9, frei_transit) on the dtaus a run left on the device.

Two shapes: one atmosphere of --layers (60) x --single-lam (500k) wavelengths after
Engine.run(n_timesteps=1), and --atm (64) atmospheres of --layers x --batch-lam (100k) after
BatchEngine.run(n_timesteps=1, keep_dtaus=True); synthetic C3 tables of two species (the
opacities only have to leave realistic dtaus behind).  Per shape the call is warmed once, then
repeated until about --target-ms of kernel time has run (at most --max-reps calls), --rounds
times over, with and without the slant optical depths written.  The time is HIP events around
the kernel only (frei_post_timing: uploads of radii and chord weights and the read-back
excluded).

Algorithmic bytes per wavelength and atmosphere: 8 (n_layers - 1) read + 8 written (+ 8
(n_layers - 1) written with tau_slant); arithmetic: (n_layers - 1) n_layers / 2 multiply-add
pairs and n_layers - 1 expm1.  Peak HBM bandwidth taken as 8 TB/s, peak fp64 vector rate as
78.6 TFLOP/s (2 per fused multiply-add: 39.3 T unfused operations per second).  Prints one JSON
line per (shape, tau) with the median, minimum and maximum per-call kernel milliseconds over the
rounds.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BW = 8e12
PEAK_OPS = 39.3e12      # unfused fp64 vector multiplies or adds per second
R_J, R_SUN = 7.1492e9, 6.957e10


def measure(eng, radii, want_tau, a):
    eng.transit(radii, R_SUN, want_tau=want_tau)      # warm-up
    ms = eng.post_timing()
    # with tau_slant every call reads n_layers - 1 rows per wavelength back to the host
    cap = 3 if want_tau else a.max_reps
    reps = int(min(cap, max(3, np.ceil(a.target_ms / max(ms, 1e-3)))))
    xs = []
    for _ in range(a.rounds):
        tot = 0.0
        for _ in range(reps):
            eng.transit(radii, R_SUN, want_tau=want_tau)
            tot += eng.post_timing()
        xs.append(tot / reps)
    return reps, xs


def record(shape, n_atm, nL, n, want_tau, reps, xs):
    med = float(np.median(xs))
    nbytes = 8.0 * n_atm * n * ((nL - 1) + 1 + ((nL - 1) if want_tau else 0))
    ops = float(n_atm) * n * (nL - 1) * nL        # one multiply and one add per (i, j) pair
    t = med * 1e-3
    return dict(shape=shape, n_atm=n_atm, n_layers=nL, n_lam=n, tau_slant=bool(want_tau),
                reps=reps, kernel_ms=dict(median=med, min=float(min(xs)), max=float(max(xs))),
                algorithmic_bytes=nbytes, fraction_of_8TBps=nbytes / t / PEAK_BW,
                multiply_add_ops=ops, fraction_of_fp64_unfused_peak=ops / t / PEAK_OPS)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--single-lam", type=int, default=500_000)
    ap.add_argument("--batch-lam", type=int, default=100_000)
    ap.add_argument("--atm", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=50.0)
    ap.add_argument("--max-reps", type=int, default=50)
    ap.add_argument("--tau", default="0,1", help="0: depth only, 1: with tau_slant, in this order")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import frei_amd as fa
    from frei_amd.constants import G_JUPITER, M_BAR_HOT_JUPITER
    from frei_amd.workloads import c3
    lines = []

    def tables(w):
        return {n: fa.SeparableTable(w["base"][s], w["fp"][s], w["fT"][s], w["p"], w["T_nodes"])
                for s, n in enumerate(w["names"])}

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    nL = a.layers
    taus = [bool(int(t)) for t in a.tau.split(",")]
    if a.single_lam > 0:
        w = c3(n_layers=nL, n_lam=a.single_lam, species=["1H2-16O", "12C-16O"])
        eng = fa.Engine(w["lam"], w["p"], tables(w), g=G_JUPITER, m_bar=M_BAR_HOT_JUPITER,
                        mmr=w["mmr"])
        try:
            out = eng.run(w["T0"], n_timesteps=1)
            radii = fa.level_radii(out["final_T"], w["p"], G_JUPITER, M_BAR_HOT_JUPITER, R_J)
            for want_tau in taus:
                reps, xs = measure(eng, radii, want_tau, a)
                emit(record("single", 1, nL, a.single_lam, want_tau, reps, xs))
        finally:
            eng.close()
    if a.batch_lam > 0:
        w = c3(n_layers=nL, n_lam=a.batch_lam, species=["1H2-16O", "12C-16O"])
        g = np.linspace(800.0, 6000.0, a.atm)
        T0 = np.array([fa.temperature_grid(w["p"], t, 0.1, 0.1)
                       for t in np.linspace(1100.0, 2500.0, a.atm)])
        mmr = np.broadcast_to(w["mmr"], (a.atm,) + w["mmr"].shape)
        eng = fa.BatchEngine(w["lam"], w["p"], tables(w), g=g, mmr=mmr,
                             m_bar=M_BAR_HOT_JUPITER)
        try:
            out = eng.run(T0, n_timesteps=1, keep_dtaus=True)
            radii = np.array([fa.level_radii(out["final_T"][m], w["p"], g[m],
                                             M_BAR_HOT_JUPITER, R_J) for m in range(a.atm)])
            for want_tau in taus:
                reps, xs = measure(eng, radii, want_tau, a)
                emit(record("batched", a.atm, nL, a.batch_lam, want_tau, reps, xs))
        finally:
            eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
