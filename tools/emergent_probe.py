"""Time the emergent-intensity kernel (K11, frei_emergent) on the dtaus a run left on the device.

Two shapes: one atmosphere of --layers (60) x --single-lam (500k) wavelengths after
Engine.run(n_timesteps=1), and --atm (64) atmospheres of --layers x --batch-lam (100k) after
BatchEngine.run(n_timesteps=1, keep_dtaus=True); synthetic C3 tables of two species (the
opacities only have to leave realistic dtaus behind).  Per shape and per --n-mu (1, 4, 8, 16
Gauss angles), with the flux alone and with the intensities written too, the call is warmed
once, then repeated until about --target-ms of kernel time has run (at most --max-reps calls),
--rounds times over.  The time is HIP events around the kernel only (frei_post_timing: uploads
and the read-back excluded).

Algorithmic bytes per wavelength and atmosphere: 8 (n_layers - 1) read + 8 written (+ 8 n_mu
written with the intensities); the column's re-reads by further angle tiles are not counted.
Exponentials: one per (shell, angle) and one Planck exponential per shell and angle tile of 8.
Peak HBM bandwidth taken as 8 TB/s.  Prints one JSON line per (shape, n_mu, intensity) with the
median, minimum and maximum per-call kernel milliseconds over the rounds.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BW = 8e12
TILE = 8                # angles per pass of the kernel (frei_emergent.hip kTile)


def measure(eng, T, mu, w, want_int, a):
    eng.emergent(T, mu, w, want_intensity=want_int)      # warm-up
    ms = eng.post_timing()
    # with the intensities every call reads n_mu rows per wavelength back to the host
    cap = 3 if want_int else a.max_reps
    reps = int(min(cap, max(3, np.ceil(a.target_ms / max(ms, 1e-3)))))
    xs = []
    for _ in range(a.rounds):
        tot = 0.0
        for _ in range(reps):
            eng.emergent(T, mu, w, want_intensity=want_int)
            tot += eng.post_timing()
        xs.append(tot / reps)
    return reps, xs


def record(shape, n_atm, nL, n, n_mu, want_int, reps, xs):
    med = float(np.median(xs))
    nbytes = 8.0 * n_atm * n * ((nL - 1) + 1 + (n_mu if want_int else 0))
    passes = -(-n_mu // TILE)
    exps = float(n_atm) * n * (nL - 1) * (n_mu + passes)
    t = med * 1e-3
    return dict(shape=shape, n_atm=n_atm, n_layers=nL, n_lam=n, n_mu=n_mu,
                intensity=bool(want_int), reps=reps,
                kernel_ms=dict(median=med, min=float(min(xs)), max=float(max(xs))),
                algorithmic_bytes=nbytes, fraction_of_8TBps=nbytes / t / PEAK_BW,
                exponentials=exps, exponentials_per_s=exps / t)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--single-lam", type=int, default=500_000)
    ap.add_argument("--batch-lam", type=int, default=100_000)
    ap.add_argument("--atm", type=int, default=64)
    ap.add_argument("--n-mu", default="1,4,8,16")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=50.0)
    ap.add_argument("--max-reps", type=int, default=50)
    ap.add_argument("--intensity", default="0,1",
                    help="0: flux only, 1: with the intensities, in this order")
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
    n_mus = [int(k) for k in a.n_mu.split(",")]
    ints = [bool(int(t)) for t in a.intensity.split(",")]

    def sweep(eng, shape, n_atm, n, T):
        for n_mu in n_mus:
            mu, w = fa.gauss_angles(n_mu)
            for want_int in ints:
                reps, xs = measure(eng, T, mu, w, want_int, a)
                emit(record(shape, n_atm, nL, n, n_mu, want_int, reps, xs))

    if a.single_lam > 0:
        w = c3(n_layers=nL, n_lam=a.single_lam, species=["1H2-16O", "12C-16O"])
        eng = fa.Engine(w["lam"], w["p"], tables(w), g=G_JUPITER, m_bar=M_BAR_HOT_JUPITER,
                        mmr=w["mmr"])
        try:
            out = eng.run(w["T0"], n_timesteps=1)
            sweep(eng, "single", 1, a.single_lam, out["final_T"])
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
            sweep(eng, "batched", a.atm, a.batch_lam, out["final_T"])
        finally:
            eng.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
