"""Time the stellar-spectrum binning (K8, frei_sspec_bin) in both forms and find their crossover.

Library: --spectra (64) seeded synthetic spectra on a PHOENIX-like axis — piecewise-constant
spacing over 0.05-5.5 µm, about 1.5 M points — resident on the device as float64.  It is binned
onto log-spaced grids of --bins (500, 100k and 500k) bins over 0.5-10 µm (wavelength_grid), each
with form 1 (one lane per bin) and form 2 (one wave per bin) forced and then with form 0
(automatic).  Per grid every form is warmed once; then the forms alternate over --rounds rounds,
each round repeating the call until about --target-ms of kernel time has run (at most
--max-reps calls).  The time is HIP events around the kernel only (plan upload and read-back
excluded; the result stays on the device).

Algorithmic bytes: 8 P (n_spec + ceil(n_spec / 4)) read — P the points inside the grid, the
wavelength axis once per tile of 4 spectra — plus 8 n_spec n_bins written.  Peak HBM bandwidth
taken as 8 TB/s.  Prints one JSON line per (grid, form) with the median, minimum and maximum
per-call kernel milliseconds over the rounds; the crossover of the automatic rule is read off the
mean points per non-empty bin of the grids where the faster form changes (use more --bins).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12
TILE = 4


def axis():
    seg = [(0.05, 0.3, 2e-6), (0.3, 1.0, 1e-6), (1.0, 2.5, 3e-6), (2.5, 5.5, 1.5e-5)]
    return np.concatenate([lo + d * np.arange(int(round((hi - lo) / d))) for lo, hi, d in seg])


def library(wl, n_spec, seed):
    rng = np.random.default_rng(seed)
    flux = np.empty((n_spec, wl.size))
    for m, T in enumerate(np.linspace(2500.0, 9000.0, n_spec)):
        flux[m] = 1e15 * wl ** -5 / np.expm1(1.4388e4 / (wl * T)) * (0.5 + rng.random(wl.size))
    return flux


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--spectra", type=int, default=64)
    ap.add_argument("--bins", default="500,100000,500000")
    ap.add_argument("--forms", default="1,2,0", help="forms to time, in this order")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=100.0)
    ap.add_argument("--max-reps", type=int, default=100)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import frei_amd as fa
    wl = axis()
    assert np.all(np.diff(wl) > 0)
    lib = fa.StellarSpectra(wl, library(wl, a.spectra, a.seed))
    lines = []
    try:
        for nb in [int(b) for b in a.bins.split(",")]:
            _, wl_bins, _ = fa.wavelength_grid(0.5, 10, nb)
            times = {int(f): [] for f in a.forms.split(",")}
            reps, used = {}, {}
            for form in times:      # warm-up, and how many calls make up the target
                lib.timing(reset=True)
                _, counts = lib.bin(wl_bins, form=form, counts=True, out=False)
                ms, _ = lib.timing(reset=True)
                used[form] = lib.form_used
                reps[form] = int(min(a.max_reps, max(3, np.ceil(a.target_ms / max(ms, 1e-3)))))
            for _ in range(a.rounds):
                for form in times:
                    for _ in range(reps[form]):
                        lib.bin(wl_bins, form=form, out=False)
                    ms, n = lib.timing(reset=True)
                    times[form].append(ms / n)
            P, filled = int(counts.sum()), int((counts > 0).sum())
            nbytes = 8.0 * P * (a.spectra + -(-a.spectra // TILE)) + 8.0 * a.spectra * nb
            for form, xs in times.items():
                med = float(np.median(xs))
                rec = dict(n_bins=nb, form=form, form_used=used[form], n_spec=a.spectra,
                           n_hi=int(wl.size), points_in_grid=P, non_empty_bins=filled,
                           mean_points_per_bin=P / max(filled, 1), reps=reps[form],
                           kernel_ms=dict(median=med, min=float(min(xs)), max=float(max(xs))),
                           algorithmic_bytes=nbytes,
                           fraction_of_8TBps=nbytes / (med * 1e-3) / PEAK)
                lines.append(json.dumps(rec))
                print(lines[-1], flush=True)
    finally:
        lib.release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
