"""Time the broadening kernels (K13, frei_brd_apply), both forms, and find the form-0 threshold.

Workload: --lam (500k) log-spaced native points over 0.5-10 um; for every window width of
--widths (9, 33, 129, 513 points) a bell-shaped table of that half-width, and for every
atmosphere count of --atm (1, 4, 8, 16, 64) random spectra.  Per configuration every form is
warmed once, then the forms take turns for --reps rounds; the time is HIP events around the
kernel only (x is uploaded anew for every call; the result is kept on the device, so there is no
read-back).

Two yardsticks, both measured here on the same device:
  bytes: the least traffic, 16 n_atm n_lam (x read once, out written once) + 32 n_lam (u, tw,
    norm, first, count), against the HBM rate of a device-to-device copy of 1 GiB (torch, CUDA
    events, median of 9; 2 bytes moved per byte copied);
  FLOP: 2 n_atm sum_i count_i (the multiply-adds of the definition; forming the weights is not
    counted), against the fp64 FMA rate of tools/fma_rate.hip (a register-only loop, built on
    first use, run as a child process before this process opens the device).
Then the only way to do this work without K13: Instrument.gaussian(lam, centres=lam,
resolving_power=R).apply(x) with R giving the --inst-width (129) window, on --inst-atm (64)
atmospheres of the same x: its plan's size, its kernel ms and the wall-clock time of the call
(upload, kernel, read-back of the result), against Broadening.apply(x) (upload, kernel,
read-back) and Broadening.apply(x, keep=True) of a Gaussian table of the same width.  Prints one
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


def hbm_rate():
    """Bytes per second moved by a device-to-device copy of 1 GiB, and its record."""
    import torch
    n = 1 << 27
    a = torch.empty(n, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    a.fill_(1.0)
    b.copy_(a)
    ms = []
    for _ in range(9):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    del a, b
    torch.cuda.empty_cache()
    med = float(np.median(ms))
    rate = 2.0 * 8.0 * n / (med * 1e-3)
    return rate, dict(what="hbm_rate", copy_bytes=8 * n, ms=dict(median=med, min=min(ms),
                                                                max=max(ms)),
                      bytes_per_s=rate)


def bell(fa, half_width_kms, h=64):
    k = np.arange(-h, h + 1)
    return fa.BroadeningKernel(half_width_kms / h, np.exp(-0.5 * (k / (0.25 * h)) ** 2))


def measure(b, x, forms, reps):
    used, xs = {}, {f: [] for f in forms}
    for f in forms:
        b.apply(x, form=f, keep=True)
        used[f] = b.form_used
    for _ in range(reps):
        for f in forms:
            b.timing(reset=True)
            b.apply(x, form=f, keep=True)
            xs[f].append(b.timing()[0])
    return used, xs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lam", type=int, default=500000)
    ap.add_argument("--atm", default="1,4,8,16,64")
    ap.add_argument("--widths", default="9,33,129,513")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inst-width", type=int, default=129)
    ap.add_argument("--inst-atm", type=int, default=64)
    ap.add_argument("--no-instrument", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(lines[-1] + "\n")

    from crosscorr_probe import SPEC_SHEET_FP64, fma_rate
    fma, rec = fma_rate()           # a child process, before this one opens the device
    rec["spec_sheet_flop_per_s_not_measured"] = SPEC_SHEET_FP64
    emit(rec)
    hbm, rec = hbm_rate()
    emit(rec)

    import frei_amd as fa
    from frei_amd.broaden import C_KMS, FORMS
    forms = (*FORMS, 0)
    rng = np.random.default_rng(13)
    lam = np.exp(np.linspace(np.log(0.5), np.log(10.0), a.lam))
    step = C_KMS * (np.log(10.0) - np.log(0.5)) / (a.lam - 1)
    atm = [int(v) for v in a.atm.split(",") if v]
    x_all = 10 ** rng.uniform(3, 4, (max(atm + [a.inst_atm]), a.lam))

    for width in [int(v) for v in a.widths.split(",") if v]:
        b = fa.Broadening(lam, bell(fa, (0.5 * (width - 1) + 0.5) * step))
        taps = int(b.count.astype(np.int64).sum())
        try:
            for n_atm in atm:
                x = np.ascontiguousarray(x_all[:n_atm])
                used, xs = measure(b, x, forms, a.reps)
                flop = 2.0 * n_atm * taps
                nbytes = 16.0 * n_atm * a.lam + 32.0 * a.lam
                for f in forms:
                    med = float(np.median(xs[f]))
                    emit(dict(what="scan", n_lam=a.lam, width=width,
                              interior_count=int(b.count[a.lam // 2]), n_atm=n_atm, form=f,
                              form_used=used[f],
                              kernel_ms=dict(median=med, min=float(min(xs[f])),
                                             max=float(max(xs[f]))),
                              flop=flop, flop_per_s=flop / (med * 1e-3),
                              fraction_of_measured_fma_rate=flop / (med * 1e-3) / fma,
                              least_bytes=nbytes, bytes_per_s=nbytes / (med * 1e-3),
                              fraction_of_measured_hbm_rate=nbytes / (med * 1e-3) / hbm))
        finally:
            b.release()

    if not a.no_instrument:
        # FWHM such that 4 standard deviations either side span the window
        half = (0.5 * (a.inst_width - 1) + 0.5) * step
        fwhm = half / 4.0 * 2.0 * np.sqrt(2.0 * np.log(2.0))
        x = np.ascontiguousarray(x_all[:a.inst_atm])
        t0 = time.perf_counter()
        inst = fa.Instrument.gaussian(lam, centres=lam, resolving_power=C_KMS / fwhm)
        t_plan = time.perf_counter() - t0
        b = fa.Broadening(lam, fa.BroadeningKernel.gaussian(fwhm_kms=fwhm))
        try:
            inst.apply(x)
            b.apply(x)
            wall = {"instrument": [], "broadening": [], "broadening_keep": []}
            kern = {"instrument": [], "broadening": []}
            for _ in range(a.reps):
                inst.timing(reset=True)
                t0 = time.perf_counter()
                inst.apply(x)
                wall["instrument"].append(1e3 * (time.perf_counter() - t0))
                kern["instrument"].append(inst.timing()[0])
                b.timing(reset=True)
                t0 = time.perf_counter()
                b.apply(x)
                wall["broadening"].append(1e3 * (time.perf_counter() - t0))
                kern["broadening"].append(b.timing()[0])
                t0 = time.perf_counter()
                b.apply(x, keep=True)
                wall["broadening_keep"].append(1e3 * (time.perf_counter() - t0))
            med = {k: float(np.median(v)) for k, v in wall.items()}
            emit(dict(what="instrument_path", n_lam=a.lam, n_atm=a.inst_atm,
                      instrument_mean_points=float(inst.count.mean()),
                      broadening_interior_count=int(b.count[a.lam // 2]),
                      instrument_plan_bytes=int(inst.weights.nbytes + inst.first.nbytes +
                                                inst.count.nbytes),
                      instrument_plan_build_s=t_plan,
                      broadening_plan_bytes=int(32 * a.lam + b.tab.nbytes),
                      spectra_bytes=int(x.nbytes), broadening_form_used=b.form_used,
                      kernel_ms={k: dict(median=float(np.median(v)), min=float(min(v)),
                                         max=float(max(v))) for k, v in kern.items()},
                      wall_ms={k: dict(median=med[k], min=float(min(v)), max=float(max(v)))
                               for k, v in wall.items()},
                      wall_ratio_instrument_over_broadening=med["instrument"] / med["broadening"],
                      kernel_ratio_instrument_over_broadening=float(
                          np.median(kern["instrument"]) / np.median(kern["broadening"]))))
        finally:
            inst.release()
            b.release()


if __name__ == "__main__":
    main()
