"""Time the Doppler cross-correlation kernels (K12, frei_ccf_apply), both forms, and find the
form-0 threshold.

Workload: --atm (64) atmospheres x --lam (500k) log-spaced native points over 0.5-10 um;
--orders (20) spectral orders of --order-pix (2048) pixels inside 1-2.5 um (40 960 pixels);
--exp (64) exposures; --vel (401) velocities over +-200 km/s (a plan of 197 MB).  Then the
small-problem corner (1 atmosphere, 8 exposures, 41 velocities) and a scan over the number of
exposures (--scan, at 8 atmospheres x 101 velocities), which is where the forms cross: the MFMA
form spends a whole 16-exposure block on however few exposures there are.  Per configuration
every form is warmed once, then the forms take turns for --reps rounds; the time is HIP events
around the kernels only (uploads and the read-back excluded; x is uploaded anew for every call).

FLOP/s = 2 n_atm n_vel n_pix (n_exp + 2) / t.  The yardstick is the fp64 FMA rate this probe
measures itself on the same device with a register-only loop (tools/fma_rate.hip, built on first
use, run as a child process before this process opens the device); the spec-sheet figure is
printed beside it and marked as not measured.  Prints one JSON line per configuration and form
with the median, minimum and maximum kernel milliseconds.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SPEC_SHEET_FP64 = 78.6e12      # FLOP/s, vector and matrix alike; not measured here


def fma_rate():
    """The device's measured fp64 rate (FLOP/s) from tools/fma_rate, and its JSON record."""
    from frei_amd.build import _hipcc
    src, exe = os.path.join(ROOT, "tools", "fma_rate.hip"), os.path.join(ROOT, "tools", "fma_rate")
    if not os.path.exists(exe):
        subprocess.run([_hipcc(), "-O3", "--offload-arch=gfx950", src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rec = json.loads(out.strip().splitlines()[-1])
    return rec["flop_per_s"], rec


def pixels(orders, per_order, lo=1.0, hi=2.5):
    """`orders` spectral orders back to back, each `per_order` pixels linear in wavelength,
    neighbours overlapping by 5 % of their span."""
    edges = np.exp(np.linspace(np.log(lo), np.log(hi), orders + 1))
    wl = []
    for k in range(orders):
        span = edges[k + 1] - edges[k]
        wl.append(np.linspace(edges[k], min(edges[k + 1] + 0.05 * span, hi), per_order))
    return np.concatenate(wl)


def measure(cc, x, forms, reps):
    """Kernel milliseconds per form, the forms taking turns call by call (so a drift of the
    machine falls on all of them alike) after one warm-up call each."""
    used, xs = {}, {f: [] for f in forms}
    for f in forms:
        cc.correlate(x, form=f)
        used[f] = cc.form_used
    for _ in range(reps):
        for f in forms:
            cc.timing(reset=True)
            cc.correlate(x, form=f)
            xs[f].append(cc.timing()[0])
    return used, xs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--atm", type=int, default=64)
    ap.add_argument("--lam", type=int, default=500000)
    ap.add_argument("--orders", type=int, default=20)
    ap.add_argument("--order-pix", type=int, default=2048)
    ap.add_argument("--exp", type=int, default=64)
    ap.add_argument("--vel", type=int, default=401)
    ap.add_argument("--scan", default="1,4,8,16,20,24,32")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    rate, rec = fma_rate()          # a child process, before this one opens the device
    rec["spec_sheet_flop_per_s_not_measured"] = SPEC_SHEET_FP64
    emit(rec)

    import frei_amd as fa
    from frei_amd.crosscorr import FORMS
    forms = (*FORMS, 0)
    rng = np.random.default_rng(12)
    lam = np.exp(np.linspace(np.log(0.5), np.log(10.0), a.lam))
    wl = pixels(a.orders, a.order_pix)
    w = rng.uniform(0.5, 1.5, wl.size)

    def run(what, n_atm, n_exp, n_vel):
        x = 1e-3 * rng.uniform(0.4, 1.0, (n_atm, a.lam))
        flux = rng.normal(0.0, 1e-4, (n_exp, wl.size))
        vel = np.linspace(-200.0, 200.0, n_vel)
        cc = fa.CrossCorrelator(lam, wl, flux, vel, weights=w)
        try:
            used, xs = measure(cc, x, forms, a.reps)
        finally:
            cc.release()
        flop = 2.0 * n_atm * n_vel * wl.size * (n_exp + 2)
        for f in forms:
            med = float(np.median(xs[f]))
            emit(dict(what=what, n_atm=n_atm, n_lam=a.lam, n_pix=int(wl.size), n_exp=n_exp,
                      n_vel=n_vel, plan_bytes=12 * n_vel * int(wl.size), form=f,
                      form_used=used[f],
                      kernel_ms=dict(median=med, min=float(min(xs[f])), max=float(max(xs[f]))),
                      flop=flop, flop_per_s=flop / (med * 1e-3),
                      fraction_of_measured_fma_rate=flop / (med * 1e-3) / rate,
                      fraction_of_spec_sheet_not_measured=flop / (med * 1e-3) / SPEC_SHEET_FP64))

    run("workload", a.atm, a.exp, a.vel)
    run("small", 1, 8, 41)
    for n_exp in [int(v) for v in a.scan.split(",") if v]:
        run("scan", 8, n_exp, 101)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
