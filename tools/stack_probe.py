"""Time the orbital stack (K14, frei_stack_apply) against the two paths it stands beside.

Shapes (--shapes): "headline" — 64 atmospheres x 64 exposures x 401 velocities stacked onto 301
K_p x 401 V_sys — and "small" — 1 x 8 x 41 onto 31 x 41.  Per shape, in one process:
  correlate    CrossCorrelator.correlate(x, keep=True, want=()) of random templates on --lam
               (500k) native points against --pix (40 960) pixels: its kernel time (HIP events
               around the kernels only), the first yardstick;
  stack        OrbitStack.stack(values) of the log-likelihood as a host array: the stack kernel
               alone (statistic 0);
  statistic + stack    OrbitStack.stack(res, "loglike") from the kept sums and from the host
               sums: both kernels; the statistic's time is the difference of the medians;
  bytes        the stack's time against the bytes it must write, 8 n_atm n_kp n_vsys, at the
               rate of a device-to-device copy of 1 GiB measured here (2 bytes moved per byte
               copied);
  host         the wall time of frei_amd.kp_vsys_map on the same values, the second yardstick
               (--host-atm atmospheres of them, 2 by default, and the time per atmosphere
               scaled to the batch: the loop is linear in the atmospheres).
Everything is warmed once, then the device calls take turns for --reps rounds; medians and
spread.  The condition of the design: at the headline shape statistic + stack
take less kernel time than correlate.  Prints one JSON line per record.
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

SHAPES = {"headline": dict(n_atm=64, n_exp=64, n_vel=401, n_kp=301, n_vsys=401),
          "small": dict(n_atm=1, n_exp=8, n_vel=41, n_kp=31, n_vsys=41)}


def stats(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="headline,small")
    ap.add_argument("--lam", type=int, default=500000)
    ap.add_argument("--pix", type=int, default=40960)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-atm", type=int, default=2)
    ap.add_argument("--no-host", action="store_true")
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
    from frei_amd.stack import FORMS
    for name in [s for s in a.shapes.split(",") if s]:
        sh = SHAPES[name]
        A, E, V, K, S = (sh[k] for k in ("n_atm", "n_exp", "n_vel", "n_kp", "n_vsys"))
        rng = np.random.default_rng(14)
        lam = np.exp(np.linspace(np.log(1.0), np.log(1.05), a.lam))
        wl = np.sort(rng.uniform(1.005, 1.045, a.pix))
        vel = np.linspace(-200.0, 200.0, V)
        x = rng.normal(0.0, 0.1, (A, a.lam))
        x -= x.mean(axis=1, keepdims=True)
        flux = 1.0 + rng.normal(0.0, 0.05, (E, a.pix))
        phases = np.linspace(0.30, 0.70, E)
        Kp, Vsys = np.linspace(0.0, 150.0, K), np.linspace(-50.0, 50.0, S)
        cc = fa.CrossCorrelator(lam, wl, flux, vel)
        st = fa.OrbitStack(vel, Kp, Vsys, phases=phases)
        try:
            host = cc.correlate(x)                               # the sums on the host
            values = host.loglike()
            kept = cc.correlate(x, keep=True, want=())
            ref = st.stack(kept, "loglike")
            assert np.array_equal(ref, st.stack(host, "loglike"))
            for f in FORMS:
                assert np.array_equal(st.stack(kept, "loglike", form=f), ref)
            ms = dict(correlate=[], stack=[], statistic_stack_kept=[], statistic_stack_host=[],
                      stack_form2=[])
            wall = dict(stack_kept=[], stack_host=[])
            for _ in range(a.reps):
                cc.timing(reset=True)
                kept = cc.correlate(x, keep=True, want=())
                ms["correlate"].append(cc.timing()[0])
                for key, arg, kw in (("stack", values, {}),
                                     ("stack_form2", values, dict(form=2)),
                                     ("statistic_stack_kept", kept, dict(statistic="loglike")),
                                     ("statistic_stack_host", host, dict(statistic="loglike"))):
                    st.timing(reset=True)
                    t0 = time.perf_counter()
                    st.stack(arg, **kw)
                    dt = 1e3 * (time.perf_counter() - t0)
                    ms[key].append(st.timing()[0])
                    if key == "statistic_stack_kept":
                        wall["stack_kept"].append(dt)
                    if key == "statistic_stack_host":
                        wall["stack_host"].append(dt)
            med = {k: float(np.median(v)) for k, v in ms.items()}
            out_bytes = 8.0 * A * K * S
            rec = dict(what="stack", shape=name, **sh, n_lam=a.lam, n_pix=a.pix, reps=a.reps,
                       correlate_form=cc.form_used, stack_form=1,
                       kernel_ms={k: stats(v) for k, v in ms.items()},
                       statistic_ms_by_difference=med["statistic_stack_kept"] - med["stack"],
                       wall_ms={k: stats(v) for k, v in wall.items()},
                       interpolations=float(A) * K * S * E,
                       interpolations_per_s=float(A) * K * S * E / (med["stack"] * 1e-3),
                       map_bytes=out_bytes, map_write_ms_at_copy_rate=out_bytes / hbm * 1e3,
                       stack_over_map_write=med["stack"] / (out_bytes / hbm * 1e3),
                       statistic_stack_over_correlate=med["statistic_stack_kept"] /
                       med["correlate"],
                       condition_met=bool(med["statistic_stack_kept"] < med["correlate"]))
            if not a.no_host:
                n = min(a.host_atm, A)
                t0 = time.perf_counter()
                hmap = fa.kp_vsys_map(values[:n], vel, phases, Kp, Vsys)
                dt = time.perf_counter() - t0
                scale = float(np.max(np.abs(hmap)))
                rec.update(host_kp_vsys_map=dict(
                    n_atm=n, wall_s=dt, wall_s_scaled_to_batch=dt * A / n,
                    max_abs_difference_from_device_over_max=float(
                        np.max(np.abs(hmap - st.stack(values[:n]))) / scale),
                    device_wall_ms_over_host_scaled=float(
                        np.median(wall["stack_kept"]) / (1e3 * dt * A / n))))
            emit(rec)
        finally:
            st.release()
            cc.release()


if __name__ == "__main__":
    main()
