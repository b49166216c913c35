"""Time the line-by-line cross-section kernel (K17, frei_xsec_create_lines) in one process.

Shapes: "realistic" — --lines (1e5) lines over 2.5-5 µm, an axis of --points (1.5 M) log-spaced
points, 16 T x 10 p nodes, cutoff 25 cm^-1; "ab" — the same lines and axis on 2 T x 4 p nodes,
where the forms are compared: line parameters from LDS-staged chunks (l) or by scalar loads (s),
pressure tiles of 1, 2 and 4 nodes (FREI_LINES_FORM, read by the library at every call); "small" — 1e3
lines, 1e5 points, one node (so tiles of 1 only), and the NumPy restatement (tests/lines_ref.py) on the
host, the path the kernel replaces, whose time is then scaled to the realistic shape by the
number of Voigt evaluations (scaled, not measured there).

Every measurement is repeated --reps (10) times after one warm-up, the forms taking turns; the
kernel time is the call's own HIP events around the main kernel.  The pre-pass runs on the host
inside the call: what is reported for it is the call's wall time minus the kernel (argument
checks, pre-pass, plan, allocation and uploads together).

Voigt evaluations are counted on the host: per point the lines within the cutoff (the plan's
comparison), times the nodes; per branch from each (T, p, line)'s window |nu - nu0| <
alpha sqrt(64 - y^2) on the axis (|z| < 8; split at y = 1e-3).  The far branch is 96 fp64
operations per evaluation in the source (voigt_far and its call site: 55 fma, 39 mul / add,
2 divisions), 151 flop with an fma as two and a division as one; the roof is the fp64 FMA rate
this probe measures itself in a register-only loop (tools/fma_rate.hip, a child process run
before this one opens the device).  Prints JSON lines; --out appends them to a file.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOP_FAR = 151.0
FORMS = ("l1", "s1", "l2", "s2", "l4", "s4")     # the library's default first


def fma_rate():
    from frei_amd.build import _hipcc
    src, exe = os.path.join(ROOT, "tools", "fma_rate.hip"), os.path.join(ROOT, "tools", "fma_rate")
    if not os.path.exists(exe):
        subprocess.run([_hipcc(), "-O3", "--offload-arch=gfx950", src, "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    rec = json.loads(out.strip().splitlines()[-1])
    return rec["flop_per_s"], rec


def line_list(n, seed):
    import frei_amd as fa
    rng = np.random.default_rng(seed)
    part = (np.array([50.0, 296.0, 1000.0, 4000.0]), np.array([20.0, 108.0, 380.0, 5000.0]))
    return fa.LineList(rng.uniform(2000.0, 4000.0, n), 10.0 ** rng.uniform(-26.0, -19.0, n),
                       rng.uniform(0.0, 5000.0, n), rng.uniform(0.03, 0.1, n),
                       rng.uniform(0.4, 0.8, n), 28.0, partition=part)


def count_evaluations(ll, T, p, wl, cutoff):
    """(total, far, rational, taylor) Voigt evaluations of one call."""
    from tests import lines_ref as R
    nu = R.wavenumbers(wl)[::-1]                       # ascending
    per_point = (np.searchsorted(ll.nu0, nu + cutoff, "right") -
                 np.searchsorted(ll.nu0, nu - cutoff, "left")).sum()
    total = int(per_point) * T.size * p.size
    _, ia, ga = R.line_parameters(ll.nu0, ll.S, ll.E_low, ll.gamma, ll.n_exp, ll.mass, ll.T_ref,
                                  ll.q_ratio(T), T)
    rational = taylor = 0
    for t in range(T.size):
        for pk in p:
            y = ga[t] * pk
            w = np.minimum(np.sqrt(np.maximum(64.0 - y * y, 0.0)) / ia[t], cutoff)
            n = (np.searchsorted(nu, ll.nu0 + w, "right") -
                 np.searchsorted(nu, ll.nu0 - w, "left")) * (y < 8.0)
            taylor += int(n[y < 1e-3].sum())
            rational += int(n[y >= 1e-3].sum())
    return total, total - rational - taylor, rational, taylor


def measure(ll, T, p, wl, cutoff, forms, reps):
    """Per form: kernel ms and the rest of the call's wall ms, `reps` times after a warm-up."""
    ker, rest = {f: [] for f in forms}, {f: [] for f in forms}
    for r in range(-1, reps):
        for f in forms:
            os.environ["FREI_LINES_FORM"] = f
            t0 = time.perf_counter()
            xs = ll.cross_section(T, p, wl, cutoff=cutoff)
            wall = (time.perf_counter() - t0) * 1e3
            if r >= 0:
                ker[f].append(xs.kernel_ms)
                rest[f].append(wall - xs.kernel_ms)
            xs.release()
    os.environ.pop("FREI_LINES_FORM", None)
    return ker, rest


def stats(v):
    return dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lines", type=int, default=100000)
    ap.add_argument("--points", type=int, default=1500000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--skip-realistic", action="store_true")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    out = []

    def emit(rec):
        out.append(json.dumps(rec))
        print(out[-1], flush=True)

    rate, rec = fma_rate()          # a child process, before this one opens the device
    emit(rec)
    from tests import lines_ref as R

    def run(what, ll, T, p, wl, cutoff, forms):
        total, far, rational, taylor = count_evaluations(ll, T, p, wl, cutoff)
        ker, rest = measure(ll, T, p, wl, cutoff, forms, a.reps)
        for f in forms:
            med = float(np.median(ker[f])) * 1e-3
            emit(dict(what=what, form=f, n_line=len(ll), n_hi=int(wl.size), n_T=int(T.size),
                      n_p=int(p.size), cutoff=cutoff, kernel_ms=stats(ker[f]),
                      call_minus_kernel_ms=stats(rest[f]),
                      evaluations=dict(total=total, far=far, rational=rational, taylor=taylor),
                      evaluations_per_s=total / med,
                      far_flop_per_evaluation=FLOP_FAR,
                      fraction_of_measured_fma_rate=total * FLOP_FAR / med / rate))
        return total

    big = line_list(a.lines, 1)
    wl_big = np.exp(np.linspace(np.log(2.5), np.log(5.0), a.points))
    T16, p10 = np.linspace(300.0, 3000.0, 16), 10.0 ** np.linspace(-6.0, 2.0, 10)
    small = line_list(1000, 2)
    wl_small = np.exp(np.linspace(np.log(2.5), np.log(5.0), 100000))
    T1, p1 = np.array([1000.0]), np.array([0.1])

    n_small = run("small", small, T1, p1, wl_small, 25.0, FORMS[:2])   # one node: width 1 only
    t0 = time.perf_counter()
    R.cross_section(small.nu0, small.S, small.E_low, small.gamma, small.n_exp, small.mass,
                    small.T_ref, 25.0, small.q_ratio(T1), T1, p1, wl_small)
    host_s = time.perf_counter() - t0
    run("ab", big, T16[[0, 15]], p10[[0, 3, 6, 9]], wl_big, 25.0, FORMS)
    if not a.skip_realistic:
        n_big = run("realistic", big, T16, p10, wl_big, 25.0, FORMS[:1])
        emit(dict(what="host restatement (NumPy), small shape", seconds=host_s,
                  evaluations=n_small, evaluations_per_s=n_small / host_s,
                  scaled_to_realistic_seconds_not_measured=host_s * n_big / n_small))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
