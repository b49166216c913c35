"""Time the random-overlap mix of k-tables (K19: frei_klib_mix) and the path it replaces.

Workload: K18's probe shape — --n-T (16) x --n-p (10) nodes, bins at R ~ 100 and R ~ 1000 over
2.5-5 um — with seeded k-tables of n_src = 2 and 5 species at n_g = 8, 16, 32 (and 2 and 4, for
the choice of form), mixed for n_comp = 1 and 256 compositions through every kernel form that can
take the n_g (form=, as frei_klib_mix takes it).  Per configuration one warm-up, then --reps
calls; the time is HIP events around the kernel only and the result stays on the device.
Reported: kernel time, pairs sorted per second (items x folds x n_g^2 / time), and for n_g <= 8
the automatic form's choice against the faster measured form, with the run-to-run spread
(max - min over the reps).

Beside it, in the same process, the path a new composition takes without K19 for two species:
frei_xsec_mix + frei_xsec_kdist on the --points (1.5 M) axis at R ~ 1000, n_g = 16, and the bytes
each path keeps resident.  Prints one JSON line per record.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from kdist_probe import log_edges  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--points", type=int, default=1500000)
    ap.add_argument("--n-T", type=int, default=16)
    ap.add_argument("--n-p", type=int, default=10)
    ap.add_argument("--n-comp", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    from frei_amd.binning import CrossSection, KLibrary
    from frei_amd.kdist import gauss_g
    T = np.linspace(500.0, 3000.0, a.n_T)
    p = np.logspace(-6, 2, a.n_p)
    nodes = a.n_T * a.n_p
    rng = np.random.default_rng(19)

    def timed(lib, x, form):
        lib.mix(x, form=form, out=False)
        ms = []
        for _ in range(a.reps):
            lib.mix(x, form=form, out=False)
            ms.append(lib.kernel_ms)
        return ms

    for grid, R in (("R100", 100), ("R1000", 1000)):
        edges = log_edges(2.5, 5.0, R)
        n_bins = edges.size - 1
        for n_g in (2, 4, 8, 16, 32):
            g, w = gauss_g(n_g)
            for n_src in (2, 5):
                tabs = {f"s{k}": np.sort(rng.lognormal(-20.0, 3.0, (a.n_p, a.n_T, n_bins, n_g)),
                                         axis=-1) for k in range(n_src)}
                lib = KLibrary(tabs, edges, g, w, T, p)
                for n_comp in (1, a.n_comp):
                    x = rng.uniform(1e-4, 1e-2, (n_comp, n_src, a.n_T, a.n_p))
                    items = n_comp * nodes * n_bins
                    res = {}
                    for form, name in ((1, "wave"), (2, "block")):
                        if form == 1 and n_g > 8:
                            continue
                        ms = timed(lib, x, form)
                        med = float(np.median(ms))
                        res[name] = (med, max(ms) - min(ms))
                        emit(dict(what="kmix", grid=grid, n_bins=n_bins, n_g=n_g, n_src=n_src,
                                  n_comp=n_comp, nodes=nodes, form=name, items=items,
                                  kernel_ms=dict(median=med, min=min(ms), max=max(ms)),
                                  pairs_per_s=items * (n_src - 1) * n_g * n_g / (med * 1e-3),
                                  resident_bytes=lib.resident_bytes,
                                  result_bytes=8 * items * n_g))
                    if len(res) == 2:
                        best = min(res, key=lambda k: res[k][0])
                        auto = "wave" if n_g <= 2 else "block"     # frei_kmix.hip, kAutoWaveG
                        spread = max(v[1] for v in res.values())
                        emit(dict(what="kmix_auto", grid=grid, n_g=n_g, n_src=n_src,
                                  n_comp=n_comp, auto=auto, best=best,
                                  auto_over_best=res[auto][0] / res[best][0],
                                  auto_minus_best_ms=res[auto][0] - res[best][0],
                                  spread_ms=spread,
                                  slower_than_spread=bool(res[auto][0] - res[best][0] > spread)))
                lib.release()

    # ---- the path one new composition takes without K19: premix, then sort the mixture
    wl = np.exp(np.linspace(np.log(2.5), np.log(5.0), a.points + 2)[1:-1])
    srcs = [CrossSection.synthetic(T, p, wl, seed=s) for s in (1, 2)]
    wgt = rng.uniform(1e-4, 1e-2, (2, a.n_T, a.n_p))
    edges = log_edges(2.5, 5.0, 1000)
    g, w = gauss_g(16)
    mix_ms, sort_ms = [], []
    for k in range(a.reps + 1):
        mixed = CrossSection.mix(srcs, wgt)
        mixed.timing(1)
        mixed.kdist(edges, g, T, p, out=False)
        tot, n = mixed.timing(0)
        if k:
            mix_ms.append(mixed.kernel_ms)
            sort_ms.append(tot / n)
        mixed.release()
    emit(dict(what="premix_path", n_src=2, points=a.points, nodes=nodes, n_bins=edges.size - 1,
              n_g=16, mix_kernel_ms=dict(median=float(np.median(mix_ms)), min=min(mix_ms),
                                         max=max(mix_ms)),
              kdist_kernel_ms=dict(median=float(np.median(sort_ms)), min=min(sort_ms),
                                   max=max(sort_ms)),
              resident_bytes=2 * 4 * nodes * a.points,
              mixture_bytes=4 * nodes * a.points))
    # the same two species through K19: sorted once into the library, then one mix per composition
    lib = KLibrary({"s1": srcs[0], "s2": srcs[1]}, edges, g, w, T, p)
    ms = timed(lib, wgt, 0)
    emit(dict(what="kmix_path", n_src=2, nodes=nodes, n_bins=edges.size - 1, n_g=16,
              kernel_ms=dict(median=float(np.median(ms)), min=min(ms), max=max(ms)),
              resident_bytes=lib.resident_bytes))
    lib.release()
    for s in srcs:
        s.release()


if __name__ == "__main__":
    main()
