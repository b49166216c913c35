"""Time a batch of correlated-k atmospheres, one composition each (K20), and the path it replaces.

Workload: --n-p (60) layers on the library's 60 pressure nodes x --n-T (16) temperature nodes,
bins at R ~ 1000 over 2.5-5 um, n_g = 16, --n-atm (64) atmospheres, seeded k-tables of n_src = 2
and 5 species.  In one process, after a warm-up of each step, host clock around calls that end in
a stream synchronisation:
  fill:     frei_set_table_kmix_batch (species 0's table, the metadata build and the K19 mix of
            every atmosphere's used rows into the per-atmosphere tables);
  set_mix:  BatchEngine.set_mix of all atmospheres (frei_kmix_batch_update: the mix alone);
  run:      BatchEngine.run of --iters (10) T-P iterations, convergence off;
  single:   the path this replaces, per composition: KGrid.set_mix (the context is torn down),
            then KGrid.emission_spectrum of the same iterations on a new context
            (frei_set_table_kmix), for --n-single (4) of the compositions; the figure for the
            whole batch is that mean times n_atm, and is labelled as projected.
Also reported: the bytes of the per-atmosphere tables, n_atm * n_p * n_T * pitch * 8.
Prints one JSON line per record.
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

from kdist_probe import log_edges  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n-T", type=int, default=16)
    ap.add_argument("--n-p", type=int, default=60)
    ap.add_argument("--n-atm", type=int, default=64)
    ap.add_argument("--n-g", type=int, default=16)
    ap.add_argument("--R", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n-single", type=int, default=4)
    ap.add_argument("--n-src", type=int, nargs="+", default=[2, 5])
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")

    import frei_amd as fa
    from frei_amd import _native as N
    from frei_amd.binning import KLibrary
    from frei_amd.kdist import KGrid, gauss_g
    T_nodes = np.linspace(500.0, 3000.0, a.n_T)
    p = np.logspace(2, -6, a.n_p)                      # bar, bottom first: layers and nodes
    edges = log_edges(2.5, 5.0, a.R)
    n_bins = edges.size - 1
    g, w = gauss_g(a.n_g)
    n_col = n_bins * a.n_g
    pitch = (n_col + 63) // 64 * 64
    rng = np.random.default_rng(20)
    T0 = np.linspace(2200.0, 900.0, a.n_p)
    run_kw = dict(n_timesteps=a.iters, n_zero_crossings=10 ** 6, convergence_dT=-1.0)

    def stats(ms):
        return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))

    def clock(fn):
        t = time.perf_counter()
        fn()
        return (time.perf_counter() - t) * 1e3

    for n_src in a.n_src:
        tabs = {f"s{k}": np.sort(rng.lognormal(1.0, 2.0, (a.n_p, a.n_T, n_bins, a.n_g)), axis=-1)
                for k in range(n_src)}
        lib = KLibrary(tabs, edges, g, w, T_nodes, p)
        x = rng.uniform(1e-3, 1e-1, (a.n_atm, n_src, a.n_T, a.n_p))
        grav = rng.uniform(800.0, 4000.0, a.n_atm)
        shape = dict(n_src=n_src, n_atm=a.n_atm, n_layers=a.n_p, n_T=a.n_T, n_bins=n_bins,
                     n_g=a.n_g, n_col=n_col, iters=a.iters)
        pl = fa.Planet.from_hot_jupiter()
        grid = KGrid(pl, edges, g=g, weights=w, pressures=p, init_temperatures=T0)
        tables = lib.tables(x)
        eng = fa.BatchEngine(grid.col_lam, p, {"mix": tables}, grav, m_bar=pl.m_bar,
                             quad_weights=grid.col_weights)          # (the warm-up of the fill)
        clib, h = N.lib(), lib.handle()
        fill = [clock(lambda: N.check(clib.frei_set_table_kmix_batch(eng._ctx, h,
                                                                     N.dptr(tables.x), 0)))
                for _ in range(a.reps)]
        eng.set_mix(x)
        remix = [clock(lambda: eng.set_mix(x)) for _ in range(a.reps)]
        eng.run(T0, **run_kw)
        run = [clock(lambda: eng.run(T0, **run_kw)) for _ in range(a.reps)]
        eng.close()
        emit(dict(what="kbatch", **shape, fill_ms=stats(fill), set_mix_ms=stats(remix),
                  run_ms=stats(run), table_bytes=a.n_atm * a.n_p * a.n_T * pitch * 8,
                  library_bytes=lib.resident_bytes))
        # ---- the path this replaces: one context per composition
        grid.load_opacities(klibrary=lib, mix=x[0])
        grid.emission_spectrum(**run_kw)                                         # warm-up
        single = []
        for m in range(1, min(a.n_single, a.n_atm - 1) + 1):
            pl.g = float(grav[m])

            def one():
                grid.set_mix(x[m])
                grid.emission_spectrum(**run_kw)
                grid.engine().synchronize()
            single.append(clock(one))
        grid._close_engine()
        emit(dict(what="single_path", **shape, n_timed=len(single), per_composition_ms=stats(single),
                  projected_batch_ms=float(np.mean(single)) * a.n_atm))
        lib.release()


if __name__ == "__main__":
    main()
