#!/usr/bin/env python
"""Grid sweep with T-dependent chemistry: a loop of single contexts against the batched engine.

Workload: the C3 tables (60 layers x 100k wavelengths x 16 T nodes, 8 species; the T nodes are
widened to hold every atmosphere of the sweep), 32 atmospheres = 8 T_ref (1000..2400 K) x 4
gravities ordered by T_ref, two chemistry tables (c3_chemistry at 0 and +0.5 dex, alternating).
A warm-up block, then `--repeats` timed blocks: state_init (untimed), then `--iters` fixed-work
T-P iterations timed by a host clock around a synchronise — every block does the same work from
the same start, and stays within the iterations a start far from equilibrium survives.

  --variant single   what a user does without the batch: one Engine(mmr=ChemistryTable) per
                     atmosphere, one after the other (the times of the 32 contexts are added)
  --variant tile1|tile2|tile4   BatchEngine with FREI_ATM_TILE = 1, 2, 4
  --compare DIR      compare the final T and spectra the tile variants dumped into DIR

Each variant appends one JSON line to DIR/results.jsonl and (tile variants) dumps
DIR/<variant>.npz.  Run every variant as its own process, alternating them (a GPU's clocks
drift over minutes), and read the spread off the repeats.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12   # bytes/s, MI355X


def workload(n_lam, n_layers=60, n_T=16):
    import frei_amd as fa
    from frei_amd.tp import temperature_grid
    from frei_amd.workloads import c3, c3_chemistry
    w = c3(n_layers=n_layers, n_lam=n_lam, n_T=n_T)
    T_ref = np.repeat(np.linspace(1000.0, 2400.0, 8), 4)
    g = np.tile(np.array([800.0, 1500.0, 2478.65, 4000.0]), 8)
    T0 = np.array([temperature_grid(w["p"], t, 0.1, 0.1) for t in T_ref])
    Tn = np.linspace(0.8 * T0.min(), 1.2 * T0.max(), n_T)   # every atmosphere inside the hull
    fT = np.array([(Tn / 1000.0) ** 0.5 for _ in w["names"]])
    tabs = {n: fa.SeparableTable(w["base"][s], w["fp"][s], fT[s], w["p"], Tn)
            for s, n in enumerate(w["names"])}
    c0 = c3_chemistry(w)
    c1 = fa.ChemistryTable({n: v * 10 ** 0.5 for n, v in c0.values.items()}, c0.temperature,
                           c0.pressure)
    atm_tab = np.arange(T_ref.size) % 2
    return dict(w=w, tabs=tabs, Tn=Tn, T0=T0, g=g, chem=[c0, c1], atm_tab=atm_tab)


def timed_blocks(eng, T0, iters, repeats):
    out = []
    for k in range(repeats + 1):   # block 0 is the warm-up
        eng.state_init(T0)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.iterate(iters)
        eng.synchronize()
        if k:
            out.append(time.perf_counter() - t0)
    return np.array(out)


def shared_brackets(T, Tn, tile):
    """Host count over (tile, layer) pairs of consecutive atmospheres: the share whose T
    brackets all coincide, and the row-set loads of the tiled sweep relative to one per
    (atmosphere, layer) (a load whenever the bracket differs from the atmosphere before it)."""
    br = np.searchsorted(Tn, T, side="right")
    A, nL = br.shape
    same = loads = pairs = 0
    for m0 in range(0, A, tile):
        b = br[m0:m0 + tile]
        same += int(np.sum(np.all(b == b[0], axis=0)))
        loads += int(nL + np.sum(b[1:] != b[:-1]))
        pairs += nL
    return same / pairs, loads / (A * nL)


def run_variant(a):
    import frei_amd as fa
    from frei_amd.workloads import bytes_per_update
    x = workload(a.n_lam)
    w, A = x["w"], x["g"].size
    nL, S = w["p"].size, len(w["names"])
    updates = 2.0 * (nL - 1) * a.n_lam * A * a.iters   # per timed block, all atmospheres
    rec = dict(variant=a.variant, n_lam=a.n_lam, n_layers=nL, n_species=S, n_atm=A,
               iters=a.iters, repeats=a.repeats)
    if a.variant == "single":
        secs = np.zeros(a.repeats)
        for m in range(A):
            eng = fa.Engine(w["lam"], w["p"], x["tabs"], g=x["g"][m],
                            mmr=x["chem"][x["atm_tab"][m]])
            try:
                secs += timed_blocks(eng, x["T0"][m], a.iters, a.repeats)
            finally:
                eng.close()
    else:
        tile = int(a.variant[4:])
        os.environ["FREI_ATM_TILE"] = str(tile)
        eng = fa.BatchEngine(w["lam"], w["p"], x["tabs"], g=x["g"],
                             mmr=[x["chem"][k] for k in x["atm_tab"]])
        try:
            path = eng.path()
            assert not path["contracted"] and path["atm_tile"] == tile, path
            secs = timed_blocks(eng, x["T0"], a.iters, a.repeats)
            T = eng.get_temperatures()
            up, _ = eng.get_fluxes()
            np.savez(os.path.join(a.out, a.variant + ".npz"), T=T, spectra=up[:, -1])
            rec["path"] = path
            rec["finite"] = bool(np.all(np.isfinite(T)) and np.all(np.isfinite(up[:, -1])))
            rec["nonfinite_T_per_atm"] = np.sum(~np.isfinite(T), axis=1).tolist()
            rec["nonfinite_spectrum_per_atm"] = np.sum(~np.isfinite(up[:, -1]), axis=1).tolist()
            rec["T_min_max"] = [float(np.nanmin(T)), float(np.nanmax(T))]
            for t in (2, 4):
                same, loads = shared_brackets(T, x["Tn"], t)
                rec[f"brackets_coincide_tile{t}"] = same
                rec[f"row_loads_tile{t}"] = loads
        finally:
            eng.close()
    rec["seconds"] = [float(s) for s in secs]
    rec["ms_per_iter_per_atm"] = [float(1e3 * s / a.iters / A) for s in secs]
    rec["updates_per_s"] = [float(updates / s) for s in secs]
    bpu = bytes_per_update(S, live_only=True)
    rec["bytes_per_update"] = bpu
    rec["hbm_fraction"] = [float(updates / s * bpu / HBM_PEAK) for s in secs]
    with open(os.path.join(a.out, "results.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


def compare(out):
    d = {v: np.load(os.path.join(out, v + ".npz")) for v in ("tile1", "tile2", "tile4")
         if os.path.exists(os.path.join(out, v + ".npz"))}
    rec = dict(compare=sorted(d))
    for v in d:
        if v == "tile1" or "tile1" not in d:
            continue
        rec[v + "_T_bitwise"] = bool(np.array_equal(d[v]["T"], d["tile1"]["T"], equal_nan=True))
        rec[v + "_spectra_bitwise"] = bool(np.array_equal(d[v]["spectra"], d["tile1"]["spectra"],
                                                          equal_nan=True))
    rec["finite"] = bool(all(np.all(np.isfinite(x["T"])) and np.all(np.isfinite(x["spectra"]))
                             for x in d.values()))
    with open(os.path.join(out, "results.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    return 0 if rec["finite"] and all(v for k, v in rec.items() if k.endswith("bitwise")) else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--variant", choices=["single", "tile1", "tile2", "tile4"])
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--out", default="profiles/r07/batch_chem")
    ap.add_argument("--n-lam", type=int, default=100_000)
    ap.add_argument("--iters", type=int, default=6)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.compare:
        return compare(a.out)
    if not a.variant:
        ap.error("--variant or --compare")
    run_variant(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
