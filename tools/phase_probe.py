"""Time the phase-curve kernel (K16, frei_phs_apply) on the dtaus a batched run left on the
device, beside frei_emergent on the same context and the host path it replaces.

Shapes (--shapes, any of a, b, c, run in the order given): (a) --layers (60) x 100k wavelengths,
16 x 8 cells, 32 phases; (b) the same axis, 32 x 16 cells, 64 phases; (c) 500k wavelengths, one
latitude band of 16 cells, 32 phases.  Cells are lonlat_cells at inclination 90 degrees, phases
(k + 1/4) / n_phase (no ray grazes the limb exactly).  Every cell has an atmosphere of its own up
to --max-atm (128); beyond it cell c reads atmosphere c mod max-atm (the kernel's arithmetic does
not depend on it; more of the column reads then come from L2).  Synthetic C3 tables of two
species, BatchEngine.run(n_timesteps=1, keep_dtaus=True): the opacities only have to leave
realistic dtaus behind.

Per shape, in one process, --rounds times over, the three taking turns:
  phase     PhaseCurve.integrate(keep=True): HIP events around the kernel (frei_phs_apply's
            kernel_ms), repeated until about --target-ms of kernel time has run.  Work: one shell
            step per visible pair (p, c), shell and wavelength.
  emergent  BatchEngine.emergent at 8 Gauss angles, flux only (frei_post_timing): one shell step
            per atmosphere, angle, shell and wavelength.
  replaced  (--replaced: the shapes to do it for, once each) the path without K16, wall clock:
            the distinct visible angles of the plan (mu rounded to 12 digits; the grid's
            symmetry leaves few) in calls of at most 64 to
            BatchEngine.emergent(want_intensity=True), each downloading [n_atm][n_mu][n_lam],
            then the sum over the cells on the host in the kernel's order.  Its result is
            compared with the kernel's (max relative difference).
Prints one JSON line per shape.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"a": (100_000, 16, 8, 32), "b": (100_000, 32, 16, 64), "c": (500_000, 16, 1, 32)}


def kernel_ms(call, read, a):
    """Warm ``call`` once -> (calls per round, a function that runs one round and returns its
    mean kernel ms per call); ``read`` gives the last call's kernel ms."""
    call()
    reps = int(min(a.max_reps, max(2, np.ceil(a.target_ms / max(read(), 1e-3)))))

    def one_round():
        tot = 0.0
        for _ in range(reps):
            call()
            tot += read()
        return tot / reps
    return reps, one_round


def replaced_path(eng, T, pc, n_lam):
    """-> (seconds, calls, bytes downloaded, out[n_phase][n_lam])."""
    t0 = time.perf_counter()
    key = np.round(pc.mu, 12)
    uniq = np.unique(key[pc.mu > 0])
    where = {}
    nbytes, calls = 0, 0
    chunks = []
    for k0 in range(0, uniq.size, 64):
        inten = eng.emergent(T, mu=uniq[k0:k0 + 64])        # [n_atm][k][n_lam], downloaded
        nbytes += inten.nbytes
        calls += 1
        for k in range(inten.shape[1]):
            where[uniq[k0 + k]] = (len(chunks), k)
        chunks.append(inten)
    out = np.zeros((pc.n_phase, n_lam))
    for p in range(pc.n_phase):
        acc = None
        for c in np.flatnonzero(pc.mu[p] > 0):
            i, k = where[key[p, c]]
            term = pc.coef[p, c] * chunks[i][pc.select[c], k]
            acc = term if acc is None else acc + term
        if acc is not None:
            out[p] = acc
    return time.perf_counter() - t0, calls, nbytes, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="a,b,c")
    ap.add_argument("--layers", type=int, default=60)
    ap.add_argument("--max-atm", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--target-ms", type=float, default=200.0)
    ap.add_argument("--max-reps", type=int, default=20)
    ap.add_argument("--replaced", default="a,b,c", help="shapes whose replaced path is timed")
    ap.add_argument("--scale", type=float, default=1.0,
                    help="multiplies the wavelength counts (a rehearsal at a small size)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import frei_amd as fa
    from frei_amd.constants import M_BAR_HOT_JUPITER
    from frei_amd.phasecurve import PHASE_TILE
    from frei_amd.workloads import c3
    nL = a.layers
    lines = []
    engines = {}        # (n_lam, n_atm) -> (engine, final T): shapes a and b share theirs

    def engine(n_lam, n_atm):
        if (n_lam, n_atm) not in engines:
            for e, _ in engines.values():
                e.close()
            engines.clear()
            w = c3(n_layers=nL, n_lam=n_lam, species=["1H2-16O", "12C-16O"])
            tabs = {n: fa.SeparableTable(w["base"][s], w["fp"][s], w["fT"][s], w["p"],
                                         w["T_nodes"]) for s, n in enumerate(w["names"])}
            T0 = np.array([fa.temperature_grid(w["p"], t, 0.1, 0.1)
                           for t in np.linspace(1100.0, 2500.0, n_atm)])
            mmr = np.broadcast_to(w["mmr"], (n_atm,) + w["mmr"].shape)
            eng = fa.BatchEngine(w["lam"], w["p"], tabs, g=np.linspace(800.0, 6000.0, n_atm),
                                 mmr=mmr, m_bar=M_BAR_HOT_JUPITER)
            out = eng.run(T0, n_timesteps=1, keep_dtaus=True)
            engines[(n_lam, n_atm)] = (eng, np.asarray(out["final_T"], dtype=float))
        return engines[(n_lam, n_atm)]

    try:
        for name in a.shapes.split(","):
            n_lam, n_lon, n_lat, n_phase = SHAPES[name]
            n_lam = max(2, int(n_lam * a.scale))
            lon, lat, area = fa.lonlat_cells(n_lon, n_lat)
            n_cell = lon.size
            n_atm = min(n_cell, a.max_atm)
            pc = fa.PhaseCurve(lon, lat, area, (np.arange(n_phase) + 0.25) / n_phase,
                               select=np.arange(n_cell) % n_atm)
            eng, T = engine(n_lam, n_atm)
            g_mu, g_w = fa.gauss_angles(8)
            pairs = int(pc.n_visible.sum())
            tile_pairs = [int(np.any(pc.mu[t:t + PHASE_TILE] > 0, axis=0).sum())
                          for t in range(0, n_phase, PHASE_TILE)]
            reps_p, round_p = kernel_ms(lambda: pc.integrate(eng, T, keep=True),
                                        lambda: pc.timing(reset=True)[0], a)
            reps_e, round_e = kernel_ms(lambda: eng.emergent(T, g_mu, g_w), eng.post_timing, a)
            xp, xe = [], []
            for _ in range(a.rounds):
                xp.append(round_p())
                xe.append(round_e())
            steps_p = float(pairs) * n_lam * (nL - 1)
            steps_e = float(n_atm) * 8 * n_lam * (nL - 1)
            mp, me = float(np.median(xp)), float(np.median(xe))
            rec = dict(shape=name, n_layers=nL, n_lam=n_lam, n_cell=n_cell, n_atm=n_atm,
                       n_phase=n_phase, visible_pairs=pairs, visits=sum(tile_pairs),
                       mean_rays_per_visit=pairs / max(1, sum(tile_pairs)),
                       phase=dict(reps=reps_p, kernel_ms=dict(median=mp, min=min(xp), max=max(xp)),
                                  shell_steps=steps_p, shell_steps_per_s=steps_p / (mp * 1e-3)),
                       emergent8=dict(reps=reps_e,
                                      kernel_ms=dict(median=me, min=min(xe), max=max(xe)),
                                      shell_steps=steps_e,
                                      shell_steps_per_s=steps_e / (me * 1e-3)))
            rec["rate_over_emergent8"] = (rec["phase"]["shell_steps_per_s"] /
                                          rec["emergent8"]["shell_steps_per_s"])
            if name in a.replaced.split(","):
                t0 = time.perf_counter()
                got = pc.integrate(eng, T)
                wall = time.perf_counter() - t0
                sec, calls, nbytes, ref = replaced_path(eng, T, pc, n_lam)
                ok = ref != 0
                rec["replaced"] = dict(
                    seconds=sec, emergent_calls=calls, bytes_downloaded=nbytes,
                    phase_call_wall_s=wall, speedup_wall=sec / wall,
                    speedup_over_kernel=sec / (mp * 1e-3),
                    max_rel_diff=float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))))
            pc.release()
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
    finally:
        for e, _ in engines.values():
            e.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
