"""bench.py's plain run and --dump-outputs, on a small grid (12 layers x 4100 wavelengths: not a
multiple of the 256-wavelength block, several blocks).

A plain run reports the headline figures only, and --dump-outputs writes the state the last timed
step left.  Two runs with the same inputs and the same total number of T-P iterations, split
differently between warm-up and timed steps (1 + 2 and 2 + 1), must write the same arrays: the
inputs are identical from run to run, --steps sets the number of timed steps, and the dump is taken
right after them.  The comparison allows the 1e-10 of tests/parity.py (fp64 sums whose order may
differ between runs) rather than asking for equal bits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("temperatures", "spectrum", "flux_up_sample", "flux_down_sample", "sample_columns")
N_LAYERS, N_LAM = 12, 4100


def _bench(out_dir, steps, warmup, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", str(steps), "--warmup", str(warmup),
                        "--n-layers", str(N_LAYERS), "--n-lam", str(N_LAM),
                        "--dump-outputs", str(out_dir), *extra],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_headline_and_dumped_outputs(tmp_path):
    a = _bench(tmp_path / "a", steps=2, warmup=1)
    b = _bench(tmp_path / "b", steps=1, warmup=2)
    for line, steps in ((a, 2), (b, 1)):
        assert line["steps"] == steps
        assert line["unit"] == "updates/s" and line["dtype"] == "f64"
        assert line["higher_is_better"] is True
        assert line["ms_per_step"] > 0
        updates = 2 * (N_LAYERS - 1) * N_LAM        # one step: emit + absorb sweep
        assert line["value"] == pytest.approx(updates / (line["ms_per_step"] * 1e-3), rel=1e-9)
        # the legs with runs of their own are behind --full
        for leg in ("roofline", "rad_eq", "per_species", "chemistry", "provider", "cpu_baseline",
                    "k6_binning", "c5_batched"):
            assert leg not in line, leg
    total = 0
    for name in NAMES:
        pa, pb = tmp_path / "a" / (name + ".npy"), tmp_path / "b" / (name + ".npy")
        total += os.path.getsize(pa)
        xa, xb = np.load(pa), np.load(pb)
        assert xa.dtype == np.float64 and xa.shape == xb.shape, name
        assert a["dumped_outputs"]["arrays"][name] == list(xa.shape)
        assert np.all(np.isfinite(xa)), name
        assert np.allclose(xa, xb, rtol=1e-10, atol=0.0), name
    assert total <= 64 * 1000 * 1000
    T = np.load(tmp_path / "a" / "temperatures.npy")
    spec = np.load(tmp_path / "a" / "spectrum.npy")
    up = np.load(tmp_path / "a" / "flux_up_sample.npy")
    cols = np.load(tmp_path / "a" / "sample_columns.npy").astype(int)
    assert T.shape == (N_LAYERS,) and np.all(T > 0)
    assert spec.shape == (N_LAM,) and np.any(spec > 0)
    assert up.shape == (N_LAYERS, cols.size) and cols.size == N_LAM   # small grid: every column
    assert np.array_equal(up[-1], spec[cols])       # the emergent spectrum is F_up's last row
