"""The sweep form the default options choose at each slice-size threshold of a 256-CU device,
through the path report (frei_ctx_path, built from the plan run_sweep launches from).  No sweep
runs: the engines only build their metadata.  Every other test forces its form with options;
this one holds the thresholds themselves (quad_max_blocks 208, pipe_min_blocks 208, the CU
count 256 as pipe_max_blocks with two CUs left for the trailing update, pair_max_blocks 420,
shared_max_blocks 640, kLam2MinBlocks 1400), in 256-wavelength blocks of the slice."""
import ctypes

import pytest

from tests.test_gpu_lam2 import _engine

pytestmark = pytest.mark.gpu

ONE_LANE = dict(paired=False, quad=False, pipe=0, lam2=False)

# n_lam, 256-wavelength blocks, the path() entries that must hold
CASES = [
    (53_248, 208, dict(quad=True, pipe=0, lds_steps=True)),
    (53_249, 209, dict(pipe=4, tail=True, quad=False, paired=False)),
    (65_024, 254, dict(pipe=4, tail=True)),
    (65_025, 255, dict(pipe=4, tail=False)),
    (65_536, 256, dict(pipe=4, tail=False)),
    (65_537, 257, dict(paired=True, pipe=0)),
    (107_520, 420, dict(paired=True)),
    (107_521, 421, dict(ONE_LANE, lds_steps=True)),
    (163_840, 640, dict(ONE_LANE, lds_steps=True)),
    (163_842, 641, dict(ONE_LANE, lds_steps=False)),
    (358_144, 1399, dict(lam2=False)),
    (358_400, 1400, dict(lam2=True, lazy_k3=True, lds_steps=False)),
    (358_401, 1401, dict(lam2=False)),
]


def _cu_count():
    """multiProcessorCount of device 0, asked of the HIP runtime the library is linked against
    (hipGetDevicePropertiesR0600: the suffix pins the struct's layout, in which the count is the
    int at byte 388 — after name[256], uuid, luid, the memory and launch limits, the compute
    capability, the texture alignments and deviceOverlap)."""
    from frei_amd import _native
    prop = ctypes.create_string_buffer(4096)
    assert _native.lib().hipGetDevicePropertiesR0600(prop, 0) == 0
    return ctypes.c_int.from_buffer(prop, 388).value


@pytest.fixture(scope="module")
def fa():
    import frei_amd
    n_cu = _cu_count()
    if n_cu != 256:
        pytest.skip(f"the default thresholds asserted here are those of 256 CUs, not {n_cu}")
    return frei_amd


@pytest.mark.parametrize("n_lam,blocks,want", CASES, ids=[str(c[0]) for c in CASES])
def test_default_form_at_threshold(fa, n_lam, blocks, want):
    assert (n_lam + 255) // 256 == blocks
    eng, _, _ = _engine(fa, n_lam, nL=8)
    try:
        path = eng.path()
    finally:
        eng.close()
    print(n_lam, blocks, path)
    got = {k: path[k] for k in want}
    assert got == want, path
