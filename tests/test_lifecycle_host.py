"""frei_live_resources without a GPU: declared, bound, callable before any handle exists."""
import ctypes
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_live_resources_is_declared_bound_and_zero_before_any_handle():
    from frei_amd import _native as N
    header = open(os.path.join(ROOT, "include", "frei_hip.h")).read()
    assert re.search(r"\bint\s+frei_live_resources\s*\(\s*int64_t\s*\*", header)
    assert N.SIGNATURES["frei_live_resources"] == (ctypes.c_int,
                                                   [ctypes.POINTER(ctypes.c_int64)] * 4)
    # a null pointer skips its figure; the call needs no device and no handle
    lib = N.lib()
    one = ctypes.c_int64(-7)
    assert lib.frei_live_resources(None, None, ctypes.byref(one), None) == 0 and one.value >= 0
    assert lib.frei_live_resources(None, None, None, None) == 0
    # a failed create (no such layer count: refused before any device call) counts nothing
    before = N.live_resources()
    ctx = ctypes.c_void_p()
    assert lib.frei_ctx_create(ctypes.byref(ctx), 0, 2, 100, 1) != 0
    assert N.live_resources() == before
    # before any handle exists (a fresh process: this one may hold other tests' handles)
    r = subprocess.run([sys.executable, "-c",
                        "from frei_amd import _native as N; print(N.live_resources())"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.strip() == "(0, 0, 0, 0)"
