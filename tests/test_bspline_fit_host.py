"""csrc/mm_bspline_fit.h -- the code lane 0 of k_bspline_fit runs -- compiled for the CPU (unfused, like the library) and
compared with the checker bit for bit, no GPU: every fixture, every degree on odd sizes, and the inputs on which a fit
must stop rather than search on: finite coordinates whose chord or residuals overflow."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mm_checkers import bspline as B  # noqa: E402
from test_bspline_host import fixtures  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.fixture(scope="module")
def host_fit(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or (HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc"))
    assert cxx, "no C++ compiler"
    lib = str(tmp_path_factory.mktemp("bspl") / "libbspline_fit_host.so")
    cmd = [cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-DMM_HD=inline",
           "-I" + os.path.join(ROOT, "multimoda-rs_amd", "csrc"), os.path.join(ROOT, "tests", "bspline_fit_host.cpp"),
           "-o", lib]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    L = C.CDLL(lib)
    L.bspline_fit_host.restype = C.c_int
    L.bspline_fit_host.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.POINTER(C.c_double),
                                   C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def run(P, s, k):
        P = np.ascontiguousarray(P, dtype=np.float64)
        m = P.shape[0]
        out = np.zeros((m, 3))
        fp, nk, ok = C.c_double(), C.c_int(), C.c_int()
        st = L.bspline_fit_host(P.ctypes.data, m, k, s, out.ctypes.data, C.byref(fp), C.byref(nk), C.byref(ok))
        assert ok.value == 1, "the fit wrote past its work arrays"
        return st, out, fp.value, nk.value
    return run


def agree(host_fit, P, s, k, tag, want=None):
    want = want or B.fit_closed(P, s, k)
    st, out, fp, nk = host_fit(P, s, k)
    assert st == want["status"], (tag, st, want["status"])
    if st in (B.UNCHANGED_SHORT, B.UNCHANGED_ZERO_CHORD, B.UNCHANGED_NONFINITE):
        return st
    assert np.array_equal(out.view(np.uint64), want["points"].view(np.uint64)), tag
    assert fp == want["fp"] and nk == want["n_knots"], (tag, fp, want["fp"], nk, want["n_knots"])
    return st


def test_header_matches_the_checker_on_every_fixture(host_fit):
    n = 0
    for c in fixtures():
        if c["m"] < c["k"] + 1:
            continue                                    # screened by the host before the kernel
        agree(host_fit, c["in"], c["s"], c["k"], c["id"], c["res"])
        n += 1
    assert n > 180


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_header_matches_the_checker_on_small_systems(host_fit, k):
    rng = np.random.default_rng(k)
    for m in (k + 1, k + 2, 9, 33):
        th = np.linspace(0, 2 * np.pi, m, endpoint=False)
        P = np.stack([2 * np.cos(th), 1.5 * np.sin(th), 0.1 * rng.normal(size=m)], 1) + 0.05 * rng.normal(size=(m, 3))
        for s in (0.0, 0.003 * m, 0.05 * m, 50.0):
            agree(host_fit, P, s, k, (k, m, s))


def test_overflowing_contours_stop_and_come_back_unchanged(host_fit):
    rng = np.random.default_rng(5)
    th = np.linspace(0, 2 * np.pi, 16, endpoint=False)
    P = np.stack([2 * np.cos(th), 1.5 * np.sin(th), 0.1 * rng.normal(size=16)], 1)
    for scale in (1e160, 8e307):                           # the squared chord overflows
        for s, k in ((0.0, 3), (0.1, 3), (0.0, 2), (0.1, 1), (1e300, 5)):
            assert agree(host_fit, P * scale, s, k, (scale, s, k)) == B.UNCHANGED_NONFINITE
    for scale in (1e150, 1e153, 1e120):                    # the chord is finite; squared residuals may overflow
        for s, k in ((0.0, 3), (0.1, 3), (1.0, 2), (1e300, 3), (0.1, 5)):
            agree(host_fit, P * scale, s, k, (scale, s, k))
