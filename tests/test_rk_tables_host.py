"""The Runge-Kutta coefficient tables of the device-resident solvers (csrc/rk_tableau.h), checked on the host.

tests/host/rk_tables_check.cpp includes only that header; it is built with AddressSanitizer + UndefinedBehaviorSanitizer, run once as a
stand-alone program, and prints rk_forward6 and rk_adjoint8 as hex floats for Euler and Tsit5 at dt = 0.02, 1 / 50 and 0.1f widened to
double.  The reference is independent of the header: node.py's tableau (_TSIT5_A, _TSIT5_B), laid out by the index formulas the kernels
read the tables by, each entry numpy.float32(numpy.float64(dt) * x).  Every entry must match bit for bit, and every slot the formulas
do not name must be +0.0.
"""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from ngpde_amd import node

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "neuralgraphpde.jl_amd", "csrc")
DTS = (np.float64(0.02), np.float64(1.0) / np.float64(50.0), np.float64(np.float32(0.1)))
TABLEAUS = ("euler", "tsit5")


def expected_forward6(a, b, dt):
    """{slot: float32}: stage i's epilogue forms the next stage's input (after the last stage the step update), so its row is
    a[i + 1] (b for i = S - 1): the weight of k_j, j < i, at i * 6 + j, of k_i itself at 36 + i"""
    S, out = len(b), {}
    for i in range(S):
        row = b if i == S - 1 else a[i + 1]
        for j in range(i):
            out[i * 6 + j] = np.float32(dt * np.float64(row[j]))
        out[36 + i] = np.float32(dt * np.float64(row[i]))
    return out


def expected_adjoint8(a, b, dt):
    """{slot: float32}: cb[i][i] = dt b_i, cb[i][j] (j > i) = dt a[j][i], rows 8 wide"""
    S, out = len(b), {}
    for i in range(S):
        out[i * 8 + i] = np.float32(dt * np.float64(b[i]))
        for j in range(i + 1, S):
            out[i * 8 + j] = np.float32(dt * np.float64(a[j][i]))
    return out


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """{(table, tableau, dt index): [float, ...]} as the program printed them"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("rk_tables") / "rk_tables_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-I", CSRC, os.path.join(HERE, "host", "rk_tables_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    report = r.stdout + r.stderr
    assert r.returncode == 0, report[-3000:]
    assert "AddressSanitizer" not in report and "runtime error" not in report and "LeakSanitizer" not in report, report[-3000:]
    out = {}
    for line in r.stdout.splitlines():
        table, name, k, *vals = line.split()
        out[(table, name, int(k))] = [float.fromhex(v) for v in vals]
    assert len(out) == 2 * len(TABLEAUS) * len(DTS)
    return out


@pytest.mark.parametrize("k", range(len(DTS)))
@pytest.mark.parametrize("name", TABLEAUS)
@pytest.mark.parametrize("table", ("forward6", "adjoint8"))
def test_table_matches_the_python_tableau_bit_for_bit(printed, table, name, k):
    a, b = node.TABLEAUS[name]
    assert (a, b) == (([[]], [1.0]) if name == "euler" else (node._TSIT5_A, node._TSIT5_B))
    want = (expected_forward6 if table == "forward6" else expected_adjoint8)(a, b, DTS[k])
    got = printed[(table, name, k)]
    assert len(got) == (42 if table == "forward6" else 8 * len(b))
    assert want and max(want) < len(got)
    for slot, v in enumerate(got):
        if slot in want:
            assert np.float32(v).tobytes() == want[slot].tobytes(), (slot, v, float(want[slot]))
        else:
            assert v == 0.0 and math.copysign(1.0, v) == 1.0, (slot, v)
