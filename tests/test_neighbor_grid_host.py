"""The neighbour search's cell grid (csrc/neighbor_grid.h), checked on the host.

tests/host/neighbor_grid_check.cpp includes only that header; it is built with AddressSanitizer + UndefinedBehaviorSanitizer and
-ffp-contract=off (the library's flag: the float rule d2 <= r*r is stated without fused multiply-add) and run once as a stand-alone
program.  It checks what neighbors.hip's kernels take for granted: make_grid ends, with a finite positive cell and inverse and cell
counts inside the caps, for every combination of extents and `want` from 0 and the smallest denormal to FLT_MAX and inf; every pair
the float rule accepts lies in adjacent cells (ordinary, capped and coarsened grids, clouds at magnitudes where squares overflow or
underflow); a k-NN ring stop never cuts off a point that sorts among the k smallest; a cell coordinate is within 1e-3 cells of its
exact value.  No GPU.
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "neuralgraphpde.jl_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("neighbor_grid") / "neighbor_grid_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "host", "neighbor_grid_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    return r.returncode, r.stdout, r.stdout + r.stderr


def test_grid_ends_covers_and_bounds_rings_at_every_magnitude(report):
    code, out, text = report
    assert code == 0, text[-4000:]
    assert "AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-4000:]
    m = re.search(r"^(\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 500000, text[-4000:]


def test_the_sweep_reaches_every_kind_of_grid(report):
    _, out, text = report
    m = re.search(r"^grids: (\d+) ordinary, (\d+) capped, (\d+) coarsened, (\d+) one-cell; (\d+) accepted pairs, (\d+) ring pairs$", out, re.M)
    assert m, text[-4000:]
    ordinary, capped, coarsened, one_cell, accepted, ring = map(int, m.groups())
    assert min(ordinary, capped, coarsened, one_cell) >= 10 and accepted > 10 ** 6 and ring > 10 ** 6


def test_the_library_sizes_its_grids_with_the_header():
    with open(os.path.join(CSRC, "neighbors.hip"), encoding="utf-8") as f:
        src = f.read()
    assert '#include "neighbor_grid.h"' in src
    # one definition of each: the kernels' file keeps none of its own
    for name in ("struct Grid", "struct Quant", "make_grid(int", "cell_budget(int", "kMaxCellsPerDim ="):
        assert name not in src, name
    for call in ("make_grid(DIM,", "radius_want(r)", "knn_want(DIM,", "make_quant(DIM,", "span_is_finite(dim,", "ring_reach2(g,", "cell_of<DIM>(g,"):
        assert call in src, call
