"""The caller-provided workspaces (csrc/workspace.h): every *_workspace_bytes query that takes no handle returns what it returned before
the queries and the entries were written over one layout description each -- tests/golden/workspace_sizes.json, section "host":
argument tuples and sizes recorded from the build before that change, across every branch of the formulas (n of 0, 1, around a
64-row tile and a few thousand; Dense with and without the split-K region; CG across a slab of 64 columns; shortest paths with one
and two row sets, one row and a row per source; the sizes each query refuses, which return 0) -- and the header's own allocator,
exercised under the address and undefined-behaviour sanitizers by a stand-alone program (tests/host/workspace_check.cpp).  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

from ngpde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = json.load(open(os.path.join(ROOT, "tests", "golden", "workspace_sizes.json")))


def test_the_table_crosses_the_branches_it_names():
    host = SIZES["host"]
    assert set(host) == {"ngpde_dense_workspace_bytes", "ngpde_csr_cg_workspace_bytes", "ngpde_csr_lambda_max_workspace_bytes",
                         "ngpde_csr_random_walk_pe_workspace_bytes", "ngpde_coo_components_workspace_bytes",
                         "ngpde_csr_hop_distance_workspace_bytes", "ngpde_csr_shortest_paths_workspace_bytes",
                         "ngpde_bias_act_workspace_bytes"}
    for name, rows in host.items():
        if name != "ngpde_bias_act_workspace_bytes":
            assert {0, 1, 63, 64, 65} <= {a[0] for a, _ in rows} and any(a[0] > 4000 for a, _ in rows), name
        if name not in ("ngpde_dense_workspace_bytes", "ngpde_bias_act_workspace_bytes"):
            assert any(size == 0 for _, size in rows), name          # the refused sizes
    dense = host["ngpde_dense_workspace_bytes"]
    assert {(din < 256, dout < 512) for (_, din, dout), _ in dense} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {a[2] for a, _ in host["ngpde_csr_cg_workspace_bytes"]} >= {63, 64, 65, 128, 129}
    paths = host["ngpde_csr_shortest_paths_workspace_bytes"]
    assert {(a[2] > 0, a[4]) for a, _ in paths} == {(False, 0), (False, 1), (True, 0), (True, 1)}


@pytest.mark.parametrize("name", sorted(SIZES["host"]))
def test_size_queries_return_the_recorded_sizes(name):
    fn = getattr(_lib.load(), name)
    wrong = [(args, want, fn(*args)) for args, want in SIZES["host"][name] if fn(*args) != want]
    assert not wrong, wrong[:5]


def test_the_header_carves_what_it_measures_under_the_sanitizers(tmp_path):
    """workspace.h needs no HIP: the host compiler builds tests/host/workspace_check.cpp with -fsanitize=address,undefined; the program
    measures three layouts, carves each into a heap buffer of exactly the measured size and checks that every piece lies inside it,
    starts on a 256-byte granule, ends before the next begins and that the carve ends at the measured size"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "workspace_check")
    src = os.path.join(ROOT, "tests", "host", "workspace_check.cpp")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "neuralgraphpde.jl_amd", "csrc"), src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "workspace_check ok" in out.stdout
