"""The Delaunay block (include/ngpde_mesh.h, _lib.MESH_SIGNATURES, ngpde_amd.mesh) held, on the host, to what tests/test_abi.py and
tests/test_interp_host.py hold the first two blocks to: the header equals the binding table and the library exports it; the first
two headers and tables declare none of it; `stream` is the last parameter; every entry refuses NULL and negative arguments by name
without a device; the Python wrappers raise their size and `dim` errors before the library is entered and the no-device error on a
well-shaped call.  The numpy restatement of tests/mesh_spec.py is checked on the five clouds tests/test_mesh_gpu.py uses: against
Qhull where no decision is near a tie (asserted on Qhull alone), against the 8-neighbour stencil on lattices.  csrc/delaunay_star.h,
the kernels' geometry, runs every point's star of small clouds against an exact brute force in tests/host/delaunay_star_check.cpp,
a stand-alone program under ASan + UBSan.  No GPU.
"""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch
from scipy.spatial import Delaunay

import ngpde_amd as ng
from ngpde_amd import _lib

import mesh_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "neuralgraphpde.jl_amd", "csrc")
INVALID = _lib.ERR_INVALID_ARGUMENT


def functions_of(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ngpde_[a-z0-9_]+)\s*\(", src)))


# ---- header, table, module -------------------------------------------------------------------------------------------------------
def test_header_and_binding_table_agree():
    assert functions_of("ngpde_mesh.h") == sorted(_lib.MESH_SIGNATURES)
    assert len(_lib.MESH_SIGNATURES) == 3


def test_library_exports_every_symbol_with_its_types():
    lib = _lib.load()
    for name, (res, args) in _lib.MESH_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_the_first_two_headers_and_tables_declare_none_of_them():
    for header, table in (("ngpde.h", _lib.SIGNATURES), ("ngpde_interp.h", _lib.INTERP_SIGNATURES)):
        assert not set(functions_of(header)) & set(_lib.MESH_SIGNATURES)
        assert not set(table) & set(_lib.MESH_SIGNATURES)
    src = open(os.path.join(ROOT, "include", "ngpde_mesh.h")).read()
    assert '#include "ngpde.h"' in src
    for cite in ("docs/src/tutorials/VMH.md:53-55", "NGPDE_DELAUNAY_MAX_DEGREE 2048", "#define NGPDE_DELAUNAY_TIE_BOUND 1.33", "TIED TRIANGLES OVERLAP",
                 "keep when in doubt", "What a call allocates", "no gradient to the positions"):
        assert cite in src, cite
    bound = float(re.search(r"#define NGPDE_DELAUNAY_TIE_BOUND (\S+)", src).group(1))
    assert bound == S.TIE_BOUND == 12 * 2.0 ** -53
    star = open(os.path.join(CSRC, "delaunay_star.h")).read()
    assert "kTieBound = 12.0 * kU" in star and "hip/" not in star                     # the bound's one definition; nothing from HIP


def test_every_stream_entry_of_the_header_ends_with_the_stream():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngpde_mesh.h")).read(), flags=re.S)
    protos = re.findall(r"\b(ngpde_[a-z0-9_]+)\s*\(([^)]*)\)", src)
    with_stream = [name for name, args in protos if "ngpde_stream_t" in args]
    assert sorted(with_stream) == ["ngpde_delaunay_graph", "ngpde_delaunay_triangles"]
    for name, args in protos:
        if name in with_stream:
            assert args.strip().endswith("ngpde_stream_t stream"), name


def test_the_module_is_a_submodule_with_its_own_names():
    assert ng.mesh.__all__ == ["delaunay_graph", "delaunay_triangles"]
    for name in ng.mesh.__all__:
        assert name not in ng.__all__ and callable(getattr(ng.mesh, name))
    assert "mesh" not in ng.__all__


# ---- the C entries refuse by name, without a device ------------------------------------------------------------------------------
def _refused(status, *words):
    msg = _lib.load().ngpde_last_error().decode()
    assert status == INVALID, (status, msg)
    for w in words:
        assert w in msg, msg


def test_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    out = (C.c_int32 * 64)()
    p, o = C.addressof(buf), C.addressof(out)
    cnt = C.c_int64(-7)
    graph = lambda n, pts, gid, ng_, r, cap, s, t, c: lib.ngpde_delaunay_graph(n, pts, gid, ng_, 1, r, 0, 0, cap, s, t, c, None)
    _refused(graph(-1, p, None, 1, math.inf, 0, None, None, C.byref(cnt)), "delaunay_graph", "points")
    _refused(graph(4, None, None, 1, math.inf, 0, None, None, C.byref(cnt)), "points is NULL")
    _refused(graph(4, p, None, 0, math.inf, 0, None, None, C.byref(cnt)), "n_graphs")
    _refused(graph(4, p, None, 2, math.inf, 0, None, None, C.byref(cnt)), "graph_id")
    _refused(graph(4, p, None, 1, -1.0, 0, None, None, C.byref(cnt)), "max_edge_length")
    _refused(graph(4, p, None, 1, math.nan, 0, None, None, C.byref(cnt)), "max_edge_length")
    _refused(graph(4, p, None, 1, math.inf, -1, o, o, C.byref(cnt)), "capacity")
    _refused(graph(4, p, None, 1, math.inf, 8, o, None, C.byref(cnt)), "s and t")
    _refused(graph(4, p, None, 1, math.inf, 0, None, None, None), "count pointer is NULL")
    tri = lambda n, pts, gid, ng_, r, cap, t, c: lib.ngpde_delaunay_triangles(n, pts, gid, ng_, 1, r, 0, cap, t, c, None)
    _refused(tri(-1, p, None, 1, math.inf, 0, None, C.byref(cnt)), "delaunay_triangles", "points")
    _refused(tri(4, None, None, 1, math.inf, 0, None, C.byref(cnt)), "points is NULL")
    _refused(tri(4, p, None, 0, math.inf, 0, None, C.byref(cnt)), "n_graphs")
    _refused(tri(4, p, None, 2, math.inf, 0, None, C.byref(cnt)), "graph_id")
    _refused(tri(4, p, None, 1, -0.5, 0, None, C.byref(cnt)), "max_edge_length")
    _refused(tri(4, p, None, 1, math.inf, -1, o, C.byref(cnt)), "capacity")
    _refused(tri(4, p, None, 1, math.inf, 0, None, None), "count pointer is NULL")
    assert cnt.value == -7                                              # refused calls write nothing
    assert graph(0, None, None, 1, math.inf, 0, None, None, C.byref(cnt)) == 0 and cnt.value == 0      # n = 0 gives nothing
    cnt.value = -7
    assert tri(0, None, None, 1, 2.0, 0, None, C.byref(cnt)) == 0 and cnt.value == 0
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert lib.ngpde_delaunay_last_passes(C.byref(a), C.byref(b)) == 0 and (a.value, b.value) == (0, 0)
    assert lib.ngpde_delaunay_last_passes(None, None) == 0


# ---- the Python errors come before the library -----------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def entered():
        raise AssertionError("the library was entered")
    monkeypatch.setattr(_lib, "load", entered)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_wrong_sizes_and_dim_are_refused_before_the_library(no_library):
    M = ng.mesh
    pts = np.zeros((2, 5), np.float32)
    cases = [
        lambda: M.delaunay_graph(np.zeros((3, 5), np.float32)),                      # dim != 2
        lambda: M.delaunay_graph(np.zeros((1, 5), np.float32)),
        lambda: M.delaunay_graph(np.zeros(5, np.float32)),
        lambda: M.delaunay_graph(np.zeros((2, 5, 1))),
        lambda: M.delaunay_graph(pts, graph_indicator=np.ones(4, np.int64)),
        lambda: M.delaunay_triangles(torch.zeros(3, 5)),
        lambda: M.delaunay_triangles(pts, graph_indicator=torch.ones(6, dtype=torch.int64)),
    ]
    for call in cases:
        with pytest.raises(ng.DimensionMismatch, match="DimensionMismatch"):
            call()
    with pytest.raises(ng.ArgumentError, match="max_edge_length"):
        M.delaunay_graph(pts, max_edge_length=-1.0)
    with pytest.raises(ng.ArgumentError, match="max_edge_length"):
        M.delaunay_triangles(pts, max_edge_length=float("nan"))
    with pytest.raises(ng.ArgumentError, match="complex"):
        M.delaunay_graph(pts.astype(np.complex64))
    with pytest.raises(ValueError, match="dir must be"):
        M.delaunay_graph(pts, dir="both")


def test_a_well_shaped_call_without_a_device_names_the_missing_device(no_library):
    M = ng.mesh
    pts = torch.zeros(2, 5)
    for call in (lambda: M.delaunay_graph(pts), lambda: M.delaunay_triangles(pts, max_edge_length=0.5),
                 lambda: M.delaunay_graph(pts, graph_indicator=np.ones(5, np.int64))):
        with pytest.raises(ng.NgpdeError, match="no HIP device.*no CPU fallback") as e:
            call()
        assert e.value.code == _lib.ERR_HIP


# ---- the restatement on the clouds the GPU tests use --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniform", "clustered", "circle"])
def test_the_restatement_equals_qhull_away_from_ties(kind):
    for seed in (0, 1, 2):                                               # (seed 0 of each kind is the GPU test's input)
        p = S.cloud(kind, seed)
        d = Delaunay(p.astype(np.float64))
        assert S.min_margin(p, d.simplices) >= 1024 * S.TIE_BOUND        # Qhull alone: no tested decision is in the doubt zone
        e = S.edges_brute(p)
        assert np.array_equal(e, S.edges_of_simplices(d.simplices))
        assert np.array_equal(S.triangles_from_rows(p, e), S.canonical_triangles(p, d.simplices))
        if kind == "circle":
            assert np.bincount(e[:, 0])[-1] == len(p) - 1                # the centre is joined to every point


@pytest.mark.parametrize("shape,edges", [((5, 4), 55), ((7, 7), 156)])
def test_the_restatement_gives_the_8_neighbour_stencil_on_a_lattice(shape, edges):
    p = S.lattice(*shape)
    e = S.edges_brute(p)
    assert np.array_equal(e, S.stencil8(*shape)) and len(e) == 2 * edges
    tri = S.triangles_from_rows(p, e)
    area2 = lambda t: (p[t[1], 0] - p[t[0], 0]) * (p[t[2], 1] - p[t[0], 1]) - (p[t[1], 1] - p[t[0], 1]) * (p[t[2], 0] - p[t[0], 0])
    assert all(area2(t) == 1.0 for t in tri)                             # half squares, counter-clockwise
    assert sum(area2(t) for t in tri) > 2 * (shape[0] - 1) * (shape[1] - 1)          # tied triangles overlap


def test_the_filter_is_the_float32_rule():
    p = S.cloud("uniform", 0)
    e = S.edges_brute(p)
    i, j = e[5]
    dx, dy = np.float32(p[i, 0] - p[j, 0]), np.float32(p[i, 1] - p[j, 1])
    d2 = np.float32(np.float32(dx * dx) + np.float32(dy * dy))
    r = np.float32(np.sqrt(d2))
    keep = bool(d2 <= np.float32(r * r))
    assert ([int(i), int(j)] in S.filter_edges(p, e, float(r)).tolist()) == keep
    assert len(S.filter_edges(p, e, math.inf)) == len(e) and len(S.filter_edges(p, e, 0.0)) == 0


# ---- csrc/delaunay_star.h against an exact brute force ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("delaunay_star") / "delaunay_star_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "host", "delaunay_star_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    return r.returncode, r.stdout, r.stdout + r.stderr


def test_every_star_equals_the_exact_brute_force(report):
    code, out, text = report
    assert code == 0, text[-4000:]
    assert "AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-4000:]
    m = re.search(r"^(\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 300000, text[-4000:]


def test_the_clouds_reach_ties_unbounded_cells_stops_and_a_hub(report):
    _, out, text = report
    rows = {m.group(1): tuple(map(int, m.groups()[1:])) for m in re.finditer(
        r"^(\w+): (\d+) points, (\d+) edges, largest cell (\d+), largest degree (\d+), (\d+) unbounded cells, (\d+) stops$", out, re.M)}
    assert set(rows) == {"random", "lattice", "collinear", "circle", "three", "two", "hub"}, text[-4000:]
    assert rows["lattice"][1] == 55 and rows["lattice"][3] == 8
    assert rows["collinear"][1] == rows["collinear"][0] - 1 and rows["collinear"][3] == 2
    n = rows["circle"][0]
    assert rows["circle"][1] == n * (n - 1) // 2                         # cocircular: every pair is tied and kept
    assert rows["three"][1] == 3 and rows["two"][1] == 1
    assert rows["hub"][1] == 2 * n and rows["hub"][3] == n and rows["hub"][2] > 24
    assert rows["random"][5] > 0 and rows["random"][4] > 0               # the stop was taken, and hull points have unbounded cells


def test_the_kernels_use_the_headers_geometry():
    src = open(os.path.join(CSRC, "delaunay.hip"), encoding="utf-8").read()
    assert '#include "delaunay_star.h"' in src and '#include "neighbor_cells.h"' in src
    for call in ("clip(P, &m, kLaneCap, l, line_of)", "is_cut(", "cross_vertex(", "touches(", "certified(r2max, ring_reach2(cl.g, ring))", "rho2("):
        assert call in src, call
    for own in ("double kU", "kTieBound =", "bool certified("):
        assert own not in src, own
