"""The coarsening block (include/ngpde_coarsen.h, _lib.COARSEN_SIGNATURES, ngpde_amd.coarsen) held, on the host, to what
tests/test_abi.py, tests/test_interp_host.py and tests/test_mesh_host.py hold the first three blocks to: the header equals the
binding table and the library exports it; the other headers and tables declare none of it; `stream` is the last parameter; the
Python wrappers raise every argument refusal by name before a device is asked for; ngpde_fps_plan_create refuses bad host tables
without a device.  csrc/coarsen_rule.h -- the selection comparator, the cell / key rule and the plan's work layout -- runs against a
plain brute force in tests/host/coarsen_rule_check.cpp, a stand-alone program under ASan + UBSan.  No GPU.
"""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

import coarsen_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "neuralgraphpde.jl_amd", "csrc")
INVALID = _lib.ERR_INVALID_ARGUMENT
K = ng.coarsen


def functions_of(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ngpde_[a-z0-9_]+)\s*\(", src)))


# ---- header, table, module -------------------------------------------------------------------------------------------------------
def test_header_and_binding_table_agree():
    assert functions_of("ngpde_coarsen.h") == sorted(_lib.COARSEN_SIGNATURES)
    assert len(_lib.COARSEN_SIGNATURES) == 8


def test_library_exports_every_symbol_with_its_types():
    lib = _lib.load()
    for name, (res, args) in _lib.COARSEN_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_the_other_headers_and_tables_declare_none_of_them():
    for header, table in (("ngpde.h", _lib.SIGNATURES), ("ngpde_interp.h", _lib.INTERP_SIGNATURES), ("ngpde_mesh.h", _lib.MESH_SIGNATURES)):
        assert not set(functions_of(header)) & set(_lib.COARSEN_SIGNATURES)
        assert not set(table) & set(_lib.COARSEN_SIGNATURES)
    src = open(os.path.join(ROOT, "include", "ngpde_coarsen.h")).read()
    assert '#include "ngpde.h"' in src
    for cite in ("THE RULE", "LARGEST KEY", "SMALLEST\n *      INDEX", "no fused multiply-add", "ORDER CONTRACT", "PRECONDITION",
                 "cell size too small for the cloud's extent", "BITWISE EQUAL"):
        assert cite in src, cite
    cap = int(re.search(r"#define NGPDE_FPS_TILE_MAX_POINTS (\d+)", src).group(1))
    threads = int(re.search(r"#define NGPDE_FPS_TILE_THREADS (\d+)", src).group(1))
    assert cap == S.TILE_MAX_POINTS == K.TILE_MAX_POINTS >= 16384 and threads == S.TILE_THREADS == K.TILE_THREADS
    rule = open(os.path.join(CSRC, "coarsen_rule.h")).read()
    assert "hip/" not in rule and "kFpsTileMaxPoints = kFpsTileThreads * kFpsTileMaxPerThread" in rule      # host-includable; the cap's one definition


def test_every_stream_entry_of_the_header_ends_with_the_stream():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngpde_coarsen.h")).read(), flags=re.S)
    protos = re.findall(r"\b(ngpde_[a-z0-9_]+)\s*\(([^)]*)\)", src)
    with_stream = sorted(name for name, args in protos if "ngpde_stream_t" in args)
    assert with_stream == ["ngpde_cluster_pool_backward", "ngpde_cluster_pool_forward", "ngpde_fps", "ngpde_fps_plan_create", "ngpde_grid_cluster"]
    for name, args in protos:
        if name == "ngpde_fps_plan_create":                                   # a create: the handle it returns comes last, as in ngpde_readout_create
            assert args.strip().endswith("ngpde_stream_t stream, ngpde_fps_plan_t **plan"), name
        elif name in with_stream:
            assert args.strip().endswith("ngpde_stream_t stream"), name


def test_the_module_is_a_submodule_with_its_own_names():
    assert K.__all__ == ["fps", "grid_cluster", "Clusters", "pool", "pool_positions", "pool_graph"]
    for name in K.__all__:
        assert name not in ng.__all__ and callable(getattr(K, name))
    assert "coarsen" not in ng.__all__
    assert callable(K.Clusters.from_labels) and callable(K.Clusters.unpool)


def test_the_kernels_use_the_headers_rules_and_read_no_environment():
    src = open(os.path.join(CSRC, "coarsen.hip"), encoding="utf-8").read()
    assert '#include "coarsen_rule.h"' in src and '#include "row_lanes.h"' in src and '#include "coo_compact.h"' in src
    for call in ("pick(", "better(", "updated_key(", "dist2<DIM>(", "fps_layout(", "cell_quotient(", "cell_fits(", "key_bits(", "cell_key("):
        assert call in src, call
    assert "getenv" not in src and "atomicAdd" not in src
    fps_part = src[src.index("the tile path"):src.index("grid clusters ---")]
    assert "atomic" not in fps_part                                          # neither FPS kernel uses an atomic


# ---- the C entries refuse by name, without a device ------------------------------------------------------------------------------
def _refused(status, *words):
    msg = _lib.load().ngpde_last_error().decode()
    assert status == INVALID, (status, msg)
    for w in words:
        assert w in msg, msg


def _create(graph_ptr, sample_ptr, dim=2, path=0, n_graphs=None):
    lib = _lib.load()
    gp = None if graph_ptr is None else np.asarray(graph_ptr, dtype=np.int64)
    sp = None if sample_ptr is None else np.asarray(sample_ptr, dtype=np.int64)
    plan = C.c_void_p(7)
    G = (len(gp) - 1) if n_graphs is None else n_graphs
    st = lib.ngpde_fps_plan_create(G, _lib.ptr(gp), _lib.ptr(sp), dim, path, None, C.byref(plan))
    return st, plan


def test_fps_plan_create_refuses_bad_host_tables_without_a_device():
    lib = _lib.load()
    cap = S.TILE_MAX_POINTS
    cases = [
        (dict(graph_ptr=[0, 5, 3], sample_ptr=[0, 1, 2]), ("graph_ptr decreases", "graph 1")),
        (dict(graph_ptr=[0, 5, 9], sample_ptr=[0, 2, 1]), ("sample_ptr decreases", "graph 1")),
        (dict(graph_ptr=[0, 5, 9], sample_ptr=[0, 2, 7]), ("graph 1 has 4 points, 5 samples",)),
        (dict(graph_ptr=[1, 5], sample_ptr=[0, 2]), ("must start at 0",)),
        (dict(graph_ptr=[0, 5], sample_ptr=[0, 2], dim=0), ("dim must be 1, 2 or 3",)),
        (dict(graph_ptr=[0, 5], sample_ptr=[0, 2], dim=4), ("dim must be 1, 2 or 3",)),
        (dict(graph_ptr=[0, 5], sample_ptr=[0, 2], path=3), ("path must be",)),
        (dict(graph_ptr=[0, 5], sample_ptr=[0, 2], n_graphs=-1), ("n_graphs",)),
        (dict(graph_ptr=None, sample_ptr=[0, 2], n_graphs=1), ("is NULL",)),
        (dict(graph_ptr=[0, 4, 4 + cap + 1], sample_ptr=[0, 2, 4], path=1), ("graph 1", "FPS_TILE_MAX_POINTS = ", str(cap + 1))),
        (dict(graph_ptr=[0, 2 ** 31], sample_ptr=[0, 1], path=2), ("graph 0", "2^31")),
    ]
    for kw, words in cases:
        st, plan = _create(**kw)
        _refused(st, "fps_plan_create", *words)
        assert plan.value is None                                          # a refused create leaves NULL
    _refused(lib.ngpde_fps_plan_create(1, None, None, 2, 0, None, None), "plan is NULL")
    # a plan without work touches no device: it can be made, asked and destroyed here
    st, plan = _create([0, 0, 7, 7], [0, 0, 0, 0])
    assert st == 0 and plan.value
    info = (C.c_int64 * 6)()
    assert lib.ngpde_fps_plan_info(plan, info) == 0 and list(info) == [7, 0, 0, 0, 0, 0]
    assert lib.ngpde_fps_workspace_bytes(plan) == 0
    assert lib.ngpde_fps(plan, None, None, 0, None, None, None, 0, None) == 0      # no samples: nothing to do
    assert lib.ngpde_fps_plan_destroy(plan) == 0 and lib.ngpde_fps_plan_destroy(None) == 0
    _refused(lib.ngpde_fps_plan_info(None, info), "NULL")
    _refused(lib.ngpde_fps(None, None, None, 0, None, None, None, 0, None), "plan is NULL")
    assert lib.ngpde_fps_workspace_bytes(None) == 0


def test_grid_cluster_and_pool_entries_refuse_by_name():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    out = (C.c_int32 * 64)()
    p, o = C.addressof(buf), C.addressof(out)
    cnt = C.c_int64(-7)
    f32 = lambda *v: np.asarray(v, dtype=np.float32)
    i64 = lambda *v: np.asarray(v, dtype=np.int64)
    P = _lib.ptr

    def grid(n=4, dim=2, pts=p, G=1, gp=i64(0, 4), size=f32(1, 1), origin=None, count=cnt):
        return lib.ngpde_grid_cluster(n, dim, pts, G, P(gp), P(size), P(origin), o, o, o, o, None if count is None else C.byref(count), None)
    _refused(grid(count=None), "grid_cluster", "count pointer is NULL")
    _refused(grid(n=-1), "number of points")
    _refused(grid(dim=4), "dim must be 1, 2 or 3")
    _refused(grid(G=0), "n_graphs")
    _refused(grid(gp=None), "is NULL")
    _refused(grid(gp=i64(0, 3)), "graph_ptr must run from 0 to n")
    _refused(grid(G=2, gp=i64(0, 5, 4)), "graph_ptr decreases at graph 1")
    _refused(grid(size=f32(1, 0)), "size[1]", "finite and > 0")
    _refused(grid(size=f32(-1, 1)), "size[0]")
    _refused(grid(size=f32(np.inf, 1)), "size[0]")
    _refused(grid(size=f32(np.nan, 1)), "size[0]")
    _refused(grid(origin=f32(0, np.nan)), "origin[1]")
    _refused(grid(pts=None), "is NULL")
    assert cnt.value == -7                                                  # refused calls write nothing
    fwd = lambda n, c, d, aggr, ptr=o, order=o, x=p, y=p: lib.ngpde_cluster_pool_forward(n, c, d, aggr, ptr, order, x, y, None)
    assert fwd(4, 2, 0, 0) == _lib.ERR_DIMENSION_MISMATCH and "feature width" in lib.ngpde_last_error().decode()
    _refused(fwd(4, 2, 3, 4), "cluster_pool_forward", "aggr")
    _refused(fwd(-1, 2, 3, 0), "number of points")
    _refused(fwd(4, -2, 3, 0), "number of clusters")
    _refused(fwd(4, 2, 3, 0, ptr=None), "ptr or out is NULL")
    _refused(fwd(4, 2, 3, 0, x=None), "order or x is NULL")
    assert fwd(4, 0, 3, 0, None, None, None, None) == 0                       # no clusters: nothing to do
    bwd = lambda n, c, d, aggr, lab=o, ptr=o, x=p, y=p, dy=p, dx=p: lib.ngpde_cluster_pool_backward(n, c, d, aggr, lab, ptr, x, y, dy, dx, None)
    assert bwd(4, 2, -1, 0) == _lib.ERR_DIMENSION_MISMATCH
    _refused(bwd(4, 2, 3, 7), "cluster_pool_backward", "aggr")
    _refused(bwd(4, 2, 3, 0, lab=None), "labels or dx is NULL")
    _refused(bwd(4, 2, 3, 0, dy=None), "dout is NULL")
    _refused(bwd(4, 2, 3, 1, ptr=None), "ptr is NULL")
    _refused(bwd(4, 2, 3, 2, x=None), "x or out is NULL")
    assert bwd(0, 2, 3, 0, None, None, None, None, None, None) == 0


# ---- the Python errors come before the library -----------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def entered():
        raise AssertionError("the library was entered")
    monkeypatch.setattr(_lib, "load", entered)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_wrong_shapes_are_refused_before_the_library(no_library):
    pts = np.zeros((2, 6), np.float32)
    cl = K.Clusters(torch.zeros(6, dtype=torch.int32), 1, torch.tensor([0, 6], dtype=torch.int32), torch.arange(6, dtype=torch.int32),
                    torch.ones(1, dtype=torch.int32), 1)
    g = ng.GNNGraph([1, 2], [2, 3], num_nodes=5)
    cases = [
        lambda: K.fps(np.zeros((4, 6), np.float32), num=1),                          # dim outside 1:3
        lambda: K.fps(np.zeros((2, 6, 1)), num=1),
        lambda: K.fps(pts, num=1, graph_indicator=np.ones(5, np.int64)),
        lambda: K.fps(pts, num=1, start=[0, 1]),                                     # one start per graph
        lambda: K.grid_cluster(np.zeros((4, 6), np.float32), 1.0),
        lambda: K.grid_cluster(pts, 1.0, graph_indicator=torch.ones(7, dtype=torch.int64)),
        lambda: K.grid_cluster(pts, [1.0, 2.0, 3.0]),
        lambda: K.grid_cluster(pts, 1.0, origin=[0.0]*3),
        lambda: K.pool(cl, np.zeros((3, 5), np.float32), "+"),
        lambda: K.pool(cl, np.zeros(6, np.float32), "+"),
        lambda: K.pool_positions(cl, np.zeros((2, 7), np.float32)),
        lambda: cl.unpool(np.zeros((3, 2), np.float32)),
        lambda: K.pool_graph(g, cl),
        lambda: K.Clusters.from_labels(np.zeros(6, np.int64), graph_indicator=np.ones(5, np.int64)),
    ]
    for i, call in enumerate(cases):
        with pytest.raises(ng.DimensionMismatch, match="DimensionMismatch"):
            call()


def test_every_argument_refusal_is_named_before_a_device_is_asked_for(no_library):
    pts = np.arange(12, dtype=np.float32).reshape(2, 6)
    gi = np.array([1, 1, 1, 2, 2, 2])
    refusals = [
        (lambda: K.fps(pts), "exactly one of num and ratio"),
        (lambda: K.fps(pts, num=2, ratio=0.5), "exactly one of num and ratio"),
        (lambda: K.fps(pts, ratio=0.0), r"ratio must lie in \(0, 1\]"),
        (lambda: K.fps(pts, ratio=1.5), r"ratio must lie in \(0, 1\]"),
        (lambda: K.fps(pts, num=-1), "num must be >= 0"),
        (lambda: K.fps(pts, num=2.5), "num must be an integer"),
        (lambda: K.fps(pts, num=[1, 2, 3], graph_indicator=gi), "one integer per graph"),
        (lambda: K.fps(pts, num=7), "graph 1 has 6 points, 7 samples"),
        (lambda: K.fps(pts, num=[3, 4], graph_indicator=gi), "graph 2 has 3 points, 4 samples"),
        (lambda: K.fps(pts, num=1, graph_indicator=[1, 1, 2, 1, 2, 2]), "non-decreasing.*decreases at position 3"),
        (lambda: K.fps(pts, num=1, graph_indicator=torch.tensor([2, 2, 2, 1, 1, 1])), "decreases at position 3"),
        (lambda: K.fps(pts, num=1, graph_indicator=[0, 0, 0, 1, 1, 1]), "1-based"),
        (lambda: K.fps(pts, num=1, start=[6]), "start 6 lies outside graph 1"),
        (lambda: K.fps(pts, num=1, start=[0, 2], graph_indicator=gi), "start 2 lies outside graph 2, whose points are 3:5"),
        (lambda: K.fps(pts, num=1, start=[-1]), "start -1 lies outside graph 1"),
        (lambda: K.fps(pts, num=1, start=[0], random_start=True), "exclude each other"),
        (lambda: K.fps(pts, num=1, random_start=True, seed=-3), "seed"),
        (lambda: K.fps(pts.astype(np.complex64), num=1), "complex"),
        (lambda: K.grid_cluster(pts, 0.0), "size must be finite and > 0"),
        (lambda: K.grid_cluster(pts, [1.0, -2.0]), "size must be finite and > 0"),
        (lambda: K.grid_cluster(pts, float("inf")), "size must be finite and > 0"),
        (lambda: K.grid_cluster(pts, float("nan")), "size must be finite and > 0"),
        (lambda: K.grid_cluster(pts, 1.0, origin=[0.0, float("nan")]), "origin must be finite"),
        (lambda: K.grid_cluster(pts, 1.0, graph_indicator=[1, 2, 1, 2, 2, 2]), "decreases at position 2"),
    ]
    for call, words in refusals:
        with pytest.raises(ng.ArgumentError, match=words) as e:
            call()
        assert e.value.code == INVALID
    cl = K.Clusters(torch.zeros(6, dtype=torch.int32), 1, torch.tensor([0, 6], dtype=torch.int32), torch.arange(6, dtype=torch.int32),
                    torch.ones(1, dtype=torch.int32), 1)
    with pytest.raises(ng.ArgumentError, match="unsupported aggregation"):
        K.pool(cl, pts, "*")
    with pytest.raises(ng.ArgumentError, match="unsupported aggregation"):
        K.pool_graph(ng.GNNGraph([1, 2], [2, 3], num_nodes=6), cl, aggr="prod")


def test_a_well_formed_call_without_a_device_names_the_missing_device(no_library):
    pts = torch.zeros(2, 6)
    gi = np.array([1, 1, 1, 3, 3, 3])                                       # graph 2 is empty: fine
    for call in (lambda: K.fps(pts, num=2), lambda: K.fps(pts, ratio=0.5, graph_indicator=gi, start=[1, 3, 4]),
                 lambda: K.fps(pts, num=[3, 0, 0], graph_indicator=gi, random_start=True, seed=4),
                 lambda: K.grid_cluster(pts, [1.0, 2.0], graph_indicator=gi), lambda: K.grid_cluster(pts, 0.5, origin=[0.0, 0.0]),
                 lambda: K.Clusters.from_labels([0, 0, 1, 1, 2, 2])):
        with pytest.raises(ng.NgpdeError, match="no HIP device.*no CPU fallback") as e:
            call()
        assert e.value.code == _lib.ERR_HIP


def test_the_sample_counts_and_the_drawn_starts_are_the_documented_ones():
    ptr = np.array([0, 3, 3, 10, 3010], dtype=np.int64)
    assert K._sample_counts(None, 0.25, ptr).tolist() == [1, 0, 2, 750]      # math.ceil(ratio * n_g)
    assert K._sample_counts(None, 1.0, ptr).tolist() == [3, 0, 7, 3000]
    assert K._sample_counts(0, None, ptr).tolist() == [0, 0, 0, 0]
    assert K._sample_counts([3, 0, 7, 1], None, ptr).tolist() == [3, 0, 7, 1]
    assert K._graph_ptr(torch.tensor([1, 1, 1, 3, 3, 4]), 6).tolist() == [0, 3, 3, 5, 6]
    gen = torch.Generator()
    gen.manual_seed(11)
    want = [int(ptr[g]) + (int(torch.randint(int(ptr[g + 1] - ptr[g]), (1,), generator=gen)) if ptr[g + 1] > ptr[g] else 0) for g in range(4)]
    got = K._starts(None, True, 11, ptr)
    assert got.dtype == np.int32 and got.tolist() == want and K._starts(None, True, 11, ptr).tolist() == want
    assert all(ptr[g] <= want[g] < ptr[g + 1] for g in (0, 2, 3))
    assert K._starts(None, False, None, ptr) is None


# ---- the restatement, on inputs whose answer is known by hand ------------------------------------------------------------------------
def test_the_restatement_on_hand_checked_inputs():
    line = np.array([[0.0], [1.0], [2.0], [3.0], [10.0]], dtype=np.float32)
    idx, d2 = S.fps_graph(line, 5)
    assert idx.tolist() == [0, 4, 3, 1, 2] and d2.tolist() == [np.inf, 100.0, 9.0, 1.0, 1.0]      # 1 and 2 tie at distance 1: the smaller index
    idx, _ = S.fps_graph(line, 3, start=2)
    assert idx.tolist() == [2, 4, 0]
    same = np.zeros((4, 2), np.float32)
    assert S.fps_graph(same, 4, start=2)[0].tolist() == [2, 0, 1, 3]         # coincident: index order once all keys are 0
    pts = np.array([[0.0, 0.0], [1.9, 0.0], [2.0, 0.0], [0.0, 2.0], [5.0, 5.0], [5.5, 5.0]], dtype=np.float32)
    ref = S.grid_cluster_brute(pts, 2.0, [0, 4, 6])
    assert ref["labels"].tolist() == [0, 0, 1, 2, 3, 3] and ref["count"] == 4 and ref["graph_indicator"].tolist() == [1, 1, 1, 2]
    assert ref["ptr"].tolist() == [0, 2, 3, 4, 6] and ref["order"].tolist() == [0, 1, 2, 3, 4, 5]
    assert S.grid_cluster_brute(pts, 2.0, [0, 4, 6], origin=[0.5, 0.0]) == "below"
    assert S.grid_cluster_brute(pts * np.float32(1e6), 1e-4, [0, 6]) == "too small"
    out, mag, sizes = S.pool_ref(np.array([[1.0], [2.0], [4.0]], np.float32), np.array([0, 1, 0]), 2, "mean")
    assert out.tolist() == [[2.5], [2.0]] and sizes.tolist() == [2, 1]


# ---- csrc/coarsen_rule.h against a plain brute force ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("coarsen_rule") / "coarsen_rule_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "host", "coarsen_rule_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    return r.returncode, r.stdout, r.stdout + r.stderr


def test_the_rules_equal_the_brute_force(report):
    code, out, text = report
    assert code == 0, text[-4000:]
    assert "AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-4000:]
    m = re.search(r"^(\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 1000000, text[-4000:]


def test_the_inputs_reach_ties_both_paths_and_every_regime(report):
    _, out, text = report
    rows = [tuple([m.group(1)] + list(map(int, m.groups()[1:]))) for m in re.finditer(
        r"^(\w+): (\d+) points, dim (\d+), (\d+) samples, (\d+) tied rounds, (\d+) mismatches$", out, re.M)]
    names = {r[0] for r in rows}
    assert names == {"random", "slices", "lattice", "coincident", "underflow", "denormal", "overflow"}, text[-4000:]
    assert all(r[5] == 0 for r in rows)
    by = {r[0]: r for r in rows}
    assert by["lattice"][4] >= 40 and by["coincident"][4] >= 9 and by["underflow"][4] >= 98 and by["overflow"][4] > 0
    assert by["slices"][1] > 2 * 2048 and {r[2] for r in rows if r[0] == "random"} == {1, 2, 3}
    m = re.search(r"^layout: (\d+) graphs on the tile path, (\d+) on the round path$", out, re.M)
    assert m and int(m.group(1)) > 100 and int(m.group(2)) > 100, text[-4000:]
    m = re.search(r"^cells: (\d+) key pairs ordered$", out, re.M)
    assert m and int(m.group(1)) > 100000
