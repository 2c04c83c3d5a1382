"""The two-set search and k-NN interpolation block (include/ngpde_interp.h, _lib.INTERP_SIGNATURES, ngpde_amd.interp) held, on the
host, to what tests/test_abi.py, tests/test_host_api.py and tests/test_neighbor_grid_host.py hold the first block to: the header
equals the binding table and the library exports it; the first header and `ng.__all__` are untouched by it; every entry refuses
NULL or negative arguments by name without a device; the Python wrappers raise their size errors before the library is entered and
the no-device error on a well-shaped call; the numpy restatements of tests/interp_spec.py equal plain Python loops on <= 12
points; and csrc/neighbor_grid.h's cell_of_query keeps covering and the ring bound for clamped queries
(tests/host/neighbor_query_check.cpp, a stand-alone program under ASan + UBSan).  No GPU.
"""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

import interp_spec as S

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
    assert functions_of("ngpde_interp.h") == sorted(_lib.INTERP_SIGNATURES)
    assert len(_lib.INTERP_SIGNATURES) == 7


def test_library_exports_every_symbol_with_its_types():
    lib = _lib.load()
    for name, (res, args) in _lib.INTERP_SIGNATURES.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def test_the_first_header_and_table_declare_none_of_them():
    first = functions_of("ngpde.h")
    assert not set(first) & set(_lib.INTERP_SIGNATURES)
    assert not set(_lib.SIGNATURES) & set(_lib.INTERP_SIGNATURES)
    src = open(os.path.join(ROOT, "include", "ngpde_interp.h")).read()
    assert '#include "ngpde.h"' in src
    for cite in ("docs/src/tutorials/VMH.md:53", "src/NeuralGraphPDE.jl:4", "NearestNeighbors", "knn_interpolate", "FLT_MIN",
                 "no gradient to the positions"):
        assert cite in src, cite


def test_every_stream_entry_of_the_header_ends_with_the_stream():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngpde_interp.h")).read(), flags=re.S)
    protos = re.findall(r"\b(ngpde_[a-z0-9_]+)\s*\(([^)]*)\)", src)
    with_stream = [name for name, args in protos if "ngpde_stream_t" in args]
    assert sorted(with_stream) == sorted(n for n in _lib.INTERP_SIGNATURES if not n.endswith("_workspace_bytes"))
    for name, args in protos:
        if name in with_stream:
            assert args.strip().endswith("ngpde_stream_t stream"), name


def test_the_module_is_a_submodule_with_its_own_names():
    assert ng.interp.__all__ == ["knn", "inrange", "KNNInterpolator", "knn_interpolate"]
    for name in ng.interp.__all__:
        assert name not in ng.__all__ and callable(getattr(ng.interp, name))
    assert "interp" not in ng.__all__


# ---- the C entries refuse by name, without a device ------------------------------------------------------------------------------
def _refused(status, *words):
    msg = _lib.load().ngpde_last_error().decode()
    assert status == INVALID, (status, msg)
    for w in words:
        assert w in msg, msg


def test_search_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    out = (C.c_int32 * 64)()
    p, o = C.addressof(buf), C.addressof(out)
    found = C.c_int64(-7)
    knn = lambda n, m, pts, qs, k, gp, gq, ng_, idx: lib.ngpde_knn_query(n, m, 2, pts, qs, k, gp, gq, ng_, 1, 0, idx, None, None)
    _refused(knn(-1, 4, p, p, 1, None, None, 1, o), "knn_query", "points")
    _refused(knn(4, -1, p, p, 1, None, None, 1, o), "knn_query", "queries")
    _refused(knn(4, 4, None, p, 1, None, None, 1, o), "points is NULL")
    _refused(knn(4, 4, p, None, 1, None, None, 1, o), "queries is NULL")
    _refused(knn(4, 4, p, p, 1, None, None, 0, o), "n_graphs")
    _refused(knn(4, 4, p, p, 1, None, None, 2, o), "point_graph_id")
    _refused(knn(4, 4, p, p, 1, None, None, 1, None), "idx is NULL")
    _refused(knn(4, 4, p, p, 5, None, None, 1, o), "fewer than k = 5")
    _refused(knn(4, 4, p, p, -1, None, None, 1, o), "k must be")
    assert knn(4, 4, p, p, 129, None, None, 1, o) == _lib.ERR_UNSUPPORTED
    assert lib.ngpde_knn_query(4, 4, 4, p, p, 1, None, None, 1, 1, 0, o, None, None) == _lib.ERR_UNSUPPORTED
    assert knn(4, 0, p, None, 3, None, None, 1, None) == 0 and knn(4, 4, p, p, 0, None, None, 1, None) == 0     # nothing to do

    rad = lambda n, m, pts, qs, r, cap, ptr, nbr, nf: lib.ngpde_radius_query(n, m, 2, pts, qs, r, None, None, 1, 1, 0, cap, ptr, nbr, nf, None)
    _refused(rad(-1, 4, p, p, 1.0, 0, None, None, C.byref(found)), "radius_query", "points")
    _refused(rad(4, 4, None, p, 1.0, 0, None, None, C.byref(found)), "points is NULL")
    _refused(rad(4, 4, p, None, 1.0, 0, None, None, C.byref(found)), "queries is NULL")
    _refused(rad(4, 4, p, p, 1.0, 0, None, None, None), "n_found is NULL")
    _refused(rad(4, 4, p, p, -1.0, 0, None, None, C.byref(found)), "radius")
    _refused(rad(4, 4, p, p, float("nan"), 0, None, None, C.byref(found)), "radius")
    _refused(rad(4, 4, p, p, 1.0, 8, None, o, C.byref(found)), "ptr")
    _refused(rad(4, 4, p, p, 1.0, -1, o, o, C.byref(found)), "capacity")
    assert found.value == -7                                            # refused calls write nothing
    assert rad(0, 0, None, None, 1.0, 0, None, None, C.byref(found)) == 0 and found.value == 0


def test_interpolation_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    _refused(lib.ngpde_knn_interp_weights(-1, 3, p, p, None), "knn_interp_weights", "queries")
    _refused(lib.ngpde_knn_interp_weights(4, -3, p, p, None), "k must be")
    _refused(lib.ngpde_knn_interp_weights(4, 3, None, p, None), "NULL")
    _refused(lib.ngpde_knn_interp_weights(4, 3, p, None, None), "NULL")
    assert lib.ngpde_knn_interp_weights(0, 3, None, None, None) == 0

    fwd = lib.ngpde_knn_interp_forward
    _refused(fwd(-1, 4, 3, 2, p, p, p, p, None), "knn_interp_forward", "points")
    _refused(fwd(4, -4, 3, 2, p, p, p, p, None), "queries")
    _refused(fwd(4, 4, -3, 2, p, p, p, p, None), "k must be")
    _refused(fwd(4, 4, 3, 0, p, p, p, p, None), "feature width")
    _refused(fwd(4, 4, 3, 2, p, p, p, None, None), "y is NULL")
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        _refused(fwd(4, 4, 3, 2, *args, p, None), "NULL")
    assert fwd(4, 0, 3, 2, None, None, None, None, None) == 0

    size = lib.ngpde_knn_interp_transpose_workspace_bytes
    assert size(-1, 4, 3) == 0 and size(4, -4, 3) == 0 and size(4, 4, -3) == 0 and size(4, 2 ** 30, 4) == 0
    assert size(4, 0, 3) == 0 and size(0, 4, 3) == 256 and size(10, 100, 3) == 1280 and size(10, 64, 1) == 256 and size(10, 65, 1) == 512
    tr = lib.ngpde_knn_interp_transpose
    _refused(tr(-1, 4, 3, p, p, p, p, 4096, None), "knn_interp_transpose", "points")
    _refused(tr(4, 4, -3, p, p, p, p, 4096, None), "k must be")
    _refused(tr(4, 4, 3, p, None, p, p, 4096, None), "ptr is NULL")
    _refused(tr(4, 4, 3, None, p, p, p, 4096, None), "NULL")
    _refused(tr(4, 4, 3, p, p, None, p, 4096, None), "NULL")
    assert tr(4, 4, 3, p, p, p, None, 4096, None) == _lib.ERR_WORKSPACE and b"256 needed" in lib.ngpde_last_error()
    assert tr(4, 4, 3, p, p, p, p, 255, None) == _lib.ERR_WORKSPACE

    bwd = lib.ngpde_knn_interp_backward
    _refused(bwd(-1, 4, 3, 2, p, p, p, p, p, None), "knn_interp_backward", "points")
    _refused(bwd(4, -4, 3, 2, p, p, p, p, p, None), "queries")
    _refused(bwd(4, 4, 3, 0, p, p, p, p, p, None), "feature width")
    _refused(bwd(4, 4, 3, 2, p, p, p, p, None, None), "xbar is NULL")
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        _refused(bwd(4, 4, 3, 2, *args, p, None), "NULL")
    assert bwd(0, 4, 3, 2, None, None, None, None, None, None) == 0


# ---- the Python errors come before the library -----------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def entered():
        raise AssertionError("the library was entered")
    monkeypatch.setattr(_lib, "load", entered)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)


def test_wrong_sizes_are_dimension_mismatches_before_the_library(no_library):
    I = ng.interp
    pts, qs = np.zeros((2, 5), np.float32), np.zeros((2, 7), np.float32)
    cases = [
        lambda: I.knn(pts, np.zeros((3, 7), np.float32), 2),
        lambda: I.knn(np.zeros((4, 5)), np.zeros((4, 7)), 2),
        lambda: I.knn(np.zeros((2, 5, 1)), qs, 2),
        lambda: I.knn(pts, qs, 2, graph_indicator=np.ones(4, np.int64), query_graph_indicator=np.ones(7, np.int64)),
        lambda: I.knn(pts, qs, 2, graph_indicator=np.ones(5, np.int64), query_graph_indicator=np.ones(6, np.int64)),
        lambda: I.inrange(pts, np.zeros((1, 7), np.float32), 0.5),
        lambda: I.inrange(pts, qs, 0.5, query_graph_indicator=np.ones(8, np.int64)),
        lambda: I.KNNInterpolator(pts, np.zeros((3, 7), np.float32)),
        lambda: I.knn_interpolate(np.zeros((4, 6), np.float32), pts, qs),
        lambda: I.knn_interpolate(np.zeros(5, np.float32), pts, qs),
    ]
    for i, call in enumerate(cases):
        with pytest.raises(ng.DimensionMismatch, match="DimensionMismatch"):
            call()
    with pytest.raises(ng.ArgumentError, match="k must be"):
        I.knn(pts, qs, -1)
    with pytest.raises(ng.ArgumentError, match="complex"):
        I.knn(pts.astype(np.complex64), qs, 1)


def test_a_well_shaped_call_without_a_device_names_the_missing_device(no_library):
    I = ng.interp
    pts, qs = torch.zeros(2, 5), torch.zeros(2, 7)
    for call in (lambda: I.knn(pts, qs, 2), lambda: I.inrange(pts, qs, 0.5), lambda: I.KNNInterpolator(pts, qs),
                 lambda: I.knn_interpolate(torch.zeros(4, 5), pts, qs)):
        with pytest.raises(ng.NgpdeError, match="no HIP device.*no CPU fallback") as e:
            call()
        assert e.value.code == _lib.ERR_HIP


# ---- the restatements against plain Python loops ---------------------------------------------------------------------------------
def f32(v):
    return struct.unpack("f", struct.pack("f", v))[0]     # a Python float rounded to float32 (inf on overflow is not reached here)


def loop_d2(p, q):   # float32 rounding after every operation, coordinate order
    d2 = 0.0
    for a, b in zip(q, p):
        df = f32(a - b)
        d2 = f32(d2 + f32(df * df))
    return d2


def small_sets(dim, seed, n=12, m=9, sites=5):
    rng = np.random.default_rng(seed)
    pts = (rng.integers(0, sites, (n, dim)) * 0.25 + rng.integers(0, 2, (n, dim)) * 1e-3).astype(np.float32)     # ties and near-ties
    qs = (rng.integers(-2, 7, (m, dim)) * 0.25 + 0.125).astype(np.float32)
    qs[0] = pts[3]                                                                                            # a coincident pair
    return pts, qs


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_brute_force_lists_equal_plain_loops(dim):
    pts, qs = small_sets(dim, {1: 1, 2: 2, 3: 2}[dim], sites=5 - dim)            # fewer lattice sites per coordinate as the dimension grows: ties in each
    gp = np.array([1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3])
    gq = np.array([1, 1, 1, 2, 2, 2, 3, 3, 3])
    for graphs in (None, (gp, gq)):
        k = 3
        idx, d2 = S.knn_brute(pts, qs, k, *(graphs or ()))
        r = 0.5
        ptr, nbr = S.radius_brute(pts, qs, r, *(graphs or ()))
        ties = 0
        for q in range(len(qs)):
            pairs = sorted((loop_d2(pts[i].tolist(), qs[q].tolist()), i) for i in range(len(pts)) if graphs is None or gp[i] == gq[q])
            assert [i for _, i in pairs[:k]] == idx[q].tolist()
            assert [np.float32(d).tobytes() for d, _ in pairs[:k]] == [v.tobytes() for v in d2[q]]
            ties += sum(pairs[j][0] == pairs[j + 1][0] for j in range(len(pairs) - 1))
            r2 = f32(r * r)
            assert sorted(i for d, i in pairs if d <= r2) == nbr[ptr[q]:ptr[q + 1]].tolist()
        assert ties > 0 and d2[0, 0] == 0 and 0 < ptr[-1] < len(pts) * len(qs)
    with pytest.raises(ValueError, match="fewer than k = 4"):
        S.knn_brute(pts, qs, 4, gp, gq)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_interpolation_and_pullback_equal_plain_loops(dtype):
    rnd = f32 if dtype is np.float32 else float
    rng = np.random.default_rng(5)
    pts, qs = small_sets(2, 2)            # (seeds chosen so that the conditions asserted at the end of each test hold)
    n, m, k, d = len(pts), len(qs), 3, 4
    idx, d2 = S.knn_brute(pts, qs, k)
    d2[1] = np.inf                                                                   # the all-ones rule
    x = rng.standard_normal((n, d)).astype(np.float32)
    ybar = rng.standard_normal((m, d)).astype(np.float32)
    w = S.interp_weights(d2, dtype)
    y = S.interp_forward(idx, w, x, dtype)
    xbar = S.interp_backward(idx, w, ybar, n, dtype)
    assert w.dtype == y.dtype == xbar.dtype == dtype
    flt_min = 2.0 ** -126
    for q in range(m):
        c = [max(float(v), flt_min) for v in d2[q]]
        raw = [1.0 if c[0] == float("inf") else rnd(c[0] / cj) for cj in c]
        W = 0.0
        for v in raw:
            W = rnd(W + v)
        want = [rnd(v / W) for v in raw]
        assert want == w[q].tolist() and raw[0] == 1.0 and 1.0 <= W <= k
        for f in range(d):
            acc = 0.0
            for j in range(k):
                acc = rnd(acc + rnd(want[j] * float(x[idx[q, j], f])))
            assert acc == float(y[q, f])
    assert w[0, 0] == 1.0 and (w[0, 1:] < 1e-30).all()                               # beside a coincident point
    assert w[1].tolist() == [dtype(1) / dtype(3)] * 3
    ptr, slot = S.transpose_rows(idx, n)
    untouched = 0
    for i in range(n):
        slots = [pos for pos in range(m * k) if idx.reshape(-1)[pos] == i]
        assert slots == slot[ptr[i]:ptr[i + 1]].tolist()
        untouched += not slots
        for f in range(d):
            acc = 0.0
            for pos in slots:
                acc = rnd(acc + rnd(float(w.reshape(-1)[pos]) * float(ybar[pos // k, f])))
            assert acc == float(xbar[i, f])
    assert untouched > 0


# ---- the clamped-query argument of neighbor_grid.h, by brute force -----------------------------------------------------------------
@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("neighbor_query") / "neighbor_query_check")
    subprocess.check_call(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-g", "-O1", "-ffp-contract=off", "-I", CSRC, os.path.join(HERE, "host", "neighbor_query_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    return r.returncode, r.stdout, r.stdout + r.stderr


def test_clamped_queries_keep_covering_and_the_ring_bound(report):
    code, out, text = report
    assert code == 0, text[-4000:]
    assert "AddressSanitizer" not in text and "runtime error" not in text and "LeakSanitizer" not in text, text[-4000:]
    m = re.search(r"^(\d+) checks, 0 failed$", out, re.M)
    assert m and int(m.group(1)) > 100000, text[-4000:]
    m = re.search(r"^queries: (\d+) clamped, (\d+) far coordinates; (\d+) accepted pairs \((\d+) clamped\), (\d+) ring pairs \((\d+) clamped\)$",
                  out, re.M)
    assert m, text[-4000:]
    clamped, far, accepted, accepted_clamped, ring, ring_clamped = map(int, m.groups())
    assert clamped > 10 ** 4 and far > 10 ** 3 and accepted_clamped > 10 ** 4 and ring_clamped > 10 ** 5


def test_the_search_uses_the_headers_query_cell_and_shares_its_kernels():
    src = open(os.path.join(CSRC, "neighbors.hip"), encoding="utf-8").read()
    assert "cell_of_query<DIM>(g," in src and "span_is_finite(dim, ulo, uhi)" in src
    # one ring walk, one block walk, one insertion list and one sort: the kernels are templated on the searcher, not copied
    for once in ("__global__ void knn_kernel(", "__global__ void radius_kernel(", "void for_block(", "int32_t sort_into_cells(",
                 "auto offer = [&]"):
        assert src.count(once) == 1, once
    for form in ("knn_kernel<DIM, false>", "knn_kernel<DIM, true>", "radius_kernel<DIM, true, true>", "radius_kernel<DIM, false, true>"):
        assert form in src, form
