"""Host-side checks of the graph matrices (matrices.py over csrc/graph_matrix.hip; src/NeuralGraphPDE.jl:4 of the reference re-exports
adjacency_matrix, laplacian_matrix, normalized_laplacian, scaled_laplacian, laplacian_lambda_max, khop_adj and has_isolated_nodes from
GNNGraphs): the exported names, the argument errors the package raises before any device call, and what the new C entries refuse
before they touch the device.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

NAMES = ("GraphMatrix", "adjacency_matrix", "laplacian_matrix", "normalized_laplacian", "scaled_laplacian", "laplacian_lambda_max",
         "khop_adj", "has_isolated_nodes")
ENTRIES = ("ngpde_coo_matrix", "ngpde_csr_check_symmetric", "ngpde_csr_lambda_max_workspace_bytes", "ngpde_csr_lambda_max",
           "ngpde_csr_spgemm_count", "ngpde_csr_spgemm")


def graph(**kw):
    return ng.GNNGraph([0, 0, 1, 2], [1, 2, 0, 0], num_nodes=3, index_base=0, **kw)


def test_names_are_exported():
    for name in NAMES:
        assert name in ng.__all__, name
        assert callable(getattr(ng, name)), name


def test_entries_are_declared_bound_and_cited():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngpde.h")).read()
    block = header[header.index("graph matrices on a device COO list"):header.index("GNOConv message (src/layers.jl:527-530)")]
    lib = _lib.load()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        assert name + "(" in block, name
    assert block.count("src/NeuralGraphPDE.jl:4") >= 5          # the block and each entry cite the re-export


def test_argument_errors_come_before_any_device_call():
    g = graph()
    for bad in ("both", "IN", 0, None, True):
        for call in (lambda d: ng.adjacency_matrix(g, dir=d), lambda d: ng.laplacian_matrix(g, dir=d),
                     lambda d: ng.normalized_laplacian(g, dir=d), lambda d: ng.scaled_laplacian(g, dir=d, lambda_max=2.0),
                     lambda d: ng.scaled_laplacian(g, dir=d), lambda d: ng.laplacian_lambda_max(g, dir=d), lambda d: ng.khop_adj(g, 2, dir=d),
                     lambda d: ng.has_isolated_nodes(g, dir=d)):
            with pytest.raises(ng.ArgumentError, match="dir must be"):
                call(bad)
    for k in (0, -1, 1.5, 2.0, "2", None, True, [2]):
        with pytest.raises(ng.ArgumentError, match="k must be"):
            ng.khop_adj(g, k)
    for max_iter in (0, -3, 2.5, "8", None, True):
        with pytest.raises(ng.ArgumentError, match="max_iter"):
            ng.laplacian_lambda_max(g, max_iter=max_iter)
    for tol in (-1e-9, float("nan"), float("inf"), "1e-5", None, True):
        with pytest.raises(ng.ArgumentError, match="tol"):
            ng.laplacian_lambda_max(g, tol=tol)
    for seed in (-1, 2 ** 64, 1.5, "7", True):
        with pytest.raises(ng.ArgumentError, match="seed"):
            ng.laplacian_lambda_max(g, seed=seed)
    for lam in (0.0, -2.0, float("nan"), float("inf"), "2", True, [2.0, 2.0]):
        with pytest.raises(ng.ArgumentError, match="lambda_max"):
            ng.scaled_laplacian(g, lambda_max=lam)
    gb = ng.GNNGraph([0, 2], [1, 3], num_nodes=4, index_base=0, graph_indicator=[0, 1, 0, 1])
    with pytest.raises(ng.ArgumentError, match="non-decreasing"):
        ng.laplacian_lambda_max(gb)


# ---- the C entries --------------------------------------------------------------------------------------------------------------

ONE = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)


def matrix(lib, n=3, e=4, s=ONE, t=ONE, kind=1, dir=0, loops=0, n_graphs=1, graph_of=None, scale=None, outs=(ONE,) * 7, nnz=True):
    n64 = C.c_int64(7)
    rows, cols, vals, row_ptr, group_ptr, member, group_of = outs
    st = lib.ngpde_coo_matrix(n, e, s, t, 0, kind, dir, loops, None, n_graphs, graph_of, scale, rows, cols, vals, row_ptr, group_ptr, member,
                              group_of, None, None, None, C.byref(n64) if nnz else None, None)
    return st, n64.value


def test_coo_matrix_refuses_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    assert matrix(lib, s=None, t=None) == (bad, 0) and b"s / t is NULL" in lib.ngpde_last_error()
    for n, e in ((-1, 0), (3, -1)):
        assert matrix(lib, n=n, e=e)[0] == bad and b"negative" in lib.ngpde_last_error()
    for n, e in ((2 ** 31, 0), (3, 2 ** 31), (2 ** 30, 2 ** 30)):          # (the last: nodes + edges copies to sort)
        assert matrix(lib, n=n, e=e) == (bad, 0) and b"2^31" in lib.ngpde_last_error()
    assert matrix(lib, n=0, e=4)[0] == _lib.ERR_DIMENSION_MISMATCH
    assert matrix(lib, nnz=False)[0] == bad and b"nnz_out is NULL" in lib.ngpde_last_error()
    for kind in (-1, 3):
        assert matrix(lib, kind=kind)[0] == bad and b"kind" in lib.ngpde_last_error()
    for dir in (-1, 2):
        assert matrix(lib, dir=dir)[0] == bad and b"dir" in lib.ngpde_last_error()
    for kind in (0, 1):
        assert matrix(lib, kind=kind, loops=1)[0] == bad and b"add_self_loops" in lib.ngpde_last_error()
        assert matrix(lib, kind=kind, scale=ONE)[0] == bad and b"scale" in lib.ngpde_last_error()
    assert matrix(lib, kind=2, scale=ONE, n_graphs=0)[0] == bad and b"scale" in lib.ngpde_last_error()
    assert matrix(lib, kind=2, scale=ONE, n_graphs=2)[0] == bad and b"graph_of" in lib.ngpde_last_error()
    for k in range(7):
        outs = [ONE] * 7
        outs[k] = None
        assert matrix(lib, outs=tuple(outs))[0] == bad and b"NULL" in lib.ngpde_last_error(), k


def test_check_symmetric_and_lambda_max_refuse_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT

    def symmetric(n=3, nnz=4, lists=(ONE, ONE, ONE, ONE)):
        return lib.ngpde_csr_check_symmetric(n, nnz, *lists, None, None)

    for n, nnz in ((-1, 0), (3, -1)):
        assert symmetric(n, nnz) == bad and b"negative" in lib.ngpde_last_error()
    for n, nnz in ((2 ** 31, 1), (3, 2 ** 31)):
        assert symmetric(n, nnz) == bad and b"2^31" in lib.ngpde_last_error()
    for k in range(4):
        lists = [ONE] * 4
        lists[k] = None
        assert symmetric(lists=tuple(lists)) == bad and b"NULL" in lib.ngpde_last_error()
    assert symmetric(nnz=0, lists=(None,) * 4) == 0          # nothing to check is not an error

    def lanczos(n=3, nnz=4, lists=(ONE, ONE, ONE), n_graphs=1, graph_of=None, max_iter=8, tol=1e-5, lam=ONE, ws=ONE, ws_bytes=1 << 30):
        return lib.ngpde_csr_lambda_max(n, nnz, *lists, n_graphs, graph_of, max_iter, tol, 0, lam, None, None, None, ws, ws_bytes, None)

    for n, nnz in ((-1, 0), (3, -1)):
        assert lanczos(n, nnz) == bad and b"negative" in lib.ngpde_last_error()
    for n, nnz in ((2 ** 31, 1), (3, 2 ** 31)):
        assert lanczos(n, nnz) == bad and b"2^31" in lib.ngpde_last_error()
    assert lanczos(n_graphs=0) == bad and b"n_graphs" in lib.ngpde_last_error()
    assert lanczos(n_graphs=2) == bad and b"graph_of is NULL" in lib.ngpde_last_error()
    for max_iter in (0, -1, 4097):
        assert lanczos(max_iter=max_iter) == bad and b"max_iter" in lib.ngpde_last_error()
    for tol in (-1.0, float("nan"), float("inf")):
        assert lanczos(tol=tol) == bad and b"tol" in lib.ngpde_last_error()
    assert lanczos(lam=None) == bad and b"lambda_out is NULL" in lib.ngpde_last_error()
    for k in range(3):
        lists = [ONE] * 3
        lists[k] = None
        assert lanczos(lists=tuple(lists)) == bad and b"NULL" in lib.ngpde_last_error()
    assert lanczos(ws=None) == _lib.ERR_WORKSPACE
    assert lanczos(ws_bytes=64) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    # the workspace holds the basis: max_iter x n floats, and more
    assert lib.ngpde_csr_lambda_max_workspace_bytes(1000, 3, 64) >= 64 * 1000 * 4
    for n, n_graphs, max_iter in ((-1, 1, 8), (10, 0, 8), (10, 1, 0), (10, 1, 4097)):
        assert lib.ngpde_csr_lambda_max_workspace_bytes(n, n_graphs, max_iter) == 0


def test_spgemm_entries_refuse_null_and_negative_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT

    def count(n=3, nnz_p=4, p_cols=ONE, nnz_a=4, a_row_ptr=ONE, limit=100, out=True):
        n64 = C.c_int64(7)
        return lib.ngpde_csr_spgemm_count(n, nnz_p, p_cols, nnz_a, a_row_ptr, limit, None, C.byref(n64) if out else None, None), n64.value

    def product(n=3, nnz_p=4, p=(ONE, ONE, ONE), nnz_a=4, a=(ONE, ONE, ONE), offsets=ONE, total=5, outs=(ONE, ONE, ONE, ONE), out=True):
        n64 = C.c_int64(7)
        return lib.ngpde_csr_spgemm(n, nnz_p, *p, nnz_a, *a, offsets, total, *outs, C.byref(n64) if out else None, None), n64.value

    for call in (count, product):
        for kw in (dict(n=-1), dict(nnz_p=-1), dict(nnz_a=-1)):
            assert call(**kw)[0] == bad and b"negative" in lib.ngpde_last_error()
        for kw in (dict(n=2 ** 31), dict(nnz_p=2 ** 31), dict(nnz_a=2 ** 31)):
            assert call(**kw)[0] == bad and b"2^31" in lib.ngpde_last_error()
        assert call(n=0)[0] == _lib.ERR_DIMENSION_MISMATCH
        assert call(out=False)[0] == bad and b"is NULL" in lib.ngpde_last_error()
    assert count(p_cols=None)[0] == bad and b"NULL" in lib.ngpde_last_error()
    assert count(a_row_ptr=None)[0] == bad and b"NULL" in lib.ngpde_last_error()
    for limit in (-1, 2 ** 31):
        assert count(limit=limit) == (bad, 0) and b"limit" in lib.ngpde_last_error()
    assert count(nnz_p=0, p_cols=None, a_row_ptr=None) == (0, 0)          # an empty P expands to nothing
    for total in (-1, 2 ** 31):
        assert product(total=total) == (bad, 0) and b"total" in lib.ngpde_last_error()
    assert product(outs=(ONE, ONE, ONE, None))[0] == bad and b"row_ptr_out is NULL" in lib.ngpde_last_error()
    assert product(offsets=None)[0] == bad and b"offsets" in lib.ngpde_last_error()
    assert product(nnz_p=0, total=5)[0] == bad and b"without entries" in lib.ngpde_last_error()
    for k in range(3):
        for which in ("p", "a", "outs"):
            lists = [ONE] * (4 if which == "outs" else 3)
            lists[k] = None
            assert product(**{which: tuple(lists)})[0] == bad and b"NULL" in lib.ngpde_last_error(), (which, k)
