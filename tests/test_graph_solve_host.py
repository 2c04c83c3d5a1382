"""Host-side checks of the conjugate-gradient solve on graph matrices (linsolve.py over csrc/graph_solve.hip): the exported names, the
argument errors the package raises before any device call, and what the two C entries refuse before they touch the device.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

ONE = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)


def matrix(n=3, **kw):
    """a GraphMatrix whose lists live on the host: enough for every check that comes before the device"""
    rows, cols = torch.tensor([0, 1, 2], dtype=torch.int32), torch.tensor([0, 1, 2], dtype=torch.int32)
    return ng.GraphMatrix(n, rows, cols, torch.ones(3), torch.tensor([0, 1, 2, 3], dtype=torch.int32), **kw)


def test_names_are_exported():
    for name in ("cg_solve", "CGInfo"):
        assert name in ng.__all__ and callable(getattr(ng, name)), name
    assert callable(ng.GraphMatrix.solve) and callable(ng.GraphMatrix.diagonal)


def test_entries_are_declared_with_their_sum_orders():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ngpde.h")).read()
    block = header[header.index("---- graph solves"):header.index("---- graph queries by node and by pair")]
    lib = _lib.load()
    for name in ("ngpde_csr_cg_workspace_bytes", "ngpde_csr_cg"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name + "(" in block, name
    for words in ("ascending column from 0.0f", "balanced binary tree", "chunk of 256 rows", "in chunk order", "check_every"):
        assert words in block, words


def test_argument_errors_come_before_any_device_call():
    M, B = matrix(), torch.ones(2, 3)
    with pytest.raises(ng.ArgumentError, match="takes a GraphMatrix"):
        ng.cg_solve(torch.eye(3), B)
    for rtol in (-1e-9, float("nan"), float("inf"), "1e-5", None, True):
        with pytest.raises(ng.ArgumentError, match="rtol must be"):
            ng.cg_solve(M, B, rtol=rtol)
    for atol in (-1.0, float("nan"), "0", True):
        with pytest.raises(ng.ArgumentError, match="atol must be"):
            ng.cg_solve(M, B, atol=atol)
    for name in ("shift", "scale"):
        for v in (float("nan"), float("inf"), "1", None, True):
            with pytest.raises(ng.ArgumentError, match=name + " must be"):
                ng.cg_solve(M, B, **{name: v})
    for p in ("ilu", "Jacobi", 1, True):
        with pytest.raises(ng.ArgumentError, match="precondition must be"):
            ng.cg_solve(M, B, precondition=p)
    for k in (-1, 1.5, "16", None, True):
        with pytest.raises(ng.ArgumentError, match="check_every must be"):
            ng.cg_solve(M, B, check_every=k)
    for k in (-1, 2.5, "8", True):
        with pytest.raises(ng.ArgumentError, match="max_iter must be"):
            ng.cg_solve(M, B, max_iter=k)
    with pytest.raises(ng.ArgumentError, match="B must be a torch tensor"):
        ng.cg_solve(M, np.ones((2, 3), np.float32))
    for bad in (torch.ones(2, 3, dtype=torch.float64), torch.ones(2, 3, dtype=torch.int32)):
        with pytest.raises(ng.ArgumentError, match="B must hold float32"):
            ng.cg_solve(M, bad)
    for bad in (torch.ones(3), torch.ones(3, 2), torch.ones(0, 3), torch.ones(1, 2, 3)):
        with pytest.raises(ng.DimensionMismatch, match="B has shape"):
            ng.cg_solve(M, bad)
    with pytest.raises(ng.DimensionMismatch, match="x0 has shape"):
        ng.cg_solve(M, B, x0=torch.ones(1, 3))
    with pytest.raises(ng.ArgumentError, match="x0 must hold float32"):
        ng.cg_solve(M, B, x0=torch.ones(2, 3, dtype=torch.float64))
    with pytest.raises(ng.ArgumentError, match="non-decreasing"):
        ng.cg_solve(matrix(num_graphs=2, graph_indicator=np.array([0, 1, 0], np.int32)), B)
    with pytest.raises(ng.ArgumentError, match="no graph_indicator"):
        ng.cg_solve(matrix(num_graphs=2), B)


def cg(lib, n=3, nnz=4, lists=(ONE, ONE, ONE), n_graphs=1, graph_of=None, shift=1.0, scale=1.0, n_rhs=2, B=ONE, x0=None, X=ONE, pre=1,
       rtol=1e-5, atol=0.0, max_iter=8, check_every=16, info=(ONE, ONE, ONE), ws=ONE, ws_bytes=1 << 30):
    return lib.ngpde_csr_cg(n, nnz, *lists, n_graphs, graph_of, shift, scale, n_rhs, B, x0, X, pre, rtol, atol, max_iter, check_every, *info,
                            ws, ws_bytes, None)


def test_the_entry_refuses_null_negative_and_small_arguments():
    lib = _lib.load()
    bad = _lib.ERR_INVALID_ARGUMENT
    for n, nnz in ((-1, 0), (3, -1)):
        assert cg(lib, n, nnz) == bad and b"negative" in lib.ngpde_last_error()
    for n, nnz in ((2 ** 31, 1), (3, 2 ** 31)):
        assert cg(lib, n, nnz) == bad and b"2^31" in lib.ngpde_last_error()
    assert cg(lib, n_graphs=0) == bad and b"n_graphs" in lib.ngpde_last_error()
    assert cg(lib, n_graphs=2) == bad and b"graph_of is NULL" in lib.ngpde_last_error()
    assert cg(lib, n_rhs=0) == bad and b"n_rhs" in lib.ngpde_last_error()
    for v in (float("nan"), float("inf")):
        assert cg(lib, shift=v) == bad and b"shift" in lib.ngpde_last_error()
        assert cg(lib, scale=v) == bad and b"scale" in lib.ngpde_last_error()
    for pre in (-1, 2):
        assert cg(lib, pre=pre) == bad and b"precondition" in lib.ngpde_last_error()
    for v in (-1.0, float("nan"), float("inf")):
        assert cg(lib, rtol=v) == bad and b"rtol" in lib.ngpde_last_error()
        assert cg(lib, atol=v) == bad and b"atol" in lib.ngpde_last_error()
    assert cg(lib, max_iter=-1) == bad and b"max_iter" in lib.ngpde_last_error()
    assert cg(lib, check_every=-1) == bad and b"check_every" in lib.ngpde_last_error()
    for k in range(3):
        lists = [ONE] * 3
        lists[k] = None
        assert cg(lib, lists=tuple(lists)) == bad and b"NULL" in lib.ngpde_last_error()
        info = [ONE] * 3
        info[k] = None
        assert cg(lib, info=tuple(info)) == bad and b"info array is NULL" in lib.ngpde_last_error()
    assert cg(lib, B=None) == bad and b"B / X is NULL" in lib.ngpde_last_error()
    assert cg(lib, X=None) == bad and b"B / X is NULL" in lib.ngpde_last_error()
    assert cg(lib, ws=None) == _lib.ERR_WORKSPACE
    assert cg(lib, ws_bytes=64) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    need = lib.ngpde_csr_cg_workspace_bytes(3, 1, 2)
    assert cg(lib, ws_bytes=need - 1) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()


def test_the_workspace_holds_the_state():
    lib = _lib.load()
    # x, r, p, q node-major, the columns of the last slab padded to a power of two: 65 -> 64 + 1, 3 -> 4
    assert lib.ngpde_csr_cg_workspace_bytes(1000, 3, 65) >= 4 * 1000 * 65 * 4
    assert lib.ngpde_csr_cg_workspace_bytes(1000, 1, 3) >= 4 * 1000 * 4 * 4
    assert lib.ngpde_csr_cg_workspace_bytes(1000, 1, 3) < lib.ngpde_csr_cg_workspace_bytes(1000, 1, 5)
    for n, n_graphs, n_rhs in ((-1, 1, 1), (2 ** 31, 1, 1), (10, 0, 1), (10, 1, 0)):
        assert lib.ngpde_csr_cg_workspace_bytes(n, n_graphs, n_rhs) == 0
