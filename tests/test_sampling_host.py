"""Host-side checks of the random graph sampling (sample_neighbors, rand_edge_split; src/NeuralGraphPDE.jl:4 of the reference re-exports
them from GNNGraphs): the exported names, the argument errors the package raises before any device call, and what the three new C
entries refuse before they touch the device.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def graph(**kw):
    return ng.GNNGraph([0, 0, 1, 2], [1, 2, 0, 0], num_nodes=3, index_base=0, **kw)


def test_names_are_exported():
    for name in ("sample_neighbors", "rand_edge_split"):
        assert name in ng.__all__, name
        assert callable(getattr(ng, name)), name


def test_row_bound_matches_the_header():
    src = open(os.path.join(ROOT, "include", "ngpde.h")).read()
    assert int(re.search(r"#define\s+NGPDE_SAMPLE_LDS_ROW_MAX\s+(\d+)", src).group(1)) == _lib.SAMPLE_LDS_ROW_MAX


def test_bad_k_is_refused():
    for k in (-2, -100, 1.5, "3", None, True):
        with pytest.raises(ng.ArgumentError, match="K"):
            ng.sample_neighbors(graph(), None, k)
    with pytest.raises(ng.ArgumentError, match="replace"):
        ng.sample_neighbors(graph(), None, -1, replace=True)
    with pytest.raises(ng.ArgumentError, match="replace"):
        ng.sample_neighbors(graph(), [0], replace=True)          # K defaults to -1


def test_unknown_dir_is_refused():
    for dir in ("both", "inout", "IN", None, 0):
        with pytest.raises(ng.ArgumentError, match="dir"):
            ng.sample_neighbors(graph(), None, 2, dir=dir)


def test_bad_frac_is_refused():
    for frac in (-0.1, 1.0001, 2, float("nan"), "half", None):
        with pytest.raises(ng.ArgumentError, match="frac"):
            ng.rand_edge_split(graph(), frac)
        with pytest.raises(ng.ArgumentError, match="frac"):
            ng.rand_edge_split(graph(), frac, bidirected=False, seed=1)


def test_non_integer_seed_is_refused():
    for seed in (1.5, "7", [1], True, -1, 2 ** 64):
        with pytest.raises(ng.ArgumentError, match="seed"):
            ng.sample_neighbors(graph(), None, 2, seed=seed)
        with pytest.raises(ng.ArgumentError, match="seed"):
            ng.rand_edge_split(graph(), 0.5, seed=seed)


# ---- the C entries --------------------------------------------------------------------------------------------------------------

ONE = C.c_void_p(16)     # (never dereferenced: the checks come before any device call)


def sample(lib, n=3, e=4, s=ONE, t=ONE, dir=1, n_listed=0, nodes=None, k=2, replace=0, outs=(ONE, ONE, ONE), n_out=True):
    n64 = C.c_int64(7)
    st = lib.ngpde_coo_sample_neighbors(n, e, s, t, 0, dir, n_listed, nodes, k, replace, 5, outs[0], outs[1], outs[2],
                                        C.byref(n64) if n_out else None, None)
    return st, n64.value


def split(lib, n=3, e=4, s=ONE, t=ONE, n_first=2, by_pair=0, outs=(ONE, ONE, ONE), n_out=True):
    n64 = C.c_int64(7)
    st = lib.ngpde_coo_rand_split(n, e, s, t, 0, n_first, by_pair, 5, outs[0], outs[1], outs[2], C.byref(n64) if n_out else None, None)
    return st, n64.value


def test_random_keys_checks():
    lib = _lib.load()
    assert lib.ngpde_random_keys(1, 1, 0, 0, -1, ONE, None) == _lib.ERR_INVALID_ARGUMENT and b"negative" in lib.ngpde_last_error()
    assert lib.ngpde_random_keys(1, 1, 0, 0, 5, None, None) == _lib.ERR_INVALID_ARGUMENT and b"out is NULL" in lib.ngpde_last_error()
    assert lib.ngpde_random_keys(1, 1, 0, 0, 0, None, None) == 0          # nothing to do is not an error


def test_null_and_negative_arguments_are_refused():
    lib = _lib.load()
    for name, call in (("ngpde_coo_sample_neighbors", sample), ("ngpde_coo_rand_split", split)):
        st, count = call(lib, s=None, t=None)
        assert st == _lib.ERR_INVALID_ARGUMENT and count in (0, 7), name
        msg = lib.ngpde_last_error()
        assert b"NULL" in msg and name.encode() in msg, (name, msg)
        for n, e in ((-1, 0), (3, -1)):
            assert call(lib, n=n, e=e)[0] == _lib.ERR_INVALID_ARGUMENT, name
            assert b"negative" in lib.ngpde_last_error(), name
        assert call(lib, e=2 ** 31)[0] == _lib.ERR_INVALID_ARGUMENT and b"2^31" in lib.ngpde_last_error(), name
        assert call(lib, n_out=False)[0] == _lib.ERR_INVALID_ARGUMENT and b"is NULL" in lib.ngpde_last_error(), name
        for k in range(3):
            outs = [ONE, ONE, ONE]
            outs[k] = None
            st, count = call(lib, outs=tuple(outs))
            assert st == _lib.ERR_INVALID_ARGUMENT and count == 0 and b"output is NULL" in lib.ngpde_last_error(), name


def test_sample_neighbors_checks():
    lib = _lib.load()
    for k in (-2, -7):
        assert sample(lib, k=k)[0] == _lib.ERR_INVALID_ARGUMENT and b"k is" in lib.ngpde_last_error()
    assert sample(lib, k=-1, replace=1)[0] == _lib.ERR_INVALID_ARGUMENT and b"replacement" in lib.ngpde_last_error()
    for dir in (2, -1, 5):
        assert sample(lib, dir=dir)[0] == _lib.ERR_INVALID_ARGUMENT and b"dir" in lib.ngpde_last_error()
    assert sample(lib, n_listed=-1, nodes=ONE)[0] == _lib.ERR_INVALID_ARGUMENT and b"n_listed" in lib.ngpde_last_error()
    assert sample(lib, n_listed=2, nodes=None)[0] == _lib.ERR_INVALID_ARGUMENT and b"nodes is NULL" in lib.ngpde_last_error()
    assert sample(lib, n=2 ** 20, k=2 ** 12, replace=1)[0] == _lib.ERR_INVALID_ARGUMENT and b"draws" in lib.ngpde_last_error()
    assert sample(lib, n=0, e=4)[0] == _lib.ERR_DIMENSION_MISMATCH
    assert sample(lib, e=0, s=None, t=None, outs=(None, None, None)) == (0, 0)          # nothing to do is not an error


def test_rand_split_checks():
    lib = _lib.load()
    for n_first in (-1, 5):
        assert split(lib, n_first=n_first)[0] == _lib.ERR_INVALID_ARGUMENT and b"n_first" in lib.ngpde_last_error()
    assert split(lib, n=0, e=4)[0] == _lib.ERR_DIMENSION_MISMATCH
    assert split(lib, e=0, n_first=0, s=None, t=None, outs=(None, None, None)) == (0, 0)
