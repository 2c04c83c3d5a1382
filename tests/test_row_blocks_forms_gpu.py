"""The five entries of csrc/row_blocks.hip on their own: ngpde_row_blocks_gather / _scatter over the recombinations the
edge-function layers ask for (src/layers.jl:106, :316, :409-410, :523 of the reference) and over the limits of the segment list,
ngpde_transpose, ngpde_rows_scale and ngpde_rows_index in both directions.

Every entry copies, or rounds once per element, or adds signed copies in a fixed order from 0: each is held bit for bit to the numpy
float32 restatement of test_flat_kernel_bounds.py (shown there to stay inside its float64 bound).  Outputs are sentinel-filled windows
with guard bands (test_optim_forms_gpu.Window): a row the kernel must zero shows if it is not written, and so does a write outside."""
import ctypes as C

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from test_flat_kernel_bounds import (MAX_SEG, ROW_BLOCK_KINDS, D, F, adjoint_gap_bound, adjoint_sides, bits, index_list, row_block_data,
                                     row_blocks_gather_f32, row_blocks_gather_ref, row_blocks_scatter_f32, row_blocks_scatter_ref,
                                     rows_index_f32, rows_scale_f32)
from test_optim_forms_gpu import DEV, Window, lib, readonly, same_bits, sync, unchanged

pytestmark = pytest.mark.gpu
WIDTHS = [1, 3, 64, 67]
BAD_ARG, BAD_DIM = _lib.ERR_INVALID_ARGUMENT, _lib.ERR_DIMENSION_MISMATCH


# ---- row blocks ------------------------------------------------------------------------------------------------------------------

def blocks_call(fn, width, src_rows, src_ptr, segs, mat_ptrs, mat_rows):
    n = len(segs)
    col = lambda k, ty: (ty * max(n, 1))(*[s[k] for s in segs])
    mats = (C.c_void_p * max(len(mat_ptrs), 1))(*mat_ptrs)
    rows = (C.c_int32 * max(len(mat_rows), 1))(*mat_rows)
    return getattr(lib(), fn)(width, src_rows, src_ptr, n, col(0, C.c_int32), col(1, C.c_int32), col(2, C.c_int32), col(3, C.c_int32),
                              col(4, C.c_float), len(mat_ptrs), mats, rows, _lib.current_stream())


def device_gather(width, src_rows, out_rows, segs, src):
    S = readonly(src)
    outs = [Window(n=r * width) for r in out_rows]
    _lib.check(blocks_call("ngpde_row_blocks_gather", width, src_rows, S[0].data_ptr(), segs, [o.ptr for o in outs], out_rows))
    sync()
    assert unchanged(S) and all(o.guards_intact() for o in outs)
    return outs


def device_scatter(width, src_rows, out_rows, segs, douts):
    Ds = [readonly(d) if d is not None else None for d in douts]
    dsrc = Window(n=src_rows * width)
    _lib.check(blocks_call("ngpde_row_blocks_scatter", width, src_rows, dsrc.ptr, segs, [d[0].data_ptr() if d is not None else None for d in Ds],
                           out_rows))
    sync()
    assert dsrc.guards_intact() and all(unchanged(d) for d in Ds if d is not None)
    return dsrc


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("kind", ROW_BLOCK_KINDS)
def test_row_blocks_gather_and_scatter_bit_for_bit(kind, width):
    src_rows, out_rows, segs, src, douts = row_block_data(kind, width, 10 * width + len(kind))
    outs = device_gather(width, src_rows, out_rows, segs, src)
    expect = row_blocks_gather_f32(width, src, out_rows, segs)
    _, gbnd, covers = row_blocks_gather_ref(width, src, out_rows, segs)
    for o, (w, e, c) in enumerate(zip(outs, expect, covers)):
        assert same_bits(w, e), o                        # every entry: the signed copies added in segment order from 0.f
        got = w.bits().reshape(e.shape)
        assert not np.any(got[c == 0])                   # rows no segment covers are +0.0, not the sentinel
    got_outs = [w.host().reshape(e.shape) for w, e in zip(outs, expect)]
    for drop in (None, 0):                               # once with a NULL gradient, which counts as zero
        dl = [None if k == drop else d for k, d in enumerate(douts)]
        if out_rows[0] == 0 and drop == 0:
            continue
        dsrc = device_scatter(width, src_rows, out_rows, segs, dl)
        pulled = row_blocks_scatter_f32(width, src_rows, dl, segs)
        _, sbnd, reads = row_blocks_scatter_ref(width, src_rows, dl, segs)
        assert same_bits(dsrc, pulled), drop             # every source row written ...
        got = dsrc.host().reshape(pulled.shape)
        assert not np.any(bits(got)[reads == 0])         # ... and rows nothing reads are +0.0
        # <gather(W), D> == <W, scatter(D)> on the device's results, both sides summed in float64
        left, right = adjoint_sides(src, dl, got_outs, got)
        assert abs(left - right) <= adjoint_gap_bound(src, dl, gbnd, sbnd, sum(out_rows) * width + src_rows * width), (drop, left, right)
        assert abs(left) > 0


def test_row_blocks_refuse_what_the_header_rules_out():
    width = 3
    src_rows, out_rows, segs, src, douts = row_block_data("vmh", width, 1)
    S = readonly(src)
    outs = [Window(n=r * width) for r in out_rows]
    dsrc = Window(n=src_rows * width)
    Ds = [readonly(d) for d in douts]
    optr, dptr = [o.ptr for o in outs], [d[0].data_ptr() for d in Ds]

    def both(segs_, mats_g, mats_s, rows_, status):
        assert blocks_call("ngpde_row_blocks_gather", width, src_rows, S[0].data_ptr(), segs_, mats_g, rows_) == status
        assert blocks_call("ngpde_row_blocks_scatter", width, src_rows, dsrc.ptr, segs_, mats_s, rows_) == status

    one = (1, 0, 0, 1, 1.0)
    both([one] * (MAX_SEG + 1), optr, dptr, out_rows, BAD_ARG)                                      # 17 segments
    both([], optr, dptr, out_rows, BAD_ARG)                                                         # none
    extra = Window(n=width)
    both(segs, optr + [extra.ptr] * 3, dptr + [extra.ptr] * 3, out_rows + [1] * 3, BAD_ARG)         # 5 matrices
    both(segs + [(1, out_rows[1] - 1, 0, 2, 1.0)], optr, dptr, out_rows, BAD_DIM)                   # a segment past its output
    both(segs + [(2, 0, 0, 1, 1.0)], optr, dptr, out_rows, BAD_DIM)                                 # a segment of an output that is not there
    both(segs + [(1, 0, src_rows - 1, 2, 1.0)], optr, dptr, out_rows, BAD_DIM)                      # a segment past the source
    assert blocks_call("ngpde_row_blocks_gather", 0, src_rows, S[0].data_ptr(), segs, optr, out_rows) == BAD_ARG
    assert blocks_call("ngpde_row_blocks_gather", width, src_rows, None, segs, optr, out_rows) == BAD_ARG
    assert blocks_call("ngpde_row_blocks_gather", width, src_rows, S[0].data_ptr(), segs, [optr[0], None], out_rows) == BAD_ARG
    assert blocks_call("ngpde_row_blocks_scatter", width, src_rows, None, segs, dptr, out_rows) == BAD_ARG
    sync()
    assert all(o.untouched() for o in outs) and dsrc.untouched() and extra.untouched()
    assert unchanged(S) and all(unchanged(d) for d in Ds)


# ---- transpose -------------------------------------------------------------------------------------------------------------------

def transpose_call(rows, cols, src, dst):
    return lib().ngpde_transpose(rows, cols, src, dst, _lib.current_stream())


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 100])
def test_transpose_bit_for_bit(rows):
    rng = np.random.default_rng(rows)
    for cols in (1, 31, 32, 33, 257):
        a = rng.normal(size=(rows, cols)).astype(F)
        a[0, 0], a[-1, -1] = -0.0, np.nan
        S, T = readonly(a), Window(n=rows * cols)
        _lib.check(transpose_call(rows, cols, S[0].data_ptr(), T.ptr))
        sync()
        assert unchanged(S) and T.guards_intact() and same_bits(T, np.ascontiguousarray(a.T)), cols


def test_transpose_zero_sizes_and_aliasing():
    a = np.arange(12, dtype=F)
    S, T = readonly(a), Window(a)
    for rows, cols in ((0, 5), (5, 0), (0, 0)):
        assert transpose_call(rows, cols, None, None) == _lib.OK
        assert transpose_call(rows, cols, S[0].data_ptr(), T.ptr) == _lib.OK
    assert transpose_call(3, 4, T.ptr, T.ptr) == BAD_ARG                     # in place is not a transpose this kernel can do
    assert transpose_call(3, 4, None, T.ptr) == BAD_ARG and transpose_call(3, 4, S[0].data_ptr(), None) == BAD_ARG
    assert transpose_call(-1, 4, S[0].data_ptr(), T.ptr) == BAD_ARG
    sync()
    assert unchanged(S) and T.guards_intact() and same_bits(T, a)


# ---- rows_scale ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", [1, 3, 64])
def test_rows_scale_bit_for_bit(d):
    rng = np.random.default_rng(d)
    for n in (1, 255, 257, 5000):
        x = (rng.normal(size=(n, d)) * 10.0 ** rng.integers(-3, 3, (n, d))).astype(F)
        s = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, n)).astype(F)
        s[0] = -0.0
        X, Sc, out = readonly(x), readonly(s), Window(n=n * d)
        _lib.check(lib().ngpde_rows_scale(n, d, X[0].data_ptr(), Sc[0].data_ptr(), out.ptr, _lib.current_stream()))
        sync()
        assert unchanged(X) and unchanged(Sc) and out.guards_intact() and same_bits(out, rows_scale_f32(x, s)), n
    assert lib().ngpde_rows_scale(0, d, None, None, None, _lib.current_stream()) == _lib.OK
    assert lib().ngpde_rows_scale(5, 0, X[0].data_ptr(), Sc[0].data_ptr(), out.ptr, _lib.current_stream()) == BAD_ARG
    sync()
    assert same_bits(out, rows_scale_f32(x, s))


# ---- rows_index ------------------------------------------------------------------------------------------------------------------

N_ROWS = 300


def index_call(outer, n_rows, n_index, d, index, src, dst, scatter):
    return lib().ngpde_rows_index(outer, n_rows, n_index, d, index, src, dst, int(scatter), _lib.current_stream())


def device_index(x, idx, n_rows, scatter):
    """gather or scatter of x [outer][.][d] by the list idx on the device, into a sentinel-filled window; returned as numpy"""
    outer, _, d = x.shape
    n_index = len(idx)
    I = torch.as_tensor(idx, dtype=torch.int64, device=DEV)
    snap = I.clone()
    X = readonly(x)
    shape = (outer, n_rows if scatter else n_index, d)
    out = Window(n=int(np.prod(shape)))
    _lib.check(index_call(outer, n_rows, n_index, d, I.data_ptr() if n_index else None, X[0].data_ptr() if x.size else None, out.ptr, scatter))
    sync()
    assert torch.equal(I, snap) and unchanged(X) and out.guards_intact()
    return out.host().reshape(shape)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("outer", [1, 3])
def test_rows_index_gather_and_scatter_bit_for_bit(outer, d):
    rng = np.random.default_rng(10 * d + outer)
    x = rng.normal(size=(outer, N_ROWS, d)).astype(F)
    for n_index in (0, 1, 257, 300):
        y = rng.normal(size=(outer, n_index, d)).astype(F)
        for out_of_range in (False, True):               # -1, n_rows, 2^40 among the entries: a zero row / a skipped entry
            idx = index_list(N_ROWS, n_index, n_index + d, out_of_range)
            assert not out_of_range or n_index == 0 or np.any((idx < 0) | (idx >= N_ROWS))
            gx = device_index(x, idx, N_ROWS, False)
            assert np.array_equal(bits(gx), bits(rows_index_f32(x, idx, N_ROWS, False))), (n_index, out_of_range)
            sy = device_index(y, idx, N_ROWS, True)     # from the sentinel: every row no entry names is zero-filled, n_index = 0 included
            assert np.array_equal(bits(sy), bits(rows_index_f32(y, idx, N_ROWS, True))), (n_index, out_of_range)
            # each direction is the other's pullback: both sides are the same products, added in float64 in another order
            left, right = float((gx.astype(D) * y).sum()), float((x.astype(D) * sy).sum())
            assert abs(left - right) <= x.size * 2.0 ** -52 * float((np.abs(gx.astype(D) * y)).sum() + 1e-300)
    perm = index_list(N_ROWS, N_ROWS, 99 + d, False)
    assert np.array_equal(np.sort(perm), np.arange(N_ROWS))
    back = device_index(device_index(x, perm, N_ROWS, True), perm, N_ROWS, False)
    assert np.array_equal(bits(back), bits(x))          # gather after scatter over a permutation: the identity


def test_rows_index_refused_arguments_write_nothing():
    x = np.random.default_rng(0).normal(size=(2, 10, 3)).astype(F)
    X, out = readonly(x), Window(n=2 * N_ROWS * 3)
    I = torch.arange(10, dtype=torch.int64, device=DEV)
    for scatter in (0, 1):
        assert index_call(2, N_ROWS, 10, 3, None, X[0].data_ptr(), out.ptr, scatter) == BAD_ARG      # before the scatter's zero fill
        assert index_call(2, N_ROWS, 10, 3, I.data_ptr(), None, out.ptr, scatter) == BAD_ARG
        assert index_call(2, N_ROWS, 10, 3, I.data_ptr(), X[0].data_ptr(), None, scatter) == BAD_ARG
        assert index_call(2, N_ROWS, 10, 0, I.data_ptr(), X[0].data_ptr(), out.ptr, scatter) == BAD_ARG
        assert index_call(-1, N_ROWS, 10, 3, I.data_ptr(), X[0].data_ptr(), out.ptr, scatter) == BAD_ARG
    assert index_call(0, N_ROWS, 10, 3, None, None, None, 1) == _lib.OK
    sync()
    assert out.untouched() and unchanged(X)
