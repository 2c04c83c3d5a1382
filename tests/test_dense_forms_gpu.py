"""The Dense family against float64 across every form and boundary.

Every entry point picks its kernel(s) from the shape, the pointers' alignment and tile-count thresholds.  tests/dense_forms_spec.py
restates those choices (fwd_form, bwd_form, pair_fwd_fused, chain2_fused, pair_bwd_grid; its docstring describes the dispatch, and
tests/test_dense_forms_host.py ties it to the library's csrc/dense_forms.h); this file asserts for every case that it lands where
it means to, and compares the outputs with float64.

NGPDE_DENSE_NARROW, _NO_GEMM128, _NO_STREAM, _NO_SMALL_FWD and _NO_SMALL_BWD are read once per process (any value): the restatement
reads them at import and follows them; under one of them (the suite's switch matrix) the cases' fixed expectations are not asserted,
the values are.  NGPDE_DENSE_NO_STREAM2 and _NO_STREAM_BWD are read per call ("1"): the cases clear them, and set them to compare the
one-launch forms with their composed paths.

The reference is torch float64 on the CPU: act(vcat(blocks repeated by row_div)[:n] @ W + b), gradients by autograd with row_div > 1
blocks detached; test_reference_matches_the_oracle ties it to oracle.ngpde_oracle.mlp_forward / mlp_backward.  It runs over row
chunks so that the 10^6-row case stays small.  A pullback is handed z as the float32 rounding of the float64 pre-activation: rounding
never changes a sign, so relu / leakyrelu / elu take the same branch in both precisions and no redraw is needed (forward outputs are
continuous in z, so the forwards need none either).

Every output, the workspace and every gradient block start as NaN inside guard words; the guards must come back unchanged, and so must a
gradient buffer passed for a row_div > 1 block.  No form uses atomics: a second call gives the same bits.  Tolerances are the suite's:
forward 1e-4 * max|ref| + 1e-5, gradients 3e-4 relative (5e-4 past 10^5 rows of weight-gradient accumulation).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from dense_forms_spec import (ONCE, PER_CALL, align256, bwd_form, cdiv, chain2_fused, din_main, fwd_form, pair_bwd_grid, pair_bwd_workspace,
                              pair_fwd_fused, small_bwd_grid, stream_bwd_grid, stream_main_blocks, table, weight_chunks, workspace_bytes)
from ngpde_amd import _lib
from oracle import ngpde_oracle as O
from test_edge_mlp_forms_gpu import ACTS
from test_mp_gpu import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ALL_ACTS = ("identity", "relu", "tanh", "sigmoid", "swish", "gelu", "leakyrelu", "elu", "softplus")
SWITCHED = any(ONCE.values())
GRAD = dict(rtol=3e-4, atol=1e-5)
GUARD = 64                                     # guard words on each side of every device buffer
CHUNK = 1 << 17                                # rows per chunk of the float64 reference


@pytest.fixture(autouse=True)
def _per_call_switches(monkeypatch):
    for v in PER_CALL:
        monkeypatch.delenv(v, raising=False)


def assert_form(form, expected, what=""):
    """a fixed expectation holds without the once-per-process switches; under one of them the restatement follows the switch"""
    if not SWITCHED:
        assert form == expected, f"{what}: form {form} != expected {expected}"


# ---- guarded device buffers -----------------------------------------------------------------------------------------------------

class Buf:
    """a float32 [shape] view `shift` words past GUARD NaN words, followed by GUARD more; every word starts as 0xFFFFFFFF (a NaN, the
    pattern of test_gat_forms_gpu.nan_ws), so that the guards and untouched buffers can be checked bitwise"""

    def __init__(self, shape, shift=0, data=None):
        numel = int(np.prod(shape)) if len(shape) else 1
        self.lo, self.hi = GUARD + shift, GUARD + shift + numel
        self.raw = torch.full(((self.hi + GUARD) * 4,), 0xFF, dtype=torch.uint8, device=DEV)
        self.t = self.raw.view(torch.float32)[self.lo:self.hi].view(*shape)
        if data is not None:
            self.t.copy_(torch.as_tensor(data, dtype=torch.float32))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards(self):
        w = self.raw.view(torch.int32)
        return bool((w[:self.lo] == -1).all()) and bool((w[self.hi:] == -1).all())

    def untouched(self):
        return bool((self.raw == 0xFF).all())


class Workspace:
    """nbytes carved at a 256-byte offset out of a NaN-filled buffer with 256 guard bytes on both sides"""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.raw = torch.full((self.n + 512,), 0xFF, dtype=torch.uint8, device=DEV)
        self.ptr = self.raw.data_ptr() + 256

    def guards(self):
        return bool((self.raw[:256] == 0xFF).all()) and bool((self.raw[256 + self.n:] == 0xFF).all())


def bits(t):
    return t.detach().contiguous().view(torch.int32).clone()


def ptr_array(ptrs):
    arr = (C.c_void_p * len(ptrs))()
    for i, p in enumerate(ptrs):
        arr[i] = p or None
    return arr


def int_array(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


def lib():
    return _lib.load()


def stream():
    return _lib.current_stream()


# ---- a Dense problem and its float64 reference ----------------------------------------------------------------------------------

class Block:
    def __init__(self, n, w, rd, shift, rng):
        self.w, self.rd, self.rows = w, rd, cdiv(n, rd) if n else 0
        self.h = torch.from_numpy(rng.standard_normal((self.rows, w), dtype=np.float32))
        self.buf = Buf((self.rows, w), shift, self.h) if w else None

    @property
    def ptr(self):
        return self.buf.ptr if self.buf else 0


class Dense:
    """n rows of vcat(blocks) => dout; blocks may be shared with another problem (first=...)"""

    def __init__(self, n, widths, dout, act="identity", bias=True, rds=None, shifts=None, seed=0, first=None):
        rng = np.random.default_rng(seed)
        rds = rds or (1,) * len(widths)
        shifts = shifts or (0,) * len(widths)
        self.n, self.dout, self.act, self.widths, self.rds = n, dout, act, tuple(widths), tuple(rds)
        self.blocks = [first if (i == 0 and first is not None) else Block(n, w, rd, sh, rng)
                       for i, (w, rd, sh) in enumerate(zip(widths, rds, shifts))]
        self.din = sum(widths)
        self.wt_h = torch.from_numpy((rng.standard_normal((self.din, dout)) / math.sqrt(max(self.din, 1))).astype(np.float32))
        self.b_h = torch.from_numpy((0.3 * rng.standard_normal(dout)).astype(np.float32)) if bias else None
        self.wt = self.wt_h.to(DEV)
        self.b = self.b_h.to(DEV) if bias else None
        self.rng = rng
        self._z = None

    @property
    def T(self):
        return table([b.ptr for b in self.blocks], self.widths, self.rds)

    def args(self):
        return (len(self.blocks), ptr_array([b.ptr for b in self.blocks]), int_array(self.widths), int_array(self.rds))

    def x64(self, r0, r1, leaves=None):
        parts, rows = [], torch.arange(r0, r1)
        for b in self.blocks:
            if not b.w:
                continue
            if b.rd == 1:
                xb = b.h[r0:r1].double()
                if leaves is not None:
                    xb.requires_grad_(True)
                    leaves.append((b, xb))
            else:
                xb = b.h[rows // b.rd].double()
            parts.append(xb)
        return torch.cat(parts, 1) if parts else torch.zeros(r1 - r0, 0, dtype=torch.float64)

    def z64(self):
        if self._z is None:
            W = self.wt_h.double()
            b = self.b_h.double() if self.b_h is not None else 0.0
            self._z = torch.empty(self.n, self.dout, dtype=torch.float64)
            for r0 in range(0, self.n, CHUNK):
                r1 = min(self.n, r0 + CHUNK)
                self._z[r0:r1] = self.x64(r0, r1) @ W + b
        return self._z

    def y64(self):
        return ACTS[self.act](self.z64())

    def grads64(self, dy):
        """{'dweight', 'dbias', block index: dX} by autograd, row chunk by row chunk (row_div > 1 blocks detached)"""
        W = self.wt_h.double().requires_grad_(True)
        b = (self.b_h.double() if self.b_h is not None else torch.zeros(self.dout, dtype=torch.float64)).requires_grad_(True)
        dX = {i: torch.zeros(bl.rows, bl.w, dtype=torch.float64) for i, bl in enumerate(self.blocks) if bl.rd == 1}
        for r0 in range(0, self.n, CHUNK):
            r1 = min(self.n, r0 + CHUNK)
            leaves = []
            y = ACTS[self.act](self.x64(r0, r1, leaves) @ W + b)
            y.backward(dy[r0:r1].double())
            for bl, xb in leaves:
                dX[self.blocks.index(bl)][r0:r1] = xb.grad
        out = dict(dweight=W.grad if W.grad is not None else torch.zeros_like(W), dbias=b.grad if b.grad is not None else torch.zeros_like(b))
        out.update(dX)
        return out

    # -- calls --
    def forward(self, save_z=True, yshift=0, zshift=0):
        y = Buf((self.n, self.dout), yshift)
        z = Buf((self.n, self.dout), zshift) if save_z else None
        n_seg, p, w, r = self.args()
        st = lib().ngpde_dense_forward(self.n, n_seg, p, w, r, self.dout, _lib.ACT[self.act], self.wt.data_ptr(), _lib.ptr(self.b),
                                       y.ptr, z.ptr if z else None, stream())
        return st, y, z

    def fwd_form(self, y, z):
        return fwd_form(self.n, self.T, self.dout, self.wt.data_ptr(), y.ptr, z.ptr if z else 0)


def check_forward(P, expected, what, save_z=True, yshift=0, zshift=0):
    """form, values against float64, guards, save_z NULL giving the same y, and a bitwise repeat"""
    st, y, z = P.forward(save_z, yshift, zshift)
    form = P.fwd_form(y, z)
    assert_form(form, expected, what)
    _lib.check(st)
    torch.cuda.synchronize()
    close(y.t, P.y64().numpy(), what=f"y {what}")
    if z:
        close(z.t, P.z64().numpy(), what=f"save_z {what}")
        assert z.guards(), f"save_z guards {what}"
    assert y.guards(), f"y guards {what}"
    st, y2, z2 = P.forward(save_z, yshift, zshift)
    _lib.check(st)
    assert torch.equal(bits(y.t), bits(y2.t)) and (z is None or torch.equal(bits(z.t), bits(z2.t))), f"repeat {what}"
    return form, y


def act_at(i):
    return ALL_ACTS[i % len(ALL_ACTS)]


# ---- the reference and the restatement against the library --------------------------------------------------------------------

def test_reference_matches_the_oracle():
    P = Dense(300, (5, 7, 3), 11, "swish", rds=(1, 7, 1), seed=3)
    dy = torch.from_numpy(P.rng.standard_normal((P.n, P.dout)).astype(np.float32))
    X = P.x64(0, P.n).numpy()
    layer = [dict(weight=P.wt_h.double().numpy().T, bias=P.b_h.double().numpy(), act="swish")]
    yo, cache = O.mlp_forward(layer, X.T)
    dxo, gro = O.mlp_backward(layer, cache, dy.double().numpy().T)
    g = P.grads64(dy)
    np.testing.assert_allclose(P.y64().numpy(), yo.T, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g["dweight"].numpy(), gro[0]["weight"].T, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g["dbias"].numpy(), gro[0]["bias"].reshape(-1), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g[0].numpy(), dxo[:5].T, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(g[2].numpy(), dxo[12:].T, rtol=1e-12, atol=1e-12)
    assert 1 not in g                                              # the per-graph block: detached


@pytest.mark.parametrize("n", [0, 1, 64, 65, 1000, 4096, 33023, 33024, 65536, 65537, 10 ** 6, 2 ** 24])
def test_workspace_and_chain_queries_agree_with_the_restatement(n):
    for din, dout in ((1, 1), (64, 64), (128, 2048), (130, 1024), (132, 2052), (128, 8192), (17, 65)):
        assert lib().ngpde_dense_workspace_bytes(n, din, dout) == workspace_bytes(n, din, dout), (n, din, dout)
    x = torch.empty(1024, device=DEV)                            # (the query reads no data)
    p64, p64b, pu = x.data_ptr(), x.data_ptr() + 256, x.data_ptr() + 4
    for widths, ptrs, dmid, dout in (((64,), (p64,), 64, 64), ((64, 64, 2), (p64, p64b, p64), 64, 40), ((64, 5), (p64, p64), 64, 64),
                                     ((64,), (pu,), 64, 64), ((32, 32), (p64, p64b), 64, 64), ((64,), (p64,), 32, 64), ((64,), (p64,), 64, 65)):
        T = table(ptrs, widths, (1,) * len(widths))
        got = lib().ngpde_dense_chain2_fused(n, len(widths), ptr_array(ptrs), int_array(widths), None, dmid, dout)
        assert got == int(chain2_fused(n, T, dmid, dout)), (n, widths, dmid, dout)


# ---- small forward ---------------------------------------------------------------------------------------------------------------

SMALL_FWD = [  # n, widths, rds, shifts, dout, expected
    (1, (17,), None, None, 1, "dense_small_fwd_kernel"),
    (63, (64,), None, None, 64, "dense_small_fwd_kernel"),
    (64, (30, 34), None, None, 64, "dense_small_fwd_kernel"),
    (64, (16,), None, None, 20, "dense_mfma_fwd_kernel"),                 # din 16: one K step of the general kernel
    (64, (65,), None, None, 20, "dense_mfma_fwd_kernel"),
    (500, (20, 5, 3), None, None, 65, "dense_mfma_fwd_kernel"),           # dout 65
    (1000, (7, 3, 10), (1, 3, 1), None, 30, "dense_small_fwd_kernel"),    # not 16-byte loadable; n % 3 != 0
    (1000, (17,), None, (1,), 8, "dense_small_fwd_kernel"),               # unaligned block
    (65536, (33, 31), (1, 1000), None, 64, "dense_small_fwd_kernel"),
    (65537, (33, 31), (1, 1000), None, 64, "dense_wide_fwd_kernel"),
    (65537, (64,), None, None, 64, "dense_stream64_fwd_kernel"),
]


@pytest.mark.parametrize("i", range(len(SMALL_FWD)))
def test_small_forward(i):
    n, widths, rds, shifts, dout, expected = SMALL_FWD[i]
    P = Dense(n, widths, dout, act_at(i), bias=i % 3 != 1, rds=rds, shifts=shifts, seed=100 + i)
    check_forward(P, expected, f"small {SMALL_FWD[i]}")


# ---- general forward -------------------------------------------------------------------------------------------------------------

GENERAL_FWD = [
    (3000, (5,), None, 33),
    (2000, (100,), None, 70),
    (2000, (10, 20, 30, 40), (1, 1, 7, 1), 50),
    (500, (8, 0, 4), None, 20),                # a zero-width (NULL) block
    (300, (3, 5, 0, 2), None, 130),
]


@pytest.mark.parametrize("i", range(len(GENERAL_FWD)))
def test_general_forward(i):
    n, widths, rds, dout = GENERAL_FWD[i]
    P = Dense(n, widths, dout, act_at(i + 4), bias=i % 2 == 0, rds=rds, seed=200 + i)
    check_forward(P, "dense_mfma_fwd_kernel", f"general {GENERAL_FWD[i]}")


def test_zero_width_block_in_the_small_forward():
    P = Dense(500, (16, 0, 8), 20, "elu", seed=210)
    assert P.blocks[1].ptr == 0
    check_forward(P, "dense_small_fwd_kernel", "small zero-width")


# ---- gemm128 forward ------------------------------------------------------------------------------------------------------------

GEMM_FWD = [  # n, din, dout, save_z, zshift, expected
    (4000, 32, 2052, True, 0, "dense_gemm128_fwd_kernel"),              # ragged last column tile
    (4000, 32, 2052, False, 0, "dense_gemm128_fwd_kernel"),
    (4000, 32, 2052, True, 1, "dense_wide_fwd_kernel"),                 # unaligned save_z falls back
    (65408, 32, 128, True, 0, "dense_wide_fwd_kernel"),                 # 511 tiles
    (65409, 32, 128, True, 0, "dense_gemm128_fwd_kernel"),              # 512 tiles
    (40000, 48, 132, True, 0, "dense_gemm128_fwd_kernel"),
    (40000, 40, 132, True, 0, "dense_wide_fwd_kernel"),                 # din % 16 != 0
]


@pytest.mark.parametrize("i", range(len(GEMM_FWD)))
def test_gemm128_forward(i):
    n, din, dout, save_z, zshift, expected = GEMM_FWD[i]
    P = Dense(n, (din,), dout, ("tanh", "gelu", "relu", "identity", "softplus", "swish", "sigmoid")[i], bias=i != 1, seed=300 + i)
    check_forward(P, expected, f"gemm128 {GEMM_FWD[i]}", save_z=save_z, zshift=zshift)


# ---- wide and streaming forwards ------------------------------------------------------------------------------------------------

WIDE_FWD = [  # n, widths, rds, shifts, dout, expected, din_main
    (70000, (96, 8), None, None, 64, "dense_wide_fwd_kernel", 96),
    (70000, (40, 3, 5), None, None, 48, "dense_wide_fwd_kernel", 48),
    (70000, (64, 9), None, None, 64, "dense_wide_fwd_kernel", 73),
    (70000, (64, 3, 5), (1, 1, 700), None, 64, "dense_stream64_fwd_kernel", 64),
    (70000, (64,), None, (1,), 8, "dense_wide_fwd_kernel", 64),          # unaligned 64-wide block
    (40000, (96, 4), None, None, 100, "dense_wide_fwd_kernel", 96),       # two column tiles
    (40000, (100, 4), None, None, 100, "dense_wide_fwd_kernel", 104),     # offset 100: the narrow block stays in the K loop
    (70001, (64,), None, None, 64, "dense_stream64_fwd_kernel", 64),
    (65409, (64, 4, 4), (1, 1, 999), None, 40, "dense_stream64_fwd_kernel", 64),
    (65408, (64, 4, 4), (1, 1, 999), None, 40, "dense_mfma_fwd_kernel", 64),   # 511 tiles of 128 rows
    (70001, (32, 32, 2), None, None, 24, "dense_stream64_fwd_kernel", 64),
    (70001, (32, 32, 2), None, (0, 1, 0), 24, "dense_wide_fwd_kernel", 64),
]


@pytest.mark.parametrize("i", range(len(WIDE_FWD)))
def test_wide_and_streaming_forward(i):
    n, widths, rds, shifts, dout, expected, dm = WIDE_FWD[i]
    P = Dense(n, widths, dout, act_at(i + 2), bias=i % 4 != 3, rds=rds, shifts=shifts, seed=400 + i)
    assert din_main(P.T) == dm
    check_forward(P, expected, f"wide {WIDE_FWD[i]}")


# ---- multi forward -------------------------------------------------------------------------------------------------------------

MULTI = [
    [(500, (20,), 30, "relu", True, True)],
    [(1000, (64,), 64, "tanh", True, False), (0, (8,), 16, "gelu", True, True)],
    [(300, (5, 7), 100, "gelu", False, True), (65, (3,), 1, "softplus", True, True), (2000, (33, 2), 64, "elu", True, False)],
    [(1000, (64,), 64, "leakyrelu", True, True), (0, (8,), 16, "swish", False, True), (300, (5, 7, 1, 2), 100, "sigmoid", False, False),
     (129, (3,), 70, "identity", True, True)],
]


@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_multi_forward(count):
    probs = [Dense(n, w, d, a, bias=b, seed=500 + 10 * count + q) for q, (n, w, d, a, b, _) in enumerate(MULTI[count - 1])]
    for q, P in enumerate(probs):
        if P.n == 0:
            for bl in P.blocks:
                bl.buf = None                                      # a zero-row problem's blocks may be NULL
    saves = [s for *_, s in MULTI[count - 1]]

    def run():
        ys = [Buf((P.n, P.dout)) for P in probs]
        zs = [Buf((P.n, P.dout)) if s else None for P, s in zip(probs, saves)]
        st = lib().ngpde_dense_multi_forward(
            count, (C.c_int64 * count)(*[P.n for P in probs]), int_array([len(P.blocks) for P in probs]),
            ptr_array([b.ptr for P in probs for b in P.blocks]), int_array([w for P in probs for w in P.widths]),
            int_array([r for P in probs for r in P.rds]), int_array([P.dout for P in probs]), int_array([_lib.ACT[P.act] for P in probs]),
            ptr_array([P.wt.data_ptr() for P in probs]), ptr_array([_lib.ptr(P.b) for P in probs]), ptr_array([y.ptr for y in ys]),
            ptr_array([z.ptr if z else 0 for z in zs]), stream())
        _lib.check(st)
        return ys, zs
    ys, zs = run()
    torch.cuda.synchronize()
    for P, y, z in zip(probs, ys, zs):
        what = f"multi {count} {P.n} {P.widths} {P.dout}"
        if P.n == 0:
            assert y.untouched() and (z is None or z.untouched()), what
            continue
        close(y.t, P.y64().numpy(), what=what)
        if z:
            close(z.t, P.z64().numpy(), what=what)
            assert z.guards()
        assert y.guards(), what
    ys2, _ = run()
    assert all(torch.equal(bits(a.t), bits(b.t)) for a, b in zip(ys, ys2))


def test_multi_forward_with_no_rows_launches_nothing():
    P = Dense(0, (8,), 16, seed=590)
    y = Buf((1, 16))
    st = lib().ngpde_dense_multi_forward(1, (C.c_int64 * 1)(0), int_array([1]), ptr_array([0]), int_array([8]), int_array([1]),
                                         int_array([16]), int_array([0]), ptr_array([P.wt.data_ptr()]), ptr_array([0]), ptr_array([y.ptr]),
                                         ptr_array([0]), stream())
    _lib.check(st)
    torch.cuda.synchronize()
    assert y.untouched()


# ---- pair forward ---------------------------------------------------------------------------------------------------------------

PAIR_FWD = [  # n, widths_a, rds_a, dout_a, widths_b, dout_b, share, fused
    (65409, (64, 2, 2), (1, 1, 1000), 64, (64, 4), 32, True, True),
    (65408, (64, 2, 2), (1, 1, 1000), 64, (64, 4), 32, True, False),
    (70001, (64,), None, 64, (64,), 48, True, True),
    (70001, (64, 5), None, 64, (64,), 48, True, False),               # five narrow features on one side
    (70001, (64, 1, 3), None, 64, (64, 2, 2), 65, True, False),       # dout 65
    (70001, (64, 1), None, 40, (64, 1), 40, False, False),            # two different leading blocks
]


@pytest.mark.parametrize("i", range(len(PAIR_FWD)))
def test_pair_forward(i, monkeypatch):
    n, wa, rda, da, wb, db, share, fused = PAIR_FWD[i]
    A = Dense(n, wa, da, act_at(i + 1), rds=rda, seed=600 + i)
    B = Dense(n, wb, db, act_at(i + 5), bias=False, seed=650 + i, first=A.blocks[0] if share else None)

    def run():
        ya, yb = Buf((n, da)), Buf((n, db))
        za, zb = Buf((n, da)), Buf((n, db))
        na, pa, wa_, ra = A.args()
        nb, pb, wb_, rb = B.args()
        st = lib().ngpde_dense_pair_forward(n, na, pa, wa_, ra, da, _lib.ACT[A.act], A.wt.data_ptr(), _lib.ptr(A.b), ya.ptr, za.ptr,
                                            nb, pb, wb_, rb, db, _lib.ACT[B.act], B.wt.data_ptr(), None, yb.ptr, zb.ptr, stream())
        _lib.check(st)
        torch.cuda.synchronize()
        return ya, yb, za, zb, pair_fwd_fused(n, A.T, da, B.T, db)
    ya, yb, za, zb, got = run()
    if not SWITCHED:
        assert got == fused
    for P, y, z, w in ((A, ya, za, "a"), (B, yb, zb, "b")):
        close(y.t, P.y64().numpy(), what=f"pair y_{w} {PAIR_FWD[i]}")
        close(z.t, P.z64().numpy(), what=f"pair z_{w} {PAIR_FWD[i]}")
        assert y.guards() and z.guards()
    ya2, yb2, *_ = run()
    assert torch.equal(bits(ya.t), bits(ya2.t)) and torch.equal(bits(yb.t), bits(yb2.t))
    if got:                                                        # against the two-launch path on the same inputs
        monkeypatch.setenv("NGPDE_DENSE_NO_STREAM2", "1")
        ya3, yb3, _, _, again = run()
        monkeypatch.delenv("NGPDE_DENSE_NO_STREAM2")
        assert not again
        close(ya.t, ya3.t.cpu().double().numpy(), rtol=2e-5, atol=2e-6, what="pair vs two launches a")
        close(yb.t, yb3.t.cpu().double().numpy(), rtol=2e-5, atol=2e-6, what="pair vs two launches b")


# ---- chain2 forward ---------------------------------------------------------------------------------------------------------------

CHAIN = [  # n, widths, rds, dmid, dout, save, expected
    (65409, (64, 3), (1, 1), 64, 40, False, "dense_chain_fwd_kernel<1>"),
    (65409, (64, 3), (1, 1), 64, 40, True, "dense_chain_fwd_kernel<1>"),
    (70001, (64, 64, 2), (1, 1, 5000), 64, 64, True, "dense_chain_fwd_kernel<2>"),
    (70001, (64, 64, 2), (1, 1, 5000), 64, 64, False, "dense_chain_fwd_kernel<2>"),
    (65408, (64, 3), (1, 1), 64, 40, True, "two"),
    (70001, (64, 3), (1, 1), 32, 40, True, "two"),                # dmid 32
    (70001, (64,), (1,), 64, 65, True, "two"),                    # dout 65
]


def chain_ref(P1, P2):
    """(y, z2, a1, z1) in float64 with the second layer applied to the float64 a1"""
    a1 = P1.y64()
    z2 = a1 @ P2.wt_h.double() + (P2.b_h.double() if P2.b_h is not None else 0.0)
    return ACTS[P2.act](z2), z2, a1, P1.z64()


@pytest.mark.parametrize("i", range(len(CHAIN)))
def test_chain2_forward(i, monkeypatch):
    n, widths, rds, dmid, dout, save, expected = CHAIN[i]
    P1 = Dense(n, widths, dmid, act_at(i + 2), rds=rds, seed=700 + i)
    P2 = Dense(1, (dmid,), dout, act_at(i + 6), bias=i % 2 == 0, seed=750 + i)
    n_seg, p, w, r = P1.args()
    fused = lib().ngpde_dense_chain2_fused(n, n_seg, p, w, r, dmid, dout)
    assert fused == int(chain2_fused(n, P1.T, dmid, dout))
    if not SWITCHED:
        assert (f"dense_chain_fwd_kernel<{stream_main_blocks(P1.T)}>" if fused else "two") == expected

    def run(keep):
        y, z2 = Buf((n, dout)), Buf((n, dout)) if keep else None
        a1, z1 = (Buf((n, dmid)), Buf((n, dmid))) if keep else (None, None)
        st = lib().ngpde_dense_chain2_forward(n, n_seg, p, w, r, dmid, _lib.ACT[P1.act], P1.wt.data_ptr(), _lib.ptr(P1.b),
                                              a1.ptr if a1 else None, z1.ptr if z1 else None, dout, _lib.ACT[P2.act], P2.wt.data_ptr(),
                                              _lib.ptr(P2.b), y.ptr, z2.ptr if z2 else None, stream())
        return st, y, z2, a1, z1
    if not fused:
        st, *_ = run(False)
        assert st == _lib.ERR_INVALID_ARGUMENT                      # the two-launch path needs a1
    st, y, z2, a1, z1 = run(save or not fused)
    _lib.check(st)
    torch.cuda.synchronize()
    yr, z2r, a1r, z1r = chain_ref(P1, P2)
    what = f"chain {CHAIN[i]}"
    close(y.t, yr.numpy(), what=f"y {what}")
    assert y.guards()
    if a1:
        close(a1.t, a1r.numpy(), what=f"a1 {what}")
        close(z1.t, z1r.numpy(), what=f"z1 {what}")
        close(z2.t, z2r.numpy(), what=f"z2 {what}")
        assert a1.guards() and z1.guards() and z2.guards()
    st, y2, *_ = run(save or not fused)
    _lib.check(st)
    assert torch.equal(bits(y.t), bits(y2.t))
    if fused:
        monkeypatch.setenv("NGPDE_DENSE_NO_STREAM2", "1")
        assert lib().ngpde_dense_chain2_fused(n, n_seg, p, w, r, dmid, dout) == 0
        st, y3, *_ = run(True)
        monkeypatch.delenv("NGPDE_DENSE_NO_STREAM2")
        _lib.check(st)
        close(y.t, y3.t.cpu().double().numpy(), rtol=2e-5, atol=2e-6, what=f"chain vs two launches {what}")


# ---- pullbacks -----------------------------------------------------------------------------------------------------------------

def run_backward(P, dy, z, grads, bias=True, dshifts=None, dyshift=0):
    """(status, form, outputs) of ngpde_dense_backward with NaN-started guarded outputs; grads: per block True / False / None (NULL)"""
    dshifts = dshifts or (0,) * len(P.blocks)
    dyb = Buf((P.n, P.dout), dyshift, dy)
    zb = Buf((P.n, P.dout), 0, z) if z is not None else None
    dseg = [Buf((bl.rows, bl.w), sh) if (g and bl.w) else None for bl, g, sh in zip(P.blocks, grads, dshifts)]
    dW, db = Buf((P.din, P.dout)), Buf((P.dout,)) if bias else None
    ws = Workspace(lib().ngpde_dense_workspace_bytes(P.n, P.din, P.dout))
    n_seg, p, w, r = P.args()
    dptrs = [d.ptr if d else 0 for d in dseg]
    form = bwd_form(P.n, P.T, P.dout, P.act, P.wt.data_ptr(), dyb.ptr, dptrs, bias, ws.ptr)
    st = lib().ngpde_dense_backward(P.n, n_seg, p, w, r, P.dout, _lib.ACT[P.act], P.wt.data_ptr(), zb.ptr if zb else None, dyb.ptr,
                                    ptr_array(dptrs), dW.ptr, db.ptr if db else None, ws.ptr, ws.n, stream())
    torch.cuda.synchronize()
    return st, form, dict(dweight=dW, dbias=db, dseg=dseg, ws=ws)


def check_backward(P, expected, what, grads=None, bias=True, dshifts=None, dyshift=0, tol=GRAD, ref=None):
    grads = grads or [True] * len(P.blocks)
    dy = torch.from_numpy(np.random.default_rng(P.n + P.din).standard_normal((P.n, P.dout), dtype=np.float32))
    z = P.z64().float() if P.act != "identity" else None          # identity: z may be NULL
    st, form, out = run_backward(P, dy, z, grads, bias, dshifts, dyshift)
    assert_form(form, expected, what)
    _lib.check(st)
    g = ref if ref is not None else P.grads64(dy)
    close(out["dweight"].t, g["dweight"].numpy(), what=f"dweight {what}", **tol)
    if bias:
        close(out["dbias"].t, g["dbias"].numpy(), what=f"dbias {what}", **tol)
    for i, (d, bl) in enumerate(zip(out["dseg"], P.blocks)):
        if d is None:
            continue
        if bl.rd > 1:
            assert d.untouched(), f"the gradient buffer of a row_div > 1 block was written {what}"
        else:
            close(d.t, g[i].numpy(), what=f"dX{i} {what}", **tol)
            assert d.guards(), f"dX{i} guards {what}"
    assert out["ws"].guards(), f"workspace guards {what}"
    assert out["dweight"].guards() and (not bias or out["dbias"].guards()), what
    st, _, out2 = run_backward(P, dy, z, grads, bias, dshifts, dyshift)
    _lib.check(st)
    assert torch.equal(bits(out["dweight"].t), bits(out2["dweight"].t)), f"repeat dweight {what}"
    for d, d2 in zip(out["dseg"], out2["dseg"]):
        assert d is None or torch.equal(bits(d.t), bits(d2.t)), f"repeat dX {what}"
    return form, out, dy, z, g


STREAM_BWD = [  # n, widths, rds, grads, dshifts, act, grid, expected
    (40000, (64,), None, (True,), None, "swish", 512, ("dense_stream64_bwd_kernel<1>", "dense_weight_reduce_kernel")),
    (40000, (64, 64, 2), (1, 1, 9000), (True, True, True), None, "relu", 305, ("dense_stream64_bwd_kernel<2>", "dense_weight_reduce_kernel")),
    (40000, (2, 64), (1, 1), (False, True), None, "leakyrelu", 512, ("dense_stream64_bwd_kernel<1>", "dense_weight_reduce_kernel")),
    (40000, (64, 1, 1, 2), (1, 1, 3, 1), (True, None, False, False), None, "identity", 512,
     ("dense_stream64_bwd_kernel<1>", "dense_weight_reduce_kernel")),
    (33024, (64, 64), None, (True, False), None, "elu", 256, ("dense_stream64_bwd_kernel<2>", "dense_weight_reduce_kernel")),
    (33023, (64, 64), None, (True, False), None, "elu", 0,
     ("dense_dz_kernel", "dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_wide_bwd_input_kernel")),
    (40000, (64,), None, (True,), (1,), "tanh", 0,                 # unaligned gradient block falls back
     ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),
    (70000, (64,), None, (True,), (1,), "softplus", 0,
     ("dense_dz_kernel", "dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_wide_bwd_input_kernel")),
    (40000, (64, 2), None, (True, True), None, "gelu", 0,          # a narrow block asking for a gradient falls back
     ("dense_dz_kernel", "dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_wide_bwd_input_kernel")),
]


@pytest.mark.parametrize("i", range(len(STREAM_BWD)))
def test_streaming_pullback(i, monkeypatch):
    n, widths, rds, grads, dshifts, act, grid, expected = STREAM_BWD[i]
    P = Dense(n, widths, 64, act, bias=i % 3 != 2, rds=rds, seed=800 + i)
    what = f"stream bwd {STREAM_BWD[i][:6]}"
    form, out, dy, z, g = check_backward(P, expected, what, grads=list(grads), bias=i % 3 != 2, dshifts=dshifts, ref=None)
    dptrs = [d.ptr if d else 0 for d in out["dseg"]]
    if not SWITCHED:
        assert stream_bwd_grid(n, P.T, 64, dptrs)[0] == grid
        if grid:                                                   # slabs inside the [n][64] dz area of the workspace
            assert grid * (P.din + 1) * 64 * 4 <= align256(n * 64 * 4)
    if form[0].startswith("dense_stream64_bwd_kernel"):
        monkeypatch.setenv("NGPDE_DENSE_NO_STREAM_BWD", "1")
        st, form2, out2 = run_backward(P, dy, z, list(grads), i % 3 != 2, dshifts)
        monkeypatch.delenv("NGPDE_DENSE_NO_STREAM_BWD")
        _lib.check(st)
        assert not form2[0].startswith("dense_stream64_bwd_kernel")
        close(out["dweight"].t, out2["dweight"].t.cpu().double().numpy(), what=f"vs composed {what}", **GRAD)
        for d, d2 in zip(out["dseg"], out2["dseg"]):
            if d is not None and d2 is not None and not d.untouched():
                close(d.t, d2.t.cpu().double().numpy(), rtol=2e-5, atol=2e-6, what=f"dX vs composed {what}")


SMALL_BWD = [  # n, widths, rds, grads, dout, expected
    (65, (64,), None, (True,), 64, ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),          # grid 1 by n / (din + 1)
    (64, (64,), None, (True,), 64, ("dense_dz_kernel", "dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel",
                                    "dense_mfma_bwd_input_kernel")),                                    # n / (din + 1) = 0
    (1000, (1,), None, (True,), 1, ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),
    (1000, (64,), None, (True,), 1, ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),
    (1000, (1,), None, (True,), 64, ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),
    (1000, (7, 3, 10), (1, 4, 1), (True, True, None), 30, ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),
    (65536, (33, 31), (1, 1), (True, False), 64, ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),
    (3, (2,), None, (True,), 5, ("dense_small_bwd_kernel", "dense_weight_reduce_kernel")),
]


@pytest.mark.parametrize("i", range(len(SMALL_BWD)))
def test_small_pullback(i):
    n, widths, rds, grads, dout, expected = SMALL_BWD[i]
    P = Dense(n, widths, dout, act_at(i + 1), rds=rds, seed=900 + i)
    bias = i % 2 == 0
    form, *_ = check_backward(P, expected, f"small bwd {SMALL_BWD[i][:5]}", grads=list(grads), bias=bias)
    if form and form[0] == "dense_small_bwd_kernel":
        assert small_bwd_grid(n, P.din, dout) * (P.din + 1) * dout * 4 <= align256(n * dout * 4)


COMPOSED_BWD = [  # n, widths, dout, act, bias, dyshift, no_stream_bwd, expected
    (10 ** 6, (64,), 64, "tanh", True, 0, True,
     ("dense_dz_kernel", "dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_wide_bwd_input_kernel")),
    (5000, (100,), 100, "relu", True, 0, False,
     ("dense_dz_kernel", "dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_mfma_bwd_input_kernel")),
    (5000, (40, 60), 100, "identity", False, 0, False,
     ("dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_mfma_bwd_input_kernel")),
    (4096, (128,), 256, "identity", False, 0, False,
     ("dense_gemm128_split_kernel<true,false>", "dense_weight_reduce_kernel", "dense_mfma_bwd_input_kernel")),
    (4096, (128,), 256, "identity", False, 1, False,              # unaligned dy (= dz): the general weight kernel
     ("dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_mfma_bwd_input_kernel")),
    (4100, (128,), 256, "identity", False, 0, False,              # n % 16 != 0
     ("dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_mfma_bwd_input_kernel")),
    (4096, (128,), 256, "identity", True, 0, False,               # dbias: the general weight kernel
     ("dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_mfma_bwd_input_kernel")),
    (1024, (128,), 2048, "identity", False, 0, False,
     ("dense_gemm128_split_kernel<true,false>", "dense_weight_reduce_kernel", "dense_gemm128_split_kernel<false,true>", "add_partials_kernel")),
    (1000, (130,), 1024, "identity", True, 0, False,              # din % 4 != 0: the split over z without gemm128
     ("dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_wide_bwd_input_kernel", "add_partials_kernel")),
    (1000, (130,), 1024, "sigmoid", False, 0, False,
     ("dense_dz_kernel", "dense_mfma_bwd_weight_kernel", "dense_weight_reduce_kernel", "dense_wide_bwd_input_kernel", "add_partials_kernel")),
]


@pytest.mark.parametrize("i", range(len(COMPOSED_BWD)))
def test_composed_pullback(i, monkeypatch):
    n, widths, dout, act, bias, dyshift, no_stream, expected = COMPOSED_BWD[i]
    if no_stream:
        monkeypatch.setenv("NGPDE_DENSE_NO_STREAM_BWD", "1")
    P = Dense(n, widths, dout, act, bias=bias, seed=1000 + i)
    if n == 10 ** 6:                                               # 1 024 chunks of 992 rows: the last 15 hold no row
        rpc = max(16, cdiv(cdiv(n, weight_chunks(n, 64, 64)), 16) * 16)
        assert weight_chunks(n, 64, 64) == 1024 and rpc == 992 and cdiv(n, rpc) == 1009
    # 10^6 rows of fp32 weight-gradient sums: the suite's looser gradient tolerance
    tol = dict(rtol=5e-4, atol=1e-5) if n > 10 ** 5 else GRAD
    check_backward(P, expected, f"composed {COMPOSED_BWD[i][:7]}", bias=bias, dyshift=dyshift, tol=tol)


def test_zero_rows_backward_zeroes_the_weight_gradients():
    P = Dense(0, (8, 4), 16, "tanh", seed=1100)
    for bl in P.blocks:
        bl.buf = None
    dW, db = Buf((12, 16)), Buf((16,))
    n_seg, p, w, r = P.args()
    st = lib().ngpde_dense_backward(0, n_seg, p, w, r, 16, _lib.ACT["tanh"], P.wt.data_ptr(), None, None, None, dW.ptr, db.ptr, None, 0, stream())
    _lib.check(st)
    torch.cuda.synchronize()
    assert bool((dW.t == 0).all()) and bool((db.t == 0).all()) and dW.guards() and db.guards()
    st = lib().ngpde_dense_backward(0, n_seg, p, w, r, 16, _lib.ACT["tanh"], P.wt.data_ptr(), None, None, None, dW.ptr, None, None, 0, stream())
    _lib.check(st)


# ---- the pair pullback --------------------------------------------------------------------------------------------------------

PAIR_BWD = [  # n, narrow_a, rds_a, narrow_b, addend
    (40000, (2, 2), (1, 5000), (1,), "separate"),
    (40000, (), (), (4,), "none"),
    (40000, (1, 1, 2), (1, 7, 1), (3,), "alias"),
    (32768, (4,), (1,), (), "alias"),
    (70001, (1, 3), (1, 1), (2, 1, 1), "separate"),
]


@pytest.mark.parametrize("i", range(len(PAIR_BWD)))
def test_pair_pullback(i):
    n, nwa, rda, nwb, addend = PAIR_BWD[i]
    A = Dense(n, (64,) + nwa, 64, bias=True, rds=(1,) + rda, seed=1200 + i)
    B = Dense(n, (64,) + nwb, 64, bias=i % 2 == 0, seed=1250 + i, first=A.blocks[0])
    rng = np.random.default_rng(1300 + i)
    dya = torch.from_numpy(rng.standard_normal((n, 64), dtype=np.float32))
    dyb = torch.from_numpy(rng.standard_normal((n, 64), dtype=np.float32))
    add = torch.from_numpy(rng.standard_normal((n, 64), dtype=np.float32))
    na, pa, wa, ra = A.args()
    nb, pb, wb, rb = B.args()
    wsb = lib().ngpde_dense_pair_backward_workspace_bytes(n, na, pa, wa, ra, nb, pb, wb, rb, 64)
    grid = pair_bwd_grid(n, A.T, B.T, 64)
    assert wsb == pair_bwd_workspace(grid, A.din, B.din)
    if not SWITCHED:
        assert grid == min(cdiv(n, 64), 512)

    def run():
        dya_b, dyb_b = Buf((n, 64), 0, dya), Buf((n, 64), 0, dyb)
        dWa, dWb = Buf((A.din, 64)), Buf((B.din, 64))
        dba, dbb = Buf((64,)), Buf((64,)) if B.b is not None else None
        dx = Buf((n, 64), 0, add if addend == "alias" else None)
        addb = Buf((n, 64), 0, add) if addend == "separate" else None
        ws = Workspace(wsb)
        st = lib().ngpde_dense_pair_backward(n, na, pa, wa, ra, A.wt.data_ptr(), dya_b.ptr, dWa.ptr, dba.ptr, nb, pb, wb, rb, B.wt.data_ptr(),
                                             dyb_b.ptr, dWb.ptr, dbb.ptr if dbb else None, 64, dx.ptr,
                                             dx.ptr if addend == "alias" else addb.ptr if addb else None, ws.ptr, ws.n, stream())
        _lib.check(st)
        torch.cuda.synchronize()
        return dict(dWa=dWa, dWb=dWb, dba=dba, dbb=dbb, dx=dx, ws=ws)
    out = run()
    ga, gb = A.grads64(dya), B.grads64(dyb)
    what = f"pair bwd {PAIR_BWD[i]}"
    dx_ref = ga[0] + gb[0] + (add.double() if addend != "none" else 0.0)
    close(out["dx"].t, dx_ref.numpy(), what=f"dx {what}")
    close(out["dWa"].t, ga["dweight"].numpy(), what=f"dWa {what}", **GRAD)
    close(out["dWb"].t, gb["dweight"].numpy(), what=f"dWb {what}", **GRAD)
    close(out["dba"].t, ga["dbias"].numpy(), what=f"dba {what}", **GRAD)
    if out["dbb"] is not None:
        close(out["dbb"].t, gb["dbias"].numpy(), what=f"dbb {what}", **GRAD)
    for k in ("dWa", "dWb", "dba", "dx"):
        assert out[k].guards(), f"{k} guards {what}"
    assert out["ws"].guards(), f"workspace guards {what}"
    out2 = run()
    for k in ("dWa", "dWb", "dx"):
        assert torch.equal(bits(out[k].t), bits(out2[k].t)), f"repeat {k} {what}"


def test_pair_pullback_refusals():
    n = 40000
    A = Dense(n, (64, 2), 64, seed=1400)
    base = A.blocks[0]

    def query_and_call(nn, Ta_w, Tb_w, dout, shareb=True, ashift=0):
        a = Dense(nn, Ta_w, dout, shifts=(ashift,) + (0,) * (len(Ta_w) - 1), seed=1401) if ashift else Dense(nn, Ta_w, dout, seed=1401, first=base)
        b = Dense(nn, Tb_w, dout, seed=1402, first=a.blocks[0] if shareb else None)
        na, pa, wa, ra = a.args()
        nb, pb, wb, rb = b.args()
        q = lib().ngpde_dense_pair_backward_workspace_bytes(nn, na, pa, wa, ra, nb, pb, wb, rb, dout)
        assert q == pair_bwd_workspace(pair_bwd_grid(nn, a.T, b.T, dout), a.din, b.din)
        assert q == 0
        t = torch.empty(1 << 16, device=DEV)
        st = lib().ngpde_dense_pair_backward(nn, na, pa, wa, ra, a.wt.data_ptr(), t.data_ptr(), t.data_ptr(), None, nb, pb, wb, rb,
                                             b.wt.data_ptr(), t.data_ptr(), t.data_ptr(), None, dout, t.data_ptr(), None, t.data_ptr(),
                                             t.numel() * 4, stream())
        assert st == _lib.ERR_UNSUPPORTED
    query_and_call(n, (64, 2), (64,), 32)                          # dout != 64
    query_and_call(32767, (64,), (64,), 64)                        # too few rows
    query_and_call(n, (64,), (64,), 64, shareb=False)              # two different leading blocks
    query_and_call(n, (64,), (64,), 64, ashift=1)                  # unaligned shared block
    query_and_call(n, (64, 5), (64,), 64)                          # five narrow features


# ---- refusals -----------------------------------------------------------------------------------------------------------------

def test_argument_refusals():
    P = Dense(100, (8,), 16, seed=1500)
    y = Buf((100, 16))
    x = P.blocks[0].ptr
    L = lib()
    five = ptr_array([x] * 5)
    st = L.ngpde_dense_forward(100, 5, five, int_array([8] * 5), None, 16, 0, P.wt.data_ptr(), None, y.ptr, None, stream())
    assert st == _lib.ERR_INVALID_ARGUMENT
    st = L.ngpde_dense_forward(100, 1, ptr_array([x]), int_array([-8]), None, 16, 0, P.wt.data_ptr(), None, y.ptr, None, stream())
    assert st == _lib.ERR_DIMENSION_MISMATCH
    st = L.ngpde_dense_forward(100, 1, ptr_array([x]), int_array([8]), None, 16, 9, P.wt.data_ptr(), None, y.ptr, None, stream())
    assert st == _lib.ERR_INVALID_ARGUMENT
    ws = Workspace(L.ngpde_dense_workspace_bytes(100, 8, 16))
    st = L.ngpde_dense_backward(100, 5, five, int_array([8] * 5), None, 16, 0, P.wt.data_ptr(), None, y.ptr, None, y.ptr, None,
                                ws.ptr, ws.n, stream())
    assert st == _lib.ERR_INVALID_ARGUMENT
    st = L.ngpde_dense_backward(100, 1, ptr_array([x]), int_array([8]), None, 16, 9, P.wt.data_ptr(), y.ptr, y.ptr, None, y.ptr, None,
                                ws.ptr, ws.n, stream())
    assert st == _lib.ERR_INVALID_ARGUMENT
    st = L.ngpde_dense_multi_forward(5, (C.c_int64 * 5)(*[100] * 5), int_array([1] * 5), five, int_array([8] * 5), None, int_array([16] * 5),
                                     int_array([0] * 5), ptr_array([P.wt.data_ptr()] * 5), ptr_array([0] * 5), ptr_array([y.ptr] * 5),
                                     ptr_array([0] * 5), stream())
    assert st == _lib.ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
    assert y.untouched()
