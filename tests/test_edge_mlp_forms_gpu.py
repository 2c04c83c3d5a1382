"""The one-launch message-MLP kernels against float64 across their tile envelope.

ngpde_edge_mlp_forward / ngpde_edge_mlp_backward run three kernel families, each of which picks its LDS layout, grid and
summation form from the graph's tile geometry -- max_halo, the largest number of distinct rows one 32-row tile stages (own rows,
padding rows included, plus distinct foreign sources; capped at 96), and the tile count:
  a. csrc/edge_mlp64.hip, the 64 => 64 two-layer specialisation (six activation pairs, + / mean).  LDS (halo + 225) * 272 B:
     up to a halo of 61 two workgroups per CU (64 per XCD), from 62 one (the forward 32 per XCD, the pullback half the grid).
     The pullback sums dz1 by source inside its launch ("DQ", no [E][64] array) iff there is no per-edge term and the halo is at
     most kDqStride = 48 rows; NGPDE_EDGE64_NO_DQ=1 (read per call) keeps the [E][64] array + by-source pass.
  b. csrc/edge_mlp_fused.hip, the general forward <n_tail 0..3> (two workgroups per CU iff (halo + 161 + 64 n_tail) * 272 B + 2 KB
     fits in 80 KB: always at n_tail 0, up to halo 68 at n_tail 1, never from n_tail 2) and the pullback <0, 1> (all five aggregations).
  c. csrc/edge_mlp_deep_bwd.hip, the one-launch pullback of 3- and 4-layer message MLPs ((halo + 97 + 128 n_tail) * 272 B: 153 KB at
     n_tail 3 and halo 96).
All of them are persistent grids of at most 8 x {32, 64} workgroups; tile ranges are split per XCD (n_tiles / 8 and the remainder),
so beyond 512 tiles every kernel has workgroups that walk several tiles.

Every case builds its handle with ngpde_graph_create_device and an explicit node order (tiles = consecutive 32-node runs of it),
asserts the regime it claims with tile_geometry() and the library's queries, and compares every output and gradient with a plain
float64 restatement (torch double on the CPU, autograd for the MLP, the aggregation pullback as ngpde.h states it).  Outputs the
contract says are written are pre-filled with NaN, and so is the workspace.

The halo thresholds (48, 61, 68) are derived from those LDS formulas in tests/edge_mlp_forms_spec.py, the restatement of
csrc/edge_mlp_forms.h, where every choice above is made; the last test pins the queries' answers to tests/golden/edge_mlp_forms.json.

Tolerances are the suite's: forward 1e-4 * max|ref| + 1e-5, gradients 5e-4 relative.
"""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from ngpde_amd.functional import _int_array, _ptr_array
import ngpde_amd as ng
import edge_mlp_forms_spec as S
# 48 (kDqStride), 61 and 68: derived there from the LDS formulas of csrc/edge_mlp_forms.h
from edge_mlp_forms_spec import DQ_MAX_HALO, E64_FULL_GRID_MAX_HALO, FWD1_TWO_PER_CU_MAX_HALO, SWITCHES
from test_mp_gpu import close

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS, HALO_CAP, SLOT_WIDTH = 32, 96, 32
MULTI_TILE = 8 * 64 + 1     # more tiles than any of these grids has workgroups (<= 64 per XCD)
E64_PAIRS = [("swish", "swish"), ("swish", "identity"), ("relu", "relu"), ("relu", "identity"), ("tanh", "tanh"),
             ("tanh", "identity")]
AGGRS = ("+", "mean", "max", "min", "*")


def clear_switches(monkeypatch):
    # the suite may run under one of these: every case here names the form it tests
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


# ---- graphs of chosen tile geometry -----------------------------------------------------------------------------------------------

def tile_geometry(s, t, order, n):
    """(halo of every tile, largest row degree, edges of every tile) for the tiles = consecutive 32-node runs of `order`.
    A tile's halo is its 32 own rows (padding rows of a ragged last tile included) plus its distinct foreign sources."""
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    n_tiles = -(-n // ROWS)
    tt, ts = pos[t] // ROWS, pos[s] // ROWS
    foreign = tt != ts
    pairs = np.unique(tt[foreign] * n + np.asarray(s, dtype=np.int64)[foreign])
    halo = ROWS + np.bincount(pairs // n, minlength=n_tiles)
    deg = np.bincount(t, minlength=n)
    return halo, int(deg.max(initial=0)), np.bincount(tt, minlength=n_tiles)


def spread(total, rows, rng, cap=SLOT_WIDTH):
    """`total` edges over `rows` rows, at most `cap` per row, at random"""
    assert 0 <= total <= rows * cap
    d = np.zeros(rows, dtype=np.int64)
    left = total
    while left:
        free = np.flatnonzero(d < cap)
        take = rng.choice(free, size=min(left, free.size), replace=False)
        d[take] += 1
        left -= take.size
    return d


def tiled_graph(n, spec, seed):
    """COO lists + node order of a graph whose tile k (positions 32k .. of the order) has exactly spec(k, rows, rng) = (F, degrees):
    F distinct foreign sources (so halo 32 + F) and the given in-degree per row; a row's sources are distinct.  Nodes are a random
    permutation of the positions and the COO list is shuffled."""
    rng = np.random.default_rng(seed)
    n_tiles = -(-n // ROWS)
    S, T = [], []
    for k in range(n_tiles):
        lo, hi = k * ROWS, min(n, (k + 1) * ROWS)
        rows = hi - lo
        F, degs = spec(k, rows, rng)
        F = min(F, n - rows)                                        # (a graph of one tile has no foreign rows)
        degs = np.asarray(degs, dtype=np.int64)
        assert degs.size == rows and degs.sum() >= F and degs.max(initial=0) <= rows + F
        outside = rng.choice(n - rows, size=F, replace=False)
        outside = outside + (outside >= lo) * rows                 # skip the tile's own positions
        pool = np.concatenate([np.arange(lo, hi), outside])
        keys = rng.random((rows, pool.size))
        if F:                                                       # every foreign source on one randomly chosen edge slot
            row_of_slot = np.repeat(np.arange(rows), degs)
            keys[row_of_slot[rng.choice(row_of_slot.size, size=F, replace=False)], rows + np.arange(F)] = -1.0
        pick = pool[np.argsort(keys, axis=1)]
        S.append(pick[np.arange(pool.size)[None, :] < degs[:, None]])
        T.append(np.repeat(np.arange(lo, hi), degs))
    s_pos, t_pos = np.concatenate(S), np.concatenate(T)
    order = rng.permutation(n).astype(np.int32)                     # order[position] = node
    perm = rng.permutation(s_pos.size)
    return order[s_pos][perm].astype(np.int64), order[t_pos][perm].astype(np.int64), order


def random_degrees(rows, rng, F, hi=12):
    """in-degrees below `hi` at random, at least F edges in all, no row beyond its distinct candidate sources"""
    cap = min(SLOT_WIDTH, rows + F)
    d = np.minimum(rng.integers(0, hi, rows), cap)
    while d.sum() < F:
        d[rng.choice(np.flatnonzero(d < cap))] += 1
    return d


def halo_spec(H, hot_every=5, hi=12):
    """max halo exactly H: every hot_every-th tile at H, the others anywhere in 32 .. H"""
    def spec(k, rows, rng):
        F = H - ROWS if k % hot_every == 0 else int(rng.integers(0, H - ROWS + 1))
        F = min(F, SLOT_WIDTH * rows)                               # (a ragged last tile of few rows)
        return F, random_degrees(rows, rng, F, hi)
    return spec


class TileGraph:
    """ngpde_graph_t built on the device with an explicit node order (or the handle's own: order=None), GCN normalisation set
    (it builds the tile schedule and halos), plus the host-side facts the cases assert and the reference needs"""

    def __init__(self, s, t, n, order):
        lib = _lib.load()
        self.n, self.s, self.t = n, np.asarray(s, dtype=np.int64), np.asarray(t, dtype=np.int64)
        ds = torch.as_tensor(self.s.astype(np.int32), device=DEV)
        dt = torch.as_tensor(self.t.astype(np.int32), device=DEV)
        do = None if order is None else torch.as_tensor(np.asarray(order, dtype=np.int32), device=DEV)
        out = C.c_void_p()
        _lib.check(lib.ngpde_graph_create_device(n, self.s.size, _lib.ptr(ds), _lib.ptr(dt), 32, 0, 1, _lib.ptr(do), _lib.current_stream(),
                                                 C.byref(out)))
        self.ptr = out
        _lib.check(lib.ngpde_graph_set_gcn_norm_device(out, 0, None, 0, _lib.current_stream()))
        if order is None:
            order = np.empty(n, dtype=np.int32)
            _lib.check(lib.ngpde_graph_node_order(out, order.ctypes.data))
        self.order = np.asarray(order)
        self.halo, self.max_deg, self.tile_edges = tile_geometry(self.s, self.t, self.order, n)
        self.n_tiles = self.halo.size
        self.max_halo = int(self.halo.max())
        p = np.argsort(self.t, kind="stable")                       # p order: CSR by target, COO order inside a row
        self.sp, self.tp = torch.as_tensor(self.s[p]), torch.as_tensor(self.t[p])
        self.deg = torch.as_tensor(np.bincount(self.t, minlength=n))
        self.E = self.s.size

    def close(self):
        if self.ptr is not None:
            _lib.destroy_later("ngpde_graph_destroy", self.ptr)
            self.ptr = None

    def fits(self):
        return self.max_halo <= HALO_CAP and self.max_deg <= SLOT_WIDTH


_graphs = {}


@pytest.fixture(scope="module", autouse=True)
def _release_graphs():
    yield
    for g in _graphs.values():
        g.close()
    _graphs.clear()


def graph(key, make):
    """graphs are shared between the cases of the module (a handle is immutable)"""
    if key not in _graphs:
        _graphs[key] = make()
    return _graphs[key]


def halo_graph(H, n_tiles=24, ragged=5, seed=None):
    def make():
        n = n_tiles * ROWS - ragged
        s, t, order = tiled_graph(n, halo_spec(H, hi=6 if n_tiles > 256 else 12), seed if seed is not None else 1000 + H + n_tiles)
        g = TileGraph(s, t, n, order)
        assert g.max_halo == H and g.n_tiles == n_tiles and g.fits(), (H, g.max_halo, g.n_tiles)
        return g
    return graph(("halo", H, n_tiles, ragged, seed), make)


# ---- the float64 restatement ------------------------------------------------------------------------------------------------------

_GELU_C = math.sqrt(2.0 / math.pi)
ACTS = {
    "identity": lambda z: z,
    "relu": torch.relu,
    "tanh": torch.tanh,
    "sigmoid": torch.sigmoid,
    "swish": lambda z: z * torch.sigmoid(z),
    "gelu": lambda z: 0.5 * z * (1.0 + torch.tanh(_GELU_C * (z + 0.044715 * z ** 3))),
    "leakyrelu": lambda z: torch.where(z > 0, z, 0.01 * z),
    "elu": lambda z: torch.where(z > 0, z, torch.expm1(torch.clamp(z, max=0.0))),
    "softplus": lambda z: torch.logaddexp(torch.zeros_like(z), z),
}


def f64(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.float64)


def aggregate(g, M, aggr):
    N, d = g.n, M.shape[1]
    idx = g.tp[:, None].expand(-1, d)
    if aggr in ("+", "mean"):
        out = torch.zeros(N, d, dtype=M.dtype).index_add_(0, g.tp, M)
        return out / g.deg.clamp(min=1)[:, None].to(M.dtype) if aggr == "mean" else out
    init, how = {"max": (-math.inf, "amax"), "min": (math.inf, "amin"), "*": (1.0, "prod")}[aggr]
    return torch.full((N, d), init, dtype=M.dtype).scatter_reduce(0, idx, M, how, include_self=True)


def aggregate_pullback(g, M, out, dout, aggr):
    """dM as ngpde.h states it: max / min -- every message equal to the extremum receives the gradient; * -- every message the
    gradient times the product of the OTHERS: the one zero message of a row the product of the rest, nothing where two are zero"""
    tp = g.tp
    if aggr == "+":
        return dout[tp]
    if aggr == "mean":
        return dout[tp] / g.deg.clamp(min=1)[tp][:, None].to(M.dtype)
    if aggr in ("max", "min"):
        return dout[tp] * (M == out[tp]).to(M.dtype)
    zero = M == 0
    nz = torch.zeros_like(out).index_add_(0, tp, zero.to(M.dtype))[tp]
    pnz = aggregate(g, torch.where(zero, torch.ones_like(M), M), "*")[tp]
    other = torch.where(zero, torch.where(nz == 1, pnz, torch.zeros_like(M)),
                        torch.where(nz == 0, pnz / torch.where(zero, torch.ones_like(M), M), torch.zeros_like(M)))
    return dout[tp] * other


class Problem:
    """z1_e = P[t_e] + Q[s_e] (+ E_e); a = act1(z1); a <- act_l(a W_l + b_l) for each tail layer; out_i = aggr_{e: t_e = i} a_e"""

    def __init__(self, g, h1, act1, tail, aggr, seed, e_term=False, bias=True, scale=1.0):
        rng = np.random.default_rng(seed)
        self.g, self.h1, self.act1, self.aggr = g, h1, act1, aggr
        self.P = (scale * rng.normal(size=(g.n, h1))).astype(np.float32)
        self.Q = (scale * rng.normal(size=(g.n, h1))).astype(np.float32)
        self.Et = (scale * rng.normal(size=(g.E, h1))).astype(np.float32) if e_term else None
        self.douts, self.acts, self.W, self.b = [], [], [], []
        din = h1
        for dout, act in tail:
            self.W.append((rng.normal(size=(din, dout)) * 1.5 / np.sqrt(din)).astype(np.float32))
            self.b.append((0.3 * rng.normal(size=dout)).astype(np.float32) if bias else None)
            self.douts.append(dout)
            self.acts.append(act)
            din = dout
        self.width = din
        self.dout = rng.normal(size=(g.n, din)).astype(np.float32)
        self._ref = None
        if aggr in ("max", "min"):
            # which message attains a row's extremum is decided in float32 by the kernel: where the runner-up is within 1e-5 of it
            # (tanh saturating near +-1 gives such near-ties) the choice is not determined by the operation, and that output
            # entry gets no gradient
            with torch.no_grad():
                M = self._chain(f64(self.P), f64(self.Q), self._e64(), [f64(w) for w in self.W],
                                [f64(x) if x is not None else None for x in self.b])[1]
                ext = aggregate(g, M, aggr)
                gap = torch.where(M == ext[g.tp], math.inf, (M - ext[g.tp]).abs() / (1 + ext[g.tp].abs()))
                near = torch.zeros_like(ext).index_add_(0, g.tp, (gap < 1e-5).double()) > 0
            assert near.double().mean() < 0.01
            self.dout[near.numpy()] = 0.0

    def _e64(self):
        return f64(self.Et) if self.Et is not None else torch.zeros(self.g.E, self.h1, dtype=torch.float64)

    def _chain(self, P, Q, E, W, b):
        g = self.g
        z = P[g.tp] + Q[g.sp] + E
        zs = [z]
        a = ACTS[self.act1](z)
        for l in range(self.n_tail):
            z = a @ W[l] + (b[l] if b[l] is not None else 0.0)
            zs.append(z)
            a = ACTS[self.acts[l]](z)
        return zs, a

    @property
    def n_tail(self):
        return len(self.douts)

    def reference(self):
        """(out, [z1, z_1 .. z_n_tail] in p order, {name: gradient}) in float64"""
        if self._ref is not None:
            return self._ref
        g = self.g
        P, Q = f64(self.P).requires_grad_(), f64(self.Q).requires_grad_()
        E = self._e64().requires_grad_()
        W = [f64(w).requires_grad_() for w in self.W]
        b = [f64(x).requires_grad_() if x is not None else None for x in self.b]
        zs, M = self._chain(P, Q, E, W, b)
        out = aggregate(g, M.detach(), self.aggr)
        dM = aggregate_pullback(g, M.detach(), out, f64(self.dout), self.aggr)
        leaves = [P, Q, E] + W + [x for x in b if x is not None]
        gr = torch.autograd.grad(M, leaves, dM, allow_unused=True)
        zero = lambda x, gx: torch.zeros_like(x) if gx is None else gx
        grads = {"dP": zero(P, gr[0]), "dQ": zero(Q, gr[1]), "dE": zero(E, gr[2])}
        for l in range(self.n_tail):
            grads[f"dW{l}"] = zero(W[l], gr[3 + l])
        it = iter(gr[3 + self.n_tail:])
        for l in range(self.n_tail):
            if b[l] is not None:
                grads[f"db{l}"] = zero(b[l], next(it))
        self._ref = (out, [x.detach() for x in zs], grads)
        return self._ref

    # ---- the library ----
    def _dev(self):
        if not hasattr(self, "_d"):
            dv = lambda a: None if a is None else torch.as_tensor(a, device=DEV)
            self._d = dict(P=dv(self.P), Q=dv(self.Q), E=dv(self.Et), W=[dv(w) for w in self.W], b=[dv(x) for x in self.b],
                           dout=dv(self.dout))
        return self._d

    def _tables(self):
        n = self.n_tail
        d = self._dev()
        return ((_int_array(self.douts), _int_array([_lib.ACT[a] for a in self.acts]), _ptr_array(d["W"]),
                 _ptr_array(d["b"]) if any(x is not None for x in d["b"]) else None) if n else (None, None, None, None))

    def forward_status(self, save=False):
        """(status, out, saved pre-activations or None)"""
        lib, d, g = _lib.load(), self._dev(), self.g
        douts, acts, wts, bs = self._tables()
        out = torch.full((g.n, self.width), math.nan, device=DEV)
        saves = [torch.full((g.E, w), math.nan, device=DEV) for w in [self.h1] + self.douts] if save else None
        st = lib.ngpde_edge_mlp_forward(g.ptr, self.h1, _lib.ACT[self.act1], _lib.ptr(d["P"]), _lib.ptr(d["Q"]), _lib.ptr(d["E"]),
                                        self.n_tail, douts, acts, wts, bs, _lib.AGGR[self.aggr], _lib.ptr(out),
                                        _ptr_array(saves) if save else None, _lib.current_stream())
        return st, out, saves

    def forward(self, save=False):
        st, out, saves = self.forward_status(save)
        _lib.check(st)
        return out, saves

    def needs_edge_buffer(self):
        douts, acts, _, _ = self._tables()
        return int(_lib.load().ngpde_edge_mlp_backward_needs_edge_buffer(self.g.ptr, self.h1, _lib.ACT[self.act1], int(self.Et is not None),
                                                                          self.n_tail, douts, acts, _lib.AGGR[self.aggr]))

    def backward_status(self, with_de=True):
        """(status, {name: gradient}); dE is passed only when with_de (the DQ form needs none)"""
        lib, d, g = _lib.load(), self._dev(), self.g
        douts, acts, wts, bs = self._tables()
        nan = lambda *shape: torch.full(shape, math.nan, device=DEV)
        dP, dQ = nan(g.n, self.h1), nan(g.n, self.h1)
        dE = nan(g.E, self.h1) if with_de else None
        dW = [nan(*w.shape) for w in self.W]
        db = [nan(x.size) if x is not None else None for x in self.b]
        ws_bytes = int(lib.ngpde_edge_mlp_backward_workspace_bytes(g.ptr, self.h1, self.n_tail, douts))
        ws = torch.full((max(ws_bytes, 256),), 0xFF, dtype=torch.uint8, device=DEV)     # NaN words
        st = lib.ngpde_edge_mlp_backward(g.ptr, self.h1, _lib.ACT[self.act1], _lib.ptr(d["P"]), _lib.ptr(d["Q"]), _lib.ptr(d["E"]),
                                         self.n_tail, douts, acts, wts, bs, _lib.AGGR[self.aggr], _lib.ptr(d["dout"]), _lib.ptr(dP),
                                         _lib.ptr(dQ), _lib.ptr(dE), _ptr_array(dW) if self.n_tail else None,
                                         _ptr_array(db) if self.n_tail and bs is not None else None, _lib.ptr(ws), ws.numel(),
                                         _lib.current_stream())
        out = {"dP": dP, "dQ": dQ}
        if with_de:
            out["dE"] = dE
        for l in range(self.n_tail):
            out[f"dW{l}"] = dW[l]
            if db[l] is not None:
                out[f"db{l}"] = db[l]
        return st, out

    def backward(self, with_de=True):
        st, out = self.backward_status(with_de)
        _lib.check(st)
        return out

    # ---- checks ----
    def check_forward(self, out, saves=None, what=""):
        ref, zs, _ = self.reference()
        fin = torch.isfinite(ref)
        got_fin = torch.isfinite(out).cpu()
        assert torch.equal(got_fin, fin), f"non-finite pattern {what}"     # (max / min of an empty row: -inf / +inf, as scatter)
        assert torch.equal(out.cpu()[~fin], ref[~fin].float()), f"empty rows {what}"
        close(torch.where(fin, out.cpu().double(), 0.0), torch.where(fin, ref, 0.0).numpy(), what=f"out {what}")
        if saves is not None:
            for l, (sz, rz) in enumerate(zip(saves, zs)):
                close(sz, rz.numpy(), what=f"save_z[{l}] {what}")

    def check_backward(self, grads, what=""):
        _, _, ref = self.reference()
        for name, gv in grads.items():
            close(gv, ref[name].numpy(), rtol=5e-4, atol=1e-5, what=f"{name} {what}")


def same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) if isinstance(a, dict) else torch.equal(a, b)


def assert_regime(g, lo, hi):
    assert lo <= g.max_halo <= hi, (g.max_halo, lo, hi)
    assert int(_lib.load().ngpde_edge_mlp_supported(g.ptr, 64, 1, _int_array([64]))) == int(g.fits())


# ---- 1. geometry: the helper against the library's own queries --------------------------------------------------------------------

@pytest.mark.parametrize("H", [32, 48, 49, 61, 62, 68, 69, 96])
def test_tile_geometry_and_library_queries(H, monkeypatch):
    # the halo the helper counts is the one the library sized its tiles with: supported iff halo <= 96 and degree <= 32, and the
    # 64-wide pullback sums by source in its launch iff the halo is at most 48 rows and nothing switches that off
    clear_switches(monkeypatch)
    lib = _lib.load()
    g = halo_graph(H)
    assert g.max_halo == H and g.fits()
    d64, relu = _int_array([64]), _int_array([_lib.ACT["relu"]])
    assert lib.ngpde_edge_mlp_supported(g.ptr, 64, 1, d64) == 1
    assert lib.ngpde_edge_mlp_backward_supported(g.ptr, 64, 1, d64, _lib.AGGR["+"]) == 1
    assert lib.ngpde_edge_mlp_backward_needs_edge_buffer(g.ptr, 64, _lib.ACT["relu"], 0, 1, d64, relu, _lib.AGGR["+"]) == int(H > DQ_MAX_HALO)
    assert lib.ngpde_edge_mlp_backward_needs_edge_buffer(g.ptr, 64, _lib.ACT["relu"], 1, 1, d64, relu, _lib.AGGR["+"]) == 1
    monkeypatch.setenv("NGPDE_EDGE64_NO_DQ", "1")
    assert lib.ngpde_edge_mlp_backward_needs_edge_buffer(g.ptr, 64, _lib.ACT["relu"], 0, 1, d64, relu, _lib.AGGR["+"]) == 1


def test_default_order_handle_geometry(monkeypatch):
    # a handle built the default way (the library's own locality order) on a randomly labelled 2-D grid: the helper takes
    # ngpde_graph_node_order's order, agrees with the library's queries, and the fused forms agree with float64 on it
    clear_switches(monkeypatch)
    rng = np.random.default_rng(5)
    nx, ny = 41, 37
    n = nx * ny
    ij = np.arange(n).reshape(ny, nx)
    pairs = [(ij[:, :-1], ij[:, 1:]), (ij[:-1, :], ij[1:, :]), (ij[:-1, :-1], ij[1:, 1:])]
    a = np.concatenate([p[0].ravel() for p in pairs])
    b = np.concatenate([p[1].ravel() for p in pairs])
    label = rng.permutation(n)
    s, t = label[np.concatenate([a, b])], label[np.concatenate([b, a])]
    g = graph(("default order",), lambda: TileGraph(s, t, n, None))
    assert np.array_equal(ng.GNNGraph(s, t, num_nodes=n, index_base=0).node_order(), g.order)
    assert g.fits() and g.max_halo > ROWS
    assert_regime(g, ROWS + 1, HALO_CAP)
    lib = _lib.load()
    assert lib.ngpde_edge_mlp_backward_needs_edge_buffer(g.ptr, 64, _lib.ACT["tanh"], 0, 1, _int_array([64]), _int_array([0]),
                                                         0) == int(g.max_halo > DQ_MAX_HALO)
    pr = Problem(g, 64, "tanh", [(64, "identity")], "+", seed=3)
    pr.check_forward(pr.forward()[0], what="default order")
    pr.check_backward(pr.backward(with_de=g.max_halo > DQ_MAX_HALO), what="default order")
    pr = Problem(g, 12, "gelu", [(60, "tanh")], "max", seed=4, e_term=True)
    pr.check_forward(pr.forward()[0], what="default order, general")
    pr.check_backward(pr.backward(), what="default order, general")


def refused_graph(why):
    """ten tiles, one of them at 97 rows ("halo 97") or with one row of 33 entries ("degree 33")"""
    n = 10 * ROWS

    def spec97(k, rows, rng):
        return (65, spread(200, rows, rng)) if k == 3 else (5, random_degrees(rows, rng, 5))

    def spec33(k, rows, rng):
        d = random_degrees(rows, rng, 4)
        if k == 6:
            d[7] = 33
        return 4, d

    def make():
        s, t, order = tiled_graph(n, {"halo 97": spec97, "degree 33": spec33}[why], seed=11)
        return TileGraph(s, t, n, order)
    return graph(("refused", why), make)


def test_tiles_beyond_the_halo_cap_or_slot_width_are_refused(monkeypatch):
    # one tile at 97 rows / one row of 33 entries: every query says 0 and the entries return ERR_UNSUPPORTED (no launch)
    clear_switches(monkeypatch)
    lib = _lib.load()
    for why in ("halo 97", "degree 33"):
        g = refused_graph(why)
        assert (g.max_halo == 97) if why == "halo 97" else (g.max_deg == 33 and g.max_halo <= HALO_CAP), why
        assert not g.fits()
        for h1, tail in ((64, [(64, "relu")]), (12, []), (60, [(64, "tanh")]), (4, [(12, "tanh"), (60, "swish")]),
                         (64, [(60, "tanh"), (12, "relu"), (40, "identity")])):
            douts = _int_array([d for d, _ in tail]) if tail else None
            assert lib.ngpde_edge_mlp_supported(g.ptr, h1, len(tail), douts) == 0, why
            for aggr in ("+", "*"):
                assert lib.ngpde_edge_mlp_backward_supported(g.ptr, h1, len(tail), douts, _lib.AGGR[aggr]) == 0, why
                pr = Problem(g, h1, "relu", tail, aggr, seed=1)
                st, out, _ = pr.forward_status()
                assert st == _lib.ERR_UNSUPPORTED, (why, st)
                assert bool(torch.isnan(out).all())
                if len(tail) < 2 or aggr == "+":
                    st, gr = pr.backward_status(with_de=True)
                    assert st == _lib.ERR_UNSUPPORTED, (why, st)
                    assert all(bool(torch.isnan(v).all()) for v in gr.values())


# ---- 2. edge_mlp64: forward and pullback ------------------------------------------------------------------------------------------

def check_edge64(pr, monkeypatch, what):
    """edge_mlp64 forward (twice: bitwise), the general kernel (NGPDE_NO_EDGE64=1: bitwise the same), the pullback in the form the
    halo selects and in the [E][64] form (NGPDE_EDGE64_NO_DQ=1), each twice (bitwise), and the general pullback -- all against float64"""
    g = pr.g
    dq = g.max_halo <= DQ_MAX_HALO
    y = pr.forward()[0]
    pr.check_forward(y, what=what)
    assert same(y, pr.forward()[0]), f"forward repeat {what}"
    monkeypatch.setenv("NGPDE_NO_EDGE64", "1")
    yg = pr.forward()[0]
    monkeypatch.delenv("NGPDE_NO_EDGE64")
    assert same(y, yg), f"edge_mlp64 forward != general forward {what}"
    assert pr.needs_edge_buffer() == int(not dq), what
    gd = pr.backward(with_de=not dq)                # the DQ form gets no [E][64] buffer at all
    pr.check_backward(gd, what=f"{'DQ' if dq else '[E][64]'} {what}")
    assert same(gd, pr.backward(with_de=not dq)), f"pullback repeat {what}"
    monkeypatch.setenv("NGPDE_EDGE64_NO_DQ", "1")
    assert pr.needs_edge_buffer() == 1, what
    gn = pr.backward(with_de=True)
    pr.check_backward(gn, what=f"NO_DQ {what}")
    assert same(gn, pr.backward(with_de=True)), f"NO_DQ pullback repeat {what}"
    monkeypatch.delenv("NGPDE_EDGE64_NO_DQ")
    monkeypatch.setenv("NGPDE_NO_EDGE64", "1")
    pr.check_backward(pr.backward(with_de=True), what=f"general pullback {what}")
    monkeypatch.delenv("NGPDE_NO_EDGE64")


E64_HALOS = [ROWS, DQ_MAX_HALO, DQ_MAX_HALO + 1, E64_FULL_GRID_MAX_HALO, E64_FULL_GRID_MAX_HALO + 1, HALO_CAP]


@pytest.mark.parametrize("H", E64_HALOS)
@pytest.mark.parametrize("acts", E64_PAIRS, ids=["-".join(a) for a in E64_PAIRS])
def test_edge64_against_float64_across_halos(acts, H, monkeypatch):
    # DQ up to 48 rows, the [E][64] form above; two workgroups per CU up to 61 rows, one (and the pullback's halved grid) from 62.
    # Regression (edge_mlp64 pullback grid not a multiple of 8): from a halo of 62 the pullback launched half its usual grid,
    # 4 * ceil(n_tiles / 8) workgroups -- 12 at these 24 tiles.  The kernel walks per-XCD tile ranges with gridDim.x / 8 workgroups
    # each, so workgroups 8 .. 11 walked tiles of XCDs 0 .. 3 a second time and dW2 / db2 counted those tiles twice.
    clear_switches(monkeypatch)
    g = halo_graph(H)
    assert_regime(g, H, H)
    assert ((g.n_tiles + 7) // 8) % 2 == 1                          # (an odd tile range per XCD: the halved grid was not 8 k)
    for aggr in ("+", "mean"):
        pr = Problem(g, 64, acts[0], [(64, acts[1])], aggr, seed=H * 7 + len(aggr))
        check_edge64(pr, monkeypatch, f"halo={H} acts={acts} aggr={aggr}")


@pytest.mark.parametrize("H", [DQ_MAX_HALO, E64_FULL_GRID_MAX_HALO + 1])
@pytest.mark.parametrize("acts", E64_PAIRS, ids=["-".join(a) for a in E64_PAIRS])
def test_edge64_workgroups_walk_several_tiles(acts, H, monkeypatch):
    # 513 tiles (uneven split over the 8 XCDs, ragged last tile): every workgroup of the <= 64-per-XCD grids has two or more tiles;
    # DQ with its per-tile foreign partials at 48, the halved pullback grid at 62
    clear_switches(monkeypatch)
    g = halo_graph(H, n_tiles=MULTI_TILE, ragged=3)
    assert g.n_tiles >= MULTI_TILE and g.n_tiles % 8 != 0
    assert_regime(g, H, H)
    aggr = "mean" if E64_PAIRS.index(acts) % 2 else "+"
    pr = Problem(g, 64, acts[0], [(64, acts[1])], aggr, seed=H + E64_PAIRS.index(acts))
    check_edge64(pr, monkeypatch, f"tiles={g.n_tiles} halo={H} acts={acts} aggr={aggr}")


# ---- 3. the general kernels -------------------------------------------------------------------------------------------------------

# (h1, act1, tail): n_tail 0..3, widths from {4, 12, 60, 64} (h1 < 64 among them), every activation over the configurations
FWD_CONFIGS = {
    "t0-12": (12, "gelu", []),
    "t0-64": (64, "elu", []),
    "t1-60-64": (60, "softplus", [(64, "leakyrelu")]),
    "t1-64-12": (64, "relu", [(12, "sigmoid")]),
    "t2-4-12-60": (4, "swish", [(12, "tanh"), (60, "identity")]),
    "t3-4-12-60-40": (4, "tanh", [(12, "gelu"), (60, "swish"), (40, "sigmoid")]),
    "t3-64-60-12-4": (64, "sigmoid", [(60, "elu"), (12, "relu"), (4, "softplus")]),
}
GEOMS = {"halo40": (40, 24), "halo68": (FWD1_TWO_PER_CU_MAX_HALO, 24), "halo69": (FWD1_TWO_PER_CU_MAX_HALO + 1, 24),
         "halo96": (HALO_CAP, 24), "tiles": (80, MULTI_TILE)}


@pytest.mark.parametrize("geom", list(GEOMS))
@pytest.mark.parametrize("cfg", list(FWD_CONFIGS))
def test_general_forward_against_float64(cfg, geom, monkeypatch):
    # edge_mlp_fused_fwd_kernel<n_tail>: all five aggregations (* of an empty row = 1, max / min of one = -inf / +inf), e_term present
    # and NULL, save_z present (pre-activations in p order) and NULL; at n_tail 1 the halos 68 / 69 straddle the change from two
    # workgroups per CU to one
    clear_switches(monkeypatch)
    H, nt = GEOMS[geom]
    g = halo_graph(H, n_tiles=nt, ragged=7)
    assert_regime(g, H, H)
    h1, act1, tail = FWD_CONFIGS[cfg]
    assert _lib.load().ngpde_edge_mlp_supported(g.ptr, h1, len(tail), _int_array([d for d, _ in tail]) if tail else None) == 1
    case = 0
    for aggr in AGGRS:
        for e_term in (False, True):
            pr = Problem(g, h1, act1, tail, aggr, seed=case + 31 * len(tail) + H, e_term=e_term, bias=case % 3 != 0,
                         scale=0.5 if aggr == "*" else 1.0)
            for save in (False, True):
                out, saves = pr.forward(save=save)
                pr.check_forward(out, saves, what=f"{cfg} {geom} aggr={aggr} e_term={e_term} save_z={save}")
            case += 1
    assert g.deg.eq(0).any()                                        # empty rows were covered


PULLBACK_CONFIGS = {0: (64, "tanh", []), 1: (60, "swish", [(64, "tanh")])}


@pytest.mark.parametrize("geom", ["halo40", "halo69", "halo96", "tiles"])
@pytest.mark.parametrize("n_tail", [0, 1])
def test_general_pullback_against_float64(n_tail, geom, monkeypatch):
    # edge_mlp_fused_bwd_kernel<n_tail> + slab reduce + by-source sum, all five aggregations, e_term present and NULL.  Under * the
    # last activation is relu, so rows hold exactly one and exactly two zero messages; a run with nonzero messages follows
    clear_switches(monkeypatch)
    H, nt = GEOMS[geom]
    g = halo_graph(H, n_tiles=nt, ragged=7)
    assert_regime(g, H, H)
    h1, act1, tail = PULLBACK_CONFIGS[n_tail]
    douts = _int_array([d for d, _ in tail]) if tail else None
    lib = _lib.load()
    for aggr, zeros in (("+", False), ("mean", False), ("max", False), ("min", False), ("*", True), ("*", False)):
        assert lib.ngpde_edge_mlp_backward_supported(g.ptr, h1, n_tail, douts, _lib.AGGR[aggr]) == 1
        a1, tl = (act1, [(d, "relu") for d, _ in tail]) if zeros and tail else ("relu" if zeros else act1, tail)
        for e_term in (False, True):
            pr = Problem(g, h1, a1, tl, aggr, seed=H + 3 * n_tail + len(aggr) + e_term, e_term=e_term, scale=0.5 if aggr == "*" else 1.0)
            what = f"n_tail={n_tail} {geom} aggr={aggr}{' (zero messages)' if zeros else ''} e_term={e_term}"
            assert pr.needs_edge_buffer() == 1
            if zeros:
                M = torch.relu(pr.reference()[1][-1])
                nz = torch.zeros(g.n, M.shape[1], dtype=torch.float64).index_add_(0, g.tp, (M == 0).double())
                assert (nz == 1).any() and (nz == 2).any(), what
            pr.check_forward(pr.forward()[0], what=what)
            pr.check_backward(pr.backward(with_de=True), what=what)


# ---- 4. the deep pullback ---------------------------------------------------------------------------------------------------------

DEEP_CONFIGS = {
    "t2-60-64-12": (60, "tanh", [(64, "swish"), (12, "identity")]),
    "t3-4-12-60-40": (4, "swish", [(12, "tanh"), (60, "relu"), (40, "identity")]),
}


@pytest.mark.parametrize("geom", ["halo40", "halo96", "tiles"])
@pytest.mark.parametrize("cfg", list(DEEP_CONFIGS))
def test_deep_pullback_against_float64(cfg, geom, monkeypatch):
    # edge_mlp_deep_bwd_kernel<2 / 3>: + and mean, with and without e_term; halo 96 at n_tail 3 is the largest LDS request (153 KB)
    clear_switches(monkeypatch)
    H, nt = GEOMS[geom]
    g = halo_graph(H, n_tiles=nt, ragged=7)
    assert_regime(g, H, H)
    h1, act1, tail = DEEP_CONFIGS[cfg]
    douts = _int_array([d for d, _ in tail])
    for aggr in ("+", "mean"):
        assert _lib.load().ngpde_edge_mlp_backward_supported(g.ptr, h1, len(tail), douts, _lib.AGGR[aggr]) == 1
        for e_term in (False, True):
            pr = Problem(g, h1, act1, tail, aggr, seed=H + len(tail) + len(aggr) + e_term, e_term=e_term, bias=not (e_term and aggr == "+"))
            what = f"{cfg} {geom} aggr={aggr} e_term={e_term}"
            gr = pr.backward(with_de=True)
            pr.check_backward(gr, what=what)
            assert same(gr, pr.backward(with_de=True)), what


# ---- 5. edges per tile, row degrees, tile counts ----------------------------------------------------------------------------------

TILE_EDGES = (0, 63, 64, 65, 127, 128, 129, 1024)
ROW_DEGREES = (0, 1, 15, 16, 17, 31, 32)


def edges_graph(foreign):
    """tile k < 8 has TILE_EDGES[k] edges (64-edge chunks of edge_mlp64 / the deep pullback, 128-edge chunks of the general kernels,
    an empty tile), tile 8 has rows of every degree in ROW_DEGREES (a lane holds entries q and q + 16), the rest are random"""
    def spec(k, rows, rng):
        if k < len(TILE_EDGES):
            T = TILE_EDGES[k]
            return min(foreign, T), spread(T, rows, rng)
        if k == len(TILE_EDGES):
            d = np.array([ROW_DEGREES[i % len(ROW_DEGREES)] for i in range(rows)])
            return foreign, rng.permutation(d)
        F = int(rng.integers(0, foreign + 1))
        return F, random_degrees(rows, rng, F)

    def make():
        n = 14 * ROWS - 9
        s, t, order = tiled_graph(n, spec, seed=77 + foreign)
        g = TileGraph(s, t, n, order)
        assert list(g.tile_edges[:len(TILE_EDGES)]) == list(TILE_EDGES)
        tile = g.order[len(TILE_EDGES) * ROWS:(len(TILE_EDGES) + 1) * ROWS]
        assert sorted(set(g.deg.numpy()[tile].tolist())) == sorted(ROW_DEGREES)
        assert g.max_halo == ROWS + foreign and g.max_deg == SLOT_WIDTH
        return g
    return graph(("edges", foreign), make)


def tiles_graph(n_tiles):
    """n_tiles tiles, the last one ragged, a tile without edges, halos up to 62 rows"""
    def spec(k, rows, rng):
        if k == n_tiles // 2 and n_tiles > 2:
            return 0, np.zeros(rows, dtype=np.int64)
        F = 0 if n_tiles == 1 else 30 if k % 7 == 0 else int(rng.integers(0, 31))
        return F, random_degrees(rows, rng, F, hi=6)

    def make():
        n = n_tiles * ROWS - (ROWS - 3 if n_tiles > 1 else 11)
        s, t, order = tiled_graph(n, spec, seed=n_tiles)
        g = TileGraph(s, t, n, order)
        assert g.n_tiles == n_tiles and g.n % ROWS != 0 and g.max_halo == (62 if n_tiles > 1 else ROWS) and g.fits()
        return g
    return graph(("tiles", n_tiles), make)


def all_forms(g, monkeypatch, what, seed):
    """every kernel family on one graph: edge_mlp64 (both pullback forms), the general forward at n_tail 0..3 and pullback at 0 / 1
    (+ and *), the deep pullback at 2 / 3"""
    check_edge64(Problem(g, 64, "swish", [(64, "identity")], "mean", seed=seed), monkeypatch, what)
    for h1, act1, tail in FWD_CONFIGS.values():
        for aggr in ("+", "max"):
            pr = Problem(g, h1, act1, tail, aggr, seed=seed + h1, e_term=len(tail) % 2 == 1)
            out, saves = pr.forward(save=len(tail) == 2)
            pr.check_forward(out, saves, what=f"{what} forward n_tail={len(tail)} aggr={aggr}")
    for h1, act1, tail in PULLBACK_CONFIGS.values():
        for aggr in ("mean", "*"):
            pr = Problem(g, h1, act1, tail, aggr, seed=seed + 5, scale=0.5 if aggr == "*" else 1.0)
            pr.check_backward(pr.backward(), what=f"{what} pullback n_tail={len(tail)} aggr={aggr}")
    for h1, act1, tail in DEEP_CONFIGS.values():
        pr = Problem(g, h1, act1, tail, "+", seed=seed + 9, e_term=True)
        pr.check_backward(pr.backward(), what=f"{what} deep pullback n_tail={len(tail)}")


@pytest.mark.parametrize("foreign", [16, 64])
def test_edges_per_tile_and_row_degrees(foreign, monkeypatch):
    # chunk boundaries and the empty tile at a DQ halo (48) and at the cap (96)
    clear_switches(monkeypatch)
    g = edges_graph(foreign)
    assert_regime(g, ROWS + foreign, ROWS + foreign)
    all_forms(g, monkeypatch, f"edges/tile halo={g.max_halo}", seed=foreign)


@pytest.mark.parametrize("n_tiles", [1, 7, 9, 257, 513, 1100])
def test_tile_counts(n_tiles, monkeypatch):
    # from a single (ragged) tile to more tiles than 2 workgroups per CU cover: the per-XCD ranges split unevenly and beyond 256 / 512
    # tiles the 32- / 64-per-XCD grids walk several tiles per workgroup
    clear_switches(monkeypatch)
    g = tiles_graph(n_tiles)
    assert_regime(g, g.max_halo, g.max_halo)
    all_forms(g, monkeypatch, f"tiles={n_tiles}", seed=n_tiles)


# ---- 6. the queries' answers, pinned to the build before csrc/edge_mlp_forms.h ----------------------------------------------------

FORMS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edge_mlp_forms.json")
QUERY_HALOS = sorted({ROWS, DQ_MAX_HALO, DQ_MAX_HALO + 1, HALO_CAP} | {b + k for b in S.TWO_PER_CU_BOUNDS for k in (0, 1)})
QUERY_CONFIGS = {"e64 swish-identity": (64, "swish", [(64, "identity")]), "e64 relu-relu": (64, "relu", [(64, "relu")]),
                 "64-64 gelu-gelu": (64, "gelu", [(64, "gelu")])}
QUERY_CONFIGS.update({f"fwd {k}": v for k, v in FWD_CONFIGS.items()})
QUERY_CONFIGS.update({f"pullback {k}": v for k, v in PULLBACK_CONFIGS.items()})
QUERY_CONFIGS.update({f"deep {k}": v for k, v in DEEP_CONFIGS.items()})
QUERY_SETTINGS = [None] + [(name, "1") for name in SWITCHES if name != S.DEEP_EDGE_BWD] + [(S.DEEP_EDGE_BWD, "0"), (S.DEEP_EDGE_BWD, "1")]
SWITCHED_GRAPHS = (f"halo{DQ_MAX_HALO}", f"halo{E64_FULL_GRID_MAX_HALO + 1}")          # each switch alone, on these two


def query_graphs():
    gs = {f"halo{H}": halo_graph(H) for H in QUERY_HALOS}
    gs["halo97"] = refused_graph("halo 97")
    gs[f"tiles{MULTI_TILE}"] = halo_graph(DQ_MAX_HALO, n_tiles=MULTI_TILE, ragged=3)
    return gs


def layer_descriptor(kind, aggr, h1, act1, tail, x, ef, wt):
    """ExplicitEdgeConv on one 8-wide state block, or MPPDEConv with 3 edge features and a one-layer update; the size query reads
    the widths and tests the pointers for NULL"""
    d = _lib.EdgeLayer()
    d.kind, d.aggr, d.n_state = kind, _lib.AGGR[aggr], 1
    d.state[0], d.state_width[0] = x.data_ptr(), 8
    dims = [16, h1] + [w for w, _ in tail]
    if kind == _lib.LAYER_MPPDE:
        d.edge_feat, d.edge_feat_width = ef.data_ptr(), 3
        dims[0] += 3
        d.update.n_layers = 1
        d.update.dims[0], d.update.dims[1] = 8 + dims[-1], 8
        d.update.weight[0] = wt.data_ptr()
    d.phi.n_layers = len(dims) - 1
    for l, w in enumerate(dims):
        d.phi.dims[l] = w
    for l, a in enumerate([act1] + [a for _, a in tail]):
        d.phi.act[l] = _lib.ACT[a]
        d.phi.weight[l] = wt.data_ptr()
    return d


def query_answers(monkeypatch):
    """[graph, switch setting, configuration, answers] of the five queries (ngpde_edge_layer_workspace_bytes for two layer kinds, two
    aggregations, inference and training), as the library answers now"""
    lib = _lib.load()
    wt = torch.zeros(4096, device=DEV)
    rows = []
    for gname, g in query_graphs().items():
        x, ef = torch.zeros(g.n, 8, device=DEV), torch.zeros(max(g.E, 1), 3, device=DEV)
        for setting in QUERY_SETTINGS if gname in SWITCHED_GRAPHS else QUERY_SETTINGS[:1]:
            clear_switches(monkeypatch)
            if setting:
                monkeypatch.setenv(*setting)
            for cname, (h1, act1, tail) in QUERY_CONFIGS.items():
                n_tail = len(tail)
                douts = _int_array([w for w, _ in tail]) if tail else None
                acts = _int_array([_lib.ACT[a] for _, a in tail]) if tail else None
                ans = {"supported": int(lib.ngpde_edge_mlp_supported(g.ptr, h1, n_tail, douts)),
                       "backward_supported": [int(lib.ngpde_edge_mlp_backward_supported(g.ptr, h1, n_tail, douts, _lib.AGGR[a])) for a in AGGRS],
                       "needs_edge_buffer": [int(lib.ngpde_edge_mlp_backward_needs_edge_buffer(g.ptr, h1, _lib.ACT[act1], e, n_tail, douts, acts,
                                                                                                _lib.AGGR[a])) for e in (0, 1) for a in ("+", "max")],
                       "backward_workspace_bytes": int(lib.ngpde_edge_mlp_backward_workspace_bytes(g.ptr, h1, n_tail, douts)),
                       "layer_workspace_bytes": [int(lib.ngpde_edge_layer_workspace_bytes(
                           g.ptr, C.byref(layer_descriptor(kind, a, h1, act1, tail, x, ef, wt)), training))
                           for kind in (_lib.LAYER_EDGECONV, _lib.LAYER_MPPDE) for a in ("+", "max") for training in (0, 1)]}
                rows.append([gname, "=".join(setting) if setting else "", cname, ans])
    clear_switches(monkeypatch)
    return rows


def test_queries_answer_what_the_build_before_the_forms_header_answered(monkeypatch):
    # which kernel runs never shows in a float64 comparison; what the ABI queries say about it does.  tests/golden/edge_mlp_forms.json
    # holds their answers from the library as it was before the choices moved into csrc/edge_mlp_forms.h (the field "recorded_from"
    # names the commit), on graphs at every halo threshold, one beyond the cap and one of 513 tiles, each switch alone.  No kernel of
    # the family is launched here.
    want = json.load(open(FORMS_GOLDEN))
    got = query_answers(monkeypatch)
    assert len(got) == len(want["rows"]) and {r[1] for r in got} == {""} | {"=".join(s) for s in QUERY_SETTINGS[1:]}
    wrong = [(g, w) for g, w in zip(got, want["rows"]) if g != w]
    assert not wrong, f"{len(wrong)} of {len(got)} rows differ (now, recorded): {wrong[:4]}"
