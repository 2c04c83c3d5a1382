"""The GCNConv kernels against float64 across gathers, widths and tiles.

ngpde_gcn_forward / ngpde_gcn_backward / ngpde_gcn_backward_ew run one of two families, chosen by the widths (csrc/gcn_forms.h:
gcn_layer_form; this file takes its thresholds from the restatement tests/gcn_gat_forms_spec.py, which tests/test_gcn_gat_forms_host.py
holds to the header):
  A. the fused layer (csrc/gcn_fused.hip), din = dout = D in {16, 32, 64, 128} (fused_supported).  A workgroup owns one run of 32
     positions of the handle's node order (a tile); the forward walks the by-target lists, the pullback's aggregation the by-source
     lists.  Each direction picks its gather on its own:
       forward  (gcn_fused_fwd_form)  LDS-staged rows, gcn_fused_fwd_kernel<D, ACT, HALO=true>, iff every by-target tile fits and
                                    NGPDE_NO_HALO is not 1; else the per-row gather <D, ACT, false>.
       backward (gcn_fused_bwd_form)  the dense launch (AGG = false: dz, dW / db slabs, G = dz W^T) never gathers; the dx launch
                                    (AGG = true) stages rows iff every by-source tile fits and NGPDE_NO_HALO is not 1, else the per-row
                                    gather.  D <= 64 (fused_bwd_pairs): one 1024-thread workgroup per pair of tiles (2 b, 2 b + 1);
                                    an odd tile count's last pair repeats the last tile with every row masked out.
                                    D = 128: one tile each.
     A tile fits the halo iff every row has at most 32 entries (kSlotWidth) and its 32 rows plus its distinct foreign rows are at
     most 96 (kHaloCap); halo_ok means every tile of that direction fits (graph_device.hip: all_fit_kernel).
     ACT: RELU and IDENTITY are compiled in, the other seven take the runtime switch (ACT = -1, gcn_act_class).
     Per-row gather: the first 16 entries of a row come from the position-indexed block when D / 4 <= 16 (Geo::ELL: D <= 64), the
     rest from the CSR list (gcn_tile.h).  coop_long_rows (gcn_fused.hip): the rows of a tile (a pair half)
     with more than kCoopDeg = 48 entries, if there are at most kCoopRows = 4 of them, are walked one at a time by
     min(32, 512 / (D / 4)) lane groups (16 at D = 128); with 5 or more the plain walk serves the whole tile.  In a pair both
     halves run n = max(mine, other) rounds, the idle half with row -1.
     The slabs (fused_num_slabs: ceil(tiles / 2) for D <= 64, tiles for D = 128) are summed by reduce_slabs_kernel:
     16 parts per element, four slabs per step while b + 48 < n_slabs, then one at a time; ct = D / 16 re-lays dW out
     row-major.  Blocks are mapped to tiles by xcd_tile (gcn_tile.h: contiguous runs per XCD, the remainder over the first
     tile-count % 8 XCDs).
  B. the any-width path (csrc/gcn_generic.hip + dense_mfma.hip) for every other (din, dout):
       dout >= din   aggregate first: spmm_generic_kernel<DP> (DP = 8 / 16 / 32 / 64 for d <= 8 / 16 / 32 / above, gcn_spmm_dp;
                     rows walked in batches of 64 entries, the next batch loaded while `base + 64 < re`), then the Dense forward;
                     save_agg written.
       dout < din    multiply first: split-K Dense forward (dense_fwd_splits parts, summed by sum_partials),
                     then spmm_gcn_tail (aggregation + bias + activation in one launch); save_agg is left untouched.  The
                     pullback's bias gradient is launch_colsum2: two stages iff N > 4 * kColsumChunks = 512 (colsum_two_stage).
  C. the gradient w.r.t. the edge_weight argument (ngpde_gcn_backward_ew): gcn_ew_node_term_kernel + gcn_ew_edge_kernel after
     either family's pullback; with dx = NULL the degree term's input gradient goes to the workspace's scratch (gcn_bwd_layout).

Every case builds its handle with ngpde_graph_create_device and an explicit node order, sets the normalisation it names
(ngpde_graph_set_gcn_norm_device: self loops, edge weights, weighted or unweighted degree), asserts its regime first -- the
library's halo_ok in both directions against the host geometry, the tile count, the slab count, and the rows above kCoopDeg of
every tile -- and compares every output with oracle.ngpde_oracle.gcn_conv / gcn_conv_backward in float64 (tied to the reference by
test_oracle.py and the golden vectors).  Outputs and workspaces start as NaN with guard words behind them that must come back
intact; no GCN kernel sums with atomics, so a second call must give the same bits.

A relu / leakyrelu / elu pre-activation whose float64 value lies within 1e-5 * max|z| of 0 may take the other branch in float32;
the cotangent dy is zeroed at such entries, so the branch cannot move the gradients.  Tolerances are the suite's: forward
1e-4 * max|ref| + 1e-5, gradients (dedge_weight included) 5e-4 relative; section E uses those of the node tests in test_gcn_gpu.py.
NGPDE_NO_HALO is read once per process: cases that claim a staged direction skip when it is set.
"""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from ngpde_amd import synth as S
from oracle import ngpde_oracle as O
from test_mp_gpu import close
from test_edge_mlp_forms_gpu import HALO_CAP, ROWS, SLOT_WIDTH, TileGraph, _release_graphs, graph  # noqa: F401
from test_gat_forms_gpu import both_ways
from test_gno_forms_gpu import hexbits
import gcn_gat_forms_spec as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED = F.FUSED
COOP_DEG, COOP_ROWS = 48, 4                    # kernel-internal (gcn_fused.hip: kCoopDeg, kCoopRows)
COLSUM_TWO_STAGE = F.COLSUM_TWO_STAGE          # colsum_two_stage: two stages above this many rows
KINKED = ("relu", "leakyrelu", "elu")
OTHER_ACTS = ("tanh", "sigmoid", "swish", "gelu", "leakyrelu", "elu", "softplus")
NO_HALO = os.environ.get("NGPDE_NO_HALO", "")[:1] == "1"
GUARD = 64                                     # guard floats behind every output
SENTINEL = -1234.5
WS_GUARD = 256                                 # guard bytes behind every workspace


# ---- graphs of chosen geometry ----------------------------------------------------------------------------------------------------

def layout(n_tiles, ragged, seed, in_hubs=(), out_hubs=(), foreign=3, hi=4, dup=0, self_edges=0):
    """COO lists + node order.  Positions (of the order) in in_hubs {pos: degree} get exactly that in-degree, from distinct sources
    anywhere; positions in out_hubs exactly that out-degree.  Every other position ("plain") takes 1 .. hi-1 in-edges from plain rows
    of its own tile plus `foreign` edges per tile from plain rows elsewhere; hub edges only meet plain rows, so the hubs' degrees are
    exact.  dup: that many edges repeated; self_edges: that many explicit s == t edges on plain rows."""
    rng = np.random.default_rng(seed)
    n = n_tiles * ROWS - ragged
    in_hubs, out_hubs = dict(in_hubs), dict(out_hubs)
    special = set(in_hubs) | set(out_hubs)
    plain = np.array([p for p in range(n) if p not in special], dtype=np.int64)
    S_, T_ = [], []
    for k in range(n_tiles):
        lo, hi_ = k * ROWS, min(n, (k + 1) * ROWS)
        local = plain[(plain >= lo) & (plain < hi_)]
        rows = [p for p in range(lo, hi_) if p not in in_hubs]
        for p in rows:
            cand = local[local != p]
            d = min(int(rng.integers(1, hi)), cand.size)
            S_.append(rng.choice(cand, d, replace=False))
            T_.append(np.full(d, p))
        others = plain[(plain < lo) | (plain >= hi_)]
        if others.size and rows:
            S_.append(rng.choice(others, foreign))
            T_.append(rng.choice(np.asarray(rows), foreign))
    base = sum(a.size for a in S_)
    for p, D in in_hubs.items():
        S_.append(rng.choice(plain[plain != p], D, replace=False))
        T_.append(np.full(D, p))
    for p, D in out_hubs.items():
        S_.append(np.full(D, p))
        T_.append(rng.choice(plain[plain != p], D, replace=False))
    s_pos, t_pos = np.concatenate(S_).astype(np.int64), np.concatenate(T_).astype(np.int64)
    if dup:
        k = rng.choice(base, dup, replace=False)
        s_pos, t_pos = np.concatenate([s_pos, s_pos[k]]), np.concatenate([t_pos, t_pos[k]])
    if self_edges:
        p = rng.choice(plain, self_edges, replace=False)
        s_pos, t_pos = np.concatenate([s_pos, p]), np.concatenate([t_pos, p])
    order = rng.permutation(n).astype(np.int32)
    perm = rng.permutation(s_pos.size)
    return order[s_pos][perm].astype(np.int64), order[t_pos][perm].astype(np.int64), order


class GcnGraph(TileGraph):
    """TileGraph with the GCN normalisation a case names: self loops or not, edge weights w with the weighted degree
    (wmode "degree": the edge_weight argument) or with the unweighted one (wmode "quirk": use_edge_weight=true)"""

    def __init__(self, s, t, n, order, loops=True, wmode=None, seed=0):
        super().__init__(s, t, n, order)
        self.loops, self.wmode = loops, wmode
        self.w = (np.random.default_rng(seed).random(self.E) + 0.5).astype(np.float32) if wmode else None
        wd = torch.as_tensor(self.w, device=DEV) if wmode else None
        _lib.check(_lib.load().ngpde_graph_set_gcn_norm_device(self.ptr, int(loops), _lib.ptr(wd), int(wmode == "degree"),
                                                               _lib.current_stream()))
        torch.cuda.synchronize()
        ht, di, hs, do, _ = both_ways(self)
        self.fits_t = ht <= HALO_CAP and di <= SLOT_WIDTH
        self.fits_s = hs <= HALO_CAP and do <= SLOT_WIDTH

    def long_rows(self, direction):
        """rows above kCoopDeg entries in every tile (by target: in-degree; by source: out-degree)"""
        deg = np.bincount(self.t if direction == 0 else self.s, minlength=self.n)
        at = np.zeros(self.n_tiles * ROWS, dtype=np.int64)
        at[:self.n] = deg[self.order]
        return (at > COOP_DEG).reshape(self.n_tiles, ROWS).sum(1)

    def oracle(self):
        return O.Graph(self.s, self.t, num_nodes=self.n, index_base=0,
                       edge_weight=self.w.astype(np.float64) if self.wmode == "quirk" else None)


def halo_ok(g, direction):
    p, b = C.c_void_p(), C.c_size_t()
    _lib.check(_lib.load().ngpde_graph_array(g.ptr, direction, 13, C.byref(p), C.byref(b)))   # NGPDE_GRAPH_HALO_OK
    return bool(b.value)


def n_slabs(g, d):
    return F.n_slabs(g.n, d)


def assert_regime(g, fwd, bwd, tiles=None):
    """fwd / bwd: "staged" or "row" -- what each direction's gather must be; the library's halo_ok against the host geometry"""
    for direction, want, fits in ((0, fwd, g.fits_t), (1, bwd, g.fits_s)):
        assert halo_ok(g, direction) == fits, (direction, fits)
        assert fits == (want == "staged"), (direction, want, both_ways(g))
    if tiles is not None:
        assert g.n_tiles == tiles
    if NO_HALO and "staged" in (fwd, bwd):
        pytest.skip("NGPDE_NO_HALO=1: no LDS-staged gather in this process")


# the hub layout: (tile, row) -> degree.  By target: 1, 4 and 5 long rows in tiles 1, 3, 5; the ELL width 16 / 17, the slot width
# 32 / 33, 48 (not long) / 49 and 700; the any-width path's 64-entry batches 64 / 65 / 128 / 129.  By source: pairs (14, 15) with
# long rows in the first half only, (16, 17) in both with 2 and 4, (18, 19) with 5 (plain walk) against 1, (20, 21) in the second
# half only; the same single degrees; the odd last pair (tile 38) with one.
HUB_TILES, HUB_RAGGED = 39, 7
IN_HUBS = {(1, 5): 49, (3, 0): 49, (3, 9): 64, (3, 17): 100, (3, 30): 300, (5, 1): 49, (5, 7): 50, (5, 13): 51, (5, 20): 52,
           (5, 31): 200, (7, 4): 16, (8, 4): 17, (9, 4): 32, (10, 4): 33, (11, 4): 48, (12, 4): 700, (28, 6): 64, (29, 6): 65,
           (30, 6): 128, (31, 6): 129}
OUT_HUBS = {(14, 3): 49, (16, 2): 60, (16, 22): 49, (17, 0): 49, (17, 8): 70, (17, 15): 120, (17, 29): 250, (18, 1): 49, (18, 5): 53,
            (18, 9): 57, (18, 20): 61, (18, 27): 300, (19, 4): 80, (21, 10): 400, (22, 4): 16, (23, 4): 17, (24, 4): 32, (25, 4): 33,
            (26, 4): 48, (27, 4): 700, (32, 6): 64, (33, 6): 65, (34, 6): 128, (35, 6): 129, (38, 2): 65}
LONG_T = {1: 1, 3: 4, 5: 5, 12: 1, 28: 1, 29: 1, 30: 1, 31: 1}
LONG_S = {14: 1, 16: 2, 17: 4, 18: 5, 19: 1, 21: 1, 27: 1, 32: 1, 33: 1, 34: 1, 35: 1, 38: 1}
REGIMES = {"SS": ("staged", "staged"), "RS": ("row", "staged"), "SR": ("staged", "row"), "RR": ("row", "row")}


def build_hub_graph(kind="RR", loops=True, wmode=None, extra=False):
    """kind: which directions carry hubs (R = per-row gather); extra: repeated edges and explicit self-loop edges"""
    def make():
        pos = lambda hubs: {k * ROWS + r: d for (k, r), d in hubs.items()}
        s, t, order = layout(HUB_TILES, HUB_RAGGED, 4242 + extra, pos(IN_HUBS) if kind[0] == "R" else {},
                             pos(OUT_HUBS) if kind[1] == "R" else {}, dup=60 if extra else 0, self_edges=25 if extra else 0)
        g = GcnGraph(s, t, HUB_TILES * ROWS - HUB_RAGGED, order, loops, wmode, seed=7)
        lt, ls = g.long_rows(0), g.long_rows(1)
        assert {k: int(v) for k, v in enumerate(lt) if v} == (LONG_T if kind[0] == "R" else {})
        assert {k: int(v) for k, v in enumerate(ls) if v} == (LONG_S if kind[1] == "R" else {})
        if extra:
            assert (g.s == g.t).sum() == 25 and np.unique(np.stack([g.s, g.t]), axis=1).shape[1] < g.E - 25
        return g
    return graph(("gcn hub", kind, loops, wmode, extra), make)


def hub_graph(kind="RR", loops=True, wmode=None, extra=False):
    g = build_hub_graph(kind, loops, wmode, extra)
    assert_regime(g, *REGIMES[kind], tiles=HUB_TILES)
    return g


def build_tiles_graph(n_tiles, hubs):
    """n_tiles tiles (the last one ragged); hubs: one long row each way (per-row gather in both directions, coop)"""
    def make():
        ragged = 5 if n_tiles > 1 else 3
        n = n_tiles * ROWS - ragged
        mid, deg = (n_tiles // 2) * ROWS, min(60, n - 3)
        s, t, order = layout(n_tiles, ragged, 100 + n_tiles, {mid + 1: deg} if hubs else {},
                             {(n_tiles - 1) * ROWS: deg} if hubs else {}, foreign=3 if n_tiles > 1 else 0)
        return GcnGraph(s, t, n, order)
    return graph(("gcn tiles", n_tiles, hubs), make)


def tiles_graph(n_tiles, hubs):
    g = build_tiles_graph(n_tiles, hubs)
    assert_regime(g, *(("row", "row") if hubs else ("staged", "staged")), tiles=n_tiles)
    if hubs:
        assert g.long_rows(0).sum() == 1 and g.long_rows(1).sum() == 1
    return g


# ---- buffers with guards ----------------------------------------------------------------------------------------------------------

class Out:
    """NaN-filled device output of `shape` with GUARD sentinel floats behind it"""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.full = torch.full((n + GUARD,), math.nan, device=DEV)
        self.full[n:] = SENTINEL
        self.n, self.v = n, self.full[:n].view(*shape)

    def intact(self):
        return bool((self.full[self.n:] == SENTINEL).all())


class Ws:
    """workspace of exactly `nbytes` (NaN words) with WS_GUARD canary bytes behind it"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.full = torch.full((self.nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.full[self.nbytes:] = 0xA5

    def intact(self):
        return bool((self.full[self.nbytes:] == 0xA5).all())


# ---- one layer through the C ABI against the oracle -------------------------------------------------------------------------------

class Layer:
    def __init__(self, g, din, dout, act, seed, bias=True):
        rng = np.random.default_rng(seed)
        self.g, self.din, self.dout, self.act = g, din, dout, act
        self.x = rng.normal(size=(g.n, din)).astype(np.float32)
        self.wt = (rng.normal(size=(din, dout)) * 1.5 / np.sqrt(din)).astype(np.float32)   # [din][dout] = W^T
        self.b = (0.3 * rng.normal(size=dout)).astype(np.float32) if bias else None
        self.dy = rng.normal(size=(g.n, dout)).astype(np.float32)
        ew = g.w.astype(np.float64) if g.wmode == "degree" else None
        y, cache = O.gcn_conv(self.x.T.astype(np.float64), self.wt.T.astype(np.float64),
                              None if self.b is None else self.b.astype(np.float64), g.oracle(), act, g.loops, g.wmode == "quirk",
                              edge_weight=ew)
        z = cache["z"]
        if act in KINKED:                      # no float32 branch flip can move the gradients
            near = np.abs(z) < 1e-5 * np.abs(z).max()
            self.dy[near.T] = 0.0
        self.ref_y, self.ref_z, self.ref_agg = y.T, z.T, cache["x3"].T
        go = O.gcn_conv_backward(cache, self.dy.T.astype(np.float64))
        self.ref = dict(dx=go["x"].T, dw=go["weight"].T, db=go["bias"].reshape(-1) if bias else None, dew=go.get("edge_weight"))
        dv = lambda a: None if a is None else torch.as_tensor(a, device=DEV)
        self.d = dict(x=dv(self.x), wt=dv(self.wt), b=dv(self.b), dy=dv(self.dy))

    def forward(self):
        lib, g, d = _lib.load(), self.g, self.d
        y, agg, z = Out(g.n, self.dout), Out(g.n, self.din), Out(g.n, self.dout)
        ws = Ws(lib.ngpde_gcn_workspace_bytes(g.ptr, self.din, self.dout, 0))
        _lib.check(lib.ngpde_gcn_forward(g.ptr, self.din, self.dout, _lib.ACT[self.act], _lib.ptr(d["x"]), _lib.ptr(d["wt"]),
                                         _lib.ptr(d["b"]), _lib.ptr(y.v), _lib.ptr(agg.v), _lib.ptr(z.v), _lib.ptr(ws.full), ws.nbytes,
                                         _lib.current_stream()))
        torch.cuda.synchronize()
        assert y.intact() and agg.intact() and z.intact() and ws.intact(), "forward wrote past an output or its workspace"
        return y.v, agg.v, z.v

    def backward(self, z, agg, with_dx=True, with_db=True, ew=False):
        lib, g, d = _lib.load(), self.g, self.d
        dx, dw, db, dew = Out(g.n, self.din), Out(self.din, self.dout), Out(self.dout), Out(max(g.E, 1))
        if ew:
            ws = Ws(lib.ngpde_gcn_backward_ew_workspace_bytes(g.ptr, self.din, self.dout))
            st = lib.ngpde_gcn_backward_ew(g.ptr, self.din, self.dout, _lib.ACT[self.act], _lib.ptr(d["x"]), _lib.ptr(d["wt"]),
                                           _lib.ptr(d["b"]), _lib.ptr(z), _lib.ptr(agg), _lib.ptr(d["dy"]),
                                           _lib.ptr(dx.v) if with_dx else None, _lib.ptr(dw.v), _lib.ptr(db.v) if with_db else None,
                                           _lib.ptr(dew.v), _lib.ptr(ws.full), ws.nbytes, _lib.current_stream())
        else:
            ws = Ws(lib.ngpde_gcn_workspace_bytes(g.ptr, self.din, self.dout, 1))
            st = lib.ngpde_gcn_backward(g.ptr, self.din, self.dout, _lib.ACT[self.act], _lib.ptr(d["x"]), _lib.ptr(d["wt"]), _lib.ptr(z),
                                        _lib.ptr(agg), _lib.ptr(d["dy"]), _lib.ptr(dx.v) if with_dx else None, _lib.ptr(dw.v),
                                        _lib.ptr(db.v) if with_db else None, _lib.ptr(ws.full), ws.nbytes, _lib.current_stream())
        _lib.check(st)
        torch.cuda.synchronize()
        for name, o in (("dx", dx), ("dweight", dw), ("dbias", db), ("dedge_weight", dew)):
            assert o.intact(), f"backward wrote past {name}"
        assert ws.intact(), "backward wrote past its workspace"
        if not with_dx:
            assert bool(torch.isnan(dx.v).all())
        out = dict(dw=dw.v)
        if with_dx:
            out["dx"] = dx.v
        if with_db:
            out["db"] = db.v
        if ew:
            out["dew"] = dew.v[:g.E]
        return out

    def check(self, what, ew=False, dx_null=True, y_for_z=True):
        """forward (all three outputs, twice), backward (twice), the dx = NULL call, y in place of z (relu / identity), and with
        ew the edge-weight gradient with dx given and NULL"""
        what = f"{what} {self.din}->{self.dout} {self.act} bias={self.b is not None}"
        y, agg, z = self.forward()
        close(y, self.ref_y, what=f"y {what}")
        close(z, self.ref_z, what=f"save_z {what}")
        if self.dout >= self.din:
            close(agg, self.ref_agg, what=f"save_agg {what}")
        else:
            assert bool(torch.isnan(agg).all()), f"save_agg written although dout < din {what}"
        y2, agg2, z2 = self.forward()
        assert torch.equal(y, y2) and torch.equal(z, z2) and torch.equal(agg.nan_to_num(), agg2.nan_to_num()), f"forward repeat {what}"
        aggp = agg if self.dout >= self.din else None
        gr = self.backward(z, aggp, with_db=self.b is not None)
        for k, v in gr.items():
            close(v, self.ref[k], rtol=5e-4, atol=1e-5, what=f"{k} {what}")
        gr2 = self.backward(z, aggp, with_db=self.b is not None)
        assert all(torch.equal(gr[k], gr2[k]) for k in gr), f"backward repeat {what}"
        if dx_null:
            g0 = self.backward(z, aggp, with_dx=False, with_db=self.b is not None)
            assert all(torch.equal(gr[k], g0[k]) for k in g0), f"dx = NULL changed dweight / dbias {what}"
        if y_for_z and self.act in ("relu", "identity"):
            gy = self.backward(y, aggp, with_db=self.b is not None)
            assert all(torch.equal(gr[k], gy[k]) for k in gr), f"y in place of z {what}"
        if ew:
            ge = self.backward(z, aggp, with_db=self.b is not None, ew=True)
            for k, v in ge.items():
                close(v, self.ref[k], rtol=5e-4, atol=1e-5, what=f"ew {k} {what}")
            ge0 = self.backward(z, aggp, with_dx=False, with_db=self.b is not None, ew=True)
            assert torch.equal(ge["dew"], ge0["dew"]) and torch.equal(ge["dw"], ge0["dw"]), f"ew with dx = NULL {what}"
        return gr


# ---- A. the fused layer -----------------------------------------------------------------------------------------------------------

def test_hub_layout_regimes():
    # the builder against the library: each kind reaches the gathers it names, the long rows sit where the layout puts them, and the
    # pair halves carry (1, 0), (2, 4), (5 -> plain walk, 1), (0, 1) long rows; the odd last pair's second half is the masked repeat
    for kind in REGIMES:
        hub_graph(kind)
    g = hub_graph("RR")
    ls = g.long_rows(1)
    assert g.n_tiles % 2 == 1 and ls[-1] == 1
    halves = [(int(ls[2 * b]), int(ls[2 * b + 1])) for b in range(7, 11)]
    assert halves == [(1, 0), (2, 4), (5, 1), (0, 1)]
    assert COOP_ROWS == 4 and max(g.long_rows(0)) == 5
    for d in FUSED:
        assert n_slabs(g, d) == (20 if d <= 64 else 39)


@pytest.mark.parametrize("kind", list(REGIMES))
@pytest.mark.parametrize("act", ["relu", "identity", "tanh"])
@pytest.mark.parametrize("d", FUSED)
def test_fused_gathers(d, act, kind):
    # {staged, per-row} x {forward, backward} at every width and every activation instantiation (RELU, IDENTITY, -1); per-row
    # directions walk the hub rows: ELL width, slot width, coop with 1 / 4 / 5 rows per tile and pair halves
    g = hub_graph(kind)
    Layer(g, d, d, act, seed=d + len(act) + 31 * list(REGIMES).index(kind)).check(f"{kind}")


@pytest.mark.parametrize("d", FUSED)
def test_fused_every_generic_activation(d):
    # the runtime switch of ACT = -1 for the seven activations without a compiled-in path, staged forward + per-row pullback
    g = hub_graph("SR")
    for k, act in enumerate(OTHER_ACTS):
        Layer(g, d, d, act, seed=100 + d + k, bias=k % 2 == 0).check("SR", y_for_z=False)


VARIANTS = ("no bias", "no self loops", "weighted degree", "weighted messages", "repeated and self edges")


@pytest.mark.parametrize("kind", ["SS", "RR"])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("d", FUSED)
def test_fused_variants(d, variant, kind):
    # bias = NULL; add_self_loops = false (every row has an in-edge); the edge_weight argument (weighted degree; slot_w when staged,
    # w c in the entries when per-row); use_edge_weight (weighted messages, unweighted degree); multi-edges and s == t edges
    act = ("relu", "elu", "leakyrelu", "identity", "relu")[VARIANTS.index(variant)]
    g = hub_graph(kind, loops=variant != "no self loops",
                  wmode={"weighted degree": "degree", "weighted messages": "quirk"}.get(variant),
                  extra=variant == "repeated and self edges")
    if variant == "no self loops":
        assert np.bincount(g.t, minlength=g.n).min() > 0
    Layer(g, d, d, act, seed=7 * d + VARIANTS.index(variant), bias=variant != "no bias").check(f"{kind} {variant}")


TILE_COUNTS = (1, 2, 16, 17, 31, 33, 48, 49, 64, 65, 96, 97, 128, 129, 1033)


@pytest.mark.parametrize("n_tiles", TILE_COUNTS)
def test_fused_tile_and_slab_counts(n_tiles):
    # one tile, ragged last tiles, odd / even counts (the paired pullback's masked repeat), slab counts on both sides of every
    # reduce_slabs_kernel boundary (1, 16 / 17, 48 / 49, 64 / 65 and beyond), and 1033 tiles (> 512, not a multiple of 8); every
    # other count with a long row each way (per-row gather, coop)
    hubs = TILE_COUNTS.index(n_tiles) % 2 == 1
    g = tiles_graph(n_tiles, hubs)
    for k, d in enumerate(FUSED):
        ns = n_slabs(g, d)
        assert ns == (-(-n_tiles // 2) if d <= 64 else n_tiles)
        act = ("relu", "tanh", "identity", "swish")[(k + n_tiles) % 4]
        Layer(g, d, d, act, seed=n_tiles + d).check(f"tiles={n_tiles} slabs={ns}")


def test_slab_counts_cross_every_reduce_boundary():
    # the parametrisation above reaches slab counts 1, 16, 17, 48, 49, 64, 65 and more than 64 (four-way steps plus a tail)
    seen = {(-(-t // 2) if d <= 64 else t) for t in TILE_COUNTS for d in FUSED}
    assert {1, 16, 17, 48, 49, 64, 65} <= seen and max(seen) > 512


# ---- B. the any-width path --------------------------------------------------------------------------------------------------------

ANY_PAIRS = [(8, 12), (9, 12), (16, 20), (17, 20), (32, 40), (33, 40), (64, 70), (65, 70), (120, 130),     # aggregate first
             (12, 8), (12, 9), (20, 16), (24, 17), (40, 32), (40, 33), (70, 64), (80, 65), (150, 120),    # multiply first
             (16, 32), (32, 16), (64, 128), (128, 64), (48, 48)]


@pytest.mark.parametrize("kind", ["SS", "RR"])
@pytest.mark.parametrize("din,dout", ANY_PAIRS)
def test_any_width(din, dout, kind):
    # spmm_generic_kernel<8 / 16 / 32 / 64> on both sides of each width, both orders; RR has rows of 64 / 65 / 128 / 129 entries both
    # ways (the 64-entry batches) and 1241 rows (dout < din: two-stage column sum); save_agg untouched when dout < din
    g = hub_graph(kind)
    assert g.n > COLSUM_TWO_STAGE
    k = ANY_PAIRS.index((din, dout))
    act = ("relu", "tanh", "identity", "elu", "swish", "softplus")[k % 6]
    Layer(g, din, dout, act, seed=din * 3 + dout, bias=k % 4 != 3).check(f"any-width {kind}")


@pytest.mark.parametrize("din,dout", [(300, 20), (256, 33)])
def test_any_width_split_k_few_rows(din, dout):
    # din >= 256 on 91 rows: the multiply-first forward splits over the input features (partials summed by sum_partials), and the
    # bias gradient's column sum is one stage (N <= 512)
    g = tiles_graph(3, False)
    lib = _lib.load()
    one = (g.n * dout * 4 + 255) // 256 * 256 + 256
    assert lib.ngpde_gcn_workspace_bytes(g.ptr, din, dout, 0) > one        # more than one partial product
    assert g.n <= COLSUM_TWO_STAGE
    Layer(g, din, dout, "tanh", seed=din).check("split-K")


# ---- C. the edge-weight gradient ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["SS", "RR"])
@pytest.mark.parametrize("loops", [True, False])
@pytest.mark.parametrize("din,dout,bias", [(64, 64, True), (16, 16, False), (128, 128, True), (12, 20, True), (20, 12, False),
                                           (33, 40, True), (40, 33, True)])
def test_edge_weight_gradient(din, dout, bias, loops, kind):
    # ngpde_gcn_backward_ew after the fused and the any-width pullback, both orders, with and without self loops, bias = NULL with
    # dout < din, dx given and NULL (scratch in the workspace), widths not multiples of 16; workspace exactly the queried size
    g = hub_graph(kind, loops=loops, wmode="degree")
    act = "tanh" if din % 2 else "relu"
    Layer(g, din, dout, act, seed=din + dout + loops, bias=bias).check(f"ew {kind} loops={loops}", ew=True, y_for_z=False)


# ---- D. contracts -------------------------------------------------------------------------------------------------------------------

def handle_from_host(n, loops):
    """a handle of n nodes and no edges"""
    lib = _lib.load()
    out = C.c_void_p()
    _lib.check(lib.ngpde_graph_create(n, 0, None, None, 0, 1, C.byref(out)))
    _lib.check(lib.ngpde_graph_set_gcn_norm(out, int(loops), None, 0))
    return out


@pytest.mark.parametrize("din,dout", [(64, 64), (12, 20), (20, 12)])
def test_zero_nodes_give_zero_gradients(din, dout):
    lib = _lib.load()
    h = handle_from_host(0, True)
    try:
        dw, db = Out(din, dout), Out(dout)
        ws = Ws(lib.ngpde_gcn_workspace_bytes(h, din, dout, 1))
        _lib.check(lib.ngpde_gcn_backward(h, din, dout, _lib.ACT["relu"], None, None, None, None, None, None, _lib.ptr(dw.v),
                                          _lib.ptr(db.v), _lib.ptr(ws.full), ws.nbytes, _lib.current_stream()))
        torch.cuda.synchronize()
        assert bool((dw.v == 0).all()) and bool((db.v == 0).all()) and dw.intact() and db.intact() and ws.intact()
    finally:
        _lib.destroy_later("ngpde_graph_destroy", h)


class Edgeless:
    """n nodes, no edges, self loops: c = 1 and y = act(x W + b)"""

    def __init__(self, n):
        self.ptr, self.n, self.E, self.loops, self.wmode, self.w = handle_from_host(n, True), n, 0, True, None, None
        self.s = self.t = np.zeros(0, dtype=np.int64)

    def oracle(self):
        return O.Graph(self.s, self.t, num_nodes=self.n, index_base=0)


@pytest.mark.parametrize("din,dout", [(16, 16), (128, 128), (12, 20), (20, 12)])
def test_nodes_without_edges(din, dout):
    g = Edgeless(50)
    try:
        Layer(g, din, dout, "relu", seed=din + dout).check("no edges")
    finally:
        _lib.destroy_later("ngpde_graph_destroy", g.ptr)


# ---- E. the replayed plan on per-row graphs -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("d,tab,act,no_mask", [(16, "euler", "relu", False), (128, "euler", "relu", False), (16, "tsit5", "tanh", False),
                                               (128, "tsit5", "tanh", False), (64, "tsit5", "relu", True)])
def test_replayed_plan_on_per_row_graph(d, tab, act, no_mask, monkeypatch):
    # NeuralODE(Chain(GCNConv, GCNConv)) under NGPDE_NO_PERSISTENT=1 on the hub graph (no tile fits the halo in either direction):
    # the un-prescaled replayed plan, whose pullback launches combine the coop long rows, the dense part, the adjoint stage
    # combination and relu sign masks (or the z tape under tanh / NGPDE_NO_MASK=1)
    monkeypatch.setenv("NGPDE_NO_PERSISTENT", "1")
    if no_mask:
        monkeypatch.setenv("NGPDE_NO_MASK", "1")
    else:
        monkeypatch.delenv("NGPDE_NO_MASK", raising=False)
    hg = hub_graph("RR")
    N, nsteps, dt = hg.n, 3, 0.1
    g = ng.GNNGraph(hg.s, hg.t, num_nodes=N, index_base=0)
    og = O.Graph(hg.s, hg.t, num_nodes=N, index_base=0)
    rng = np.random.default_rng(d)
    params = [dict(weight=S.glorot_uniform(d + 10 + k, d, d), bias=rng.normal(size=(d, 1)) * 0.1) for k in range(2)]
    u0 = rng.normal(size=(d, N))
    rhs = ng.Chain(ng.GCNConv((d, d), act, initialgraph=g), ng.GCNConv((d, d), act, initialgraph=g))
    node = ng.NeuralODE(rhs, solver=tab, n_steps=nsteps, dt=dt)
    ps, st = ng.setup(0, node)
    for k, name in enumerate(["layer_1", "layer_2"]):
        ps[name]["weight"] = torch.as_tensor(params[k]["weight"].astype(np.float32))
        ps[name]["bias"] = torch.as_tensor(params[k]["bias"].astype(np.float32))
    ps = ng.to_device(ps, DEV)
    for lp in ps.values():
        for v in lp.values():
            v.requires_grad_(True)
    u = torch.as_tensor(u0.astype(np.float32), device=DEV).requires_grad_(True)
    uT, _ = node(u, ps, st)
    flags = node.plan_for(ps, st, True).flags()
    assert not ({"persistent_fwd", "persistent_bwd", "prescaled"} & flags), flags
    assert ("sign_masks" in flags) == (act == "relu" and not no_mask), flags
    uTo, du0o, acc = O.gcn2_node_loss_and_grads(params, og, u0, O.TABLEAUS[tab], dt, nsteps, act)
    close(uT, uTo, rtol=2e-4, what="u(T)")
    uT.sum().backward()
    close(u.grad, du0o, rtol=5e-4, atol=1e-4, what="du0")
    for k, name in enumerate(["layer_1", "layer_2"]):
        close(ps[name]["weight"].grad, acc[k]["weight"], rtol=5e-4, atol=1e-3, what=f"dW{k + 1}")
        close(ps[name]["bias"].grad, acc[k]["bias"], rtol=5e-4, atol=1e-3, what=f"db{k + 1}")


# ---- F. the queries' answers, pinned to the build before csrc/gcn_forms.h and csrc/gat_forms.h ----------------------------------------

FORMS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gcn_gat_forms.json")
QUERY_SETTINGS = [None] + [(name, "1") for name in F.SWITCHES]
AS_UNSWITCHED = "as unswitched"


def query_graphs():
    """name -> graph: the tile-count and hub graphs of sections A and B, built without their regime assertions (a process under
    NGPDE_NO_HALO=1 asks too)"""
    gs = {f"tiles={k} hubs={int(h)}": build_tiles_graph(k, h) for k in (1, 2, 3) for h in (False, True)}
    gs.update({f"hub {kind}": build_hub_graph(kind) for kind in REGIMES})
    assert (min(g.n for g in gs.values()), max(g.n for g in gs.values())) == (29, 1241)
    return gs


def setting_answers():
    """every query of the two families under the environment of the moment, per handle.  Yes / no answers as hexbits (the GNO file's
    encoding): gat_layer_supported one group per din over heads x head_widths(heads), node_gat_supported one group over the same
    at din = 64.  "geometry": what a size or an answer depends on, for the restatement on the CPU.  Sizes as lists: gcn_workspace_bytes [forward, backward, backward_ew] flattened over din x dout; gat_workspace_bytes
    over heads; gat_layer_workspace_bytes over heads (c does not enter)."""
    lib = _lib.load()
    hc = [(h, c) for h in F.HEADS for c in F.head_widths(h)]
    edgeless = Edgeless(50)
    handles = dict(query_graphs(), edgeless=edgeless)
    out = {}
    try:
        for name, g in handles.items():
            ptr = g.ptr
            out[name] = {
                "geometry": [g.n, g.E, int(halo_ok(g, 0)), int(halo_ok(g, 1))],   # nodes, edges, halo_ok by target / by source
                "gat_layer_supported": " ".join(hexbits(lib.ngpde_gat_layer_supported(ptr, din, h, c) for h, c in hc) for din in F.WIDTHS),
                "node_gat_supported": hexbits(lib.ngpde_node_gat_supported(ptr, F.GAT_WIDTH, h, c) for h, c in hc),
                "gcn_workspace_bytes": [int(v) for din in F.WIDTHS for dout in F.WIDTHS
                                        for v in (lib.ngpde_gcn_workspace_bytes(ptr, din, dout, 0), lib.ngpde_gcn_workspace_bytes(ptr, din, dout, 1),
                                                  lib.ngpde_gcn_backward_ew_workspace_bytes(ptr, din, dout))],
                "gat_workspace_bytes": [int(lib.ngpde_gat_workspace_bytes(ptr, h)) for h in F.HEADS],
                "gat_layer_workspace_bytes": [int(lib.ngpde_gat_layer_workspace_bytes(ptr, h, 64 // max(h, 1))) for h in F.HEADS]}
    finally:
        _lib.destroy_later("ngpde_graph_destroy", edgeless.ptr)
    return out


def query_answers(monkeypatch):
    """setting_answers() with no switch set and under each switch of the families alone; a setting the library latches once per process
    (NGPDE_NO_HALO) is asked of a fresh child process that loads the same library.  A handle's table that a switch leaves as it is
    without it says so instead of repeating it.  No kernel of the families is launched."""
    answers = {}
    for setting in QUERY_SETTINGS:
        for name in F.SWITCHES:
            monkeypatch.delenv(name, raising=False)
        if setting and setting[0] in F.LATCHED:
            tests = os.path.dirname(os.path.abspath(__file__))
            code = (f"import sys, json; sys.path[:0] = [{os.path.dirname(tests)!r}, {tests!r}]\n"
                    f"from ngpde_amd import _lib; _lib.LIB_PATH = {_lib.LIB_PATH!r}\n"
                    "import test_gcn_forms_gpu as T; print('ANSWERS ' + json.dumps(T.setting_answers()))")
            r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **{setting[0]: setting[1]}), capture_output=True, text=True, timeout=240)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
            got = json.loads([l for l in r.stdout.splitlines() if l.startswith("ANSWERS ")][-1][len("ANSWERS "):])
        else:
            if setting:
                monkeypatch.setenv(*setting)
            got = setting_answers()
        if setting:
            got = {h: {q: (AS_UNSWITCHED if table == answers[""][h][q] else table) for q, table in per.items()} for h, per in got.items()}
        answers["=".join(setting) if setting else ""] = got
    for name in F.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return {"queries": answers}


def test_queries_answer_what_the_build_before_the_forms_headers_answered(monkeypatch):
    # which kernel runs never shows in a float64 comparison; what the support queries and the workspace sizes say about it does.
    # tests/golden/gcn_gat_forms.json holds their answers from the library as it was before the choices moved into csrc/gcn_forms.h
    # and csrc/gat_forms.h (the field "recorded_from" names the commit; tools/record_forms.py --family gcn_gat wrote it).  Handles
    # are built and queries made; no kernel of the families is launched.
    want = json.load(open(FORMS_GOLDEN))["queries"]
    got = query_answers(monkeypatch)["queries"]
    assert set(got) == set(want) == {""} | {"=".join(s) for s in QUERY_SETTINGS[1:]}
    for setting, per in got.items():
        assert set(per) == set(want[setting]) and len(per) == 11
        for handle, tables in per.items():
            wrong = [q for q, table in tables.items() if table != want[setting][handle].get(q)]
            assert not wrong and set(tables) == set(want[setting][handle]), (setting or "unswitched", handle, wrong)
    # the answers are the restatement's too (the host test holds the headers to it; this holds the entries to the headers)
    for handle, tables in got[""].items():
        sizes = tables["gcn_workspace_bytes"]
        assert len(sizes) == 3 * len(F.WIDTHS) ** 2 and all(0 < f and 0 < b <= e for f, b, e in zip(sizes[0::3], sizes[1::3], sizes[2::3])), handle
    # the switches act where they are meant to: the layer's on both support queries, the solver's on its own, the others on none
    changed = {setting: {q for tables in per.values() for q, table in tables.items() if table != AS_UNSWITCHED} for setting, per in got.items() if setting}
    assert changed == {"NGPDE_NO_HALO=1": set(), "NGPDE_NO_FUSED_GAT=1": set(), "NGPDE_NO_FUSED_GAT_LAYER=1": {"gat_layer_supported", "node_gat_supported"},
                       "NGPDE_NO_PERSISTENT=1": {"node_gat_supported"}}
    fits = {h for h, tables in got[""].items() if int(tables["gat_layer_supported"].replace(" ", ""), 16)}
    assert fits == {name for name, g in query_graphs().items() if g.fits_t and g.fits_s} >= {"tiles=3 hubs=0", "hub SS"}   # staged both ways, with edges
    assert fits.isdisjoint({"edgeless", "hub RS", "hub SR", "hub RR", "tiles=3 hubs=1"})
