"""The GAT-style kernels against float64 across heads, widths and tiles.

Three families, each of which picks its layout and grid from the shape and the graph:
  A. the one-launch layer (csrc/gat_fused.hip: gat_layer_fwd_kernel<H>, gat_layer_bwd_target_kernel<H>,
     gat_layer_bwd_source_kernel<H> with kSrcTiles = 2 tiles per workgroup, gat_layer_reduce_kernel over the slabs) at heads 1 / 2 / 4,
     din = heads * c = 64.  It needs every tile to fit kHaloCap = 96 staged rows and kSlotWidth = 32 entries per row in BOTH
     directions (by target: in-degree and foreign sources; by source: out-degree and foreign targets) and at least one edge.
  B. the aggregation primitives ngpde_gat_forward / ngpde_gat_backward (csrc/gat_forms.h gat_fwd_form / gat_bwd_form decide,
     csrc/mp_kernels.hip launches): the tiled forward (gat_fused_fwd_kernel) when heads * c = 64, heads in {1, 2, 4} and the by-target tiles fit;
     the blocked forward <H> when H is a power of two <= 16 and heads * c <= 256 (rows of more than 64 / H edges take several
     blocks); the blocked pullback <H> when in addition c % 4 == 0 and wx, dout are 16-byte aligned; the row-per-wave kernels
     (lanes stride rows in steps of 64 edges) otherwise.
  C. the device-resident solver (gat_node_{fwd,bwd}_persistent[_batch]_kernel<H>) at the caps.

Every case builds its handle with ngpde_graph_create_device and an explicit node order (tiles = consecutive 32-node runs of it), asserts
its regime first -- both directions' halos and degrees, the tile count, and that the library's support query (or, for the primitives,
the restatement of gat_fwd_form's / gat_bwd_form's conditions in tests/gcn_gat_forms_spec.py, which tests/test_gcn_gat_forms_host.py
holds to the header) agrees -- and then compares every output with a float64
restatement in torch on the CPU: logits leakyrelu(a_l . Wx_t + a_r . Wx_s), softmax over each target's incoming edges (max-subtracted),
heads concatenated, bias and activation; gradients by autograd.  test_restatement_matches_the_oracle ties the restatement to
oracle.ngpde_oracle.gat_conv / gat_conv_backward once.  Outputs the contract says are written start as NaN, and so does the workspace;
no form uses atomics, so a second call must give the same bits.

Test data cannot flip a branch: a leakyrelu logit, or a relu / leakyrelu / elu pre-activation, whose float64 value lies so close to 0
that float32 takes the other branch moves dal / dar and through them dx, dW and da far from that edge.  So the inputs are drawn from a
fixed seed, the float64 logits and pre-activations are computed, and the draw is repeated deterministically (seed + 1, ...) until none
lies within 1e-5 * max|.| of zero.  At the largest tile counts (hundreds of thousands of logits) no plain draw passes, so there x is
drawn with a margin: its components along the heads' score vectors are set so that |a_r . Wx_s| is in [1.5, 2.5] and |a_l . Wx_t| <= 1
(every logit at least 0.5 from zero).  Activations with a kink are used on graphs small enough for a plain draw.

Tolerances are the suite's: forward 1e-4 * max|ref| + 1e-5, gradients 5e-4 relative; the solver's are those of
test_c3_gat_as_ode_right_hand_side_full_size_against_the_oracle (see section C for why du0's are looser).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from oracle import ngpde_oracle as O
from test_mp_gpu import close
from test_edge_mlp_forms_gpu import (ACTS, HALO_CAP, ROWS, SLOT_WIDTH, TileGraph, _release_graphs, f64, graph,  # noqa: F401
                                     random_degrees, same, spread, tile_geometry, tiled_graph)
import gcn_gat_forms_spec as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
GD = F.GAT_WIDTH
SWITCHES = (F.NO_FUSED_GAT, F.NO_FUSED_GAT_LAYER, F.NO_PERSISTENT)
KINKED = ("relu", "leakyrelu", "elu")          # activations with a branch at 0
SMOOTH = ("identity", "tanh", "sigmoid", "swish", "gelu", "softplus")
NEAR = 1e-5                                    # no logit / kinked pre-activation within NEAR * max|.| of zero


def clear_switches(monkeypatch):
    # the suite may run under one of these: every case here names the form it tests (all three are read per call / per plan)
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def nan(*shape):
    return torch.full(shape, math.nan, device=DEV)


def nan_ws(nbytes):
    return torch.full((max(int(nbytes), 256),), 0xFF, dtype=torch.uint8, device=DEV)     # NaN words


# ---- geometry in both directions ----------------------------------------------------------------------------------------------------

def both_ways(g):
    """(by-target halo, in-degree, by-source halo, out-degree, tiles) of a TileGraph; the by-source tiles are the same 32-node runs"""
    if not hasattr(g, "halo_s"):
        hs, g.max_out, _ = tile_geometry(g.t, g.s, g.order, g.n)
        g.halo_s = int(hs.max())
    return g.max_halo, g.max_deg, g.halo_s, g.max_out, g.n_tiles


def geom_of(g):
    """what the headers' choices read of a handle (csrc/tile_geom.h), from the host geometry"""
    ht, di, hs, do, _ = both_ways(g)
    return F.geom(g.n, g.E, halo_ok=ht <= HALO_CAP and di <= SLOT_WIDTH, halo_ok_s=hs <= HALO_CAP and do <= SLOT_WIDTH)


def layer_fits(g):
    return F.layer_fits(geom_of(g))


def transposed(key, base):
    return graph(("gat T",) + key, lambda: TileGraph(base.t, base.s, base.n, base.order))


def made(key, n, spec, seed):
    def make():
        s, t, order = tiled_graph(n, spec, seed)
        return TileGraph(s, t, n, order)
    return graph(("gat",) + key, make)


def two_way(H, n_tiles=12, row32=False):
    """by-target halo exactly H (every 5th tile at H, the others at most 8 foreign sources) and short rows, so that the by-source
    tiles fit too; row32: one row of 32 entries in each tile at H"""
    def spec(k, rows, rng):
        F = H - ROWS if k % 5 == 0 else min(int(rng.integers(0, 9)), H - ROWS)
        d = random_degrees(rows, rng, F, hi=6)
        if row32 and k % 5 == 0:
            d[int(rng.integers(rows))] = SLOT_WIDTH
        return F, d
    g = made(("two way", H, n_tiles, row32), n_tiles * ROWS - 5, spec, 900 + H + n_tiles)
    assert g.max_halo == H and g.n_tiles == n_tiles, (H, g.max_halo, g.n_tiles)
    return g


def degrees_graph():
    """tile 0 has rows of in-degree 0 (no self loop), 1, 2, 15, 16, 17, 31 and 32 (a lane holds entries q and q + 16), the rest random"""
    want = (0, 0, 1, 2, 15, 16, 17, 31, 32, 32)

    def spec(k, rows, rng):
        if k == 0:
            d = np.concatenate([want, rng.integers(0, 9, rows - len(want))])
            return 24, rng.permutation(d)
        F = int(rng.integers(0, 9))
        return F, random_degrees(rows, rng, F, hi=6)
    g = made(("degrees",), 8 * ROWS - 5, spec, 41)
    tile = g.deg.numpy()[g.order[:ROWS]]
    assert set(want) <= set(tile.tolist()) and g.max_deg == SLOT_WIDTH
    return g


def multi_edge_graph():
    """a halo-64 graph in which about 10 % of the edges appear twice and 5 % three times"""
    def make():
        n = 12 * ROWS - 3
        s, t, order = tiled_graph(n, lambda k, rows, rng: (32 if k % 4 == 0 else 4, random_degrees(rows, rng, 32 if k % 4 == 0 else 4, hi=6)), 43)
        rng = np.random.default_rng(43)
        two = rng.choice(s.size, size=s.size // 10, replace=False)
        three = rng.choice(two, size=s.size // 20, replace=False)
        idx = np.concatenate([np.arange(s.size), two, three])       # (three is part of two)
        idx = idx[rng.permutation(idx.size)]
        return TileGraph(s[idx], t[idx], n, order)
    g = graph(("gat", "multi"), make)
    pairs = np.unique(g.t * g.n + g.s, return_counts=True)[1]
    assert (pairs == 2).any() and (pairs == 3).any()
    return g


TILE_COUNTS = (1, 2, 3, 33, 257, 1101)


def tiles_graph(n_tiles):
    """n_tiles tiles, the last one ragged (a single tile: 21 nodes), by-target halos up to 62 rows"""
    def spec(k, rows, rng):
        F = 0 if n_tiles == 1 else 30 if k % 7 == 0 else int(rng.integers(0, 16))
        return F, random_degrees(rows, rng, F, hi=6)
    n = 21 if n_tiles == 1 else n_tiles * ROWS - (5 + n_tiles % 7)
    g = made(("tiles", n_tiles), n, spec, 500 + n_tiles)
    assert g.n_tiles == n_tiles and g.n % ROWS != 0
    return g


def refused_graphs():
    """name -> graph whose tiles break exactly one cap (the edgeless graph: no tile breaks one, the layer needs an edge)"""
    n = 10 * ROWS

    def spec97(k, rows, rng):
        return (65, spread(200, rows, rng)) if k == 3 else (5, random_degrees(rows, rng, 5))

    def spec33(k, rows, rng):
        d = random_degrees(rows, rng, 4)
        if k == 6:
            d[7] = 33
        return 4, d
    h97 = made(("halo97",), n, spec97, 47)
    d33 = made(("deg33",), n, spec33, 48)
    empty = graph(("gat", "empty"), lambda: TileGraph(np.zeros(0, np.int64), np.zeros(0, np.int64), 3 * ROWS - 4,
                                                       np.random.default_rng(0).permutation(3 * ROWS - 4).astype(np.int32)))
    return {"halo 97 by target": h97, "halo 97 by source": transposed(("halo97",), h97), "in-degree 33": d33,
            "out-degree 33": transposed(("deg33",), d33), "no edges": empty}


# ---- the float64 restatement --------------------------------------------------------------------------------------------------------

def leaky(v, slope):
    return torch.where(v > 0, v, slope * v)


def gat_aggregate(g, wx, a, heads, slope):
    """(out [N][heads*c], alpha [E][heads] p order, al, ar [N][heads], pre-logits [E][heads]) of wx [N][heads*c], a [heads][2c]"""
    N, c = g.n, a.shape[1] // 2
    w3 = wx.reshape(N, heads, c)
    al = (w3 * a[None, :, :c]).sum(-1)
    ar = (w3 * a[None, :, c:]).sum(-1)
    v = al[g.tp] + ar[g.sp]
    logit = leaky(v, slope)
    mx = torch.full((N, heads), -math.inf, dtype=wx.dtype).scatter_reduce(0, g.tp[:, None].expand(-1, heads), logit.detach(), "amax")
    ex = torch.exp(logit - mx[g.tp])
    den = torch.zeros(N, heads, dtype=wx.dtype).index_add(0, g.tp, ex)
    alpha = ex / den[g.tp]
    out = torch.zeros(N, heads, c, dtype=wx.dtype).index_add(0, g.tp, alpha[:, :, None] * w3[g.sp])
    return out.reshape(N, heads * c), alpha, al, ar, v


def gat_layer_ref(g, x, wt, a, bias, heads, slope, act):
    """(y, z, alpha, pre-logits) of the whole layer"""
    out, alpha, _, _, v = gat_aggregate(g, x @ wt, a, heads, slope)
    z = out + (bias if bias is not None else 0.0)
    return ACTS[act](z), z, alpha, v


def margin_x(rng, x, wt, a, heads):
    """x with its components along the heads' score vectors set: |a_r . Wx| in [1.5, 2.5], |a_l . Wx| <= 1"""
    c = GD // heads
    V = np.concatenate([np.stack([wt[:, k * c:(k + 1) * c].astype(np.float64) @ a[k, :c] for k in range(heads)], 1),
                        np.stack([wt[:, k * c:(k + 1) * c].astype(np.float64) @ a[k, c:] for k in range(heads)], 1)], 1)
    n = x.shape[0]
    tgt = np.concatenate([rng.uniform(-1.0, 1.0, (n, heads)), rng.choice([-1.0, 1.0], (n, heads)) * rng.uniform(1.5, 2.5, (n, heads))], 1)
    return (x + (tgt - x @ V) @ np.linalg.pinv(V)).astype(np.float32)


def near_zero(v, exempt=None):
    """entries of v within NEAR * max|v| of zero (exact zeros where `exempt`: both precisions compute those exactly)"""
    if v.numel() == 0:
        return 0
    m = v.abs() < NEAR * float(v.abs().max())
    if exempt is not None:
        m &= ~(exempt & (v == 0))
    return int(m.sum())


def branch_safe(draw, check, seed, tries=64):
    """the first deterministic redraw (seed, seed + 1, ...) whose float64 logits / kinked pre-activations all stay clear of zero"""
    for k in range(tries):
        d = draw(seed + k)
        if check(d) == 0:
            return d
    raise AssertionError(f"no branch-safe draw in {tries} seeds from {seed}")


# ---- A. the one-launch layer --------------------------------------------------------------------------------------------------------

class Layer:
    """y = act(||_k sum_e alpha_ek (x wt)_k[s_e] + b) on a TileGraph; x [N][64], wt [64][64], a [heads][2c] (= (2c x heads) column-major)"""

    def __init__(self, g, heads, act, slope, seed, bias=True, logit=None, margin=False):
        self.g, self.heads, self.c, self.act, self.slope = g, heads, GD // heads, act, slope
        self.has_bias = bias

        def draw(sd):
            rng = np.random.default_rng(sd)
            d = dict(x=rng.normal(size=(g.n, GD)).astype(np.float32),
                     wt=(rng.normal(size=(GD, GD)) * 1.5 / 8).astype(np.float32),
                     a=(rng.normal(size=(heads, 2 * self.c)) / np.sqrt(self.c)).astype(np.float32),
                     b=(0.3 * rng.normal(size=GD)).astype(np.float32) if bias else None,
                     dy=rng.normal(size=(g.n, GD)).astype(np.float32))
            if margin:
                d["x"] = margin_x(rng, d["x"].astype(np.float64), d["wt"], d["a"], heads)
            if logit is not None and g.E:
                # leakyrelu is positively homogeneous: scaling a scales every logit
                v = self._ref64(d)[3]
                d["a"] = (d["a"] * (logit / float(v.abs().max()))).astype(np.float32)
            return d

        def check(d):
            _, z, _, v = self._ref64(d)
            empty = (g.deg == 0)[:, None].expand_as(z) if not bias else None
            return near_zero(v) + (near_zero(z, empty) if act in KINKED else 0)
        self.d = branch_safe(draw, check, seed)
        self._ref = None

    def _ref64(self, d):
        with torch.no_grad():
            return gat_layer_ref(self.g, f64(d["x"]), f64(d["wt"]), f64(d["a"]), f64(d["b"]) if d["b"] is not None else None, self.heads,
                                 self.slope, self.act)

    def reference(self):
        if self._ref is None:
            d = self.d
            x, wt, a = f64(d["x"]).requires_grad_(), f64(d["wt"]).requires_grad_(), f64(d["a"]).requires_grad_()
            b = f64(d["b"] if d["b"] is not None else np.zeros(GD)).requires_grad_()
            y, z, alpha, v = gat_layer_ref(self.g, x, wt, a, b, self.heads, self.slope, self.act)
            gr = torch.autograd.grad(y, [x, wt, a, b], f64(d["dy"]), allow_unused=True)
            gr = [torch.zeros_like(p) if q is None else q for p, q in zip([x, wt, a, b], gr)]
            self._ref = dict(y=y.detach(), z=z.detach(), alpha=alpha.detach(), v=v.detach(), dx=gr[0], dweight=gr[1], da=gr[2], dbias=gr[3])
        return self._ref

    def _dev(self):
        if not hasattr(self, "_dv"):
            self._dv = {k: (torch.as_tensor(v, device=DEV) if v is not None else None) for k, v in self.d.items()}
        return self._dv

    def forward_status(self, save_alpha=True, save_z=True, din=GD, heads=None):
        lib, dv, g = _lib.load(), self._dev(), self.g
        heads = heads or self.heads
        y, al, z = nan(g.n, GD), nan(max(g.E, 1), heads) if save_alpha else None, nan(g.n, GD) if save_z else None
        st = lib.ngpde_gat_layer_forward(g.ptr, din, heads, GD // heads, self.slope, _lib.ACT[self.act], _lib.ptr(dv["x"]), _lib.ptr(dv["wt"]),
                                         _lib.ptr(dv["a"]), _lib.ptr(dv["b"]), _lib.ptr(y), _lib.ptr(al), _lib.ptr(z), _lib.current_stream())
        return st, y, al, z

    def backward_status(self, y_or_z, alpha, dx=True, dbias=True, din=GD, heads=None):
        lib, dv, g = _lib.load(), self._dev(), self.g
        heads = heads or self.heads
        out = dict(dweight=nan(GD, GD), da=nan(heads, 2 * (GD // heads)))
        if dx:
            out["dx"] = nan(g.n, GD)
        if dbias:
            out["dbias"] = nan(GD)
        ws = nan_ws(lib.ngpde_gat_layer_workspace_bytes(g.ptr, heads, GD // heads))
        st = lib.ngpde_gat_layer_backward(g.ptr, din, heads, GD // heads, self.slope, _lib.ACT[self.act], _lib.ptr(dv["x"]), _lib.ptr(dv["wt"]),
                                          _lib.ptr(dv["a"]), _lib.ptr(y_or_z), _lib.ptr(alpha), _lib.ptr(dv["dy"]), _lib.ptr(out.get("dx")),
                                          _lib.ptr(out["dweight"]), _lib.ptr(out["da"]), _lib.ptr(out.get("dbias")), _lib.ptr(ws), ws.numel(),
                                          _lib.current_stream())
        return st, out


def check_layer(L, what, dx=True, dbias=True):
    """forward with save_z present and NULL (bitwise the same y, twice: bitwise), the pullback twice (bitwise), all against float64"""
    g, ref = L.g, L.reference()
    st, y, alpha, z = L.forward_status()
    _lib.check(st)
    close(y, ref["y"].numpy(), what=f"y {what}")
    close(z, ref["z"].numpy(), what=f"save_z {what}")
    close(alpha.abs()[:g.E], ref["alpha"].numpy(), what=f"|save_alpha| {what}")
    assert torch.equal(torch.signbit(alpha[:g.E]).cpu(), ref["v"] <= 0), f"save_alpha sign != leakyrelu branch {what}"
    empty = (g.deg == 0).numpy()
    if empty.any():                                         # rows without an edge (no self loop): y = act(b)
        b = f64(L.d["b"]) if L.d["b"] is not None else torch.zeros(GD, dtype=torch.float64)
        close(y.cpu()[empty], np.broadcast_to(ACTS[L.act](b).numpy(), (int(empty.sum()), GD)), what=f"empty rows {what}")
    st, y2, alpha2, _ = L.forward_status(save_z=False)
    _lib.check(st)
    assert same(y, y2) and same(alpha, alpha2), f"forward repeat / save_z NULL {what}"
    yz = None if L.act == "identity" else y if L.act == "relu" else z          # the y_or_z contract
    st, gr = L.backward_status(yz, alpha, dx=dx, dbias=dbias)
    _lib.check(st)
    for k, v in gr.items():
        close(v, ref[k].numpy(), rtol=5e-4, atol=1e-5, what=f"{k} {what}")
    st, gr2 = L.backward_status(yz, alpha, dx=dx, dbias=dbias)
    _lib.check(st)
    assert same(gr, gr2), f"pullback repeat {what}"


def assert_layer_regime(g, heads, halo_t=None, halo_s=None, in_deg=None, out_deg=None, tiles=None, fits=True):
    ht, di, hs, do, nt = both_ways(g)
    for want, got, name in ((halo_t, ht, "by-target halo"), (halo_s, hs, "by-source halo"), (in_deg, di, "in-degree"),
                            (out_deg, do, "out-degree"), (tiles, nt, "tiles")):
        assert want is None or got == want, (name, got, want)
    assert layer_fits(g) == fits, (ht, di, hs, do)
    assert _lib.load().ngpde_gat_layer_supported(g.ptr, GD, heads, GD // heads) == int(fits)


def test_restatement_matches_the_oracle():
    # the float64 restatement here against oracle.gat_conv / gat_conv_backward (the oracle's hand-written pullback) to 1e-12
    rng = np.random.default_rng(3)
    n, E, heads, c = 40, 160, 2, 32
    s, t = rng.integers(0, n, E), rng.integers(0, n, E)

    class G:
        pass
    g = G()
    p = np.argsort(t, kind="stable")
    g.n, g.sp, g.tp = n, torch.as_tensor(s[p]), torch.as_tensor(t[p])
    x, wt, a = rng.normal(size=(n, GD)), rng.normal(size=(GD, GD)) / 8, rng.normal(size=(heads, 2 * c)) / 4
    b, dy = rng.normal(size=GD), rng.normal(size=(n, GD))
    og = O.Graph(s, t, num_nodes=n, index_base=0)
    yo, cache = O.gat_conv(x.T, wt.T, a.T, b, og, heads, c, "tanh", negative_slope=0.1, add_self_loops_=False)
    go = O.gat_conv_backward(cache, dy.T)
    X, W, A, B = (torch.tensor(v, requires_grad=True) for v in (x, wt, a, b))
    y, _, _, _ = gat_layer_ref(g, X, W, A, B, heads, 0.1, "tanh")
    gx, gw, ga, gb = torch.autograd.grad(y, [X, W, A, B], torch.tensor(dy))
    for got, ref, name in ((y.detach().numpy(), yo.T, "y"), (gx.numpy(), go["x"].T, "dx"), (gw.numpy(), go["weight"].T, "dW"),
                           (ga.numpy(), go["a"].T, "da"), (gb.numpy(), go["bias"], "db")):
        assert np.abs(got - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), name


HALOS_T = (32, 48, 64, 95, 96)


def layer_cases():
    """(id, graph maker, regime kwargs, act, slope, options); acts / slopes are rotated per head count below"""
    cases = [(f"halo{H}", (lambda H=H: two_way(H)), dict(halo_t=H)) for H in HALOS_T]
    cases += [("src-halo96", lambda: transposed(("two way", 96), two_way(96)), dict(halo_s=96)),
              ("degrees", degrees_graph, dict(in_deg=32)),
              ("degrees-T", lambda: transposed(("degrees",), degrees_graph()), dict(out_deg=32)),
              ("multi-edges", multi_edge_graph, dict(halo_t=64)),
              ("large-logits", lambda: two_way(80), dict(halo_t=80))]
    cases += [(f"tiles{n}", (lambda n=n: tiles_graph(n)), dict(tiles=n)) for n in TILE_COUNTS]
    return cases


LAYER_CASES = layer_cases()
SLOPES = (0.2, 0.01, 0.0)


def case_act(i, heads, cid):
    if cid in ("tiles257", "tiles1101"):               # too many logits / pre-activations for a plain draw: smooth activations
        return SMOOTH[(i + heads) % len(SMOOTH)]
    order = KINKED + SMOOTH
    return order[(i + 3 * heads) % len(order)]


@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("case", range(len(LAYER_CASES)), ids=[c[0] for c in LAYER_CASES])
def test_layer_against_float64(case, heads, monkeypatch):
    # halos 32 .. 96 by target (96: the staged rows span every staging round), 96 by source (a transposed halo-96 graph), rows of
    # 0 .. 32 entries in both directions, multi-edges, 1 .. 1 101 tiles (1 101: 551 by-source workgroups, the reduction folds more
    # than 512 slabs), logits up to 90 (exp overflows float32 from 88.7), every activation, slopes 0.2 / 0.01 / 0, and bias, dx,
    # dbias, save_z present and NULL
    clear_switches(monkeypatch)
    cid, make, regime = LAYER_CASES[case]
    g = make()
    assert_layer_regime(g, heads, **regime)
    if cid == "src-halo96":
        assert g.max_halo < HALO_CAP                         # (the by-target halo is incidental)
    if cid == "tiles1101":
        assert (g.n_tiles + 1) // 2 == 551
    act, slope = case_act(case, heads, cid), SLOPES[(case + heads) % 3]
    big = g.n_tiles > 64
    L = Layer(g, heads, act, slope, seed=100 * case + heads, bias=(case + heads) % 4 != 0, logit=90.0 if cid == "large-logits" else None,
              margin=big)
    if cid == "large-logits":
        assert float(L.reference()["v"].abs().max()) == pytest.approx(90.0, rel=1e-4)
    check_layer(L, f"{cid} heads={heads} act={act} slope={slope}", dx=(case + heads) % 5 != 1, dbias=(case + heads) % 3 != 2)


def test_layer_covers_every_cap_and_activation_per_head_count():
    # the grid above: every activation and every slope at each head count
    for heads in (1, 2, 4):
        acts = {case_act(i, heads, c[0]) for i, c in enumerate(LAYER_CASES)}
        assert acts == set(ACTS), (heads, set(ACTS) - acts)
        assert {SLOPES[(i + heads) % 3] for i in range(len(LAYER_CASES))} == set(SLOPES)


def test_layer_refuses_tiles_beyond_the_caps(monkeypatch):
    # halo 97 by target / by source, in-degree 33, out-degree 33, no edges; then din != 64 and heads = 8 on a graph that fits:
    # the query says 0 and both entries return ERR_UNSUPPORTED without writing
    clear_switches(monkeypatch)
    lib = _lib.load()
    gs = refused_graphs()
    assert both_ways(gs["halo 97 by target"])[0] == 97 and both_ways(gs["halo 97 by target"])[2] <= HALO_CAP
    assert both_ways(gs["halo 97 by source"])[2] == 97 and both_ways(gs["halo 97 by source"])[0] <= HALO_CAP
    assert both_ways(gs["in-degree 33"])[1] == 33 and both_ways(gs["in-degree 33"])[3] <= SLOT_WIDTH
    assert both_ways(gs["out-degree 33"])[3] == 33 and both_ways(gs["out-degree 33"])[1] <= SLOT_WIDTH
    assert gs["no edges"].E == 0
    for why, g in gs.items():
        assert not layer_fits(g), why
        for heads in (1, 2, 4):
            L = Layer(g, heads, "tanh", 0.2, seed=7)
            assert lib.ngpde_gat_layer_supported(g.ptr, GD, heads, GD // heads) == 0, why
            st, y, al, z = L.forward_status()
            assert st == _lib.ERR_UNSUPPORTED and bool(torch.isnan(y).all() and torch.isnan(z).all()), (why, st)
            st, gr = L.backward_status(z, al)
            assert st == _lib.ERR_UNSUPPORTED and all(bool(torch.isnan(v).all()) for v in gr.values()), (why, st)
    g = two_way(96)
    assert layer_fits(g)
    L = Layer(g, 4, "tanh", 0.2, seed=8)
    for din, heads in ((32, 4), (GD, 8)):
        assert lib.ngpde_gat_layer_supported(g.ptr, din, heads, GD // heads) == 0
        st, y, al, z = L.forward_status(din=din, heads=heads)
        assert st == _lib.ERR_UNSUPPORTED and bool(torch.isnan(y).all()), (din, heads, st)
        st, gr = L.backward_status(z, al, din=din, heads=heads)
        assert st == _lib.ERR_UNSUPPORTED and all(bool(torch.isnan(v).all()) for v in gr.values()), (din, heads, st)


# ---- B. the aggregation primitives --------------------------------------------------------------------------------------------------

P2 = F.GAT_BLOCKED_HEADS


def fwd_form(g, heads, c, no_fused=False):
    """gat_fwd_form's choice (csrc/gat_forms.h) by its restatement; no_fused: as under NGPDE_NO_FUSED_GAT=1"""
    with pytest.MonkeyPatch.context() as mp:
        mp.delenv(F.NO_FUSED_GAT, raising=False)
        if no_fused:
            mp.setenv(F.NO_FUSED_GAT, "1")
        return F.fwd_form(geom_of(g), heads, c)


def bwd_form(heads, c, wx, dout):
    """gat_bwd_form's choice by its restatement; the two pointers enter as one alignment bit"""
    return F.bwd_form(heads, c, (wx.data_ptr() | dout.data_ptr()) % 16 == 0)


ROW_DEGREES = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129, 130, 300)


def rows_graph():
    """every length in ROW_DEGREES (one block / exactly one / several of 64 / H edges for every H, the row-per-wave stride of 64
    wrapping once, twice, four times at the 300-edge hub) plus short random rows; sources distinct within a row"""
    def make():
        rng = np.random.default_rng(61)
        n = 400
        deg = np.concatenate([ROW_DEGREES, rng.integers(0, 7, n - len(ROW_DEGREES))])
        deg = deg[rng.permutation(n)]
        s = np.concatenate([rng.choice(n, size=k, replace=False) for k in deg])
        t = np.repeat(np.arange(n), deg)
        p = rng.permutation(s.size)
        return TileGraph(s[p], t[p], n, rng.permutation(n).astype(np.int32))
    g = graph(("gat", "rows"), make)
    assert set(ROW_DEGREES) <= set(g.deg.numpy().tolist())
    return g


class Agg:
    """ngpde_gat_forward / _backward with wx given: out, alpha (p order), al, ar; dwx, da"""

    def __init__(self, g, heads, c, slope, seed):
        self.g, self.heads, self.c, self.slope = g, heads, c, slope

        def draw(sd):
            rng = np.random.default_rng(sd)
            return dict(wx=rng.normal(size=(g.n, heads * c)).astype(np.float32),
                        a=(rng.normal(size=(heads, 2 * c)) / np.sqrt(c)).astype(np.float32),
                        dout=rng.normal(size=(g.n, heads * c)).astype(np.float32))

        def check(d):
            with torch.no_grad():
                return near_zero(gat_aggregate(g, f64(d["wx"]), f64(d["a"]), heads, slope)[4])
        self.d = branch_safe(draw, check, seed)
        wx, a = f64(self.d["wx"]).requires_grad_(), f64(self.d["a"]).requires_grad_()
        out, alpha, al, ar, _ = gat_aggregate(g, wx, a, heads, slope)
        dwx, da = torch.autograd.grad(out, [wx, a], f64(self.d["dout"]), allow_unused=True)
        z = torch.zeros_like
        self.ref = dict(out=out.detach(), alpha=alpha.detach(), al=al.detach(), ar=ar.detach(),
                        dwx=z(wx) if dwx is None else dwx, da=z(a) if da is None else da)
        self.wx, self.a, self.dout = (torch.as_tensor(self.d[k], device=DEV) for k in ("wx", "a", "dout"))

    def forward(self, wx=None):
        lib, g, H = _lib.load(), self.g, self.heads
        wx = self.wx if wx is None else wx
        f = dict(out=nan(g.n, H * self.c), alpha=nan(max(g.E, 1), H), al=nan(g.n, H), ar=nan(g.n, H))
        _lib.check(lib.ngpde_gat_forward(g.ptr, H, self.c, self.slope, _lib.ptr(wx), _lib.ptr(self.a), _lib.ptr(f["out"]), _lib.ptr(f["alpha"]),
                                         _lib.ptr(f["al"]), _lib.ptr(f["ar"]), _lib.current_stream()))
        return f

    def backward(self, f, wx=None, dout=None):
        lib, g, H = _lib.load(), self.g, self.heads
        wx, dout = self.wx if wx is None else wx, self.dout if dout is None else dout
        b = dict(dwx=nan(g.n, H * self.c), da=nan(H, 2 * self.c))
        ws = nan_ws(lib.ngpde_gat_workspace_bytes(g.ptr, H))
        _lib.check(lib.ngpde_gat_backward(g.ptr, H, self.c, self.slope, _lib.ptr(wx), _lib.ptr(self.a), _lib.ptr(f["al"]), _lib.ptr(f["ar"]),
                                          _lib.ptr(f["alpha"]), _lib.ptr(dout), _lib.ptr(b["dwx"]), _lib.ptr(b["da"]), _lib.ptr(ws), ws.numel(),
                                          _lib.current_stream()))
        return b

    def check(self, what, wx=None, dout=None):
        f = self.forward(wx)
        E = self.g.E
        for k in ("out", "al", "ar"):
            close(f[k], self.ref[k].numpy(), what=f"{k} {what}")
        close(f["alpha"][:E], self.ref["alpha"].numpy(), what=f"alpha {what}")
        f2 = self.forward(wx)
        assert all(torch.equal(f[k], f2[k]) for k in ("out", "al", "ar")) and torch.equal(f["alpha"][:E], f2["alpha"][:E]), f"forward repeat {what}"
        b = self.backward(f, wx, dout)
        for k in ("dwx", "da"):
            close(b[k], self.ref[k].numpy(), rtol=5e-4, atol=1e-5, what=f"{k} {what}")
        assert same(b, self.backward(f, wx, dout)), f"pullback repeat {what}"
        return f, b


@pytest.mark.parametrize("heads", [1, 2, 4])
def test_tiled_forward_and_its_fallback(heads, monkeypatch):
    # gat_fused_fwd_kernel on a halo-96 graph, then the same inputs with NGPDE_NO_FUSED_GAT=1 (the blocked forward); pullback blocked
    clear_switches(monkeypatch)
    g = two_way(96)
    c = GD // heads
    assert g.fits() and fwd_form(g, heads, c) == "tiled" and fwd_form(g, heads, c, no_fused=True) == "blocked"
    P = Agg(g, heads, c, 0.2, seed=200 + heads)
    assert bwd_form(heads, c, P.wx, P.dout) == "blocked"
    P.check(f"tiled heads={heads}")
    monkeypatch.setenv("NGPDE_NO_FUSED_GAT", "1")
    P.check(f"NO_FUSED_GAT heads={heads}")


BLOCKED = [(h, c) for h in P2 for c in (4, 16)] + [(h, c) for h in P2 for c in (3, 5)]


@pytest.mark.parametrize("heads,c", BLOCKED, ids=[f"H{h}-c{c}" for h, c in BLOCKED])
def test_blocked_forms(heads, c, monkeypatch):
    # gat_fwd_blocked_kernel<H> at c 4 / 16 (16 x 16 = 256: every acc[4] slot), rows of one block, exactly one full block and several;
    # c 3 / 5 (c % 4 != 0): the blocked forward with the row-per-wave pullback
    clear_switches(monkeypatch)
    g = rows_graph()
    epb = 64 // heads
    degs = set(g.deg.numpy().tolist())
    assert {epb - 1, epb, epb + 1} <= degs and max(degs) > 2 * epb       # one block, exactly one full block, several
    assert g.max_deg > SLOT_WIDTH and fwd_form(g, heads, c) == "blocked"
    P = Agg(g, heads, c, SLOPES[(heads + c) % 3], seed=300 + 17 * heads + c)
    assert bwd_form(heads, c, P.wx, P.dout) == ("blocked" if c % 4 == 0 else "row")
    P.check(f"blocked heads={heads} c={c}")


ROW_WAVE = [(3, 7), (5, 16), (6, 11), (4, 65), (5, 64), (8, 64)]


@pytest.mark.parametrize("heads,c", ROW_WAVE, ids=[f"H{h}-c{c}" for h, c in ROW_WAVE])
def test_row_per_wave_forms(heads, c, monkeypatch):
    # gat_fwd_kernel / gat_bwd_{target,source}_kernel: heads 3 / 5 / 6, heads * c 260 / 320 / 512, rows of 0 .. 300 edges
    clear_switches(monkeypatch)
    g = rows_graph()
    assert {0, 1, 63, 64, 65, 130, 300} <= set(g.deg.numpy().tolist())
    assert fwd_form(g, heads, c) == "row"
    P = Agg(g, heads, c, SLOPES[heads % 3], seed=400 + heads * c)
    assert bwd_form(heads, c, P.wx, P.dout) == "row"
    P.check(f"row-per-wave heads={heads} c={c}")


def test_misaligned_pointers_take_the_row_per_wave_pullback(monkeypatch):
    # wx and dout as views 4 bytes into larger buffers at heads 4, c 16: the row-per-wave pullback, equal to the aligned (blocked)
    # call to rounding and to float64 within tolerance
    clear_switches(monkeypatch)
    g = rows_graph()
    P = Agg(g, 4, 16, 0.2, seed=500)
    f, b = P.check("aligned")
    bw = torch.empty(P.wx.numel() + 1, device=DEV)
    bd = torch.empty(P.dout.numel() + 1, device=DEV)
    wx = bw[1:].view_as(P.wx).copy_(P.wx)
    dout = bd[1:].view_as(P.dout).copy_(P.dout)
    assert wx.data_ptr() % 16 == 4 and dout.data_ptr() % 16 == 4
    assert bwd_form(4, 16, P.wx, P.dout) == "blocked" and bwd_form(4, 16, wx, dout) == "row"
    f2, b2 = P.check("misaligned", wx=wx, dout=dout)
    assert all(torch.equal(f[k], f2[k]) for k in f)          # (the forward does not depend on the alignment)
    for k in ("dwx", "da"):
        close(b2[k], b[k].cpu().double().numpy(), rtol=1e-5, atol=1e-6, what=f"{k} misaligned vs aligned")


def test_edgeless_graph_through_every_forward_form(monkeypatch):
    # out = 0 and the pullback gives dwx = 0, da = 0 in the tiled, blocked and row-per-wave forms
    clear_switches(monkeypatch)
    g = refused_graphs()["no edges"]
    assert g.E == 0 and g.fits()
    for heads, c, no_fused, form in ((4, 16, False, "tiled"), (4, 16, True, "blocked"), (3, 5, False, "row")):
        assert fwd_form(g, heads, c, no_fused) == form
        if no_fused:
            monkeypatch.setenv("NGPDE_NO_FUSED_GAT", "1")
        P = Agg(g, heads, c, 0.2, seed=600)
        f, b = P.check(form)
        assert not bool(f["out"].any()) and not bool(b["dwx"].any()) and not bool(b["da"].any()), form
        monkeypatch.delenv("NGPDE_NO_FUSED_GAT", raising=False)


# ---- C. the device-resident solver at the caps --------------------------------------------------------------------------------------

class Plan:
    def __init__(self, g, heads, slope, act, tableau, n_steps, dt, members):
        lib = _lib.load()
        out = C.c_void_p()
        if members == 1:
            st = lib.ngpde_node_gat_create(g.ptr, heads, GD // heads, slope, _lib.ACT[act], _lib.TABLEAU[tableau], n_steps, dt, 1, C.byref(out))
        else:
            st = lib.ngpde_node_gat_create_batch(g.ptr, members, heads, GD // heads, slope, _lib.ACT[act], _lib.TABLEAU[tableau], n_steps, dt,
                                                 1, C.byref(out))
        assert st == _lib.OK, f"the solver refused the plan ({st})"
        self.ptr = out

    def fault(self):
        f = C.c_int32(-1)
        _lib.check(_lib.load().ngpde_node_gat_fault(self.ptr, _lib.current_stream(), C.byref(f)))
        return f.value

    def close(self):
        _lib.destroy_later("ngpde_node_gat_destroy", self.ptr)


SOLVER_GRAPHS = {"halo96-rows32": (lambda: two_way(96, 20, row32=True), dict(halo_t=96, in_deg=32)),
                 "src-halo96": (lambda: transposed(("two way", 96, 20), two_way(96, 20, row32=True)), dict(halo_s=96, out_deg=32)),
                 "tiles257": (lambda: tiles_graph(257), dict(tiles=257))}


@pytest.mark.parametrize("members", [1, 2])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("gid", list(SOLVER_GRAPHS))
def test_solver_at_the_caps_against_float64(gid, heads, members, monkeypatch):
    # ngpde_node_gat_create[_batch]: tanh, Tsit5 x 2 then Euler x 3; u(T), du0 and the parameter gradients against O.rk_solve /
    # O.rk_adjoint over the float64 restatement (loss = sum(u(T))), a replay bitwise, no fault.  Tolerances are C3's
    # (test_c3_gat_as_ode_right_hand_side_full_size_against_the_oracle): the stage inputs u + dt a_ij k_j cannot be redrawn, so a
    # logit of some stage may lie within rounding of zero and flip leakyrelu's branch, which moves du0 in the rows around that edge
    clear_switches(monkeypatch)
    make, regime = SOLVER_GRAPHS[gid]
    g = make()
    assert_layer_regime(g, heads, **regime)
    assert g.n_tiles <= 512                                  # config 3's 512 tiles are resident
    lib = _lib.load()
    assert lib.ngpde_node_gat_supported(g.ptr, GD, heads, GD // heads) == 1
    c, slope = GD // heads, 0.2
    rng = np.random.default_rng(800 + heads + members)
    wt = (rng.normal(size=(GD, GD)) * 1.5 / 8).astype(np.float32)
    a = (rng.normal(size=(heads, 2 * c)) / np.sqrt(c)).astype(np.float32)
    b = (0.1 * rng.normal(size=GD)).astype(np.float32)
    u0 = rng.normal(size=(members, g.n, GD)).astype(np.float32)
    W, A, B = f64(wt), f64(a), f64(b)

    def rhs(u):
        return gat_layer_ref(g, torch.as_tensor(u), W, A, B, heads, slope, "tanh")[0].numpy(), u

    def vjp(u, kbar):
        U, Wg, Ag, Bg = (v.clone().requires_grad_() for v in (torch.as_tensor(u), W, A, B))
        y = gat_layer_ref(g, U, Wg, Ag, Bg, heads, slope, "tanh")[0]
        gr = torch.autograd.grad(y, [U, Wg, Ag, Bg], torch.as_tensor(kbar))
        return gr[0].numpy(), dict(weight=gr[1].numpy(), a=gr[2].numpy(), bias=gr[3].numpy())

    dW, dA, dB = (torch.as_tensor(v, device=DEV) for v in (wt, a, b))
    for tableau, n_steps, dt in (("tsit5", 2, 0.05), ("euler", 3, 0.05)):
        acc = dict(weight=np.zeros((GD, GD)), a=np.zeros((heads, 2 * c)), bias=np.zeros(GD))

        def accumulate(gr):
            for k in acc:
                acc[k] += gr[k]
        uTo, du0o = [], []
        for m in range(members):
            uT, tape = O.rk_solve(rhs, u0[m].astype(np.float64), O.TABLEAUS[tableau], dt, n_steps)
            uTo.append(uT)
            du0o.append(O.rk_adjoint(vjp, tape, np.ones_like(uT), O.TABLEAUS[tableau], dt, accumulate))
        uTo, du0o = np.stack(uTo), np.stack(du0o)
        plan = Plan(g, heads, slope, "tanh", tableau, n_steps, dt, members)
        try:
            du = torch.as_tensor(u0, device=DEV)
            runs = []
            for _ in range(2):
                uT, du0 = nan(members, g.n, GD), nan(members, g.n, GD)
                gw, ga, gb = nan(GD, GD), nan(heads, 2 * c), nan(GD)
                _lib.check(lib.ngpde_node_gat_forward(plan.ptr, _lib.ptr(du), _lib.ptr(dW), _lib.ptr(dA), _lib.ptr(dB), _lib.ptr(uT),
                                                      _lib.current_stream()))
                ones = torch.ones_like(uT)
                _lib.check(lib.ngpde_node_gat_backward(plan.ptr, _lib.ptr(dW), _lib.ptr(dA), _lib.ptr(ones), _lib.ptr(du0), _lib.ptr(gw),
                                                       _lib.ptr(ga), _lib.ptr(gb), _lib.current_stream()))
                runs.append(dict(uT=uT, du0=du0, weight=gw, a=ga, bias=gb))
            assert plan.fault() == 0
        finally:
            plan.close()
        what = f"{gid} heads={heads} members={members} {tableau}x{n_steps}"
        assert same(runs[0], runs[1]), f"replay {what}"
        r = runs[0]
        close(r["uT"], uTo, 2e-4, what=f"u(T) {what}")
        got = r["du0"].cpu().double().numpy().reshape(-1, GD)
        ref = du0o.reshape(-1, GD)
        d = np.abs(got - ref).max(axis=1)
        bound = 5e-4 * np.abs(ref).max() + 1e-4
        assert (d > bound).sum() <= 0.005 * d.size and d.max() <= 40 * bound, f"du0 {what}: {(d > bound).sum()} of {d.size} rows, max {d.max():.2e}"
        assert abs(np.linalg.norm(got) - np.linalg.norm(ref)) <= 1e-4 * np.linalg.norm(ref), f"|du0| {what}"
        for k in acc:
            close(r[k], acc[k], 5e-4, 5e-3, f"d{k} {what}")
