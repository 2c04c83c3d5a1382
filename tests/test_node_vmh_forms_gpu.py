"""The device-resident NeuralODE(VMHConv(phi, gamma)) plan against float64 across its shape envelope.

ngpde_node_vmh_* (csrc/node_vmh.hip; plan and entries: csrc/node_vmh_plan.hip) solves du/dt = VMHConv(phi, gamma)(u) on a scalar state with ONE
persistent forward launch and ONE persistent adjoint launch, each in two template forms (vmh_geo_uncached, node_vmh.hip:1166):
  ROUNDS = false  every 16-row half tile of the handle's node order its own workgroup, all of them resident at once
                  (2 * tiles <= CUs x occupancy);
  ROUNDS = true   "tile rounds": whole 32-row tiles, workgroup b takes tiles b, b + G, b + 2 G, ... in that order in every phase
                  (node_vmh.hip:399, :446), at most kVmhMaxTurns = 64 of them.  NGPDE_NO_VMH_ROUNDS=1 (read per call, :1178) refuses
                  such graphs; ngpde_ode_create reports NGPDE_NODE_TILE_ROUNDS for them.
The regimes inside a launch, each of which a case below claims from host-side geometry BEFORE it compares anything:
  edge rounds     a unit's edges are walked in rounds of VROUND = 128 (node_vmh.hip:50; n_rounds at :413 / :463, :753 / :910).
                  One round of a half tile takes the fast paths -- `defer` (:427: tape rows stay in registers and are stored one
                  evaluation late, flushed at :683) and `one_round` (:785: the adjoint keeps the layer outputs in registers, dz rows
                  deferred, :808, :1117); more than 128 edges take the rd loops (:480, :1007) with fetch_y a round ahead (:867,
                  :1042) and immediate tape stores.  A half tile holds up to 16 x kSlotWidth = 512 edges (4 rounds), a tile of the
                  rounds form 1 024 (8).  total = 0: no round at all, the workgroup still waits and publishes its flags.
  widths          every Dense layer is staged zero-padded to 64 x 64 (stage_weight, :130); slice_matmul<NOUT, NIN> (:154) skips the
                  16-column blocks beyond a layer's widths; the bias tail ends at dout (:407).  Activations are switched per layer
                  (phi_act[l], gam_act[l]); bias pointers and whole bias arrays may be NULL (include/ngpde.h:709).
  staging tile    s_rows, the largest of 128 / 96 / 64 rows of 68 floats that fits 160 KB beside n_mats = n_phi + n_gam staged
                  matrices of 16 KB and the kernels' static LDS (vmh_lds_bytes and vmh_geo_of, :1131-1150; static LDS of this build:
                  5 968 B for the half-tile kernels, 11 664 B for the tile-round ones):
                      n_mats 4, 5, 6, 7 -> 128 in both forms (7: 114 688 + 34 816 B);
                      n_mats 8          -> 96 with half tiles (131 072 + 26 112 + 5 968 <= 163 840), 64 in tile rounds
                                           (96 rows would need 168 848 B).
  ragged ends     padding rows of the last tile have sched.x < 0 (vctx_init, :196-205); N mod 32 <= 16 leaves the last tile's second
                  half tile without rows; t.inv = 1 / in-degree per ROW under mean, 0 for a row without in-edges (:205).
  geometry        both directions' tiles within kHaloCap = 96 staged rows and kSlotWidth = 32 entries per row; a wait list of at
                  most 63 tiles (persistent_plan.hip: build_wait_lists) -- ngpde_node_vmh_supported answers for all of it, and what
                  it accepts ngpde_node_vmh_create must build (section G).

Every case builds its handle with ngpde_graph_create_device and an explicit node order (tiles = consecutive 32-node runs of it, half
tiles = 16-node runs), drives the plan through the C ABI -- weights [in][out] as host arrays of device pointers, positions [N][pd] --
and compares every output with oracle.ngpde_oracle (vmh_conv, vmh_conv_backward, rk_solve, rk_adjoint) in float64, composed as in
test_node_vmh_gpu.oracle_solve_layers.  Every output (uT or usave, du0, every dW, every db) starts as NaN with a guard run behind it
that must come back intact; the plan's fault word must be 0 after every solve; the plan sums without atomics, so a second forward and
backward on the same plan must give the same bits (asserted once per section).

Inputs: weights N(0, 1) / sqrt(din), biases 0.3 N(0, 1), u0 and cotangents N(0, 1), positions uniform in [0, 1), dt = 0.05.
Tolerances are the project's (test_node_vmh_gpu.py, test_mp_gpu.check_grads): values 2e-4 * max|ref| + 1e-5, du0 5e-4 * max|ref| + 1e-4,
parameter gradients 5e-4 * max|ref| + 2e-4, over whole arrays.

Largest error of each section as a fraction of its bound, from the run on an MI355X (256 CUs; the module prints them when it is done,
pytest -s):  A 0.007 (dphi.weight[0])   B 0.001 (dgamma.weight[2])   C 0.003 (dgamma.weight[2])   D 0.010 (dphi.bias[0])
             E 0.010 (dphi.bias[1])     F 0.004 (dgamma.bias[2])     G compares no values.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from ngpde_amd.functional import _int_array, _ptr_array
from ngpde_amd.plans import _ode_desc
from oracle import ngpde_oracle as O
from test_edge_mlp_forms_gpu import (HALO_CAP, ROWS, SLOT_WIDTH, TileGraph, _release_graphs, graph, spread)  # noqa: F401
from test_gat_forms_gpu import both_ways
from test_gcn_forms_gpu import layout
from test_node_vmh_gpu import grad_accumulators, oracle_solve_layers

pytestmark = pytest.mark.gpu
DEV = "cuda"
HALF, VROUND, MAX_NBR = 16, 128, 63
GUARD, SENTINEL = 64, -1234.5
DT = 0.05
TILE_ROUNDS = 64                      # NGPDE_NODE_TILE_ROUNDS
WORST = {}                            # section -> (largest error / bound, what): printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for sec in sorted(WORST):
        print(f"\n[vmh forms] section {sec}: worst error / bound = {WORST[sec][0]:.3f} ({WORST[sec][1]})")


@pytest.fixture(autouse=True)
def _plan_switches_off(monkeypatch):
    for v in ("NGPDE_NO_VMH_NODE", "NGPDE_NO_VMH_ROUNDS"):      # the suite may run under one of these: every case names its form
        monkeypatch.delenv(v, raising=False)


# ---- graphs of chosen geometry ----------------------------------------------------------------------------------------------------

def window_edges(deg, rng, lo=0, w=16, no_out=()):
    """(s, t) in POSITIONS lo .. lo + len(deg) - 1: row p takes exactly deg[p - lo] in-edges from distinct positions p + o, o drawn
    from the 2 w nonzero offsets -w .. w (wrapping inside the range), never from a position in no_out.  With w = 16 a position is
    a candidate of 32 rows, so no out-degree exceeds 32 whatever the in-degrees are; a tile's foreign rows lie within w positions
    of it in both directions, so both halos stay within 32 + 2 w <= 96 for w <= 32."""
    deg = np.asarray(deg, dtype=np.int64)
    n = deg.size
    assert n > 2 * w and w <= 32
    offs = np.concatenate([np.arange(-w, 0), np.arange(1, w + 1)])
    banned = np.zeros(n, dtype=bool)
    banned[np.asarray(list(no_out), dtype=np.int64) - lo] = True
    S, T = [], []
    for p in np.flatnonzero(deg):
        cand = (p + offs) % n
        cand = cand[~banned[cand]]
        assert deg[p] <= cand.size, (p, deg[p], cand.size)
        S.append(rng.choice(cand, deg[p], replace=False))
        T.append(np.full(deg[p], p))
    cat = lambda a: np.concatenate(a).astype(np.int64) + lo if a else np.zeros(0, dtype=np.int64)
    return cat(S), cat(T)


def band_edges(n, d):
    """row p takes the d positions after it (wrapping): a ring (d = 1) or band"""
    p = np.repeat(np.arange(n, dtype=np.int64), d)
    return (p + np.tile(np.arange(1, d + 1), n)) % max(n, 1), p


def shuffled(s_pos, t_pos, n, rng):
    """positions -> nodes through a random node order, the COO list shuffled: (s, t, n, order) as VmhGraph takes them"""
    order = rng.permutation(n).astype(np.int32)
    perm = rng.permutation(s_pos.size)
    return order[s_pos][perm].astype(np.int64), order[t_pos][perm].astype(np.int64), n, order


def from_layout(*args, **kw):
    s, t, order = layout(*args, **kw)
    return s, t, order.size, order


class VmhGraph(TileGraph):
    """TileGraph + what the cases assert about it (per-half-tile and per-tile edge counts, both directions' halos and degrees, the
    number of tiles every tile neighbours) + positions and the oracle's graph"""

    def __init__(self, s, t, n, order):
        super().__init__(s, t, n, order)
        self.halo_t, self.din, self.halo_s, self.dout, _ = both_ways(self)
        at = np.zeros(self.n_tiles * ROWS, dtype=np.int64)
        at[:n] = np.bincount(self.t, minlength=n)[self.order]
        self.row_deg = at
        self.half_edges = at.reshape(-1, HALF).sum(1)
        pos = np.empty(n, dtype=np.int64)
        pos[self.order] = np.arange(n)
        a, b = pos[self.s] // ROWS, pos[self.t] // ROWS
        pairs = np.unique(np.concatenate([a * self.n_tiles + b, b * self.n_tiles + a])[np.concatenate([a != b, a != b])])
        self.nbr_tiles = np.bincount(pairs // self.n_tiles, minlength=self.n_tiles)
        self.out_deg = np.bincount(self.s, minlength=n)
        self.in_deg = np.bincount(self.t, minlength=n)
        self.x = np.random.default_rng(7 * n + self.E).random((n, 3)).astype(np.float32)
        self._og = {}

    def fits_both(self):
        return max(self.halo_t, self.halo_s) <= HALO_CAP and max(self.din, self.dout) <= SLOT_WIDTH and self.nbr_tiles.max(initial=0) <= MAX_NBR

    def positions(self, pd):
        return np.ascontiguousarray(self.x[:, :pd])

    def oracle(self, pd):
        if pd not in self._og:
            self._og[pd] = O.Graph(self.s, self.t, num_nodes=self.n, index_base=0, ndata={"x": self.positions(pd).T.astype(np.float64)})
        return self._og[pd]

    def rounds_of_units(self, unit_rows):
        return -(-self.row_deg.reshape(-1, unit_rows).sum(1) // VROUND)


def degree_graph(key, n, deg_of, seed, w=16, no_out=()):
    """a graph of n nodes whose POSITION p has in-degree deg_of(rng)[p] exactly (window_edges)"""
    def make():
        rng = np.random.default_rng(seed)
        deg = np.asarray(deg_of(rng), dtype=np.int64)
        assert deg.size == n
        g = VmhGraph(*shuffled(*window_edges(deg, rng, w=w, no_out=no_out), n, rng))
        assert np.array_equal(g.row_deg[:n], deg) and g.fits_both(), (g.halo_t, g.halo_s, g.din, g.dout)
        return g
    return graph(("vmh", key), make)


def half_tile_degrees(totals, n, rng):
    """in-degree per position from the edge count of every half tile (the last ones may be short or empty: N mod 32)"""
    deg = np.zeros(n, dtype=np.int64)
    for h, tot in enumerate(totals):
        lo, hi = h * HALF, min(n, (h + 1) * HALF)
        if hi > lo:
            deg[lo:hi] = spread(tot, hi - lo, rng)
        else:
            assert tot == 0
    return deg


# ---- models -----------------------------------------------------------------------------------------------------------------------

class Model:
    """phi and gamma as the ABI takes them -- weights [in][out], biases [out] or NULL -- and as the oracle does ((out x in), (out x 1)).
    null_bias: "all" (both bias arrays NULL) or a set of ("phi" | "gam", layer) whose pointer is NULL; their gradients are not asked for"""

    def __init__(self, pd, phi_dims, phi_acts, gam_dims, gam_acts, seed=0, null_bias=()):
        assert phi_dims[0] == 2 + pd and gam_dims[0] == 1 + phi_dims[-1] and gam_dims[-1] == 1
        assert len(phi_acts) == len(phi_dims) - 1 and len(gam_acts) == len(gam_dims) - 1 and phi_acts[-1] == gam_acts[-1] == "identity"
        self.pd, self.dims, self.acts, self.null_bias = pd, (list(phi_dims), list(gam_dims)), (list(phi_acts), list(gam_acts)), null_bias
        self.key = (pd, tuple(phi_dims), tuple(phi_acts), tuple(gam_dims), tuple(gam_acts), seed, null_bias if null_bias == "all" else tuple(sorted(null_bias)))
        rng = np.random.default_rng(1000 + seed)
        self.W, self.b = [], []
        for name, dims in zip(("phi", "gam"), self.dims):
            self.W.append([(rng.normal(size=(dims[l], dims[l + 1])) / np.sqrt(dims[l])).astype(np.float32) for l in range(len(dims) - 1)])
            bs = [(0.3 * rng.normal(size=dims[l + 1])).astype(np.float32) for l in range(len(dims) - 1)]
            self.b.append([None if (null_bias == "all" or (name, l) in null_bias) else v for l, v in enumerate(bs)])

    @property
    def n_mats(self):
        return len(self.acts[0]) + len(self.acts[1])

    def oracle_layers(self):
        return [[dict(weight=W.T.astype(np.float64), bias=None if b is None else b.astype(np.float64).reshape(-1, 1), act=a)
                 for W, b, a in zip(self.W[k], self.b[k], self.acts[k])] for k in (0, 1)]

    def abi_shape(self):
        ia = lambda k: _int_array([_lib.ACT[a] for a in self.acts[k]])
        return (len(self.acts[0]), _int_array(self.dims[0]), ia(0), len(self.acts[1]), _int_array(self.dims[1]), ia(1))


def tutorial(depth, pd=2, act="tanh", width=60, msg=40, seed=0):
    """docs/src/tutorials/VMH.md:75-83's MLPs at a given depth"""
    hid = [width] * (depth - 1)
    return Model(pd, [2 + pd] + hid + [msg], [act] * (depth - 1) + ["identity"], [1 + msg] + hid + [1], [act] * (depth - 1) + ["identity"], seed)


def supported(g, m, aggr):
    return _lib.load().ngpde_node_vmh_supported(g.ptr, 1, m.pd, *m.abi_shape(), _lib.AGGR[aggr])


def ode_flags(g, m, aggr):
    """the flags ngpde_ode_create reports for this right-hand side on this handle (a forward-only plan, destroyed at once)"""
    lib = _lib.load()
    pos = torch.as_tensor(g.positions(m.pd), device=DEV)
    d = _ode_desc(_lib.RHS_VMH, "euler", 1, DT, 0, width=1, pos_width=m.pd, aggr=_lib.AGGR[aggr], pos=pos.data_ptr(), n_phi=len(m.acts[0]),
                  phi_dims=m.dims[0], phi_acts=[_lib.ACT[a] for a in m.acts[0]], n_gamma=len(m.acts[1]), gamma_dims=m.dims[1],
                  gamma_acts=[_lib.ACT[a] for a in m.acts[1]])
    out, fl = C.c_void_p(), C.c_int32()
    _lib.check(lib.ngpde_ode_create(g.ptr, C.byref(d), C.byref(out), C.byref(fl)))
    _lib.check(lib.ngpde_ode_destroy(out))
    return fl.value


# ---- the plan through the C ABI ---------------------------------------------------------------------------------------------------

def nan_buffer(numel):
    buf = torch.full((numel + GUARD,), float("nan"), device=DEV)
    buf[numel:] = SENTINEL
    return buf


def taken(buf, shape):
    numel = int(np.prod(shape))
    assert bool((buf[numel:] == SENTINEL).all()), "guard run overwritten"
    return buf[:numel].reshape(shape).clone()


def inputs(g, seed, T=1):
    rng = np.random.default_rng(50 + seed)
    return rng.normal(size=g.n).astype(np.float32), rng.normal(size=(T, g.n)).astype(np.float32)


def run_plan(g, m, aggr, solver, n_steps, u0, R, save=None, with_backward=True, solves=1):
    """`solves` forward (+ backward) solves on ONE plan; save = (save_every, save_start) goes through the saveat entries.  Returns one
    dict of torch tensors per solve: out [T][N], du0 [N], dW / db [stack][layer] (None where not asked for)."""
    lib = _lib.load()
    assert supported(g, m, aggr) == 1
    N, T = g.n, R.shape[0]
    pos = torch.as_tensor(g.positions(m.pd), device=DEV)
    W = [[torch.as_tensor(w, device=DEV) for w in ws] for ws in m.W]
    b = [[None if v is None else torch.as_tensor(v, device=DEV) for v in bs] for bs in m.b]
    wp = [_ptr_array(ws) for ws in W]
    bp = [None if m.null_bias == "all" else _ptr_array(bs) for bs in b]
    ud, Rd = torch.as_tensor(u0, device=DEV), torch.as_tensor(R, device=DEV)
    plan = C.c_void_p()
    _lib.check(lib.ngpde_node_vmh_create(g.ptr, 1, m.pd, _lib.ptr(pos), *m.abi_shape(), _lib.AGGR[aggr], _lib.TABLEAU[solver], n_steps, DT,
                                         int(with_backward), C.byref(plan)))
    stream = _lib.current_stream()

    def no_fault():
        f = C.c_int32(-1)
        _lib.check(lib.ngpde_node_vmh_fault(plan, stream, C.byref(f)))
        assert f.value == 0, "the plan's launch gave up waiting for its neighbours"

    results = []
    try:
        for _ in range(solves):
            out = nan_buffer(T * N)
            if save is None:
                _lib.check(lib.ngpde_node_vmh_forward(plan, _lib.ptr(ud), wp[0], bp[0], wp[1], bp[1], _lib.ptr(out), stream))
            else:
                _lib.check(lib.ngpde_node_vmh_forward_saveat(plan, _lib.ptr(ud), wp[0], bp[0], wp[1], bp[1], save[0], save[1], _lib.ptr(out), stream))
            no_fault()
            res = dict(out=taken(out, (T, N)))
            if with_backward:
                du0 = nan_buffer(N)
                dW = [[nan_buffer(w.numel()) for w in ws] for ws in W]
                db = [[None if v is None else nan_buffer(v.numel()) for v in bs] for bs in b]
                dwp = [_ptr_array(x) for x in dW]
                dbp = [None if m.null_bias == "all" else _ptr_array(x) for x in db]
                if save is None:
                    _lib.check(lib.ngpde_node_vmh_backward(plan, wp[0], wp[1], _lib.ptr(Rd), _lib.ptr(du0), dwp[0], dbp[0], dwp[1], dbp[1], stream))
                else:
                    _lib.check(lib.ngpde_node_vmh_backward_saveat(plan, wp[0], wp[1], save[0], save[1], _lib.ptr(Rd), _lib.ptr(du0), dwp[0], dbp[0],
                                                                  dwp[1], dbp[1], stream))
                no_fault()
                res["du0"] = taken(du0, (N,))
                res["dW"] = [[taken(x, tuple(w.shape)) for x, w in zip(xs, ws)] for xs, ws in zip(dW, W)]
                res["db"] = [[None if x is None else taken(x, tuple(v.shape)) for x, v in zip(xs, bs)] for xs, bs in zip(db, b)]
            results.append(res)
    finally:
        torch.cuda.synchronize()
        _lib.check(lib.ngpde_node_vmh_destroy(plan))
    return results


def flat(res):
    out = [res["out"]]
    if "du0" in res:
        out += [res["du0"]] + [x for k in (0, 1) for x in res["dW"][k]] + [x for k in (0, 1) for x in res["db"][k] if x is not None]
    return out


def same_bits(a, b):
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb)
    for x, y in zip(fa, fb):
        assert torch.equal(x, y), "a second solve on the same plan gave other bits"


# ---- the float64 reference --------------------------------------------------------------------------------------------------------

_oracle = {}


def reference(key, g, m, aggr, solver, n_steps, u0, R, save=None):
    """out [T][N], du0 [N], dW / db [stack][layer] in float64 ([in][out] and [out], as the ABI lays them out); one computation per key"""
    key = (key, m.key, aggr, solver, n_steps, save)
    if key in _oracle:
        return _oracle[key]
    ophi, ogam = m.oracle_layers()
    og = g.oracle(m.pd)
    u = u0.astype(np.float64).reshape(1, -1)
    Rr = R.astype(np.float64)
    if save is None:
        uT, du0, gphi, ggam = oracle_solve_layers(ophi, ogam, og, u, solver, DT, n_steps, Rr[0].reshape(1, -1), aggr=aggr)
        states = [uT]
    else:       # segment by segment; the adjoint walks the segments backwards, adding each saved state's cotangent
        k, start = save
        tab = O.TABLEAUS[solver]
        gphi, ggam, vjp, accumulate = grad_accumulators(ophi, ogam)
        states, tapes, cur = [u] if start else [], [], u
        for _ in range(n_steps // k):
            cur, tape = O.rk_solve(lambda x: O.vmh_conv(x, ophi, ogam, og, aggr=aggr), cur, tab, DT, k)
            states.append(cur); tapes.append(tape)
        lam = np.zeros_like(u)
        for j in range(len(tapes) - 1, -1, -1):
            lam = O.rk_adjoint(vjp, tapes[j], lam + Rr[j + start].reshape(1, -1), tab, DT, accumulate)
        du0 = lam + Rr[0].reshape(1, -1) if start else lam
    ref = dict(out=np.concatenate(states, axis=0), du0=du0.reshape(-1),
               dW=[[L["weight"].T for L in gs] for gs in (gphi, ggam)],
               db=[[L["bias"].reshape(-1) if "bias" in L else None for L in gs] for gs in (gphi, ggam)])
    _oracle[key] = ref
    return ref


def compare(section, res, ref):
    """every output against float64 at the project's tolerances, whole arrays; the section's worst error / bound is kept"""
    def one(what, a, r, rtol, atol):
        a = a.detach().cpu().double().numpy()
        assert a.shape == r.shape, (what, a.shape, r.shape)
        bound = rtol * (np.abs(r).max() if r.size else 0.0) + atol
        err = float(np.abs(a - r).max()) if r.size else 0.0
        if err / bound > WORST.get(section, (-1.0, ""))[0]:
            WORST[section] = (err / bound, what)
        assert err <= bound, f"section {section}, {what}: max err {err:.3e} > {bound:.3e} ({err / bound:.2f} of the bound)"
    one("values", res["out"], ref["out"], 2e-4, 1e-5)
    if "du0" in res:
        one("du0", res["du0"], ref["du0"], 5e-4, 1e-4)
        for k, name in enumerate(("phi", "gamma")):
            for l, (a, r) in enumerate(zip(res["dW"][k], ref["dW"][k])):
                one(f"d{name}.weight[{l}]", a, r, 5e-4, 2e-4)
            for l, (a, r) in enumerate(zip(res["db"][k], ref["db"][k])):
                assert (a is None) == (r is None)
                if a is not None:
                    one(f"d{name}.bias[{l}]", a, r, 5e-4, 2e-4)


def check(section, key, g, m, aggr, solver, n_steps, save=None, with_backward=True, solves=1, seed=0):
    T = 1 if save is None else n_steps // save[0] + save[1]
    u0, R = inputs(g, seed, T)
    results = run_plan(g, m, aggr, solver, n_steps, u0, R, save=save, with_backward=with_backward, solves=solves)
    for r in results[1:]:
        same_bits(results[0], r)
    compare(section, results[0], reference(key, g, m, aggr, solver, n_steps, u0, R, save=save))


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_one_tile_form(g, m, aggr):
    assert 2 * g.n_tiles <= cu_count() and not ode_flags(g, m, aggr) & TILE_ROUNDS


# ---- A. edge rounds in the one-tile form ------------------------------------------------------------------------------------------

# edges of every half tile of 12 tiles (N = 379: the last half tile has 11 rows): tile 0 pairs 1 round with 4, tile 1 no edge with 3
# rounds, tile 4 four rounds with none; 512 = all 16 rows at in-degree 32
A_HALVES = [1, 512, 0, 257, 127, 128, 129, 256, 512, 0, 96, 300, 60, 130, 384, 90, 255, 100, 20, 200, 128, 385, 140, 70]
A_N = 12 * ROWS - 5


def graph_a():
    g = degree_graph("A", A_N, lambda rng: half_tile_degrees(A_HALVES, A_N, rng), seed=11)
    assert g.half_edges.tolist() == A_HALVES and {0, 1, 127, 128, 129, 256, 257, 512} <= set(g.half_edges.tolist())
    rounds = g.rounds_of_units(HALF).reshape(-1, 2)
    assert rounds[0].tolist() == [1, 4] and rounds[1].tolist() == [0, 3] and rounds[4].tolist() == [4, 0] and rounds.max() == 4
    assert g.row_deg[HALF:2 * HALF].tolist() == [SLOT_WIDTH] * HALF
    return g


@pytest.mark.parametrize("aggr", ["mean", "+"])
@pytest.mark.parametrize("solver,n_steps", [("tsit5", 2), ("euler", 3)])
def test_a_edge_rounds_of_half_tiles(solver, n_steps, aggr):
    g, m = graph_a(), tutorial(3)
    assert_one_tile_form(g, m, aggr)
    check("A", "A", g, m, aggr, solver, n_steps, solves=2 if (solver, aggr) == ("tsit5", "mean") else 1)


def test_a_forward_only_plan_through_multi_round_half_tiles():
    # with_backward = 0: no tape, so no `defer` either (p.tape_phi == nullptr, node_vmh.hip:427)
    g, m = graph_a(), tutorial(3)
    assert_one_tile_form(g, m, "mean")
    check("A", "A", g, m, "mean", "tsit5", 2, with_backward=False)


# ---- B. ragged ends and empty graphs ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edges", ["band", "none"])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 31, 32, 33, 48, 49])
def test_b_ragged_ends_and_graphs_without_edges(N, edges):
    d = min(N - 1, 6) if edges == "band" else 0

    def make():
        rng = np.random.default_rng(300 + N)
        g = VmhGraph(*shuffled(*band_edges(N, d), N, rng))
        assert g.E == N * d and g.n_tiles == -(-N // ROWS) and g.fits_both()
        assert g.half_edges.tolist() == [d * max(0, min(HALF, N - HALF * h)) for h in range(2 * g.n_tiles)]
        return g
    g = graph(("vmh B", N, edges), make)
    m = tutorial(3, width=24, msg=16, seed=N)
    assert_one_tile_form(g, m, "mean")
    check("B", ("B", N, edges), g, m, "mean", "tsit5", 1, solves=2 if N == 17 else 1)


B_N = 6 * ROWS - 9


def graph_b_mixed():
    """rows without in-edges and rows nobody reads among rows of in-degree 32: positions 3 k + 1 are isolated (in-degree 0, never a
    source), 3 k + 2 take 32 in-edges, the others 0 .. 5; sources from a window of 24 positions either way"""
    def deg_of(rng):
        deg = rng.integers(0, 6, B_N)
        deg[1::3], deg[2::3] = 0, SLOT_WIDTH
        return deg
    g = degree_graph("B mixed", B_N, deg_of, seed=21, w=24, no_out=range(1, B_N, 3))
    iso = g.order[1::3]
    assert (g.in_deg[iso] == 0).all() and (g.out_deg[iso] == 0).all() and (g.in_deg[g.order[2::3]] == SLOT_WIDTH).all()
    assert (g.in_deg[g.order[0::3]] == 0).any() and g.out_deg.max() <= SLOT_WIDTH
    return g


@pytest.mark.parametrize("aggr", ["mean", "+"])
def test_b_isolated_rows_among_rows_of_degree_32(aggr):
    g, m = graph_b_mixed(), tutorial(3, width=24, msg=16, seed=3)
    assert_one_tile_form(g, m, aggr)
    check("B", "B mixed", g, m, aggr, "euler", 2)


# ---- C. widths, depths, activations and biases ------------------------------------------------------------------------------------

# edges of the half tiles of 6 tiles (N = 189: the last half tile has 13 rows): one and two rounds mixed, in one tile too
C_HALVES = [96, 200, 130, 60, 256, 100, 129, 90, 40, 180, 128, 70]
C_N = 6 * ROWS - 3
I, R_, T_, S_ = "identity", "relu", "tanh", "sigmoid"
# name: (pd, phi_dims, phi_acts, gam_dims, gam_acts, null_bias); n_mats and the staging tile's s_rows in the half-tile form
C_TABLE = {
    "2+2 tutorial":       (2, [4, 60, 40], [T_, I], [41, 60, 1], [T_, I], ()),                                                  # 4 -> 128
    "2+2 widest":         (3, [5, 64, 63], [S_, I], [64, 64, 1], [T_, I], ()),                                                  # 4 -> 128
    "2+2 narrowest":      (1, [3, 1, 1], [T_, I], [2, 1, 1], [S_, I], ()),                                                      # 4 -> 128
    "3+2":                (2, [4, 48, 20, 9], [R_, T_, I], [10, 63, 1], [S_, I], ()),                                            # 5 -> 128
    "2+4":                (2, [4, 33, 17], [T_, I], [18, 48, 49, 15, 1], [S_, I, T_, I], ()),                                    # 6 -> 128
    "4+2":                (2, [4, 16, 64, 32, 31], [T_, I, S_, I], [32, 17, 1], [R_, I], ()),                                    # 6 -> 128
    "4+3 block edges":    (3, [5, 7, 33, 61, 13], [T_, S_, I, I], [14, 49, 16, 1], [I, T_, I], ()),                              # 7 -> 128
    "3+4":                (1, [3, 15, 63, 16], [I, T_, I], [17, 64, 32, 33, 1], [T_, R_, S_, I], ()),                            # 7 -> 128
    "4+4":                (2, [4, 64, 49, 17, 63], [S_, T_, I, I], [64, 64, 15, 33, 1], [T_, I, S_, I], ()),                     # 8 -> 96
    "3+3 no bias arrays": (2, [4, 32, 48, 16], [T_, S_, I], [17, 40, 24, 1], [S_, T_, I], "all"),                               # 6 -> 128
    "3+3 null pointers":  (2, [4, 32, 48, 16], [T_, S_, I], [17, 40, 24, 1], [S_, T_, I], (("phi", 0), ("phi", 2), ("gam", 1))),  # 6 -> 128
}


def graph_c():
    g = degree_graph("C", C_N, lambda rng: half_tile_degrees(C_HALVES, C_N, rng), seed=31)
    assert g.half_edges.tolist() == C_HALVES and sorted(set(g.rounds_of_units(HALF).tolist())) == [1, 2]
    return g


def test_c_table_covers_what_it_claims():
    shapes = {(len(v[2]), len(v[4])) for v in C_TABLE.values()}
    assert {(2, 4), (4, 2), (3, 4), (2, 2)} <= shapes and {a + b for a, b in shapes} == {4, 5, 6, 7, 8}
    widths = {w for v in C_TABLE.values() for w in v[1] + v[3]}
    assert {1, 15, 16, 17, 32, 33, 48, 49, 63, 64} <= widths and {v[0] for v in C_TABLE.values()} == {1, 2, 3}
    hidden = [a for v in C_TABLE.values() for acts in (v[2], v[4]) for a in acts[:-1]]
    assert {I, R_, T_, S_} <= set(hidden) and any(v[2][:-1] != v[4][:-1] for v in C_TABLE.values())


@pytest.mark.parametrize("name", list(C_TABLE))
def test_c_widths_depths_activations_and_biases(name):
    pd, pdims, pacts, gdims, gacts, null_bias = C_TABLE[name]
    g = graph_c()
    m = Model(pd, pdims, pacts, gdims, gacts, seed=len(name), null_bias=null_bias if null_bias == "all" else frozenset(null_bias))
    assert_one_tile_form(g, m, "mean")
    aggr, solver, n_steps = ("+", "euler", 2) if name in ("2+4", "4+3 block edges") else ("mean", "tsit5", 1)
    check("C", "C", g, m, aggr, solver, n_steps, solves=2 if name == "4+4" else 1)


# ---- D. geometry limits -----------------------------------------------------------------------------------------------------------

def nbr_graph(n_far):
    """66 tiles; row r of tile 0 takes one in-edge from a row of tile 1 + 2 r and one from tile 2 + 2 r while they are below
    1 + n_far (a row of its own tile otherwise); every other row takes two rows of its own tile: tile 0 neighbours n_far tiles"""
    def make():
        rng = np.random.default_rng(60 + n_far)
        n_tiles = 66
        n = n_tiles * ROWS
        S, T = [], []
        for p in range(n):
            k = p // ROWS
            for j in range(2):
                far = 1 + 2 * p + j
                if k == 0 and far < 1 + n_far:
                    S.append(far * ROWS + int(rng.integers(ROWS)))
                else:
                    S.append(k * ROWS + (p % ROWS + 1 + 5 * j) % ROWS)
                T.append(p)
        g = VmhGraph(*shuffled(np.asarray(S), np.asarray(T), n, rng))
        assert g.n_tiles == n_tiles and g.nbr_tiles[0] == n_far and g.nbr_tiles[1:].max() == 1
        assert g.halo[0] == ROWS + n_far and max(g.halo_t, g.halo_s) <= HALO_CAP and max(g.din, g.dout) <= SLOT_WIDTH
        return g
    return graph(("vmh nbr", n_far), make)


def reach_edges(n_tiles, ragged, hot, rng, lo=0):
    """(s, t) in positions lo ..: every row takes 1 .. 3 rows of its own tile; a tile in `hot` also takes ALL 64 rows of the two tiles
    next to it, one edge each on a row chosen at random -- 96 staged rows by target --, the other tiles up to 10 of them.  A tile's
    rows are read by the two tiles next to it only, so the by-source halos stay below 96 unless two hot tiles share a neighbour.
    (test_edge_mlp_forms_gpu.halo_graph(96) draws its foreign sources from the whole graph: its by-source halos reach ~ 160 rows,
    which this plan, unlike the message-MLP kernels, does not take.)"""
    n = n_tiles * ROWS - ragged
    S, T = [], []
    for k in range(n_tiles):
        rows = np.arange(k * ROWS, min(n, (k + 1) * ROWS))
        for p in rows:
            d = min(int(rng.integers(1, 4)), rows.size - 1)
            S.append(rng.choice(rows[rows != p], d, replace=False))
            T.append(np.full(d, p))
        near = np.concatenate([np.arange(j * ROWS, min(n, (j + 1) * ROWS)) for j in sorted({(k - 1) % n_tiles, (k + 1) % n_tiles} - {k})])
        F = near.size if k in hot else int(rng.integers(0, 11))
        S.append(rng.choice(near, F, replace=False))
        T.append(rng.choice(rows, F))
    return np.concatenate(S).astype(np.int64) + lo, np.concatenate(T).astype(np.int64) + lo


REACH_TILES, REACH_RAGGED, REACH_HOT = 12, 5, (2, 7)


def reach_graph(transpose):
    def make():
        rng = np.random.default_rng(64)
        s, t = reach_edges(REACH_TILES, REACH_RAGGED, REACH_HOT, rng)
        return VmhGraph(*shuffled(*((t, s) if transpose else (s, t)), REACH_TILES * ROWS - REACH_RAGGED, rng))
    return graph(("vmh reach", transpose), make)


def halo_both_ways():
    """reach_edges on tiles 0 .. 11 and the transpose of another draw on tiles 12 .. 23: 96 staged rows in both directions"""
    def make():
        rng = np.random.default_rng(65)
        n1 = REACH_TILES * ROWS
        a = reach_edges(REACH_TILES, 0, REACH_HOT, rng)
        b = reach_edges(REACH_TILES, REACH_RAGGED, REACH_HOT, rng, lo=n1)
        return VmhGraph(*shuffled(np.concatenate([a[0], b[1]]), np.concatenate([a[1], b[0]]), 2 * n1 - REACH_RAGGED, rng))
    return graph(("vmh halo both",), make)


def hub_rows_graph():
    """tiles 0 .. 3: positions 5 k + 2 take 32 in-edges and are nobody's source; tiles 4 .. 7: the transpose of such a graph, so
    positions there have out-degree 32 and in-degree 0"""
    def make():
        rng = np.random.default_rng(71)
        n1 = 4 * ROWS
        parts = []
        for lo in (0, n1):
            deg = rng.integers(1, 5, n1)
            deg[2::5] = SLOT_WIDTH
            parts.append(window_edges(deg, rng, lo=lo, w=24, no_out=range(lo + 2, lo + n1, 5)))
        s = np.concatenate([parts[0][0], parts[1][1]])
        t = np.concatenate([parts[0][1], parts[1][0]])
        g = VmhGraph(*shuffled(s, t, 2 * n1, rng))
        ins, outs = g.order[2:n1:5], g.order[n1 + 2::5]
        assert (g.in_deg[ins] == SLOT_WIDTH).all() and (g.out_deg[ins] == 0).all()
        assert (g.out_deg[outs] == SLOT_WIDTH).all() and (g.in_deg[outs] == 0).all()
        return g
    return graph(("vmh hub rows",), make)


def graph_d(kind):
    if kind == "halo by target":
        g = reach_graph(False)
        assert g.halo_t == HALO_CAP and g.halo_s < HALO_CAP and (g.halo[list(REACH_HOT)] == HALO_CAP).all()
    elif kind == "halo by source":
        g = reach_graph(True)
        assert g.halo_s == HALO_CAP and g.halo_t < HALO_CAP
    elif kind == "halo both ways":
        g = halo_both_ways()
        assert g.halo_t == HALO_CAP and g.halo_s == HALO_CAP
    elif kind == "63 neighbour tiles":
        g = nbr_graph(MAX_NBR)
    elif kind == "hub rows":
        g = hub_rows_graph()
    elif kind == "self loops":
        g = graph(("vmh D", kind), lambda: VmhGraph(*from_layout(8, 3, 81, self_edges=40)))
        assert (g.s == g.t).sum() == 40
    else:
        g = graph(("vmh D", kind), lambda: VmhGraph(*from_layout(8, 3, 82, dup=60)))
        assert np.unique(np.stack([g.s, g.t]), axis=1).shape[1] == g.E - 60
    assert g.fits_both(), (g.halo_t, g.halo_s, g.din, g.dout, g.nbr_tiles.max())
    return g


@pytest.mark.parametrize("kind", ["halo by target", "halo by source", "halo both ways", "63 neighbour tiles", "hub rows", "self loops",
                                  "repeated edges"])
def test_d_geometry_limits(kind):
    g, m = graph_d(kind), tutorial(2)
    aggr = "+" if kind in ("hub rows", "repeated edges") else "mean"
    assert supported(g, m, aggr) == 1
    check("D", ("D", kind), g, m, aggr, "tsit5", 1, solves=2 if kind == "halo both ways" else 1)


# ---- E. tile rounds ---------------------------------------------------------------------------------------------------------------

# edges of a tile, by tile index mod 12: no round, one .. eight (1 024 = every row at in-degree 32); any three tiles in a row hold a
# multi-round one
E_TILES = [0, 129, 40, 300, 128, 513, 90, 1024, 96, 640, 20, 257]
E_MODELS = {
    "3+3": lambda: tutorial(3, width=16, msg=12, seed=5),                                                                      # 6 -> s_rows 128
    "2+4": lambda: Model(3, [5, 16, 9], [T_, I], [10, 16, 12, 8, 1], [S_, T_, I, I], seed=6),                                     # 6 -> 128
    "4+4": lambda: Model(2, [4, 12, 16, 8, 15], [T_, S_, T_, I], [16, 16, 10, 12, 1], [T_, T_, S_, I], seed=7),                  # 8 -> 64
}


def graph_e(which):
    cus = cu_count()
    n_tiles, ragged = {"one turn": (cus // 2 + 1, 13), "two turns, uneven": (2 * cus - 3, 20), "three turns": (2 * cus + 1, 7)}[which]
    n = n_tiles * ROWS - ragged

    def deg_of(rng):
        deg = np.zeros(n, dtype=np.int64)
        for k in range(n_tiles):
            lo, hi = k * ROWS, min(n, (k + 1) * ROWS)
            deg[lo:hi] = spread(min(E_TILES[k % len(E_TILES)], (hi - lo) * SLOT_WIDTH), hi - lo, rng)
        return deg
    g = degree_graph(("E", which, cus), n, deg_of, seed=90 + n_tiles)
    per_tile = g.row_deg.reshape(-1, ROWS).sum(1)
    assert g.n_tiles == n_tiles and 2 * n_tiles > cus and per_tile[:12].tolist() == E_TILES and n % ROWS == ROWS - ragged
    rounds = g.rounds_of_units(ROWS)
    assert {0, 1, 2, 3, 5, 8} <= set(rounds.tolist())
    grid = min(n_tiles, cus)
    turns = -(-n_tiles // grid)
    assert turns == {"one turn": 1, "two turns, uneven": 2, "three turns": 3}[which]
    if which == "two turns, uneven":     # workgroups grid - 3 .. grid - 1 walk one tile, the others two; multi-round tiles in both kinds
        assert n_tiles - grid == grid - 3 and rounds[grid - 3:grid].max() > 1 and rounds[grid:].max() > 1 and rounds[:grid - 3].max() > 1
    return g


@pytest.mark.parametrize("which,model,aggr,solver,n_steps", [
    ("one turn", "3+3", "mean", "tsit5", 1),
    ("one turn", "4+4", "+", "euler", 2),
    ("two turns, uneven", "2+4", "mean", "tsit5", 1),
    ("two turns, uneven", "4+4", "mean", "euler", 2),
    ("three turns", "3+3", "+", "euler", 2),
])
def test_e_tile_rounds(which, model, aggr, solver, n_steps, monkeypatch):
    g, m = graph_e(which), E_MODELS[model]()
    assert max(max(d) for d in m.dims) <= 16
    assert supported(g, m, aggr) == 1 and ode_flags(g, m, aggr) & TILE_ROUNDS        # the regime, from the plan
    monkeypatch.setenv("NGPDE_NO_VMH_ROUNDS", "1")
    assert supported(g, m, aggr) == 0                                                # ... and without tile rounds nobody takes this handle
    monkeypatch.delenv("NGPDE_NO_VMH_ROUNDS")
    check("E", ("E", which), g, m, aggr, solver, n_steps, solves=2 if which == "one turn" and model == "4+4" else 1)


# ---- F. saveat through multi-round tiles ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,solver,n_steps,save_every,save_start", [
    ("half tiles", "tsit5", 2, 1, 1),
    ("half tiles", "euler", 4, 2, 0),
    ("tile rounds", "euler", 4, 2, 1),
    ("tile rounds", "tsit5", 2, 1, 0),
])
def test_f_saveat_through_multi_round_tiles(form, solver, n_steps, save_every, save_start):
    if form == "half tiles":
        g, m = graph_a(), tutorial(3)
        assert_one_tile_form(g, m, "mean")
    else:
        g, m = graph_e("one turn"), E_MODELS["3+3"]()
        assert ode_flags(g, m, "mean") & TILE_ROUNDS
    check("F", ("F", form), g, m, "mean", solver, n_steps, save=(save_every, save_start), solves=2 if (form, save_every) == ("tile rounds", 2) else 1)


# ---- G. `supported` and `create` must agree ---------------------------------------------------------------------------------------

def test_g_supported_implies_create():
    # tile 0's 32 rows take two in-edges each from rows of 64 distinct tiles: both halos fit (96 staged rows by target), every degree
    # is 2, but tile 0's wait list would hold 64 tiles -- one more than the polling wave has lanes for (node_persistent_setup)
    lib = _lib.load()
    g, m = nbr_graph(64), tutorial(2)
    assert g.halo[0] == HALO_CAP and g.halo_t == HALO_CAP and g.halo_s <= HALO_CAP and g.nbr_tiles[0] == 64
    sup = supported(g, m, "mean")
    pos = torch.as_tensor(g.positions(m.pd), device=DEV)
    plan = C.c_void_p()
    st = lib.ngpde_node_vmh_create(g.ptr, 1, m.pd, _lib.ptr(pos), *m.abi_shape(), _lib.AGGR["mean"], _lib.TABLEAU["tsit5"], 1, DT, 1, C.byref(plan))
    try:
        assert (st == _lib.OK) == bool(plan.value)
        assert sup == 0 or st == _lib.OK, "ngpde_node_vmh_supported accepted a graph ngpde_node_vmh_create refuses"
        assert sup == 0 and st == _lib.ERR_UNSUPPORTED
    finally:
        _lib.check(lib.ngpde_node_vmh_destroy(plan))
    assert supported(nbr_graph(MAX_NBR), m, "mean") == 1          # ... and one tile fewer is the plan's (solved in section D)
    # NeuralODE(VMHConv) on these edges: solved and differentiated by whichever solver the library picks for its own node order
    pts = torch.as_tensor(g.positions(2).T.copy(), device=DEV)
    gg = ng.GNNGraph(g.s, g.t, num_nodes=g.n, index_base=0, ndata={"x": pts})
    phi = ng.Chain(ng.Dense(4, 60, "tanh"), ng.Dense(60, 40))
    gam = ng.Chain(ng.Dense(41, 60, "tanh"), ng.Dense(60, 1))
    node = ng.NeuralODE(ng.VMHConv(phi, gam, initialgraph=gg), solver="tsit5", n_steps=1, dt=DT)
    ps, st_ = ng.setup(2, node)
    ps = ng.to_device(ps, DEV)
    leaves = [v.requires_grad_(True) for sub in ps.values() for lp in sub.values() for v in lp.values()]
    u = torch.randn(1, g.n, device=DEV, requires_grad=True)
    out, _ = node(u, ps, st_)
    out.square().sum().backward()
    assert torch.isfinite(out).all() and torch.isfinite(u.grad).all() and all(torch.isfinite(v.grad).all() for v in leaves)


def test_g_gat_supported_implies_create():
    # ngpde_node_gat_create builds the same wait lists (node_gat_plan.hip): the same graph, the same contract
    lib = _lib.load()
    g = nbr_graph(64)
    sup = lib.ngpde_node_gat_supported(g.ptr, 64, 4, 16)
    plan = C.c_void_p()
    st = lib.ngpde_node_gat_create(g.ptr, 4, 16, 0.2, _lib.ACT["relu"], _lib.TABLEAU["euler"], 1, DT, 0, C.byref(plan))
    try:
        assert sup == 0 or st == _lib.OK, "ngpde_node_gat_supported accepted a graph ngpde_node_gat_create refuses"
        assert sup == 0 and st == _lib.ERR_UNSUPPORTED
    finally:
        _lib.check(lib.ngpde_node_gat_destroy(plan))
    assert lib.ngpde_node_gat_supported(nbr_graph(MAX_NBR).ptr, 64, 4, 16) == 1
