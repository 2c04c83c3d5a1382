"""The persistent GCN solver against float64 at its geometry caps.

ngpde_node_gcn2_create[_batch] (csrc/node.hip: node_create) solves du/dt = Chain(GCNConv(d => d, act), GCNConv(d => d, act))(u) with
ONE forward launch and ONE adjoint launch (csrc/node_persistent.hip, persistent_gcn_tile.h, persistent_sync.h) whose 32-row tiles
hand their rows over through per-tile phase flags.  Which kernels run is decided by node_persistent_mode (node_persistent.hip:1601),
restated:
  0  no persistent plan: NGPDE_NO_PERSISTENT=1, d != 64 (16 / 32 are widened onto 64 first, node.hip:572), or a handle that is not
     fused_prescaled_supported (gcn_fused.hip:859: self loops and halo_ok in BOTH directions); weights in one direction only.
     resident = CUs x the smallest occupancy of the instantiations the plan may launch (2 on an MI355X: every kernel's LDS is held to
     80 KB - 64 by a static_assert, node_persistent.hip:200, :302, :661, :1157, :1338).
  1  one tile per workgroup, tiles <= resident: node_fwd_persistent_kernel<ACT, TAPE, WGT> (:53), node_bwd_persistent_kernel<ACT,
     WGT> (:655); ACT = RELU (sign masks) or -1 (any other activation: the z tape), TAPE = the plan has a backward.  Weighted
     handles (WGT) while tiles <= CUs x the WGT kernels' occupancy and NGPDE_WEIGHTED_TILE_ROUNDS is not 1.
  2  tile pairs, resident < tiles <= 2 resident, unweighted, relu when a backward is asked for, neither NGPDE_NO_TILE_PAIRS=1 (which
     returns 0 for EVERY graph beyond resident -- "the old forms", docs/DESIGN_ROUNDS_1_4.md:497 -- not tile rounds) nor
     NGPDE_TILE_ROUNDS=1: node_*_persistent2_kernel<.., PAIR = true> (:569, :901), workgroup b holding tiles t and t + ceil(tiles / 2)
     (node_persistent_setup, persistent_plan.hip:319).
  3  tile rounds, up to kMaxTileRounds = 8 (weighted: 3) tiles per workgroup taking turns, K = ceil(tiles / resident)
     (node_persistent_rounds, :1620): node_*_persistentKP_kernel (:299, :1333), weighted handles node_*_persistentK_kernel (:197, :1152).
  A batch of `members` same-structure graphs (create_batch) runs mode 1 with relu only, two members per workgroup on
  node_*_persistent2_kernel<.., PAIR = false>, an odd last member alone; NGPDE_NO_INTERLEAVE=1: member after member on the one-tile
  kernels (node.hip:514).
The caps: kHaloCap = 96 staged rows and kSlotWidth = 32 list entries per row (csrc/edge_mlp_forms.h) in both directions, or the handle is
not halo_ok; kNbrStride - 1 = 63 tiles in a wait list (persistent_sync.h:19; build_wait_lists, persistent_plan.hip:50), or
node_persistent_setup returns NGPDE_ERR_UNSUPPORTED and node_create keeps the pre-scaled replayed plan (node.hip:481).  The self
loop is not a list entry (the kernels add the own row after the slots, persistent_gcn_tile.h:231), so a row at the slot cap has 32
constructed in-edges, 33 terms with the loop, and the first row beyond it 33.  A handle beyond a halo or slot cap goes to the hub
geometry (<.., HUB = true>, node.hip:458) where ngpde_hub_partition_host accepts it.

Sections and the instantiations they reach (every plan's flag word is asserted BEFORE anything is compared):
  A  one tile per workgroup, unweighted: <RELU, true> + bwd<RELU>; <-1, true> + bwd<-1> (tanh, sigmoid); <RELU / -1, false> (forward-only
     plans); graphs of 24 tiles with a ragged last tile at 96 staged rows by target / by source / both, rows at the slot cap by
     target / by source (rows 0 and 31 of a tile, the last real row of the ragged tile), tile 0 waiting for 63 tiles, tiles that
     wait for nobody (block diagonal; loops only), N = 1 / 31 / 32 / 33 / 65; the own-first tables on and off; d = 16 / 32 widened.
  B  one thing beyond a cap -- a 33-edge row, a 97-row halo, a 64-tile wait list: HUB_GEOMETRY or the replayed plan, by the flags.
  C  weighted handles (GcnGraph wmode "quirk"): <.., WGT = true> one-tile kernels; under NGPDE_WEIGHTED_TILE_ROUNDS=1 the K kernels, K = 1.
  D  batches of 2 and 3 members, interleaved and member by member.
  E  tile counts resident, resident + 1, 2 resident, 2 resident + 1 (resident = 2 x CUs): modes 1, 2, 2, 3 (K = 3); resident + 1 under
     NGPDE_TILE_ROUNDS=1 (K = 2, one workgroup with a lone tile) and under NGPDE_NO_TILE_PAIRS=1 (mode 0: the replayed plan).  Relu,
     Tsit5 x 1 and Euler x 2 steps (16 k to 33 k nodes: the numpy oracle's Tsit5 step takes a few seconds there).

Every case builds its handle with an explicit node order (test_node_gcn_forms_host.py holds the constructors and asserts their
geometry without a GPU), asserts the regime from the host geometry and the library's halo_ok, drives the plan through the C entry
points with uT, du0, dW1, db1, dW2, db2 starting as NaN in front of guard words, requires ngpde_node_fault == 0 after the forward and
after the backward, compares everything with the oracle's float64 gcn2_rhs / rk_solve / rk_adjoint (weighted: gcn_conv with
use_edge_weight) and solves a second time on the same plan: every output bit for bit (slabs per tile or workgroup, summed in a
fixed order by reduce4_slabs_kernel, node.hip:115; no atomics).  dt = 0.1, Tsit5 x 2 and Euler x 3 steps (section E: see above).

Tolerances are test_node_persistent_plan_against_oracle's, over whole arrays in the max norm: u(T) 2e-4 * max|ref| + 1e-5, du0
5e-4 * max|ref| + 1e-4, dW and db 5e-4 * max|ref| + 1e-3.  Relu: graphs of up to 33 nodes redraw their inputs until no float64
pre-activation lies within 1e-5 * max|z| of zero; for larger ones no draw can pass (test_node_gcn_forms_host.KINK_FREE_CASES has
the counts), and they compare every entry all the same.  On an MI355X (256 CUs) every case stays below 0.003 of its bounds except
four relu solves in which float32 takes the other branch of a relu whose float64 pre-activation is within rounding of zero.  There
the REPLAYED plan (NGPDE_NO_PERSISTENT=1, tied to float64 by test_gcn_forms_gpu.py section E) misses float64 by the same amount --
its u(T) and du0 are the persistent plan's bit for bit -- so, and only there, an output's bound is twice the replayed plan's
measured error (RAISED), and the case also requires u(T) and du0 to equal the replayed plan's bits and the parameter gradients to
agree with it as test_node_persistent_tile_pairs_beyond_512_tiles asks.  Measured max errors, persistent = replayed to three digits
(suite bound in brackets):
    D  A6, 3 members, Tsit5 x 2        du0 1.682e-2 (2.594e-3)  dW1 4.414e-1 (7.449e-3)  db1 2.317e-1 (1.385e-2)
    E  512 tiles, Euler x 2            du0 2.891e-3 (2.496e-3)  db1 1.583e-2 (1.401e-2)  dW2 7.542e-2 (1.608e-2)  db2 8.249e-2 (2.064e-2)
    E  513 tiles, Tsit5 x 1 (3 plans)  du0 1.739e-2 (2.483e-3)  dW1 6.371e-2 (6.160e-3)  db1 5.913e-2 (6.342e-3)  dW2 2.385e-1 (8.125e-3)
                                       db2 3.113e-1 (1.041e-2)
    E  1 025 tiles, Tsit5 x 1          du0 8.473e-3 (2.621e-3)  dW1 1.393e-1 (7.078e-3)  db1 9.389e-2 (1.275e-2)
Every other output of these solves keeps the suite's bound (dW1 of the 512-tile Euler solve at 1.358e-2 of 1.364e-2).  Both graphs
of section B's first test are accepted by ngpde_hub_partition_host and run in the hub geometry.  The module prints each comparison
and each section's largest error / bound (pytest -s).
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from oracle import ngpde_oracle as O
from test_mp_gpu import close
from test_edge_mlp_forms_gpu import HALO_CAP, ROWS, SLOT_WIDTH, _release_graphs, graph  # noqa: F401
from test_gat_forms_gpu import both_ways
from test_gcn_forms_gpu import GcnGraph, Out, halo_ok
from test_gcn_gpu import _oracle_node_with_seed, _oracle_weighted_node, needs_persistent_plan
from test_hub_partition import partition
import test_node_gcn_forms_host as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
PRESCALED, SIGN_MASKS, PFWD, PBWD, TILE_PAIRS, TILE_ROUNDS, WIDENED, HUB_GEOMETRY, OWN_FIRST = 1, 2, 8, 16, 32, 64, 128, 256, 512
FORMS = TILE_PAIRS | TILE_ROUNDS | HUB_GEOMETRY
WORST = {}                            # section -> (largest error / bound, what)


@pytest.fixture(scope="module", autouse=True)
def _report_worst():
    yield
    for sec in sorted(WORST):
        print(f"\n[node gcn forms] section {sec}: worst error / bound = {WORST[sec][0]:.3f} ({WORST[sec][1]})")


@pytest.fixture(autouse=True)
def _persistent_plan(monkeypatch):
    needs_persistent_plan(monkeypatch)      # skips under NGPDE_NO_HALO=1; lifts the plan-selecting switches the suite may run under


# ---- handles -----------------------------------------------------------------------------------------------------------------------

def make_handle(key, build, wmode=None):
    def make():
        s, t, n, order = build()
        g = GcnGraph(s, t, n, order, loops=True, wmode=wmode, seed=4000 + n)
        g.host, g.geo = (s, t, n, order), H.geometry(s, t, n, order)
        return g
    return graph(("node gcn", key, wmode), make)


def handle(name, wmode=None):
    return make_handle(name, H.CASES[name][0], wmode)


def assert_regime(g, name=None):
    """the host geometry the case claims, and the library's halo_ok in both directions against it"""
    geo = g.geo
    if name is not None:
        H.assert_geometry(name, geo)
    assert both_ways(g) == (geo["halo_t"], geo["din"] - 1, geo["halo_s"], geo["dout"] - 1, geo["n_tiles"])
    assert halo_ok(g, 0) == (geo["halo_t"] <= HALO_CAP and geo["din"] - 1 <= SLOT_WIDTH), geo
    assert halo_ok(g, 1) == (geo["halo_s"] <= HALO_CAP and geo["dout"] - 1 <= SLOT_WIDTH), geo


def assert_flags(flags, on, off, what=""):
    assert flags & on == on and not flags & off, f"flags {flags:#x}: expected {on:#x} set and {off:#x} clear {what}"


# ---- the plan through the C entry points -------------------------------------------------------------------------------------------

def run_plan(g, d, act, tab, n_steps, params, u0, R, members=1, with_backward=True, solves=2):
    """(the plan's flag word, one dict of outputs per solve) -- u0 and R are (d x members N), the plan's arrays [members N][d]"""
    lib = _lib.load()
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)
    w = [dv(p["weight"].T) for p in params]              # (out x in) column-major = [in][out]
    b = [dv(p["bias"].reshape(-1)) for p in params]
    ud, Rd = dv(u0.T), dv(R.T)
    rows = members * g.n
    plan, fl = C.c_void_p(), C.c_int32()
    args = (d, _lib.ACT[act], _lib.TABLEAU[tab], n_steps, H.DT, int(with_backward), C.byref(plan))
    if members == 1:
        _lib.check(lib.ngpde_node_gcn2_create(g.ptr, *args))
    else:
        _lib.check(lib.ngpde_node_gcn2_create_batch(g.ptr, members, *args))
    stream = _lib.current_stream()

    def no_fault(when):
        f = C.c_int32(-1)
        _lib.check(lib.ngpde_node_fault(plan, stream, C.byref(f)))
        assert f.value == 0, f"the {when} launch gave up waiting for its neighbours"

    results = []
    try:
        _lib.check(lib.ngpde_node_flags(plan, C.byref(fl)))
        for _ in range(solves):
            outs = dict(uT=Out(rows, d))
            _lib.check(lib.ngpde_node_gcn2_forward(plan, _lib.ptr(ud), _lib.ptr(w[0]), _lib.ptr(b[0]), _lib.ptr(w[1]), _lib.ptr(b[1]),
                                                   _lib.ptr(outs["uT"].v), stream))
            no_fault("forward")
            if with_backward:
                outs.update(du0=Out(rows, d), dW1=Out(d, d), db1=Out(d), dW2=Out(d, d), db2=Out(d))
                _lib.check(lib.ngpde_node_gcn2_backward(plan, _lib.ptr(Rd), *[_lib.ptr(outs[k].v) for k in ("du0", "dW1", "db1", "dW2", "db2")],
                                                        stream))
                no_fault("backward")
            torch.cuda.synchronize()
            assert all(o.intact() for o in outs.values()), "a solve wrote past one of its outputs"
            results.append({k: o.v.clone() for k, o in outs.items()})
    finally:
        torch.cuda.synchronize()
        _lib.check(lib.ngpde_node_destroy(plan))
    return fl.value, results


# ---- inputs and the float64 reference, one computation per key ---------------------------------------------------------------------

_inputs, _refs = {}, {}


def inputs(key, g, d, act, seed, solves, members=1):
    """(params, u0, R): relu on the graphs that can meet it follows the redraw rule (H.kink_free_draw), every other case takes the
    seed's own draw"""
    k = (key, d, act == "relu", members, solves, g.wmode)
    if k not in _inputs:
        if act == "relu" and key in H.KINK_FREE_CASES:
            _inputs[k] = H.kink_free_draw(g.host, d, seed, solves, members, g.w if g.wmode else None)[:3]
        else:
            _inputs[k] = H.draw(g.n, d, seed, members)
    return _inputs[k]


def reference(key, g, d, act, tab, n_steps, params, u0, R, members):
    k = (key, g.wmode, d, act, tab, n_steps, members)
    if k not in _refs:
        oracle = _oracle_weighted_node if g.wmode else _oracle_node_with_seed
        og, n = g.oracle(), g.n
        uT, du0 = [], []
        dW, db = [np.zeros((d, d)), np.zeros((d, d))], [np.zeros(d), np.zeros(d)]
        for m in range(members):
            sl = slice(m * n, (m + 1) * n)
            a, c, acc = oracle(params, og, u0[:, sl], R[:, sl], O.TABLEAUS[tab], H.DT, n_steps, act)
            uT.append(a.T)
            du0.append(c.T)
            for j in range(2):
                dW[j] += acc[j]["weight"].T
                db[j] += acc[j]["bias"].reshape(-1)
        _refs[k] = dict(uT=np.concatenate(uT), du0=np.concatenate(du0), dW1=dW[0], db1=db[0], dW2=dW[1], db2=db[1])
    return _refs[k]


TOL = dict(uT=(2e-4, 1e-5), du0=(5e-4, 1e-4), dW1=(5e-4, 1e-3), db1=(5e-4, 1e-3), dW2=(5e-4, 1e-3), db2=(5e-4, 1e-3))
# (case, members, tableau, steps) -> {output: the REPLAYED plan's measured max error against float64}: see the module docstring.
# Section E's keys hold for resident = 512 (256 CUs); on another device the graphs, and with them the draws, are other ones.
RAISED = {
    ("A6 63 neighbours", 3, "tsit5", 2): dict(du0=1.682e-2, dW1=4.414e-1, db1=2.317e-1),
    (("E", 512), 1, "euler", 2): dict(du0=2.891e-3, db1=1.583e-2, dW2=7.542e-2, db2=8.249e-2),
    (("E", 513), 1, "tsit5", 1): dict(du0=1.739e-2, dW1=6.371e-2, db1=5.913e-2, dW2=2.385e-1, db2=3.113e-1),
    (("E", 1025), 1, "tsit5", 1): dict(du0=8.473e-3, dW1=1.393e-1, db1=9.389e-2),
}


def compare(section, what, res, ref, raised=None):
    bounds = {}
    for k, a in res.items():
        r = ref[k]
        assert tuple(a.shape) == r.shape, (what, k, tuple(a.shape), r.shape)
        if raised and k in raised:
            bounds[k] = (0.0, 2.0 * raised[k])
        else:
            bounds[k] = TOL[k]
        err = float(np.abs(a.cpu().double().numpy() - r).max())
        frac = err / (bounds[k][0] * float(np.abs(r).max()) + bounds[k][1])
        if not frac <= WORST.get(section, (-1.0, ""))[0]:
            WORST[section] = (frac, f"{k} {what}")
        print(f"[node gcn forms] {what}: {k} max err {err:.3e} = {frac:.3f} of the bound{' (raised)' if raised and k in raised else ''}")
    for k, a in res.items():
        close(a, ref[k], rtol=bounds[k][0], atol=bounds[k][1], what=f"{k} {what}")


def assert_equals_replayed(g, d, act, tab, n_steps, params, u0, R, members, res, what):
    """a case with a raised bound: u(T) and du0 bit for bit the replayed plan's (member by member: it has no batch form), the parameter
    gradients to the rounding of another order of the per-tile sums (test_node_persistent_tile_pairs_beyond_512_tiles' bound)"""
    parts = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("NGPDE_NO_PERSISTENT", "1")
        for m in range(members):
            sl = slice(m * g.n, (m + 1) * g.n)
            flags, r = run_plan(g, d, act, tab, n_steps, params, u0[:, sl], R[:, sl], solves=1)
            assert_flags(flags, 0, PFWD | PBWD | FORMS, f"replayed {what}")
            parts.append(r[0])
    for k in ("uT", "du0"):
        assert torch.equal(res[k], torch.cat([p[k] for p in parts])), f"{k} differs from the replayed plan's bits: {what}"
    for k in ("dW1", "db1", "dW2", "db2"):
        y = sum(p[k] for p in parts)
        assert torch.allclose(res[k], y, rtol=2e-5, atol=2e-5 * float(y.abs().max())), f"{k} against the replayed plan: {what}"


def check(section, key, g, act, on, off, d=64, members=1, with_backward=True, solves=H.SOLVES, seed=None, what=""):
    """every solve of `solves` on a plan of its own: flags, two solves (no fault, guards intact), float64, the same bits again"""
    seed = H.case_seed(key) if seed is None else seed
    params, u0, R = inputs(key, g, d, act, seed, solves, members)
    on = on | PRESCALED | (SIGN_MASKS if act == "relu" and with_backward else 0) | (WIDENED if d != 64 else 0)
    on = on | (PBWD if on & PFWD and with_backward else 0)
    off = off | (0 if with_backward else PBWD) | (0 if d != 64 else WIDENED) | (0 if act == "relu" and with_backward else SIGN_MASKS)
    for tab, n_steps in solves:
        tag = f"{key} {g.wmode or ''} d={d} {act} members={members} {tab}x{n_steps} {what}"
        flags, results = run_plan(g, d, act, tab, n_steps, params, u0, R, members, with_backward)
        assert_flags(flags, on, off, tag)
        ref = reference(key, g, d, act, tab, n_steps, params, u0, R, members)
        raised = RAISED.get((key, members, tab, n_steps)) if (act, d, g.wmode, with_backward) == ("relu", 64, None, True) else None
        compare(section, tag, results[0], ref, raised)
        if raised:
            assert_equals_replayed(g, d, act, tab, n_steps, params, u0, R, members, results[0], tag)
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), f"a second solve on the same plan gave other bits: {k} {tag}"


ONE_TILE = PFWD | OWN_FIRST           # mode 1 on a graph of one wave of workgroups: the plan reads its own-first tables


# ---- A. one tile per workgroup, unweighted -----------------------------------------------------------------------------------------

A_GRAPHS = [k for k in H.CASES if k.startswith("A")]
A_COUNTS = ["N=1", "N=31", "N=32", "N=33", "N=65"]


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("name", A_GRAPHS)
def test_a_one_tile_plan_at_the_caps(name, act):
    g = handle(name)
    assert_regime(g, name)
    assert g.n_tiles in (24, 66) and (g.n % ROWS != 0) == (g.n_tiles == 24)
    check("A", name, g, act, ONE_TILE, FORMS)


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("name", A_COUNTS)
def test_a_tile_counts(name, act):
    # one node; one tile short of a row; one full tile; a one-row second tile (its row takes 31 in-edges); three tiles
    g = handle(name)
    assert_regime(g, name)
    check("A", name, g, act, ONE_TILE, FORMS)


@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("name", ["A3 halo both ways", "A4 rows by target"])
def test_a_forward_only_plan(name, act):
    # with_backward = 0: TAPE = false, no sign masks and no z tape
    g = handle(name)
    assert_regime(g, name)
    check("A", name, g, act, ONE_TILE, FORMS, with_backward=False)


@pytest.mark.parametrize("name", ["A3 halo both ways", "A4 rows by target"])
def test_a_handle_order_tables(name, monkeypatch):
    # NGPDE_NO_OWN_FIRST=1 at create: the same neighbours in the handle's order, against the same float64
    g = handle(name)
    assert_regime(g, name)
    monkeypatch.setenv("NGPDE_NO_OWN_FIRST", "1")
    check("A", name, g, "relu", PFWD, FORMS | OWN_FIRST, what="handle order")


@pytest.mark.parametrize("d", [16, 32])
@pytest.mark.parametrize("name", ["A3 halo both ways", "A6 63 neighbours"])
def test_a_widened_widths(name, d):
    # d = 16 / 32 zero-padded onto the 64-wide kernels; sigmoid(0) = 0.5 fills the padded columns of every stage, which must not leak
    g = handle(name)
    assert_regime(g, name)
    check("A", name, g, "sigmoid", ONE_TILE, FORMS, d=d)


# ---- B. just beyond the caps -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("name", ["B 33-entry row", "B 97-row halo"])
def test_b_one_direction_beyond_a_cap(name, act):
    # by target only: the handle is not halo_ok there, so not the 96-row plan; the hub geometry where its partition accepts the graph
    g = handle(name)
    assert_regime(g, name)
    assert not halo_ok(g, 0) and halo_ok(g, 1)
    s, t, n, _ = g.host
    rc, _, _, _, msg = partition(n, s, t)
    assert rc in (_lib.OK, _lib.ERR_UNSUPPORTED), msg
    if rc == _lib.OK:
        on, off = PFWD | HUB_GEOMETRY, TILE_PAIRS | TILE_ROUNDS | OWN_FIRST
    else:
        on, off = 0, PFWD | PBWD | FORMS | PRESCALED
    params, u0, R = inputs(name, g, 64, act, H.case_seed(name), H.SOLVES)
    for tab, n_steps in H.SOLVES:
        tag = f"{name} {act} {tab}x{n_steps}"
        flags, results = run_plan(g, 64, act, tab, n_steps, params, u0, R)
        assert_flags(flags, on | (PBWD if on else 0), off, tag)
        compare("B", tag, results[0], reference(name, g, 64, act, tab, n_steps, params, u0, R, 1))
        for k in results[0]:
            assert torch.equal(results[0][k], results[1][k]), f"a second solve on the same plan gave other bits: {k} {tag}"


@pytest.mark.parametrize("act", ["relu", "tanh"])
def test_b_wait_list_of_64_tiles(act):
    # both directions fit, so the plan is pre-scaled and node_persistent_mode says 1 -- but tile 0's wait list would hold 64 tiles:
    # node_persistent_setup refuses, node_create keeps the replayed plan without an error
    name = "B 64 neighbours"
    g = handle(name)
    assert_regime(g, name)
    assert halo_ok(g, 0) and halo_ok(g, 1) and g.geo["nbr"].max() == H.MAX_NBR + 1
    check("B", name, g, act, 0, PFWD | PBWD | FORMS)
    assert handle("A6 63 neighbours").geo["nbr"].max() == H.MAX_NBR      # ... one tile fewer is the persistent plan's (section A)


# ---- C. weighted graphs ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rounds", [False, True])
@pytest.mark.parametrize("act", ["relu", "tanh"])
@pytest.mark.parametrize("name", ["A3 halo both ways", "A4 rows by target", "A6 63 neighbours"])
def test_c_weighted_graphs(name, act, rounds, monkeypatch):
    # slot weights beside the slots: the WGT one-tile kernels as chosen; NGPDE_WEIGHTED_TILE_ROUNDS=1 sends the same graph through the K
    # kernels with one tile per turn
    g = handle(name, wmode="quirk")
    assert_regime(g, name)
    assert g.w is not None and g.w.size == g.E and float(g.w.min()) >= 0.5
    if rounds:
        monkeypatch.setenv("NGPDE_WEIGHTED_TILE_ROUNDS", "1")
        check("C", name, g, act, PFWD | TILE_ROUNDS | OWN_FIRST, TILE_PAIRS | HUB_GEOMETRY, what="tile rounds")
    else:
        check("C", name, g, act, ONE_TILE, FORMS)


# ---- D. batches --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("interleave", [True, False])
@pytest.mark.parametrize("members", [2, 3])
@pytest.mark.parametrize("name", ["A3 halo both ways", "A6 63 neighbours"])
def test_d_batches(name, members, interleave, monkeypatch):
    # two members per workgroup (3: the odd one alone in slot 0), or member after member under NGPDE_NO_INTERLEAVE=1; every member
    # against the float64 solve of that member alone, the parameter gradients against the sum over the members
    g = handle(name)
    assert_regime(g, name)
    if not interleave:
        monkeypatch.setenv("NGPDE_NO_INTERLEAVE", "1")
    check("D", name, g, "relu", ONE_TILE, FORMS, members=members, what="interleaved" if interleave else "member by member")


# ---- E. tile-count boundaries of the plans -----------------------------------------------------------------------------------------

def resident():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


E_CASES = {                      # name: (which count, switch, flags on, flags off, solves)
    "resident":                         ("one", None, PFWD | OWN_FIRST, FORMS, H.E_SOLVES),
    "resident + 1":                     ("pair_first", None, PFWD | TILE_PAIRS, TILE_ROUNDS | HUB_GEOMETRY | OWN_FIRST, H.E_SOLVES),
    "resident + 1, tile rounds":        ("pair_first", "NGPDE_TILE_ROUNDS", PFWD | TILE_ROUNDS, TILE_PAIRS | HUB_GEOMETRY | OWN_FIRST, H.E_SOLVES),
    "resident + 1, no tile pairs":      ("pair_first", "NGPDE_NO_TILE_PAIRS", 0, PFWD | PBWD | FORMS | OWN_FIRST, H.E_SOLVES),
    "2 resident":                       ("pair_last", None, PFWD | TILE_PAIRS, TILE_ROUNDS | HUB_GEOMETRY | OWN_FIRST, H.E_SOLVES),
    "2 resident + 1":                   ("rounds_first", None, PFWD | TILE_ROUNDS, TILE_PAIRS | HUB_GEOMETRY | OWN_FIRST, H.E_SOLVES),
}


@pytest.mark.parametrize("case", list(E_CASES))
def test_e_tile_count_boundaries(case, monkeypatch):
    which, switch, on, off, solves = E_CASES[case]
    res = resident()
    n_tiles = H.boundary_counts(res)[which]
    g = make_handle(("E", n_tiles), lambda: H.boundary(n_tiles))
    assert_regime(g)
    geo = g.geo
    assert geo["n_tiles"] == n_tiles and g.n % ROWS == ROWS - 7 and geo["halo_t"] == HALO_CAP and H.fits(geo) and geo["nbr"].max() == 2
    if switch:
        monkeypatch.setenv(switch, "1")
    check("E", ("E", n_tiles), g, "relu", on, off, solves=solves, seed=7100 + n_tiles,
          what=f"{case} ({n_tiles} tiles; if the flags differ the boundary moved: the device does not hold 2 workgroups per CU)")
