"""The persistent GCN solver's software-pipelined neighbour sums (csrc/node_persistent.hip: tile_aggregate_rounds, the forward kernel's
own and foreign rounds; tile_aggregate_rounds_rolling, the adjoint's) on graphs built to hit every shape of the round loop.

The sums run over "rounds" of four slot bytes per row; the number of rounds is uniform per wave (= four rows of a 32-row tile), the
forward kernel sums a wave's own-tile rounds before it waits and the foreign ones behind the gather.  The graph below is a union of
small components whose tiles are known from the handle's locality order (GNNGraph.node_order(): tile k = order[32 k : 32 k + 32]) and
are CHECKED, not assumed, before anything is solved:

  * P: a star p0 - p1..p31 (one tile: the seed's neighbours fill it) whose leaves also reach Q -- p0 has 31 own-tile entries and one
    foreign one (32 entries: eight rounds, the last one full), the rows beside it in its wave have three or four (padding to the
    wave's maximum);
  * Q: 32 nodes that only reach P: a tile none of whose rows has an own-tile neighbour (zero own rounds in every wave);
  * C: a star c0 - c1..c31 with chords inside: a tile without any foreign row (zero foreign rounds, nothing to gather) whose rows have
    exactly 28 (seven rounds, the last one full), 4 (one round), 5 (one and a bit) and 3 entries;
  * a closest-pairs graph with part of its reverse edges dropped (by-source and by-target lists differ) that brings the node count to
    a number that is no multiple of 32 (padding rows in the last tile).

Checked: persistent plan against the replayed plan bit for bit (u(T), du0), against the float64 oracle with the tolerances
tests/test_gcn_gpu.py uses for the same comparison, and two consecutive solves bit for bit.
"""
import numpy as np
import pytest
import torch

import ngpde_amd as ng
from oracle import ngpde_oracle as O
from ngpde_amd import synth as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = 32

PLAN_SWITCHES = ("NGPDE_NO_PERSISTENT", "NGPDE_NO_WIDEN", "NGPDE_NO_TILE_PAIRS", "NGPDE_TILE_ROUNDS", "NGPDE_NO_INTERLEAVE",
                 "NGPDE_WEIGHTED_TILE_ROUNDS", "NGPDE_NO_PRESCALE", "NGPDE_NO_MASK", "NGPDE_NO_OWN_FIRST", "NGPDE_NO_HALO")


def close(a, ref, rtol=1e-4, atol=1e-5, what=""):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    ref = np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    err = np.abs(a - ref).max() if ref.size else 0.0
    bound = rtol * (np.abs(ref).max() if ref.size else 0.0) + atol
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def round_shapes_graph(n_spatial, seed):
    """(s, t, N): the union described in the module docstring; undirected pairs are listed in both directions"""
    und = []
    # P = 0..31, Q = 32..63
    und += [(0, j) for j in range(1, 32)]
    und += [(0, 32)]                                                   # p0: 31 own-tile entries + 1 foreign = 32
    for i in range(32):                                                # q_i reaches two leaves of P, never p0
        a, b = 1 + (i % 31), 1 + ((i + 7) % 31)
        und += [(32 + i, a), (32 + i, b)]
    # C = 64..95
    c = 64
    und += [(c, c + j) for j in range(1, 32)]
    und += [(c + 1, c + j) for j in range(2, 29)]                      # c1: c0 + 27 = 28 entries
    und += [(c + j, c + j + 1) for j in range(2, 31)]                  # a path c2 - c3 - ... - c31
    und += [(c + 5, c + 10)]                                           # c5, c10: five entries
    und = sorted(set((min(a, b), max(a, b)) for a, b in und))
    s = np.array([a for a, b in und] + [b for a, b in und], dtype=np.int64)
    t = np.array([b for a, b in und] + [a for a, b in und], dtype=np.int64)
    # the spatial part, made directed: every third edge (in list order) whose source is the larger node is dropped
    _, ss, tt = S.closest_pairs_graph(n_spatial, 4 * n_spatial, seed=seed)
    ss, tt = np.asarray(ss, dtype=np.int64), np.asarray(tt, dtype=np.int64)
    back = np.flatnonzero(ss > tt)
    keep = np.ones(ss.size, dtype=bool)
    keep[back[::3]] = False
    s = np.concatenate([s, ss[keep] + 96])
    t = np.concatenate([t, tt[keep] + 96])
    return s, t, 96 + n_spatial


def tile_shapes(order, s, t, N):
    """per direction (0: lists by target, 1: by source) and node: (entries, entries from the node's own tile)"""
    tile_of = np.empty(N, dtype=np.int64)
    tile_of[np.asarray(order, dtype=np.int64)] = np.arange(N) // TILE
    out = []
    for row, col in ((t, s), (s, t)):
        n_all = np.bincount(row, minlength=N)
        n_own = np.bincount(row, weights=(tile_of[row] == tile_of[col]).astype(np.float64), minlength=N).astype(np.int64)
        out.append((n_all, n_own))
    return tile_of, out


def assert_round_shapes(g, s, t, N):
    order = np.asarray(g.node_order())
    assert sorted(order.tolist()) == list(range(N))
    tile_of, dirs = tile_shapes(order, s, t, N)
    assert N % TILE != 0
    n_tiles = (N + TILE - 1) // TILE
    for d, (n_all, n_own) in enumerate(dirs):
        assert n_all.max() <= 32, "a row beyond the 32-entry slot lists: no persistent plan"
        per_tile = [np.flatnonzero(tile_of == k) for k in range(n_tiles)]
        zero_own = [k for k, rows in enumerate(per_tile) if n_own[rows].sum() == 0 and n_all[rows].min() > 0]
        zero_foreign = [k for k, rows in enumerate(per_tile) if (n_all[rows] == n_own[rows]).all() and n_all[rows].min() > 0]
        assert zero_own, f"direction {d}: no tile without own-tile neighbours"
        assert zero_foreign, f"direction {d}: no tile without foreign neighbours"
        lengths = set(n_all.tolist())
        assert {4, 5, 28, 32} <= lengths, f"direction {d}: row lengths {sorted(lengths)}"
        # a wave sums four rows: a tile with one long row and short rows otherwise pads the short ones, wherever the long one sits
        assert any(n_all[rows].max() >= 28 and np.sort(n_all[rows])[-2] <= 8 for rows in per_tile), f"direction {d}: no wave of unequal rows"
        # one-and-a-bit rounds and a partial last round among mixed own / foreign rows
        mixed = (n_own > 0) & (n_own < n_all)
        assert mixed.any() and (n_all[mixed] % 4 != 0).any()
    by_t, by_s = dirs[0][0], dirs[1][0]
    assert not np.array_equal(by_t, by_s), "by-source and by-target lists have the same lengths: the graph is not directed"


def oracle_node(params, og, u0, seed, tableau, dt, nsteps, act):
    rhs, vjp = O.gcn2_rhs(params, og, act)
    uT, tape = O.rk_solve(rhs, u0, tableau, dt, nsteps)
    acc = [dict(weight=np.zeros_like(p["weight"]), bias=np.zeros_like(p["bias"])) for p in params]

    def accumulate(pg):
        for A, G in zip(acc, pg):
            A["weight"] += G["weight"]
            A["bias"] += G["bias"].reshape(A["bias"].shape)
    du0 = O.rk_adjoint(vjp, tape, seed.copy(), tableau, dt, accumulate)
    return uT, du0, acc


def solve(g, params, u0, R, d, tab, nsteps, dt, act, persistent):
    rhs = ng.Chain(ng.GCNConv((d, d), act, initialgraph=g), ng.GCNConv((d, d), act, initialgraph=g))
    node = ng.NeuralODE(rhs, solver=tab, n_steps=nsteps, dt=dt)
    ps, st = ng.setup(0, node)
    for k, name in enumerate(["layer_1", "layer_2"]):
        ps[name]["weight"] = torch.as_tensor(params[k]["weight"].astype(np.float32))
        ps[name]["bias"] = torch.as_tensor(params[k]["bias"].astype(np.float32))
    ps = ng.to_device(ps, DEV)
    outs = []
    for rep in range(2):   # two consecutive solves on one plan
        for lp in ps.values():
            for v in lp.values():
                v.requires_grad_(True)
                v.grad = None
        u = u0.clone().requires_grad_(True)
        uT, _ = node(u, ps, st)
        plan = next(iter(node._plans.values()))[0]
        flags = plan.flags()
        assert ({"persistent_fwd", "persistent_bwd"} <= flags) == persistent, flags
        (uT * R).sum().backward()
        assert not plan.fault()
        outs.append((uT.detach().clone(), u.grad.clone(), ps["layer_1"]["weight"].grad.clone(), ps["layer_1"]["bias"].grad.clone(),
                     ps["layer_2"]["weight"].grad.clone(), ps["layer_2"]["bias"].grad.clone()))
    return outs


@pytest.mark.parametrize("tab,act,n_spatial,nsteps", [("tsit5", "relu", 517, 3), ("tsit5", "tanh", 517, 2), ("euler", "relu", 1201, 4)])
def test_pipelined_sums_on_every_shape_of_the_round_loop(tab, act, n_spatial, nsteps, monkeypatch):
    for var in PLAN_SWITCHES:
        monkeypatch.delenv(var, raising=False)
    d, dt = 64, 0.05
    s, t, N = round_shapes_graph(n_spatial, seed=n_spatial)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    og = O.Graph(s, t, num_nodes=N, index_base=0)
    rng = np.random.default_rng(n_spatial + 1)
    params = [dict(weight=S.glorot_uniform(n_spatial + 10 + k, d, d), bias=rng.normal(size=(d, 1)) * 0.1) for k in range(2)]
    u0n, Rn = rng.normal(size=(d, N)), rng.normal(size=(d, N))
    u0 = torch.as_tensor(u0n.astype(np.float32), device=DEV)
    R = torch.as_tensor(Rn.astype(np.float32), device=DEV)

    pers = solve(g, params, u0, R, d, tab, nsteps, dt, act, persistent=True)
    assert_round_shapes(g, s, t, N)      # (the handle exists now: its locality order is what the plan's tiles are cut from)
    monkeypatch.setenv("NGPDE_NO_PERSISTENT", "1")
    repl = solve(g, params, u0, R, d, tab, nsteps, dt, act, persistent=False)

    # two consecutive solves: every output bit for bit
    for x, y, what in zip(pers[0], pers[1], ("u(T)", "du0", "dW1", "db1", "dW2", "db2")):
        assert torch.equal(x, y), f"second persistent solve differs in {what}"
    # persistent against replayed: the states bit for bit, the parameter gradients to rounding (per-tile partial sums, other order)
    assert torch.equal(pers[0][0], repl[0][0]), "u(T): persistent and replayed plans differ"
    assert torch.equal(pers[0][1], repl[0][1]), "du0: persistent and replayed plans differ"
    for k in range(2, 6):
        assert torch.allclose(pers[0][k], repl[0][k], rtol=1e-5, atol=1e-5)
    # float64 oracle, tolerances of tests/test_gcn_gpu.py (test_node_persistent_plan_against_oracle)
    uTo, du0o, acc = oracle_node(params, og, u0n, Rn, O.TABLEAUS[tab], dt, nsteps, act)
    close(pers[0][0], uTo, rtol=2e-4, what="u(T)")
    close(pers[0][1], du0o, rtol=5e-4, atol=1e-4, what="du0")
    close(pers[0][2], acc[0]["weight"], rtol=5e-4, atol=1e-3, what="dW1")
    close(pers[0][3], acc[0]["bias"], rtol=5e-4, atol=1e-3, what="db1")
    close(pers[0][4], acc[1]["weight"], rtol=5e-4, atol=1e-3, what="dW2")
    close(pers[0][5], acc[1]["bias"], rtol=5e-4, atol=1e-3, what="db2")
