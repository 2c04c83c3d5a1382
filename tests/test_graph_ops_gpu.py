"""GPU tests of the graph queries and transforms (graphops.py over csrc/graph_ops.hip; src/NeuralGraphPDE.jl:4 of the reference re-exports
them from GNNGraphs).

Structure -- every query, every transform's edge list INCLUDING ITS ORDER, the group lists of the coalesce -- is compared exactly with
the numpy restatement below.  Feature reductions and their gradients are compared with float64 numpy under a derived bound: `+` and
`mean` are one float32 sum in member order, so per element |out - ref| <= k * 2^-24 * sum|x_i| for a group of k members (k - 1 roundings
of partial sums that never exceed sum|x_i|, one more for the mean's division); the pullback is at most two terms, the mean's division
and the cast, covered by the same form with k = 4.  max / min must be exact.
"""
import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import graphops
from ngpde_amd import synth as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------


def np_degree(s, t, n, dir):
    out, inn = np.bincount(s, minlength=n), np.bincount(t, minlength=n)
    return {"out": out, "in": inn, "both": out + inn}[dir].astype(np.int32)


def np_weighted_degree(s, t, n, dir, w):
    """float32 sums in COO order (np.add.at adds one entry after the other, in float32)"""
    out, inn = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    np.add.at(out, s, w.astype(np.float32))
    np.add.at(inn, t, w.astype(np.float32))
    return {"out": out, "in": inn, "both": out + inn}[dir]


def np_flags(s, t, n):
    key, rev = s.astype(np.int64) * n + t, t.astype(np.int64) * n + s
    return (bool((s == t).any()), bool(np.unique(key).size < key.size), bool(np.array_equal(np.sort(key), np.sort(rev))))


def np_coalesce(s, t, n, symmetrize):
    """(s', t', group_ptr, member, group_of): the copies sorted stably by s*n + t, one group per distinct key"""
    e = s.size
    rows = np.arange(e, dtype=np.int64)
    ss, tt = (np.concatenate([s, t]), np.concatenate([t, s])) if symmetrize else (s, t)
    rows = np.concatenate([rows, rows]) if symmetrize else rows
    key = ss.astype(np.int64) * n + tt
    order = np.argsort(key, kind="stable")
    ks = key[order]
    head = np.ones(ks.size, dtype=bool)
    head[1:] = ks[1:] != ks[:-1]
    ptr = np.concatenate([np.flatnonzero(head), [ks.size]]).astype(np.int64)
    group_of = np.empty(ks.size, dtype=np.int64)
    group_of[order] = np.cumsum(head) - 1
    return ks[head] // max(n, 1), ks[head] % max(n, 1), ptr, rows[order], group_of


def np_induced(s, t, n, nodes):
    relabel = np.full(n, -1, dtype=np.int64)
    relabel[nodes] = np.arange(nodes.size)
    kept = np.flatnonzero((relabel[s] >= 0) & (relabel[t] >= 0))
    return relabel[s[kept]], relabel[t[kept]], kept


def edges_of(g):
    """the result's 0-based edge list, after checking that the device lists the handle builder takes are the same"""
    s, t = g.edge_index(index_base=0)
    coo = g._shared[("coo", str(torch.device("cuda", torch.cuda.current_device())))]
    assert coo[0].dtype == torch.int32 and np.array_equal(coo[0].cpu().numpy(), s) and np.array_equal(coo[1].cpu().numpy(), t)
    assert g.num_edges == s.size
    return s, t


def same_edges(g, s, t, what):
    gs, gt = edges_of(g)
    assert np.array_equal(gs, s) and np.array_equal(gt, t), what


# ---- the structure cases --------------------------------------------------------------------------------------------------------------


def high_bit_case():
    """N = 70 000: (s, t) and (s + 61356, t + 47296) have keys s*n + t that differ by exactly 2^32 (61356 * 70000 + 47296 = 2^32), so a
    32-bit key merges them; true duplicates of both are mixed in"""
    n, rng = 70000, np.random.default_rng(11)
    assert 61356 * n + 47296 == 2 ** 32
    s0, t0 = rng.integers(0, 70000 - 61356, 3000), rng.integers(0, 70000 - 47296, 3000)
    s = np.concatenate([s0, s0 + 61356, s0[:500], s0[200:400] + 61356])
    t = np.concatenate([t0, t0 + 47296, t0[:500], t0[200:400] + 47296])
    p = rng.permutation(s.size)
    return s[p], t[p], n


def cases():
    rng = np.random.default_rng(5)
    z = np.zeros(0, dtype=np.int64)
    out = {"no_edges": (z, z, 5), "one_node": (z, z, 1), "one_node_loops": (np.zeros(3, dtype=np.int64), np.zeros(3, dtype=np.int64), 1)}
    loops = rng.integers(0, 9, 20)
    out["only_self_loops"] = (loops, loops.copy(), 9)
    out["one_pair_65536"] = (np.full(2 ** 16, 3, dtype=np.int64), np.full(2 ** 16, 1, dtype=np.int64), 6)
    out["multigraph"] = (rng.integers(0, 1000, 20000), rng.integers(0, 1000, 20000), 1000)
    out["high_bits"] = high_bit_case()
    _, s, t = S.closest_pairs_graph(16384, 65536, seed=1)
    out["bench_size"] = (np.asarray(s, dtype=np.int64), np.asarray(t, dtype=np.int64), 16384)
    return out


CASES = cases()


@pytest.mark.parametrize("name", list(CASES))
def test_structure_matches_numpy(name):
    s, t, n = CASES[name]
    e = s.size
    rng = np.random.default_rng(2)
    w = rng.uniform(0.5, 1.5, e).astype(np.float32)
    x = rng.normal(size=(3, n)).astype(np.float32)
    label = rng.integers(0, 7, e)
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, ndata={"x": x}, edge_weight=w)
    ge = ng.GNNGraph(g, edata={"label": label})

    # queries
    for dir in ("out", "in", "both"):
        d = ng.degree(g, dir, edge_weight=False)
        assert d.dtype == torch.int32 and d.is_cuda and np.array_equal(d.cpu().numpy(), np_degree(s, t, n, dir)), dir
        dw = ng.degree(g, dir)                                   # the graph carries weights
        assert dw.dtype == torch.float32 and np.array_equal(dw.cpu().numpy(), np_weighted_degree(s, t, n, dir, w)), dir
        assert torch.equal(ng.degree(g, dir, edge_weight=torch.as_tensor(w)), dw)
        assert torch.equal(ng.degree(g, dir), dw)                # bitwise reproducible
    assert ng.degree(ng.GNNGraph(s, t, num_nodes=n, index_base=0)).dtype == torch.int32     # no weights: counts
    flags = np_flags(s, t, n)
    assert (ng.has_self_loops(g), ng.has_multi_edges(g), ng.is_bidirected(g)) == flags
    assert all(isinstance(f(g), bool) for f in (ng.has_self_loops, ng.has_multi_edges, ng.is_bidirected))

    # add_self_loops
    ga = ng.add_self_loops(g)
    same_edges(ga, np.concatenate([s, np.arange(n)]), np.concatenate([t, np.arange(n)]), "add_self_loops")
    assert np.array_equal(ga.edge_weight.cpu().numpy(), np.concatenate([w, np.ones(n, dtype=np.float32)]))
    assert ga.num_nodes == n and np.array_equal(ga.ndata["x"], x)

    # remove_self_loops: COO order, features follow
    keep = np.flatnonzero(s != t)
    gr = ng.remove_self_loops(ge)
    same_edges(gr, s[keep], t[keep], "remove_self_loops")
    assert np.array_equal(gr.edge_weight.cpu().numpy(), w[keep])
    assert gr.edata["label"].dtype == label.dtype and np.array_equal(gr.edata["label"], label[keep])     # kept where and as it was
    assert not ng.has_self_loops(gr)

    # coalesce: edge order, group lists, member order
    for sym in (False, True):
        so, to, ptr, member, group_of = np_coalesce(s, t, n, sym)
        gc = ng.to_bidirected(g) if sym else ng.remove_multi_edges(g)
        same_edges(gc, so, to, ("coalesce", sym))
        coal = graphops._Coalesced(g, torch.device("cuda", torch.cuda.current_device()), sym)
        m = member.size
        assert coal.n_groups == so.size
        assert np.array_equal(coal.group_ptr[:so.size + 1].cpu().numpy(), ptr)
        assert np.array_equal(coal.member[:m].cpu().numpy(), member)
        assert np.array_equal(coal.group_of[:m].cpu().numpy(), group_of)
        assert not ng.has_multi_edges(gc) and (not sym or ng.is_bidirected(gc))
        again = ng.to_bidirected(g) if sym else ng.remove_multi_edges(g)
        assert gc == again and torch.equal(gc.edge_weight, again.edge_weight)

    # induced subgraph on a shuffled half of the nodes
    nodes = rng.permutation(n)[: max(1, n // 2)]
    si, ti, kept = np_induced(s, t, n, nodes)
    gi = ng.induced_subgraph(ge, nodes)
    same_edges(gi, si, ti, "induced_subgraph")
    assert gi.num_nodes == nodes.size and np.array_equal(gi.ndata["x"].cpu().numpy(), x[:, nodes])
    assert np.array_equal(gi.edata["label"], label[kept]) and np.array_equal(gi.edge_weight.cpu().numpy(), w[kept])
    gw, nmap = ng.getgraph(g, 0, nmap=True)                      # a single graph is its own member 0
    same_edges(gw, s, t, "getgraph")
    assert nmap.dtype == torch.int64 and np.array_equal(nmap.cpu().numpy(), np.arange(n))


def test_is_bidirected():
    g = ng.rand_graph(200, 1200, bidirected=True, seed=4)
    assert ng.is_bidirected(g) and not ng.has_self_loops(g) and not ng.has_multi_edges(g)
    s, t = g.edge_index(index_base=0)
    assert not ng.is_bidirected(ng.GNNGraph(s[1:], t[1:], num_nodes=200, index_base=0))                       # one edge dropped
    doubled = ng.GNNGraph(np.concatenate([s, s[:1]]), np.concatenate([t, t[:1]]), num_nodes=200, index_base=0)   # one direction twice
    assert not ng.is_bidirected(doubled) and ng.has_multi_edges(doubled)
    both = ng.GNNGraph(np.concatenate([s, s[:1], t[:1]]), np.concatenate([t, t[:1], s[:1]]), num_nodes=200, index_base=0)
    assert ng.is_bidirected(both) and ng.has_multi_edges(both)


def test_induced_subgraph_refuses_bad_nodes():
    g = ng.rand_graph(50, 200, seed=1)
    with pytest.raises(ng.ArgumentError, match="repeated"):
        ng.induced_subgraph(g, [3, 7, 3])
    with pytest.raises(ng.ArgumentError, match="outside"):
        ng.induced_subgraph(g, [3, 50])
    with pytest.raises(ng.ArgumentError, match="outside"):
        ng.induced_subgraph(g, [-1, 2])
    assert ng.induced_subgraph(g, [3, 7, 4]).num_nodes == 3


# ---- the mesh of the VMH tutorial -------------------------------------------------------------------------------------------------------


def grid_triangles(k=40):
    """the k x k grid, every cell cut into two triangles; three directed edges a -> b -> c -> a per triangle"""
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    s = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    t = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    gx, gy = np.meshgrid(np.arange(k) / (k - 1), np.arange(k) / (k - 1), indexing="ij")
    return tri, s, t, np.stack([gx.ravel(), gy.ravel()]).astype(np.float32)


def test_to_bidirected_of_a_triangulation():
    k = 40
    n = k * k
    tri, s, t, pts = grid_triangles(k)
    g = ng.to_bidirected(ng.GNNGraph(s, t, num_nodes=n, index_base=0, ndata={"x": pts}))
    expected = [set() for _ in range(n)]          # "neighbours if they lie on the same edge of at least one triangle"
    for a, b, c in tri:
        for u, v in ((a, b), (b, c), (c, a)):
            expected[u].add(int(v))
            expected[v].add(int(u))
    gs, gt = edges_of(g)
    got = [[] for _ in range(n)]
    for u, v in zip(gs, gt):
        got[u].append(int(v))
    assert all(sorted(expected[i]) == got[i] for i in range(n))          # each neighbour once, ascending: sorted by source, then target
    assert ng.is_bidirected(g) and not ng.has_multi_edges(g) and not ng.has_self_loops(g)
    so, to = np_coalesce(s, t, n, True)[:2]
    twin = ng.GNNGraph(so, to, num_nodes=n, index_base=0, ndata={"x": pts})          # built on the host from the restatement
    assert g == twin

    # VMHConv runs on it
    phi = ng.Chain(ng.Dense(4, 16, "tanh"), ng.Dense(16, 8))
    gam = ng.Chain(ng.Dense(9, 16, "tanh"), ng.Dense(16, 1))
    vmh = ng.VMHConv(phi, gam, initialgraph=g)
    ps, st = ng.setup(0, vmh)
    ps = ng.to_device(ps, DEV)
    u = torch.as_tensor(np.sin(6 * pts[:1]) * np.cos(4 * pts[1:]), device=DEV)
    y, _ = vmh(u, ps, st)
    assert tuple(y.shape) == (1, n) and bool(torch.isfinite(y).all())
    y2, _ = vmh(u, ps, ng.updategraph(st, twin))
    assert torch.equal(y, y2)

    # GCNConv on it is bitwise the layer on the host-built twin
    d = 16
    x = torch.randn(d, n, device=DEV)
    outs = []
    for graph in (g, twin):
        gcn = ng.GCNConv((d, d), "relu", initialgraph=graph)
        ps, st = ng.setup(0, gcn)
        outs.append(gcn(x, ng.to_device(ps, DEV), st)[0])
    assert torch.equal(outs[0], outs[1]) and bool(outs[0].abs().sum() > 0)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------


def batch_members():
    rng = np.random.default_rng(8)
    gs = []
    for k, (n, e) in enumerate(((7, 15), (1, 0), (12, 40), (4, 3))):
        gs.append(ng.GNNGraph(rng.integers(0, n, e), rng.integers(0, n, e), num_nodes=n, index_base=0,
                              ndata={"x": torch.as_tensor(rng.normal(size=(3, n)).astype(np.float32)), "y": torch.as_tensor(rng.integers(0, 5, (1, n)))},
                              edata={"e": torch.as_tensor(rng.normal(size=(2, e)).astype(np.float32))},
                              gdata={"u": torch.as_tensor(rng.normal(size=(4, 1)).astype(np.float32))}))
    return gs


def test_unbatch_inverts_batch():
    gs = batch_members()
    gb = ng.batch(gs)
    back = ng.unbatch(gb)
    assert len(back) == len(gs)
    for a, b in zip(back, gs):
        assert a == b and a.num_graphs == 1 and a.graph_indicator is None
        assert a.ndata["x"].is_cuda and a.ndata["y"].dtype == torch.int64 and not a.ndata["y"].is_cuda
    assert back == gs


def test_getgraph_of_a_list():
    gs = batch_members()
    gb = ng.batch(gs)
    sub, nmap = ng.getgraph(gb, [0, 2], nmap=True)
    assert nmap.dtype == torch.int64 and nmap.is_cuda
    assert np.array_equal(nmap.cpu().numpy(), np.concatenate([np.arange(0, 7), np.arange(8, 20)]))
    assert sub.num_graphs == 2 and np.array_equal(sub.graph_indicator, np.repeat([0, 1], [7, 12]))
    assert np.array_equal(sub.gdata["u"].cpu().numpy(), gb.gdata["u"].numpy()[:, [0, 2]])
    assert sub == ng.batch([gs[0], gs[2]])
    one = ng.getgraph(gb, [3])
    assert one == gs[3] and one.graph_indicator is None
    assert ng.getgraph(gb, np.int64(1)) == gs[1]


# ---- features: values and gradients ---------------------------------------------------------------------------------------------------


def grouped_graph():
    """groups of 1, 2, 5 and 300 duplicates (and self loops, whose two copies share a group under to_bidirected), shuffled"""
    rng = np.random.default_rng(21)
    n = 40
    codes = [int(c) for c in rng.permutation(n * n) if c not in (5 * n + 5, 17 * n + 17)][:90]
    pairs = [(c // n, c % n) for c in codes] + [(5, 5), (17, 17)]
    mult = [1] * 49 + [2] * 30 + [5] * 9 + [300] * 2 + [1, 5]
    assert len(pairs) == len(mult) == 92
    s = np.concatenate([np.full(m, p[0]) for p, m in zip(pairs, mult)])
    t = np.concatenate([np.full(m, p[1]) for p, m in zip(pairs, mult)])
    p = rng.permutation(s.size)
    return s[p], t[p], n


def reference_reduce(x, R, aggr, ptr, member, group_of, copies):
    """float64: (out, sum|x| per group, count per group, dx, sum|terms| per source row)"""
    xs = x[:, member]
    count = np.diff(ptr)
    absum = np.add.reduceat(np.abs(xs), ptr[:-1], axis=1)
    if aggr in ("+", "mean"):
        out = np.add.reduceat(xs, ptr[:-1], axis=1)
        if aggr == "mean":
            out = out / count
    else:
        out = (np.maximum if aggr == "max" else np.minimum).reduceat(xs, ptr[:-1], axis=1)
    e = x.shape[1]
    dx, dabs = np.zeros_like(x), np.zeros_like(x)
    for c in range(copies):
        grp = group_of[c * e:(c + 1) * e]
        term = R[:, grp]
        if aggr == "mean":
            term = term / count[grp]
        if aggr in ("max", "min"):
            term = term * (x == out[:, grp])
        dx += term
        dabs += np.abs(term)
    return out, absum, count, dx, dabs


# remove_multi_edges with each aggregation, and to_bidirected (which combines with mean)
@pytest.mark.parametrize("aggr,sym", [("+", False), ("mean", False), ("max", False), ("min", False), ("mean", True)])
@pytest.mark.parametrize("d", [1, 3, 4, 64, 67])
def test_feature_reduction_against_float64(d, aggr, sym):
    s, t, n = grouped_graph()
    e = s.size
    rng = np.random.default_rng(100 + d)
    x = rng.normal(size=(d, e)).astype(np.float32)
    w = rng.uniform(0.5, 1.5, e).astype(np.float32)
    so, to, ptr, member, group_of = np_coalesce(s, t, n, sym)
    assert {1, 2, 5, 300} <= set(np.diff(ptr).tolist()) or sym
    xt = torch.as_tensor(x, device=DEV).requires_grad_(True)
    wt = torch.as_tensor(w, device=DEV).requires_grad_(True)
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, edata={"e": xt}, edge_weight=wt)
    R = rng.normal(size=(d, so.size))
    Rw = rng.normal(size=(1, so.size))

    def run():
        xt.grad = wt.grad = None
        out = ng.to_bidirected(g) if sym else ng.remove_multi_edges(g, aggr)
        y, yw = out.edata["e"], out.edge_weight
        ((y * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum() + (yw * torch.as_tensor(Rw[0], dtype=torch.float32, device=DEV)).sum()).backward()
        return out, y.detach().clone(), yw.detach().clone(), xt.grad.clone(), wt.grad.clone()

    out, y, yw, dx, dw = run()
    same_edges(out, so, to, "edges")
    assert tuple(y.shape) == (d, so.size) and tuple(yw.shape) == (so.size,) and y.is_cuda
    R32, Rw32 = R.astype(np.float32).astype(np.float64), Rw.astype(np.float32).astype(np.float64)
    for got, dgot, src, cot in ((y, dx, x, R32), (yw.reshape(1, -1), dw.reshape(1, -1), w.reshape(1, -1), Rw32)):
        ref, absum, count, dref, dabs = reference_reduce(src.astype(np.float64), cot, aggr, ptr, member, group_of, 2 if sym else 1)
        got, dgot = got.cpu().double().numpy(), dgot.cpu().double().numpy()
        if aggr in ("max", "min"):
            assert np.array_equal(got, ref)
        else:
            err, bound = np.abs(got - ref), count * EPS * absum
            print(f"d={d} aggr={aggr} sym={sym}: forward max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
            assert (err <= bound).all()
        derr, dbound = np.abs(dgot - dref), 4 * EPS * dabs
        print(f"d={d} aggr={aggr} sym={sym}: pullback max err/bound {np.max(derr / np.maximum(dbound, 1e-300)):.3f}")
        assert (derr <= dbound).all()
    # the same bits on a second run, forward and backward
    _, y2, yw2, dx2, dw2 = run()
    assert torch.equal(y, y2) and torch.equal(yw, yw2) and torch.equal(dx, dx2) and torch.equal(dw, dw2)


def test_one_group_of_65536_members():
    s, t, n = CASES["one_pair_65536"]
    e = s.size
    rng = np.random.default_rng(9)
    x = rng.normal(size=(3, e)).astype(np.float32)
    for aggr in ("+", "mean", "max", "min"):
        xt = torch.as_tensor(x, device=DEV).requires_grad_(True)
        out = ng.remove_multi_edges(ng.GNNGraph(s, t, num_nodes=n, index_base=0, edata={"e": xt}), aggr)
        y = out.edata["e"]
        assert tuple(y.shape) == (3, 1)
        y.sum().backward()
        x64 = x.astype(np.float64)
        got = y.detach().cpu().double().numpy()[:, 0]
        if aggr in ("max", "min"):
            ref = x64.max(1) if aggr == "max" else x64.min(1)
            assert np.array_equal(got, ref)
            assert np.array_equal(xt.grad.cpu().numpy(), (x64 == ref[:, None]).astype(np.float32))
        else:
            ref = x64.sum(1) / (e if aggr == "mean" else 1)
            assert (np.abs(got - ref) <= e * EPS * np.abs(x64).sum(1)).all()
            assert np.array_equal(xt.grad.cpu().numpy(), np.full((3, e), 1.0 / e if aggr == "mean" else 1.0, dtype=np.float32))


def test_gradients_follow_selected_features():
    rng = np.random.default_rng(13)
    n, e = 30, 200
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    s[:10] = t[:10]                                                     # some self loops
    xe = torch.randn(5, e, device=DEV, requires_grad=True)
    xn = torch.randn(2, n, device=DEV, requires_grad=True)
    w = torch.rand(e, device=DEV, requires_grad=True)
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, ndata={"x": xn}, edata={"e": xe}, edge_weight=w)
    keep = np.flatnonzero(s != t)
    gr = ng.remove_self_loops(g)
    assert torch.equal(gr.edata["e"], xe.detach()[:, keep]) and torch.equal(gr.edge_weight, w.detach()[keep])
    (gr.edata["e"].sum() * 2 + gr.edge_weight.sum() * 3).backward()
    mask = torch.as_tensor((s != t).astype(np.float32), device=DEV)
    assert torch.equal(xe.grad, (2 * mask).expand(5, e)) and torch.equal(w.grad, 3 * mask)
    xe.grad = w.grad = None
    nodes = rng.permutation(n)[:12]
    si, ti, kept = np_induced(s, t, n, nodes)
    gi = ng.induced_subgraph(g, nodes)
    assert torch.equal(gi.ndata["x"], xn.detach()[:, nodes]) and torch.equal(gi.edata["e"], xe.detach()[:, kept])
    (gi.ndata["x"].sum() + gi.edata["e"].sum()).backward()
    nm, em = np.zeros(n, dtype=np.float32), np.zeros(e, dtype=np.float32)
    nm[nodes], em[kept] = 1, 1
    assert torch.equal(xn.grad, torch.as_tensor(nm, device=DEV).expand(2, n)) and torch.equal(xe.grad, torch.as_tensor(em, device=DEV).expand(5, e))
    ga = ng.add_self_loops(ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=w))
    w.grad = None
    (ga.edge_weight * torch.arange(e + n, device=DEV)).sum().backward()
    assert torch.equal(w.grad, torch.arange(e, device=DEV, dtype=torch.float32))


# ---- as the graph of a NeuralODE ----------------------------------------------------------------------------------------------------


class UserConv(ng.AbstractGNNContainerLayer):
    """a right-hand side written on ng.propagate: h'_i = mean_j phi([h_i; h_j - h_i])"""

    layers = ("ϕ",)

    def __init__(self, ϕ, *, initialgraph=None):
        self.ϕ = ϕ
        self.initialgraph = ng.wrapgraph(initialgraph if initialgraph is not None else (lambda: ng.EMPTYGRAPH))

    def __call__(self, x, ps, st):
        def message(xi, xj, e):
            return self.ϕ(torch.cat([xi, xj - xi], dim=0), ps, st["ϕ"])[0]

        return ng.propagate(message, st["graph"], "mean", xi=x, xj=x), st


@pytest.mark.parametrize("sym", [False, True])
def test_results_as_neural_ode_graph(sym):
    s, t, n = CASES["multigraph"]
    s, t, n = s[:4000] % 300, t[:4000] % 300, 300
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    gd = ng.to_bidirected(g) if sym else ng.remove_multi_edges(g)
    so, to = np_coalesce(s, t, n, sym)[:2]
    twin = ng.GNNGraph(so, to, num_nodes=n, index_base=0)
    h = 4
    u0 = torch.randn(h, n, device=DEV)
    res = []
    for graph in (gd, twin):
        phi = ng.Chain(ng.Dense(2 * h, 16, "tanh"), ng.Dense(16, h, "tanh"))
        node = ng.NeuralODE(UserConv(phi, initialgraph=graph), solver="tsit5", n_steps=4)
        ps, st = ng.setup(5, node)
        ps = ng.to_device(ps, DEV)
        for lp in ps.values():
            for v in lp.values():
                v.requires_grad_(True)
        u = u0.clone().requires_grad_(True)
        uT, _ = node(u, ps, st)
        uT.sum().backward()                                            # one forward + backward completes
        assert bool(torch.isfinite(uT).all()) and bool(torch.isfinite(u.grad).all()) and bool(u.grad.abs().sum() > 0)
        res.append((uT.detach(), u.grad))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
