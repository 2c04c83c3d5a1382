"""GPU tests of the per-graph readouts (reduce_nodes / reduce_edges, softmax_nodes / softmax_edges, broadcast_nodes / broadcast_edges,
/root/reference/src/NeuralGraphPDE.jl:5-7) against float64 numpy: oracle.scatter / scatter_pullback / gather with the graph indicator
as the index, and a float64 softmax written here.

Tolerances as test_msgpass_gpu.py: forward 1e-4 * max|ref| + 1e-5, gradients 5e-4 relative.  The softmax is also held to
|y - ref| <= 1e-4 * ref element by element, so a wrong denominator cannot hide behind max|ref|; with logits of +-80 that bound applies
to the entries float32 can hold at all (ref >= 2^-126: below it the float64 reference has no float32 counterpart and the
max-relative bound alone applies).  An fp32 emulation of the chunked sum (256-row chunks, four accumulators, partials folded in
order) sits at 6.3e-5 against a bound of 3.6e-2 on 16 384 x 64 and at 3.8e-5 against 2.0e-2 on 24 x 3 000 x 64.

Graphs: (a) the reference's 3-node graph, (b) a batch of five graphs of 1, 7, 40, 300 and 1 000 nodes -- a single-row, a one-chunk and
a multi-chunk segment --, (c) the same graph with nodes and edges shuffled and the indicator given to the constructor (the permuted
plan), (d) an indicator with an empty graph in the middle and graphs without edges, (e) radius_graph over three clouds next to the same
graph built by hand, (f) 16 384 nodes in one graph and a batch of 24 graphs of 3 000 nodes.
"""
import functools
import gc
import zlib

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from oracle import ngpde_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
AGGRS = ["+", "mean", "max", "min"]
WIDTHS = (1, 3, 64, 130)


def close(a, ref, rtol=1e-4, atol=1e-5, what=""):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    ref = np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], ref[~fin]), f"{what}: non-finite entries differ"
    err = np.abs(a[fin] - ref[fin]).max() if fin.any() else 0.0
    bound = rtol * (np.abs(ref[fin]).max() if fin.any() else 0.0) + atol
    print(f"{what}: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def gclose(a, ref, what=""):
    close(a, ref, rtol=5e-4, atol=1e-6, what=what)


def dev(a, grad=True):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=DEV).requires_grad_(grad)


def host(t):
    return t.detach().cpu().double().numpy()


# ---- the graphs -------------------------------------------------------------------------------------------------------------------


def random_member(rng, n, e):
    return ng.GNNGraph(rng.integers(0, n, e), rng.integers(0, n, e), num_nodes=n, index_base=0)


def five():
    rng = np.random.default_rng(11)
    return ng.batch([random_member(rng, n, e) for n, e in ((1, 0), (7, 20), (40, 150), (300, 1200), (1000, 5000))])


def shuffled_five():
    """(c): (b) with node i renamed p[i] and the edges reordered by q; returns the graph, p and q"""
    b = five()
    rng = np.random.default_rng(12)
    p, q = rng.permutation(b.num_nodes), rng.permutation(b.num_edges)
    s0, t0 = b.edge_index(index_base=0)
    gi = np.empty(b.num_nodes, dtype=np.int64)
    gi[p] = b.graph_indicator
    g = ng.GNNGraph(p[s0][q], p[t0][q], num_nodes=b.num_nodes, index_base=0, graph_indicator=gi, num_graphs=b.num_graphs)
    return g, p, q


def with_empty():
    """(d): graph 3 of 4 has no nodes; graphs 3 and 4 have no edges"""
    rng = np.random.default_rng(13)
    gi = np.array([0] * 20 + [1] * 20 + [3] * 10)
    s = np.concatenate([rng.integers(0, 20, 60), rng.integers(20, 40, 70)])
    t = np.concatenate([rng.integers(0, 20, 60), rng.integers(20, 40, 70)])
    return ng.GNNGraph(s, t, num_nodes=50, index_base=0, graph_indicator=gi, num_graphs=4)


def clouds():
    rng = np.random.default_rng(14)
    sizes = (60, 200, 500)
    P = rng.random((2, sum(sizes)))
    gi1 = np.repeat([1, 2, 3], sizes)
    return P, gi1


@functools.lru_cache(maxsize=None)
def graph(name):
    if name == "reference":
        return ng.GNNGraph([1, 1, 2, 3], [2, 3, 1, 1], num_nodes=3)                  # test/runtests.jl:11-13
    if name == "five":
        return five()
    if name == "shuffled":
        return shuffled_five()[0]
    if name == "empty":
        return with_empty()
    if name == "radius":
        P, gi1 = clouds()
        return ng.radius_graph(P, 0.08, graph_indicator=gi1)
    if name == "bench":
        rng = np.random.default_rng(15)
        return random_member(rng, 16384, 65536)
    if name == "vmh":
        rng = np.random.default_rng(16)
        return ng.batch([random_member(rng, 3000, 6000) for _ in range(24)])
    raise KeyError(name)


GRAPHS = ["reference", "five", "shuffled", "empty", "radius", "bench", "vmh"]


def segments(g, kind):
    """(0-based segment id per item, number of items, number of segments)"""
    idx = ng.graph_indicator(g, edges=(kind == "edges")).astype(np.int64) - 1
    return idx, idx.size, g.num_graphs


REDUCE = {"nodes": ng.reduce_nodes, "edges": ng.reduce_edges}
SOFTMAX = {"nodes": ng.softmax_nodes, "edges": ng.softmax_edges}
BROADCAST = {"nodes": ng.broadcast_nodes, "edges": ng.broadcast_edges}


def seeded(*parts):
    return np.random.default_rng(zlib.crc32(" ".join(str(p) for p in parts).encode()))


def masked_backward(y, R):
    """sum(y .* R) over the finite entries of y, backpropagated"""
    (torch.where(torch.isfinite(y), y, torch.zeros_like(y)) * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()


# ---- reduce -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["nodes", "edges"])
@pytest.mark.parametrize("aggr", AGGRS)
@pytest.mark.parametrize("name", GRAPHS)
def test_reduce_against_float64(name, aggr, kind):
    g = graph(name)
    idx, n, S = segments(g, kind)
    rng = seeded(name, aggr, kind)
    for D in WIDTHS:
        x = rng.normal(size=(D, n))
        xt = dev(x)
        y = REDUCE[kind](aggr, g, xt)
        assert tuple(y.shape) == (D, S)
        yo = O.scatter(aggr, x, idx, S)
        close(y, yo, what=f"{kind} {aggr} D={D}")
        R = rng.normal(size=yo.shape)
        masked_backward(y, R)
        dxo = O.scatter_pullback(aggr, x, idx, S, yo, np.where(np.isfinite(yo), R, 0.0))
        gclose(xt.grad, dxo, what=f"dx {kind} {aggr} D={D}")


@pytest.mark.parametrize("kind", ["nodes", "edges"])
@pytest.mark.parametrize("aggr", ["max", "min"])
@pytest.mark.parametrize("name", GRAPHS)
def test_tied_extrema_each_receive_the_gradient(name, aggr, kind):
    g = graph(name)
    idx, n, S = segments(g, kind)
    rng = seeded("ties", name, aggr, kind)
    for D in (1, 64):
        x = rng.integers(-2, 3, size=(D, n)).astype(np.float64)          # five values: every extremum is tied many times over
        xt = dev(x)
        y = REDUCE[kind](aggr, g, xt)
        yo = O.scatter(aggr, x, idx, S)
        close(y, yo, what=f"{kind} {aggr} D={D}")
        R = rng.normal(size=yo.shape)
        masked_backward(y, R)
        dxo = O.scatter_pullback(aggr, x, idx, S, yo, np.where(np.isfinite(yo), R, 0.0))
        if n >= 20 * S:
            assert (dxo != 0).sum() > np.isfinite(yo).sum()               # ties there are
        gclose(xt.grad, dxo, what=f"dx {kind} {aggr} D={D}")


def test_shuffled_graph_agrees_with_the_batch():
    b, (c, p, q) = graph("five"), shuffled_five()
    rng = np.random.default_rng(5)
    x, e = rng.normal(size=(64, b.num_nodes)), rng.normal(size=(64, b.num_edges))
    xc, ec = np.empty_like(x), e[:, q]
    xc[:, p] = x
    for aggr in AGGRS:
        close(ng.reduce_nodes(aggr, c, dev(xc, False)), host(ng.reduce_nodes(aggr, b, dev(x, False))), what=f"nodes {aggr}")
        close(ng.reduce_edges(aggr, c, dev(ec, False)), host(ng.reduce_edges(aggr, b, dev(e, False))), what=f"edges {aggr}")
    close(ng.softmax_nodes(c, dev(xc, False))[:, torch.as_tensor(p, device=DEV)], host(ng.softmax_nodes(b, dev(x, False))), what="softmax nodes")
    close(ng.softmax_edges(c, dev(ec, False)), host(ng.softmax_edges(b, dev(e, False)))[:, q], what="softmax edges")
    u = rng.normal(size=(64, b.num_graphs))
    assert torch.equal(ng.broadcast_nodes(c, dev(u, False))[:, torch.as_tensor(p, device=DEV)], ng.broadcast_nodes(b, dev(u, False)))


def test_radius_graph_keeps_its_indicator():
    g = graph("radius")
    P, gi1 = clouds()
    s1, t1 = g.edge_index()
    assert g.num_graphs == 3 and g.num_edges > 0 and np.array_equal(ng.graph_indicator(g), gi1)
    hand = ng.GNNGraph(s1, t1, num_nodes=g.num_nodes, graph_indicator=gi1)
    k = ng.knn_graph(P, 3, graph_indicator=gi1)
    assert np.array_equal(ng.graph_indicator(k), gi1)
    rng = np.random.default_rng(6)
    x, e = dev(rng.normal(size=(64, g.num_nodes)), False), dev(rng.normal(size=(3, g.num_edges)), False)
    for aggr in AGGRS:
        assert torch.equal(ng.reduce_nodes(aggr, g, x), ng.reduce_nodes(aggr, hand, x))
        assert torch.equal(ng.reduce_edges(aggr, g, e), ng.reduce_edges(aggr, hand, e))
    assert torch.equal(ng.softmax_nodes(g, x), ng.softmax_nodes(hand, x)) and torch.equal(ng.softmax_edges(g, e), ng.softmax_edges(hand, e))
    close(ng.reduce_nodes("+", k, x), O.scatter("+", host(x), gi1 - 1, 3), what="knn_graph")


# ---- softmax ------------------------------------------------------------------------------------------------------------------------


def softmax_ref(x, idx, S):
    mx = O.scatter("max", x, idx, S)
    z = np.exp(x - O.gather(mx, idx))
    return z / O.gather(O.scatter("+", z, idx, S), idx)


F32_TINY = float(np.finfo(np.float32).tiny)


def elementwise(y, yo, what, every=False):
    """|y - ref| <= 1e-4 ref wherever float32 holds ref; every: that is every entry, so the bound leaves none out"""
    a = host(y)
    rep = yo >= F32_TINY
    assert rep.all() or not every, f"{what}: {int((~rep).sum())} reference entries below float32's smallest normal"
    err = (np.abs(a - yo)[rep] / yo[rep]).max(initial=0.0)
    print(f"{what}: max elementwise relative err {err:.3e}")
    assert err <= 1e-4, f"{what}: elementwise relative err {err:.3e}"


@pytest.mark.parametrize("kind", ["nodes", "edges"])
@pytest.mark.parametrize("name", GRAPHS)
def test_softmax_against_float64(name, kind):
    g = graph(name)
    idx, n, S = segments(g, kind)
    rng = seeded("softmax", name, kind)
    for D in WIDTHS:
        x = rng.normal(size=(D, n)) * 3
        xt = dev(x)
        y = SOFTMAX[kind](g, xt)
        yo = softmax_ref(x, idx, S)
        close(y, yo, what=f"{kind} D={D}")
        elementwise(y, yo, f"{kind} D={D}", every=True)
        sums = O.scatter("+", host(y), idx, S)
        filled = np.bincount(idx, minlength=S) > 0
        assert np.abs(sums[:, filled] - 1).max(initial=0) < 1e-5
        R = rng.normal(size=(D, n))
        (y * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
        dxo = yo * (R - O.gather(O.scatter("+", yo * R, idx, S), idx))
        gclose(xt.grad, dxo, what=f"dx {kind} D={D}")


@pytest.mark.parametrize("kind", ["nodes", "edges"])
@pytest.mark.parametrize("name", GRAPHS)
def test_softmax_large_logits_stay_finite(name, kind):
    g = graph(name)
    idx, n, S = segments(g, kind)
    rng = seeded("large", name, kind)
    x = rng.choice([-80.0, 80.0], size=(4, n)) + rng.normal(size=(4, n))
    xt = dev(x)
    y = SOFTMAX[kind](g, xt)
    assert torch.isfinite(y).all()
    yo = softmax_ref(host(xt), idx, S)                  # (of the float32 logits the kernel saw: rounding +-80.x moves exp by 4e-6)
    close(y, yo, what=kind)
    elementwise(y, yo, kind)
    y.sum().backward()
    assert torch.isfinite(xt.grad).all()
    if kind == "edges":
        yv = ng.softmax_edges(g, dev(x[0], False))      # a vector of logits: a vector back
        assert tuple(yv.shape) == (n,)
        close(yv, yo[0], what="vector of logits")


# ---- broadcast ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["nodes", "edges"])
@pytest.mark.parametrize("name", GRAPHS)
def test_broadcast_is_indexing(name, kind):
    g = graph(name)
    idx, n, S = segments(g, kind)
    rng = seeded("broadcast", name, kind)
    for D in WIDTHS:
        u = rng.normal(size=(D, S))
        ut = dev(u)
        y = BROADCAST[kind](g, ut)
        assert tuple(y.shape) == (D, n)
        assert torch.equal(y.detach(), ut.detach()[:, torch.as_tensor(idx, device=DEV)])
        R = rng.normal(size=(D, n))
        (y * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
        gclose(ut.grad, O.scatter("+", R.astype(np.float32).astype(np.float64), idx, S), what=f"du {kind} D={D}")


# ---- argument errors ----------------------------------------------------------------------------------------------------------------


def test_argument_errors():
    g = graph("five")
    N, E, S = g.num_nodes, g.num_edges, g.num_graphs
    x, e, u = dev(np.zeros((4, N)), False), dev(np.zeros((4, E)), False), dev(np.zeros((4, S)), False)
    with pytest.raises(ng.DimensionMismatch, match=f"{N - 1} columns.*{N} nodes"):
        ng.reduce_nodes("+", g, x[:, :-1])
    with pytest.raises(ng.DimensionMismatch, match=f"{N} columns.*{E} edges"):
        ng.reduce_edges("mean", g, x)
    with pytest.raises(ng.DimensionMismatch, match=f"{E} columns.*{N} nodes"):
        ng.softmax_nodes(g, e)
    with pytest.raises(ng.DimensionMismatch, match=f"{E - 1} columns.*{E} edges"):
        ng.softmax_edges(g, e[0, :-1])
    with pytest.raises(ng.DimensionMismatch, match=f"{N} columns.*{S} graphs"):
        ng.broadcast_nodes(g, x)
    with pytest.raises(ng.DimensionMismatch, match=f"{S + 1} columns.*{S} graphs"):
        ng.broadcast_edges(g, dev(np.zeros((4, S + 1)), False))
    for bad in ("*", "mul", "prod"):
        with pytest.raises(ng.ArgumentError, match="aggregation"):
            ng.reduce_nodes(bad, g, x)
        with pytest.raises(ng.ArgumentError, match="aggregation"):
            ng.reduce_edges(bad, g, e)
    s0, t0 = g.edge_index(index_base=0)
    blind = ng.GNNGraph(s0, t0, num_nodes=N, index_base=0, num_graphs=S)        # what the padded batch of batches.py looks like
    for call in (lambda: ng.reduce_nodes("+", blind, x), lambda: ng.reduce_edges("+", blind, e), lambda: ng.softmax_nodes(blind, x),
                 lambda: ng.softmax_edges(blind, e), lambda: ng.broadcast_nodes(blind, u), lambda: ng.broadcast_edges(blind, u)):
        with pytest.raises(ng.ArgumentError, match="graph_indicator"):
            call()
    with pytest.raises(ng.ArgumentError):
        ng.reduce_nodes("+", g, x.cpu())                                       # no CPU fallback


# ---- reproducibility ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", ["five", "shuffled", "bench", "vmh"])
def test_every_function_is_bitwise_reproducible(name):
    g = graph(name)
    rng = np.random.default_rng(21)
    N, E, S = g.num_nodes, g.num_edges, g.num_graphs
    x, e, u = rng.normal(size=(64, N)), rng.normal(size=(3, E)), rng.normal(size=(64, S))

    def run():
        outs, leaves = [], []
        for aggr in AGGRS:
            xt, et = dev(x), dev(e)
            outs += [ng.reduce_nodes(aggr, g, xt), ng.reduce_edges(aggr, g, et)]
            leaves += [xt, et]
        xt, et, un, ue = dev(x), dev(e), dev(u), dev(u)
        outs += [ng.softmax_nodes(g, xt), ng.softmax_edges(g, et), ng.broadcast_nodes(g, un), ng.broadcast_edges(g, ue)]
        leaves += [xt, et, un, ue]
        sum((torch.where(torch.isfinite(o), o, torch.zeros_like(o)) * (k + 1)).sin().sum() for k, o in enumerate(outs)).backward()
        return [o.detach().cpu() for o in outs] + [v.grad.cpu() for v in leaves]

    a, b = run(), run()
    assert len(a) == 24
    for k, (p, q) in enumerate(zip(a, b)):
        assert torch.equal(p, q), k


# ---- HIP-graph capture --------------------------------------------------------------------------------------------------------------


def test_capture_replays_the_eager_result():
    g = graph("vmh")
    rng = np.random.default_rng(22)
    N, S = g.num_nodes, g.num_graphs
    x = dev(rng.normal(size=(64, N)))
    Rm, Rs = dev(rng.normal(size=(64, S)), False), dev(rng.normal(size=(64, N)), False)

    def step():
        m, y = ng.reduce_nodes("mean", g, x), ng.softmax_nodes(g, x)
        gm, = torch.autograd.grad([m], [x], [Rm])
        gy, = torch.autograd.grad([y], [x], [Rs])
        return m, y, gm, gy

    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    gc_was = gc.isenabled()
    gc.disable()                                    # (a finaliser that frees device memory must not run inside the capture)
    try:
        with torch.cuda.graph(gr):
            outs = step()
    finally:
        if gc_was:
            gc.enable()
    for _ in range(2):
        for t in outs:
            t.detach().zero_()
        gr.replay()
        torch.cuda.synchronize()
        for a, b in zip(outs, eager):
            assert torch.equal(a.detach(), b)


# ---- inside a model -----------------------------------------------------------------------------------------------------------------


def test_readout_loss_through_a_neural_ode():
    d, n_steps = 16, 4
    rng = np.random.default_rng(23)
    g = ng.batch([random_member(rng, n, e) for n, e in ((30, 120), (45, 200), (12, 40), (70, 300))])
    s0, t0 = g.edge_index(index_base=0)
    og = O.Graph(s0, t0, num_nodes=g.num_nodes, index_base=0)
    idx, N, S = segments(g, "nodes")
    rhs = ng.Chain(ng.GCNConv((d, d), "relu", initialgraph=g), ng.GCNConv((d, d), "relu", initialgraph=g))
    node = ng.NeuralODE(rhs, solver="tsit5", n_steps=n_steps)
    ps, st = ng.setup(7, node)
    ps = ng.to_device(ps, DEV)
    for lp in ps.values():
        for v in lp.values():
            v.requires_grad_(True)
    u0 = rng.normal(size=(d, N))
    ut = dev(u0)
    uT, _ = node(ut, ps, st)
    R = rng.normal(size=(d, S))
    loss = (ng.reduce_nodes("mean", g, uT) * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum()
    loss.backward()

    params = [dict(weight=host(ps[k]["weight"]), bias=host(ps[k]["bias"])) for k in ("layer_1", "layer_2")]
    orhs, ovjp = O.gcn2_rhs(params, og, "relu")
    dt = 1.0 / n_steps
    uTo, tape = O.rk_solve(orhs, host(ut), O.TSIT5, dt, n_steps)
    close(uT, uTo, what="u(T)")
    mo = O.scatter("mean", uTo, idx, S)
    assert abs(float(loss.detach()) - float((mo * R).sum())) <= 1e-4 * np.abs(mo * R).sum() + 1e-5
    duT = O.scatter_pullback("mean", uTo, idx, S, mo, R)
    du0 = O.rk_adjoint(ovjp, tape, duT, O.TSIT5, dt, lambda pg: None)
    gclose(ut.grad, du0, what="du0")
