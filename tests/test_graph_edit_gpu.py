"""GPU tests of the graph editing and negative sampling (editing.py over csrc/graph_edit.hip; src/NeuralGraphPDE.jl:4 of the reference
re-exports add_nodes, add_edges, remove_edges, remove_nodes, to_unidirected, set_edge_weight and negative_sample from GNNGraphs).

Everything here is integer work and the features are moved, not recomputed, so every comparison is exact: the edited edge lists
INCLUDING THEIR ORDER against numpy restatements, the negative samples against a numpy restatement of the candidate sequence (Philox4x32-10
restated here as in test_sampling_gpu.py, stream 4, Python-integer multiply-high), moved features against plain indexing and their
gradients against counts.  The one place where floats are combined is to_unidirected's mean over a pair's copies; its bound is derived
where it is used.  The two frequency checks run over fixed seeds, so their outcome is deterministic; their 5-sigma caps are those of
the binomial distribution of one slot's count.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"

SIZES = [(n, e) for n in (1, 2, 300) for e in (0, 1, 255, 256, 257, 1000)] + [(100003, 1000)]          # the last: s * n + t needs 64 bits

# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK, S32 = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(c, k):
    c = [np.asarray(x, dtype=np.uint64) for x in c]
    k0, k1 = int(k[0]), int(k[1])
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def draw(seed, stream, c0, c1):
    """the 64-bit draw at counter (lo32(c0), lo32(c1), stream, 0)"""
    c0 = np.asarray(c0, dtype=np.uint64)
    c1 = np.broadcast_to(np.asarray(c1, dtype=np.uint64), c0.shape)
    o = philox4x32_10([c0 & MASK, c1 & MASK, np.full(c0.shape, stream, np.uint64), np.zeros(c0.shape, np.uint64)],
                      [seed & 0xFFFFFFFF, seed >> 32])
    return o[0] | (o[1] << S32)


def np_negative(s, t, n, n_target, bidirected, seed):
    """the first n_target distinct negatives of the candidate sequence, in sequence order: (a list, b list)"""
    u = n * (n - 1)
    edges = set(zip(s.tolist(), t.tolist()))
    out, seen, first = [], set(), 0
    while len(out) < n_target:
        j = np.arange(first, first + 512, dtype=np.uint64)
        for d in draw(seed, 4, j & MASK, j >> S32):
            c = (int(d) * u) >> 64
            a, b = c // (n - 1), c % (n - 1)
            b += b >= a
            if bidirected:
                a, b = min(a, b), max(a, b)
            if (a, b) in seen or (a, b) in edges or (bidirected and (b, a) in edges):
                continue
            seen.add((a, b))
            out.append((a, b))
            if len(out) == n_target:
                break
        first += 512
        assert first < 1 << 22, "the restatement found too few negatives"
    a = np.asarray([p[0] for p in out], dtype=np.int64)
    b = np.asarray([p[1] for p in out], dtype=np.int64)
    return (np.concatenate([a, b]), np.concatenate([b, a])) if bidirected else (a, b)


def np_unidirected(s, t, n):
    key = np.unique(np.minimum(s, t) * n + np.maximum(s, t))
    return key // n, key % n


def random_graph(n, e, seed, **kw):
    """e random edges on n nodes, an eighth of them parallel copies of earlier ones and an eighth reverses"""
    rng = np.random.default_rng(seed)
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    k = e // 8
    if k:
        s[-k:], t[-k:] = s[:k], t[:k]
        s[-2 * k:-k], t[-2 * k:-k] = t[k:2 * k], s[k:2 * k]
    return s, t, ng.GNNGraph(s, t, num_nodes=n, index_base=0, **kw)


def check_edges(g, s, t, n):
    """g has n nodes and exactly the edges (s, t) in this order, on the host and in the device lists the handle builder takes"""
    gs, gt = g.edge_index(index_base=0)
    assert g.num_nodes == n and g.num_edges == len(s)
    assert np.array_equal(gs, s) and np.array_equal(gt, t)
    coo = g._shared[("coo", str(torch.device("cuda", torch.cuda.current_device())))]
    assert coo[0].dtype == torch.int32 and np.array_equal(coo[0].cpu().numpy(), s) and np.array_equal(coo[1].cpu().numpy(), t)


def c_negative(s, t, n, n_target, bidirected, seed, chunk):
    """ngpde_coo_negative_sample itself: (s, t) of the result"""
    sd = torch.as_tensor(s.astype(np.int32), device=DEV)
    td = torch.as_tensor(t.astype(np.int32), device=DEV)
    m = n_target * (2 if bidirected else 1)
    so = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    to = torch.full((m,), -7, dtype=torch.int32, device=DEV)
    n_out = C.c_int64(0)
    _lib.check(_lib.load().ngpde_coo_negative_sample(n, s.size, _lib.ptr(sd), _lib.ptr(td), 0, n_target, int(bidirected), seed, chunk, _lib.ptr(so),
                                                     _lib.ptr(to), C.byref(n_out), _lib.current_stream()))
    assert n_out.value == m
    return so.cpu().numpy().astype(np.int64), to.cpu().numpy().astype(np.int64)


# ---- 1. removing edges ----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,e", SIZES)
def test_remove_edges(n, e):
    s, t, g = random_graph(n, e, 100 + e)
    rng = np.random.default_rng(n + e)
    everything = np.arange(e)
    for positions in (np.zeros(0, np.int64), rng.integers(0, max(e, 1), e // 3 + 1)[:e], np.repeat(rng.permutation(e)[:e // 2], 2), everything):
        keep = np.setdiff1d(everything, positions)
        check_edges(ng.remove_edges(g, positions), s[keep], t[keep], n)
    # pairs: some the graph has (with every parallel copy), some it has not, some listed twice
    picked = rng.permutation(e)[:e // 4 + 1][:e]
    ls = np.concatenate([s[picked], rng.integers(0, n, 5), s[picked][:3]])
    lt = np.concatenate([t[picked], rng.integers(0, n, 5), t[picked][:3]])
    gone = np.isin(s * n + t, ls * n + lt)
    assert gone[picked].all()
    by_pairs = ng.remove_edges(g, ls, lt)
    check_edges(by_pairs, s[~gone], t[~gone], n)
    assert by_pairs == ng.remove_edges(g, np.flatnonzero(gone))          # the two forms agree
    if e >= 16:          # (random_graph made parallel copies: they went with their originals)
        assert gone.sum() > np.unique((s * n + t)[gone]).size
    check_edges(ng.remove_edges(g, np.zeros(0, np.int64), np.zeros(0, np.int64)), s, t, n)
    check_edges(ng.remove_edges(g, s, t), s[:0], t[:0], n)
    check_edges(ng.remove_edges(g, torch.as_tensor(ls, device=DEV), torch.as_tensor(lt)), s[~gone], t[~gone], n)


def test_remove_edges_refuses_bad_lists():
    s, t, g = random_graph(300, 257, 1)
    for positions in ([-1], [257], [0, 1, 2 ** 40], torch.tensor([3, 300])):
        with pytest.raises(ng.ArgumentError, match="position"):
            ng.remove_edges(g, positions)
    for ls, lt in (([0, 300], [1, 2]), ([0], [-1]), ([2 ** 40], [0])):
        with pytest.raises(ng.ArgumentError, match="listed pair"):
            ng.remove_edges(g, ls, lt)
    with pytest.raises(ng.ArgumentError, match="position"):
        ng.remove_edges(random_graph(3, 0, 1)[2], [0])          # no edge, no position
    with pytest.raises(ng.DimensionMismatch):
        ng.remove_edges(g, [0, 1], [1])


# ---- 2. removing and adding nodes ------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,e", SIZES)
def test_remove_nodes(n, e):
    rng = np.random.default_rng(7 * n + e)
    x = rng.normal(size=(3, n)).astype(np.float32)
    lab = rng.integers(0, 9, (1, e))
    s, t, g = random_graph(n, e, 200 + e, ndata={"x": x}, edata={"lab": lab})
    for nodes in (np.zeros(0, np.int64), np.repeat(rng.permutation(n)[:n // 3 + 1], 2), rng.integers(0, n, n)):
        rest = np.setdiff1d(np.arange(n), nodes)
        got = ng.remove_nodes(g, nodes)
        if rest.size:
            assert got == ng.induced_subgraph(g, rest)
        relabel = np.full(n, -1)
        relabel[rest] = np.arange(rest.size)
        keep = (relabel[s] >= 0) & (relabel[t] >= 0)
        check_edges(got, relabel[s[keep]], relabel[t[keep]], rest.size)
        assert np.array_equal(got.ndata["x"].cpu().numpy(), x[:, rest]) and np.array_equal(got.edata["lab"], lab[:, keep])
    got = ng.remove_nodes(g, torch.arange(n))          # a list that names everything
    check_edges(got, s[:0], t[:0], 0)
    assert tuple(got.ndata["x"].shape) == (3, 0) and tuple(got.edata["lab"].shape) == (1, 0)


def test_remove_nodes_of_a_batch():
    members = [random_graph(n, e, 300 + n, ndata={"x": np.full((1, n), float(n), np.float32)})[2] for n, e in ((7, 15), (3, 4), (12, 40))]
    gb = ng.batch(members)
    nodes = [0, 3, 7, 8, 9, 15]          # the second member (nodes 7, 8, 9) goes entirely
    got = ng.remove_nodes(gb, nodes)
    rest = np.setdiff1d(np.arange(22), nodes)
    assert got == ng.induced_subgraph(gb, rest) and got.num_graphs == 3
    assert np.array_equal(got.graph_indicator, gb.graph_indicator[rest]) and 1 not in got.graph_indicator
    for bad in ([22], [-1], [0, 2 ** 40]):
        with pytest.raises(ng.ArgumentError, match="outside"):
            ng.remove_nodes(gb, bad)


@pytest.mark.parametrize("n,e", [(1, 0), (2, 1), (300, 257), (100003, 1000)])
def test_add_nodes(n, e):
    rng = np.random.default_rng(n)
    x = torch.as_tensor(rng.normal(size=(2, n)).astype(np.float32), device=DEV).requires_grad_(True)
    y = rng.integers(0, 5, n)
    w = rng.random(e).astype(np.float32)
    s, t, g = random_graph(n, e, 400 + e, ndata={"x": x, "y": y}, edge_weight=w)
    g.node_order()          # cache the locality order
    for k in (0, 1, 5):
        xk = torch.as_tensor(rng.normal(size=(2, k)).astype(np.float32)).requires_grad_(True)
        yk = rng.integers(0, 5, k)
        got = ng.add_nodes(g, k, {"x": xk, "y": yk})
        check_edges(got, s, t, n + k)
        assert got._shared.get("order") is None and got.edge_weight is w
        assert got.ndata["x"].is_cuda and torch.equal(got.ndata["x"].detach().cpu(), torch.cat([x.detach().cpu(), xk.detach()], dim=1))
        assert isinstance(got.ndata["y"], np.ndarray) and got.ndata["y"].dtype == y.dtype and np.array_equal(got.ndata["y"], np.concatenate([y, yk]))
        x.grad = None
        (got.ndata["x"] * torch.arange(1, n + k + 1, device=DEV)).sum().backward()
        assert torch.equal(x.grad, torch.arange(1, n + 1, device=DEV, dtype=torch.float32).expand(2, n))
        assert torch.equal(xk.grad, torch.arange(n + 1, n + k + 1, dtype=torch.float32).expand(2, k))
    assert ng.add_nodes(random_graph(n, e, 1)[2], 3).num_nodes == n + 3


# ---- 3. adding edges -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,e", SIZES)
def test_add_edges(n, e):
    s, t, g = random_graph(n, e, 500 + e)
    rng = np.random.default_rng(3 * n + e)
    for k in (0, 1, 257):
        s1, t1 = rng.integers(0, n, k), rng.integers(0, n, k)
        got = ng.add_edges(g, s1, t1)
        check_edges(got, np.concatenate([s, s1]), np.concatenate([t, t1]), n)
        assert ng.remove_edges(got, np.arange(e, e + k)) == g          # the appended positions removed: g again
    for s1, t1 in (([n], [0]), ([0], [-1]), ([0, 2 ** 40], [0, 0]), ([0, 0, 0], [0, 0, n + 5])):
        with pytest.raises(ng.DimensionMismatch, match="outside"):
            ng.add_edges(g, s1, t1)


def test_add_edges_on_a_batch():
    members = [random_graph(n, e, 600 + n)[2] for n, e in ((7, 15), (12, 40))]
    gb = ng.batch(members)
    s, t = gb.edge_index(index_base=0)
    got = ng.add_edges(gb, [0, 7, 18], [6, 18, 7])          # each inside one member
    check_edges(got, np.concatenate([s, [0, 7, 18]]), np.concatenate([t, [6, 18, 7]]), 19)
    assert got.num_graphs == 2 and np.array_equal(got.graph_indicator, gb.graph_indicator)
    for s1, t1 in (([6], [7]), ([0, 18], [1, 0])):
        with pytest.raises(ng.ArgumentError, match="different graphs"):
            ng.add_edges(gb, s1, t1)


# ---- 4. to_unidirected -----------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n,e", SIZES)
def test_to_unidirected(n, e):
    s, t, g = random_graph(n, e, 700 + e)
    want = np_unidirected(s, t, n)
    check_edges(ng.to_unidirected(g), *want, n)
    check_edges(ng.to_unidirected(ng.to_bidirected(g)), *want, n)
    assert np.array_equal(want[0] == want[1], np.isin(want[0] * n + want[1], (s * n + t)[s == t]))          # self loops stay


# ---- 5. features -----------------------------------------------------------------------------------------------------------------------


def test_features_follow_with_their_gradients():
    rng = np.random.default_rng(21)
    n, e, k = 30, 200, 9
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    s[150:], t[150:] = t[:50], s[:50]          # pairs with two and more copies, in both directions
    xe = torch.randn(5, e, device=DEV, requires_grad=True)
    w = torch.rand(e, device=DEV, requires_grad=True)
    lab = torch.as_tensor(rng.integers(0, 9, (1, e)))          # int64, on the host
    idx = rng.integers(0, 9, e).astype(np.int16)          # numpy
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, edata={"e": xe, "lab": lab, "idx": idx}, edge_weight=w)

    gone = rng.permutation(e)[:70]
    keep = np.setdiff1d(np.arange(e), gone)
    gr = ng.remove_edges(g, gone)
    assert torch.equal(gr.edata["e"], xe.detach()[:, keep]) and torch.equal(gr.edge_weight, w.detach()[keep])
    assert gr.edata["lab"].dtype == torch.int64 and not gr.edata["lab"].is_cuda and torch.equal(gr.edata["lab"], lab[:, keep])
    assert isinstance(gr.edata["idx"], np.ndarray) and gr.edata["idx"].dtype == np.int16 and np.array_equal(gr.edata["idx"], idx[keep])
    (gr.edata["e"].sum() * 2 + gr.edge_weight.sum() * 3).backward()
    mask = np.zeros(e)
    mask[keep] = 1          # float64 counts: how often each edge's feature reaches the loss
    assert np.array_equal(xe.grad.cpu().double().numpy(), np.broadcast_to(2 * mask, (5, e))) and np.array_equal(w.grad.cpu().double().numpy(), 3 * mask)
    gp = ng.remove_edges(g, s[gone], t[gone])
    left = ~np.isin(s * n + t, (s * n + t)[gone])
    assert torch.equal(gp.edata["e"], xe.detach()[:, left]) and torch.equal(gp.edata["lab"], lab[:, left])

    xe.grad = w.grad = None
    xk = torch.randn(5, k, requires_grad=True)          # on the host: the result is on the device
    wk = torch.rand(k, device=DEV, requires_grad=True)
    labk, idxk = torch.as_tensor(rng.integers(0, 9, (1, k))), rng.integers(0, 9, k)
    ga = ng.add_edges(g, rng.integers(0, n, k), rng.integers(0, n, k), {"e": xk, "lab": labk, "idx": idxk}, edge_weight=wk)
    assert ga.edata["e"].is_cuda and torch.equal(ga.edata["e"].detach().cpu(), torch.cat([xe.detach().cpu(), xk.detach()], dim=1))
    assert torch.equal(ga.edge_weight.detach(), torch.cat([w.detach(), wk.detach()]))
    assert ga.edata["lab"].dtype == torch.int64 and not ga.edata["lab"].is_cuda and torch.equal(ga.edata["lab"], torch.cat([lab, labk], dim=1))
    assert isinstance(ga.edata["idx"], np.ndarray) and ga.edata["idx"].dtype == np.int16 and np.array_equal(ga.edata["idx"], np.concatenate([idx, idxk]))
    ramp = torch.arange(1, e + k + 1, device=DEV, dtype=torch.float32)
    ((ga.edata["e"] * ramp).sum() + (ga.edge_weight * ramp).sum() * 2).backward()
    assert torch.equal(xe.grad, ramp[:e].expand(5, e)) and torch.equal(xk.grad, ramp[e:].cpu().expand(5, k))
    assert torch.equal(w.grad, 2 * ramp[:e]) and torch.equal(wk.grad, 2 * ramp[e:])

    # to_unidirected: the mean over a pair's copies.  With c copies, float32 adds c - 1 times and divides once, each within 2^-24
    # relative of a partial result bounded by sum|x|: |out - exact| <= c * 2^-24 * sum|x|.  The gradient of sum(out) with respect to a
    # copy is 1 / c, one correctly rounded division: within 2^-24 relative of the float64 quotient.
    xe.grad = w.grad = None
    gf = ng.GNNGraph(s, t, num_nodes=n, index_base=0, edata={"e": xe}, edge_weight=w)
    gu = ng.to_unidirected(gf)
    a, b = np.minimum(s, t), np.maximum(s, t)
    key, group_of, count = np.unique(a * n + b, return_inverse=True, return_counts=True)
    check_edges(gu, key // n, key % n, n)
    for got, src in ((gu.edata["e"], xe.detach().cpu().double().numpy()), (gu.edge_weight[None], w.detach().cpu().double().numpy()[None])):
        ref, absum = np.zeros((src.shape[0], key.size)), np.zeros((src.shape[0], key.size))
        np.add.at(ref, (slice(None), group_of), src)
        np.add.at(absum, (slice(None), group_of), np.abs(src))
        err = np.abs(got.detach().cpu().double().numpy() - ref / count)
        assert (err <= count * 2.0 ** -24 * absum).all(), float((err / (count * 2.0 ** -24 * absum)).max())
    (gu.edata["e"].sum() + gu.edge_weight.sum()).backward()
    ref = 1.0 / count[group_of]
    for grad in (xe.grad, w.grad[None]):
        assert (np.abs(grad.cpu().double().numpy() - ref) <= 2.0 ** -24 * ref).all()
    with pytest.raises(ng.ArgumentError, match="float32"):
        ng.to_unidirected(g)          # an int64 feature cannot be averaged


def test_set_edge_weight():
    s, t, g = random_graph(30, 100, 5)
    w = torch.rand(100, device=DEV)
    gw = ng.set_edge_weight(g, w)
    assert ng.get_edge_weight(gw) is w and ng.get_edge_weight(g) is None
    assert torch.equal(ng.remove_edges(gw, [0, 5]).edge_weight, w[torch.as_tensor(np.setdiff1d(np.arange(100), [0, 5]), device=DEV)])
    assert torch.equal(ng.degree(gw, "in"), ng.degree(g, "in", edge_weight=w))


def test_edited_graphs_run_a_layer():
    """the device lists of a result are usable as they are: a handle builds on them and GCNConv gives what it gives on a host-built twin"""
    n, e, d = 300, 1000, 16
    s, t, g = random_graph(n, e, 9)
    x = torch.randn(d, n + 2, device=DEV)
    edits = (ng.remove_edges(g, np.arange(0, e, 3)), ng.remove_edges(g, s[:50], t[:50]), ng.add_edges(g, [0, 1, 2], [5, 6, 7]), ng.to_unidirected(g),
             ng.remove_nodes(g, np.arange(0, n, 7)), ng.add_nodes(g, 2), ng.negative_sample(g, seed=3), ng.negative_sample(g, bidirected=True, seed=3))
    for got in edits:
        gs, gt = got.edge_index(index_base=0)
        twin = ng.GNNGraph(gs, gt, num_nodes=got.num_nodes, index_base=0)
        outs = []
        for graph in (got, twin):
            gcn = ng.GCNConv((d, d), "relu", initialgraph=graph)
            ps, st = ng.setup(0, gcn)
            outs.append(gcn(x[:, :got.num_nodes].contiguous(), ng.to_device(ps, DEV), st)[0])
        assert torch.equal(outs[0], outs[1]) and bool(outs[0].abs().sum() > 0)


# ---- 6. negative sampling ----------------------------------------------------------------------------------------------------------------


def check_negatives(gs, gt, s, t, n, bidirected):
    """no self loop, no duplicate, no edge of the graph; bidirected: no reverse of one either, the second half the reverse of the first"""
    assert gs.size == 0 or (gs.min() >= 0 and gs.max() < n and gt.min() >= 0 and gt.max() < n)
    assert (gs != gt).all() and np.unique(gs * n + gt).size == gs.size
    edges = s * n + t
    assert not np.isin(gs * n + gt, edges).any()
    if bidirected:
        h = gs.size // 2
        assert not np.isin(gt * n + gs, edges).any()
        assert np.array_equal(gs[h:], gt[:h]) and np.array_equal(gt[h:], gs[:h]) and (gs[:h] < gt[:h]).all()


@pytest.mark.parametrize("n,e,bidirected", [(300, 1000, False), (300, 1000, True), (300, 257, None), (100003, 1000, False), (100003, 1000, True),
                                            (300, 0, False), (300, 0, None)])
def test_negative_sample_matches_numpy(n, e, bidirected):
    s, t, g = random_graph(n, e, 800 + e)
    if bidirected is None:          # the default: what the graph is
        g = ng.to_bidirected(g) if e else g
        s, t = g.edge_index(index_base=0)
        assert ng.is_bidirected(g)
    for num, seed in ((None, 0), (0, 1), (1, 2), (513, 2 ** 64 - 1)):
        got = ng.negative_sample(g, num, bidirected=bidirected, seed=seed)
        num = g.num_edges if num is None else num
        bid = True if bidirected is None else bidirected
        want = np_negative(s, t, n, num // 2 if bid else num, bid, seed)
        check_edges(got, *want, n)
        check_negatives(*want, s, t, n, bid)
        assert not got.ndata and not got.edata and got.edge_weight is None


def test_negative_sample_on_two_nodes():
    one = ng.GNNGraph([0], [1], num_nodes=2, index_base=0)
    for seed in range(4):
        check_edges(ng.negative_sample(one, 1, bidirected=False, seed=seed), [1], [0], 2)          # the only non-edge
    with pytest.raises(ng.ArgumentError, match="not edges"):
        ng.negative_sample(one, 2, bidirected=False, seed=0)
    with pytest.raises(ng.ArgumentError, match="not edges"):
        ng.negative_sample(one, 2, bidirected=True, seed=0)          # the one pair is an edge
    none = ng.GNNGraph([], [], num_nodes=2, index_base=0)
    seen = set()
    for seed in range(8):
        want = np_negative(np.zeros(0, np.int64), np.zeros(0, np.int64), 2, 2, False, seed)
        check_edges(ng.negative_sample(none, 2, bidirected=False, seed=seed), *want, 2)
        seen.add(tuple(want[0]))
        check_edges(ng.negative_sample(none, 2, seed=seed), [0, 1], [1, 0], 2)          # (an empty graph is bidirected)
    assert seen == {(0, 1), (1, 0)}
    with pytest.raises(ng.ArgumentError, match="pairs"):
        ng.negative_sample(ng.GNNGraph([], [], num_nodes=1, index_base=0), 1, bidirected=False, seed=0)
    assert ng.negative_sample(ng.GNNGraph([0], [0], num_nodes=1, index_base=0), 0, seed=0).num_edges == 0


@pytest.mark.parametrize("n,e,bidirected", [(300, 1000, False), (300, 1000, True), (100003, 1000, True)])
def test_negative_sample_properties(n, e, bidirected):
    s, t, g = random_graph(n, e, 900 + e)
    n_target = 40
    want = np_negative(s, t, n, n_target, bidirected, 11)
    for chunk in (1, 7, 256, 0):          # the same bits for every chunk size
        got = c_negative(s, t, n, n_target, bidirected, 11, chunk)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), chunk
    a = ng.negative_sample(g, 2 * n_target, bidirected=bidirected, seed=5)
    b = ng.negative_sample(g, 2 * n_target, bidirected=bidirected, seed=5)
    c = ng.negative_sample(g, 2 * n_target, bidirected=bidirected, seed=6)
    assert a == b and a != c          # same call, same bits; another seed, another result
    for got in (a, c):
        check_negatives(*got.edge_index(index_base=0), s, t, n, bidirected)
    torch.manual_seed(3)
    d = ng.negative_sample(g, 2 * n_target, bidirected=bidirected)
    torch.manual_seed(3)
    assert d == ng.negative_sample(g, 2 * n_target, bidirected=bidirected)          # seed=None draws from torch's generator


def test_negative_sample_of_a_dense_graph():
    n = 6
    pairs = [(a, b) for a in range(n) for b in range(n) if a != b]
    missing = [(0, 3), (4, 1), (5, 2)]
    s, t = np.asarray([p for p in pairs if p not in missing]).T
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    for seed in range(5):
        gs, gt = ng.negative_sample(g, 3, bidirected=False, seed=seed).edge_index(index_base=0)
        assert sorted(zip(gs.tolist(), gt.tolist())) == missing
        want = np_negative(s, t, n, 3, False, seed)
        assert np.array_equal(gs, want[0]) and np.array_equal(gt, want[1])
    with pytest.raises(ng.ArgumentError, match="not edges"):
        ng.negative_sample(g, 4, bidirected=False, seed=0)


def frequencies(g, bidirected, n):
    counts = np.zeros(n * n, dtype=np.int64)
    for seed in range(2400):
        gs, gt = ng.negative_sample(g, 8, bidirected=bidirected, seed=seed).edge_index(index_base=0)
        assert gs.size == 8
        h = 8 if bidirected is False else 4          # (None: the graph is bidirected)
        np.add.at(counts, gs[:h] * n + gt[:h], 1)
    return counts.reshape(n, n)


def test_negative_sample_frequencies_directed():
    """every negative is as likely as every other: 2400 samples of 8 of the 192 negatives, so a slot's count is Binomial(2400, 1 / 24) --
    mean 100, sigma 9.79, 5 sigma = 49.  The numpy restatement of the rule gives 73 .. 136 (at most 17 candidates per call)."""
    n = 16
    i = np.arange(n)
    s = np.concatenate([i, i, i])
    t = np.concatenate([(i + k) % n for k in (1, 3, 7)])
    counts = frequencies(ng.GNNGraph(s, t, num_nodes=n, index_base=0), False, n)
    is_edge = np.zeros((n, n), dtype=bool)
    is_edge[s, t] = True
    negative = ~is_edge & ~np.eye(n, dtype=bool)
    assert negative.sum() == 192 and counts[~negative].sum() == 0
    print("directed counts", counts[negative].min(), counts[negative].max())
    assert (counts[negative] > 0).all()
    assert (np.abs(counts[negative] - 100) <= 49).all()


def test_negative_sample_frequencies_bidirected():
    """2400 samples of 4 of the 88 negative pairs: a pair's count is Binomial(2400, 1 / 22) -- mean 109.09, sigma 10.2, 5 sigma = 51.  The
    numpy restatement of the rule gives 90 .. 140."""
    n = 16
    i = np.arange(n)
    s = np.concatenate([i, i, (i + 1) % n, (i + 3) % n])
    t = np.concatenate([(i + 1) % n, (i + 3) % n, i, i])
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    assert ng.is_bidirected(g)
    counts = frequencies(g, None, n)
    is_edge = np.zeros((n, n), dtype=bool)
    is_edge[s, t] = True
    negative = np.triu(~is_edge, 1)
    assert negative.sum() == 88 and counts[~negative].sum() == 0
    print("bidirected counts", counts[negative].min(), counts[negative].max())
    assert (counts[negative] > 0).all()
    assert (np.abs(counts[negative] - 2400 * 4 / 88) <= 51).all()
