"""The graph traversal on the device (traversal.py over csrc/graph_traverse.hip) against the numpy restatements of
tests/test_traversal_host.py: connected_components / is_connected / split_components and hop_distance / neighborhood.  Every result is an
integer, so every comparison is exact."""
import functools
import gc

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib, traversal
from test_traversal_host import path_edges, random_edges, ref_components, ref_hop_distance, ref_rank, ref_split

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(n, e) for n in (1, 2, 300) for e in (0, 1, 255, 256, 257, 1000)] + [(100003, 1000)]
PATH_N = 4096


def host(x):
    return x.detach().cpu().numpy()


def dev32(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV)


def graph(n, s, t, **kw):
    return ng.GNNGraph(s, t, num_nodes=n, index_base=0, **kw)


@functools.lru_cache(maxsize=None)
def case(n, e):
    """(s, t, labels, rounds) of a general case, computed once"""
    s, t = random_edges(n, e, 1000 * n + e) if e else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    labels, rounds = ref_components(n, s, t)
    return s, t, labels, rounds


def path_numberings():
    seq = np.arange(PATH_N)
    out = [("sequential", seq), ("reversed", seq[::-1].copy())]
    return out + [(f"permuted{k}", np.random.default_rng(k).permutation(PATH_N)) for k in range(4)]


def star():
    """2049 leaves around a centre that carries the largest id: every hook of the first round is an atomicMin on ONE word, and the
    centre's row is longer than 2048"""
    leaves = np.arange(2049)
    return 2050, leaves, np.full(2049, 2049)


def check_components(comps, n, labels):
    rank, count, sizes, ptr, order = ref_rank(labels)
    assert comps.count == count == len(comps)
    for got, want in ((comps.labels, rank), (comps.smallest, labels), (comps.sizes, sizes), (comps.ptr, ptr), (comps.order, order)):
        assert got.dtype == torch.int32 and got.is_cuda and np.array_equal(host(got), want)
    assert comps.tolist() == [order[ptr[k]:ptr[k + 1]].tolist() for k in range(count)]
    if count:
        assert host(comps[count - 1]).tolist() == comps.tolist()[-1] and host(comps[0])[0] == 0


# ---- components -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,e", CASES)
def test_components_general(n, e):
    s, t, labels, _ = case(n, e)
    g = graph(n, s, t)
    comps = ng.connected_components(g)
    check_components(comps, n, labels)
    assert comps.rounds >= 1 and host(comps.per_graph).tolist() == [comps.count]
    assert ng.is_connected(g) is (comps.count == 1)
    perm = np.random.default_rng(7).permutation(e)
    swap = np.random.default_rng(8).integers(0, 2, e).astype(bool)          # the edges are undirected here: some turned round
    s2, t2 = np.where(swap, t[perm], s[perm]), np.where(swap, s[perm], t[perm])
    assert torch.equal(ng.connected_components(graph(n, s2, t2)).labels, comps.labels)          # a function of the edge set
    assert torch.equal(ng.connected_components(g).labels, comps.labels)                          # and of nothing else: two runs
    full = 2 * int(np.ceil(np.log2(max(n, 2)))) + 8
    for kw in (dict(check_every=1), dict(check_every=4), dict(check_every=0, max_rounds=full)):
        again = ng.connected_components(g, **kw)
        assert torch.equal(again.labels, comps.labels) and torch.equal(again.smallest, comps.smallest), kw
    # index_base = 1, at the C entry
    got, rounds = traversal._label(n, e, dev32(s + 1), dev32(t + 1), 1, None, 4)
    assert np.array_equal(host(got), labels) and host(rounds)[1] == 0 and host(rounds)[0] >= 1


@pytest.mark.parametrize("name,numbering", path_numberings(), ids=[k for k, _ in path_numberings()])
def test_components_of_a_long_path(name, numbering):
    """the compression hazard: after the first hook round the sequentially numbered path is ONE chain of depth N"""
    s, t = path_edges(numbering)
    comps = ng.connected_components(graph(PATH_N, s, t))
    print(f"{name}: {comps.rounds} rounds on the device, {ref_components(PATH_N, s, t)[1]} in the synchronous restatement")
    assert comps.count == 1 and not host(comps.labels).any() and not host(comps.smallest).any()
    assert host(comps.order).tolist() == list(range(PATH_N)) and host(comps.sizes).tolist() == [PATH_N]
    assert comps.rounds <= 64


def test_components_of_a_star_and_of_interleaved_paths():
    n, s, t = star()
    comps = ng.connected_components(graph(n, s, t))
    check_components(comps, n, np.zeros(n, np.int64))
    # two paths interleaved on the even and the odd ids
    n = 601
    ids = np.arange(n)
    s, t = np.concatenate([ids[0:-2:2], ids[1:-2:2]]), np.concatenate([ids[2::2], ids[3::2]])
    comps = ng.connected_components(graph(n, s, t))
    check_components(comps, n, ids % 2)
    assert host(comps[0]).tolist() == list(range(0, n, 2)) and host(comps[1]).tolist() == list(range(1, n, 2))
    assert not ng.is_connected(graph(n, s, t))


def test_components_per_graph_of_a_batch():
    ring = lambda k: (k, np.arange(k), (np.arange(k) + 1) % k)
    a, c = graph(*ring(5)), graph(*ring(7))
    b = graph(6, [0, 1, 3], [1, 2, 4])          # a path of three, a pair and an isolated node
    gb = ng.batch([a, b, c])
    comps = ng.connected_components(gb)
    assert comps.count == 5 and host(comps.per_graph).tolist() == [1, 3, 1]
    assert host(comps.labels).tolist() == [0] * 5 + [1, 1, 1, 2, 2, 3] + [4] * 7
    ok = ng.is_connected(gb)
    assert ok.dtype == torch.bool and ok.is_cuda and host(ok).tolist() == [True, False, True]
    assert ng.is_connected(a) is True and ng.is_connected(b) is False


def test_components_errors():
    n, e = 300, 257
    s, t, _, _ = case(n, e)
    bad_s, bad_t = s.copy(), t.copy()
    bad_s[5], bad_t[100], bad_t[200] = 1000, -3, 300
    with pytest.raises(ng.DimensionMismatch, match=r"references node -3, outside the 300 nodes"):
        traversal._label(n, e, dev32(bad_s), dev32(bad_t), 0, None, 4)
    one_s = s + 1
    one_s[9] = 301                                              # with index_base 1 the ids are 1 .. 300: 301 is node 300
    with pytest.raises(ng.DimensionMismatch, match=r"references node 300, outside the 300 nodes"):
        traversal._label(n, e, dev32(one_s), dev32(t + 1), 1, None, 1)
    g = graph(PATH_N, *path_edges(np.random.default_rng(0).permutation(PATH_N)))
    for kw in (dict(max_rounds=1), dict(max_rounds=1, check_every=0)):
        with pytest.raises(ng.NgpdeError, match="still hooking after max_rounds = 1") as err:
            ng.connected_components(g, **kw)
        assert err.value.code == _lib.ERR_STATE


def capture(step):
    """step() eagerly, then captured into a HIP graph; (the eager outputs, the captured outputs, the graph)"""
    eager = [x.clone() for x in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
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
    return eager, outs, gr


def test_components_capture_and_replay():
    n, e = 300, 257
    s, t, labels, _ = case(n, e)
    sd, td = dev32(s), dev32(t)
    out, rounds = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(2, dtype=torch.int32, device=DEV)
    ws = torch.empty(256, dtype=torch.uint8, device=DEV)
    eager, outs, gr = capture(lambda: traversal._label(n, e, sd, td, 0, 26, 0, labels=out, rounds=rounds, ws=ws))
    assert np.array_equal(host(eager[0]), labels)
    for _ in range(2):
        out.fill_(-7)
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(host(outs[0]), labels) and host(outs[1]).tolist() == host(eager[1]).tolist() and host(outs[1])[1] == 0


# ---- split_components -----------------------------------------------------------------------------------------------------------

def test_split_components_structure():
    n, e = 300, 257
    s, t, _, _ = case(n, e)
    x = np.random.default_rng(3).standard_normal((4, n)).astype(np.float32)
    marks = np.arange(n, dtype=np.int64) * 3
    g = graph(n, s, t, ndata={"x": x, "marks": marks}, edata=np.arange(e, dtype=np.float32).reshape(1, e))
    comps = ng.connected_components(g)
    gs, sub = ng.split_components(g), ng.induced_subgraph(g, comps.order)
    s2, t2, nid, indicator, count = ref_split(n, s, t)
    assert gs.num_nodes == n and gs.num_edges == e and gs.num_graphs == count == comps.count
    for got in (gs, sub):
        assert np.array_equal(got.edge_index(0)[0], s2) and np.array_equal(got.edge_index(0)[1], t2)
    assert np.array_equal(gs.graph_indicator, indicator) and np.all(np.diff(gs.graph_indicator) >= 0)
    assert gs.ndata["NID"].dtype == torch.int64 and np.array_equal(host(gs.ndata["NID"]), nid)
    assert np.array_equal(host(gs.ndata["x"]), x[:, nid]) and np.array_equal(np.asarray(gs.ndata["marks"]), marks[nid])
    assert np.array_equal(host(gs.edata["e"]), host(sub.edata["e"])) and np.array_equal(host(gs.ndata["x"]), host(sub.ndata["x"]))
    whole = ng.split_components(graph(5, [0, 1, 2, 3], [1, 2, 3, 4]))          # one component: a single graph, nothing moves
    assert whole.num_graphs == 1 and whole.graph_indicator is None and host(whole.ndata["NID"]).tolist() == [0, 1, 2, 3, 4]


def test_split_components_carries_gradients():
    n, e = 300, 257
    s, t, _, _ = case(n, e)
    rng = np.random.default_rng(4)
    x = torch.as_tensor(rng.standard_normal((3, n)).astype(np.float32), device=DEV).requires_grad_(True)
    w = torch.as_tensor(rng.standard_normal(e).astype(np.float32), device=DEV).requires_grad_(True)
    cx = torch.as_tensor(rng.standard_normal((3, n)).astype(np.float32), device=DEV)
    cw = torch.as_tensor(rng.standard_normal(e).astype(np.float32), device=DEV)
    gs = ng.split_components(graph(n, s, t, ndata=x, edge_weight=w))
    order = gs.ndata["NID"]
    assert torch.equal(gs.ndata["x"].detach(), x.detach()[:, order]) and torch.equal(gs.edge_weight.detach(), w.detach())
    ((gs.ndata["x"] * cx).sum() + (gs.edge_weight * cw).sum()).backward()
    want = torch.zeros_like(cx)
    want[:, order] = cx
    assert torch.equal(x.grad, want) and torch.equal(w.grad, cw)


def test_split_components_feeds_the_per_graph_solvers():
    """a triangle, a two-node path and an isolated pair with their ids interleaved: lambda_max of the regrouped batch is, value for
    value, that of every component's induced_subgraph"""
    pairs = [(0, 2), (2, 5), (5, 0), (1, 4), (3, 6)]
    s = np.array([a for a, b in pairs] + [b for a, b in pairs])
    t = np.array([b for a, b in pairs] + [a for a, b in pairs])
    g = graph(7, s, t)
    comps = ng.connected_components(g)
    assert comps.tolist() == [[0, 2, 5], [1, 4], [3, 6]]
    lam = host(ng.laplacian_lambda_max(ng.split_components(g)))
    alone = [ng.laplacian_lambda_max(ng.induced_subgraph(g, comps[k])) for k in range(3)]
    print("lambda_max of the batch", lam.tolist(), "of the components alone", alone)
    assert lam.tolist() == [np.float32(v) for v in alone]


# ---- hop_distance and neighborhood ----------------------------------------------------------------------------------------------------

def source_sets(n):
    rng = np.random.default_rng(n)
    several = rng.integers(0, n, 5)
    return [[n // 2], np.concatenate([several, several[:1]]).tolist(), list(range(n)), []]


@pytest.mark.parametrize("n,e", CASES)
def test_hop_distance_general(n, e):
    s, t, _, _ = case(n, e)
    g = graph(n, s, t)
    for dir in ("out", "in", "both"):
        for k, sources in enumerate(source_sets(n)):
            if n == 100003 and k == 2 and dir != "out":
                continue                                    # (all nodes as sources: once is enough at this size)
            got = ng.hop_distance(g, sources, dir=dir)
            assert got.dtype == torch.int32 and got.shape == (n,) and got.is_cuda
            assert np.array_equal(host(got), ref_hop_distance(n, s, t, sources, dir)), (dir, k)
        sources = source_sets(n)[1]
        for max_hops in (0, 1, 3):
            got = ng.hop_distance(g, sources, dir=dir, max_hops=max_hops)
            assert np.array_equal(host(got), ref_hop_distance(n, s, t, sources, dir, max_hops)), (dir, max_hops)
        want = ref_hop_distance(n, s, t, sources, dir)
        for kw in (dict(check_every=1), dict(check_every=8), dict(check_every=0, max_hops=int(want.max()) + 1)):
            assert np.array_equal(host(ng.hop_distance(g, sources, dir=dir, **kw)), want), (dir, kw)
        near = ng.neighborhood(g, sources, 2, dir=dir)
        d2 = ref_hop_distance(n, s, t, sources, dir)
        assert near.dtype == torch.int64 and np.array_equal(host(near), np.flatnonzero((d2 >= 0) & (d2 <= 2)))
    sub = ng.induced_subgraph(g, ng.neighborhood(g, [n // 2], 2, dir="both"))
    assert sub.num_nodes == int(((ref_hop_distance(n, s, t, [n // 2], "both", 2)) >= 0).sum())
    assert ng.hop_distance(g, n // 2).shape == (n,) and ng.hop_distance(g, dev32([n // 2])).shape == (n,)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_hop_distance_separate_sources(count):
    """the mask-word and pass boundaries: 64 sources per pass"""
    n, e = 300, 1000
    s, t, _, _ = case(n, e)
    g = graph(n, s, t)
    sources = np.random.default_rng(count).integers(0, n, count)
    sources[-1] = sources[0]                                    # a source listed twice gives two equal rows
    for dir in ("out", "both"):
        got = ng.hop_distance(g, sources, dir=dir, separate=True)
        assert got.dtype == torch.int32 and got.shape == (count, n)
        assert np.array_equal(host(got), ref_hop_distance(n, s, t, sources, dir, separate=True)), dir
        assert torch.equal(got[-1], got[0])
    for i in (0, count // 2, count - 1):
        assert torch.equal(got[i], ng.hop_distance(g, [int(sources[i])], dir="both"))
    got = ng.hop_distance(g, sources, dir="in", separate=True, max_hops=2)
    assert np.array_equal(host(got), ref_hop_distance(n, s, t, sources, "in", 2, separate=True))
    assert ng.hop_distance(g, [], separate=True).shape == (0, n)


def test_hop_distance_named_shapes():
    seq = np.arange(PATH_N)
    s, t = path_edges(seq)                                      # the directed path 0 -> 1 -> ...
    g = graph(PATH_N, s, t)
    assert np.array_equal(host(ng.hop_distance(g, [0], dir="out")), seq)          # 4095 levels, one launch each
    want = np.full(PATH_N, -1)
    want[0] = 0
    assert np.array_equal(host(ng.hop_distance(g, [0], dir="in")), want)          # against the edges 0 reaches only itself
    assert np.array_equal(host(ng.hop_distance(g, [PATH_N - 1], dir="both")), seq[::-1])
    n, s, t = star()                                            # a row of 2049 entries: walked by a whole wave
    g = graph(n, s, t)
    for dir in ("out", "in", "both"):
        for sources in ([7], [2049]):
            assert np.array_equal(host(ng.hop_distance(g, sources, dir=dir)), ref_hop_distance(n, s, t, sources, dir)), (dir, sources)
    got = ng.hop_distance(g, [7, 2049, 0], dir="both", separate=True)
    assert np.array_equal(host(got), ref_hop_distance(n, s, t, [7, 2049, 0], "both", separate=True))
    assert host(got[0]).max() == 2 and host(got[1]).max() == 1
    # on a batch a source only reaches its own graph
    ring = lambda k: (k, np.arange(k), (np.arange(k) + 1) % k)
    gb = ng.batch([graph(*ring(5)), graph(*ring(7))])
    d = host(ng.hop_distance(gb, [6], dir="both"))
    assert d[:5].tolist() == [-1] * 5 and d[5:].tolist() == [1, 0, 1, 2, 3, 3, 2]


def test_hop_distance_errors_and_plan_reuse():
    n, e = 300, 257
    s, t, _, _ = case(n, e)
    g = graph(n, s, t)
    for bad, named in (([5, 300, 1000], 300), ([5, -2, 300, -9], -9)):
        for kw in (dict(), dict(separate=True)):
            with pytest.raises(ng.DimensionMismatch, match=rf"sources lists node {named}, outside the 300 nodes"):
                ng.hop_distance(g, bad, **kw)
    with pytest.raises(ng.DimensionMismatch, match="sources lists node 300"):
        ng.neighborhood(g, [300], 0)
    rows = lambda: {k: v for k, v in g._shared.items() if k[0] == "rows"}
    first = rows()
    assert sorted(k[1] for k in first) == [1]                   # dir="out" pulls along the rows grouped by target, sorted once
    ng.hop_distance(g, [0], dir="out")
    ng.hop_distance(g, [1], dir="both")
    ng.hop_distance(g, [2], dir="in")
    second = rows()
    assert sorted(k[1] for k in second) == [0, 1] and all(second[k] is v for k, v in first.items())
    ng.neighborhood(ng.GNNGraph(g), [3], 1, dir="both")         # a copy shares the structure's plans
    assert all(rows()[k] is v for k, v in second.items()) and len(rows()) == 2


def test_hop_distance_capture_and_replay():
    n, e = 300, 1000
    s, t, _, _ = case(n, e)
    g = graph(n, s, t)
    sources = torch.as_tensor(np.array([3, 150, 3, 299], np.int64), device=DEV)
    ng.hop_distance(g, sources, dir="both")                     # (the rows plans are sorted here, outside the capture)
    step = lambda: [ng.hop_distance(g, sources, dir="both", max_hops=6, check_every=0),
                    ng.hop_distance(g, sources, dir="both", max_hops=6, check_every=0, separate=True)]
    eager, outs, gr = capture(step)
    assert np.array_equal(host(eager[0]), ref_hop_distance(n, s, t, host(sources), "both", 6))
    assert np.array_equal(host(eager[1]), ref_hop_distance(n, s, t, host(sources), "both", 6, separate=True))
    for _ in range(2):
        for x in outs:
            x.fill_(-7)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(outs[0], eager[0]) and torch.equal(outs[1], eager[1])
