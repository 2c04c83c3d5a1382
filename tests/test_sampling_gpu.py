"""GPU tests of the random graph sampling (sampling.py over csrc/sampling.hip; src/NeuralGraphPDE.jl:4 of the reference re-exports
sample_neighbors and rand_edge_split from GNNGraphs).

Everything here is integer work, so every comparison is exact: the generator's bits against Random123's known answers and a numpy
restatement of Philox4x32-10, the sampled edge lists INCLUDING THEIR ORDER against a numpy restatement of the selection rules, the
features against plain indexing and their gradients against float64 counts.  The two frequency checks have the fixed seed 12345, so
their outcome is deterministic; their 5-sigma caps are those of the binomial distribution of one slot's count.

The known answers with a fourth counter word other than 0 (the all-ones and the pi vector) cannot be asked of ngpde_random_keys, whose
counter is (c0, c1, stream, 0): they are checked on the numpy restatement, which the device is then compared with.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib, graphops

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROW_MAX = _lib.SAMPLE_LDS_ROW_MAX

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


def np_sample(s, t, n, nodes, k, dir, seed):
    """the COO positions sample_neighbors(replace=False) keeps, ascending"""
    e = np.arange(s.size, dtype=np.uint64)
    node = t if dir == "in" else s
    key = draw(seed, 1, e, e >> S32) if s.size else np.zeros(0, np.uint64)
    order = np.lexsort((e, key, node))                                   # by row, then (key, position)
    start = np.searchsorted(node[order], np.arange(n))
    rank = np.arange(s.size) - start[node[order]]
    listed = np.ones(n, dtype=bool) if nodes is None else np.isin(np.arange(n), nodes)
    keep = listed[node[order]] & ((rank < k) if k >= 0 else True)
    return np.sort(order[keep]).astype(np.int64)


def np_sample_replace(s, t, n, nodes, k, dir, seed):
    node = t if dir == "in" else s
    rows = np.argsort(node, kind="stable")
    start = np.searchsorted(node[rows], np.arange(n + 1))
    out = []
    for v in (range(n) if nodes is None else nodes):
        deg = int(start[v + 1] - start[v])
        if deg:
            d = draw(seed, 2, np.full(k, v), np.arange(k))
            out += [int(rows[start[v] + ((int(x) * deg) >> 64)]) for x in d]
    return np.asarray(out, dtype=np.int64)


def np_split(s, t, frac, by_pair, seed):
    """(the positions of g1, of g2), ascending"""
    e = np.arange(s.size, dtype=np.uint64)
    if not by_pair:
        n1 = int(round(frac * s.size))
        order = np.lexsort((e, draw(seed, 3, e, e >> S32)))
        first = np.zeros(s.size, dtype=bool)
        first[order[:n1]] = True
    else:
        key = draw(seed, 3, np.minimum(s, t), np.maximum(s, t))
        n1 = int(round(frac * np.count_nonzero(s <= t)))
        first = key <= np.sort(key[s <= t])[n1 - 1] if n1 else np.zeros(s.size, dtype=bool)
    return np.flatnonzero(first), np.flatnonzero(~first)


def eids_of(g):
    """a result's EID after checking it against its own edge list: int64 on the device, and the edges are those positions of the source"""
    eid = g.edata["EID"]
    assert eid.dtype == torch.int64 and eid.is_cuda and eid.numel() == g.num_edges
    return eid.cpu().numpy()


def same_edges(g, src, eid):
    got = eids_of(g)
    assert np.array_equal(got, eid)
    s, t = g.edge_index(index_base=0)
    s0, t0 = src.edge_index(index_base=0)
    assert np.array_equal(s, s0[eid]) and np.array_equal(t, t0[eid])
    coo = g._shared[("coo", str(torch.device("cuda", torch.cuda.current_device())))]          # the lists the handle builder takes
    assert coo[0].dtype == torch.int32 and np.array_equal(coo[0].cpu().numpy(), s) and np.array_equal(coo[1].cpu().numpy(), t)


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------------

KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def random_keys(seed, stream, c1, first, n):
    out = torch.empty(n, dtype=torch.int64, device=DEV)
    _lib.check(_lib.load().ngpde_random_keys(seed, stream, c1, first, n, _lib.ptr(out), _lib.current_stream()))
    return out.cpu().numpy().view(np.uint64)


def test_known_answers():
    for c, k, want in KNOWN:
        assert " ".join("%08x" % int(x) for x in philox4x32_10(c, k)) == want
        if c[3] == 0:          # the counters ngpde_random_keys can name
            got = int(random_keys(k[0] | (k[1] << 32), c[2], c[1], c[0], 1)[0])
            assert "%08x %08x" % (got & 0xFFFFFFFF, got >> 32) == want[:17]
    # the first two words of the other vectors' counters, with the fourth word 0, against the restatement
    for c, k, _ in KNOWN[1:]:
        got = random_keys(k[0] | (k[1] << 32), c[2], c[1], c[0], 1)
        assert np.array_equal(got, draw(k[0] | (k[1] << 32), c[2], [c[0]], c[1]))


@pytest.mark.parametrize("seed", [12345, 0xA4093822299F31D0])
def test_generator_matches_numpy(seed):
    n = 10000
    for stream, c1, first in ((1, 0, 0), (3, 77, 123456789), (2, 0xFFFFFFFF, 2 ** 32 - 5000), (9, 5, 2 ** 40 + 3)):
        want = draw(seed, stream, (np.uint64(first) + np.arange(n, dtype=np.uint64)) & MASK, c1)
        assert np.array_equal(random_keys(seed, stream, c1, first, n), want), (stream, c1, first)
    assert np.unique(random_keys(seed, 1, 0, 0, n)).size == n


# ---- 2. exact selection ---------------------------------------------------------------------------------------------------------------

ROW_LENGTHS = [0, 1, 2, 3, 4, 63, 64, 65, 255, 256, 257, ROW_MAX // 4, ROW_MAX // 4 + 1, ROW_MAX, ROW_MAX + 1, 3 * ROW_MAX, 0, 5]


def row_graph():
    """node v has ROW_LENGTHS[v] inbound edges from random sources: K - 1, K, K + 1 for K = 1 and 3, 63 .. 65 for K = 64 and the wave, the
    boundaries between a wave's row, a workgroup's row (a quarter of the LDS bound) and the segmented sort; the COO order is shuffled,
    so the rows interleave.  With 18 possible sources the long rows are full of parallel edges, and self loops occur."""
    rng = np.random.default_rng(21)
    n = len(ROW_LENGTHS)
    t = np.repeat(np.arange(n), ROW_LENGTHS)
    s = rng.integers(0, n, t.size)
    p = rng.permutation(t.size)
    s, t = s[p], t[p]
    assert (s == t).any() and np.unique(s * n + t).size < t.size
    return s, t, n


ROWS = row_graph()


def c_sample(s, t, n, base, dir, nodes, k, replace, seed):
    """ngpde_coo_sample_neighbors on lists with `base` added: (s', t', eid)"""
    sd, td = (torch.as_tensor((x + base).astype(np.int32), device=DEV) for x in (s, t))
    nd = None if nodes is None else torch.as_tensor(np.asarray(nodes, dtype=np.int64), device=DEV)
    bound = (n if nodes is None else len(nodes)) * k if replace else s.size
    so, to = torch.empty(bound, dtype=torch.int32, device=DEV), torch.empty(bound, dtype=torch.int32, device=DEV)
    eid = torch.empty(bound, dtype=torch.int64, device=DEV)
    m = C.c_int64(-1)
    _lib.check(_lib.load().ngpde_coo_sample_neighbors(n, s.size, _lib.ptr(sd), _lib.ptr(td), base, {"out": 0, "in": 1}[dir],
                                                      0 if nodes is None else len(nodes), _lib.ptr(nd), k, int(replace), seed, _lib.ptr(so),
                                                      _lib.ptr(to), _lib.ptr(eid), C.byref(m), _lib.current_stream()))
    return so[:m.value].cpu().numpy(), to[:m.value].cpu().numpy(), eid[:m.value].cpu().numpy()


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("dir", ["in", "out"])
@pytest.mark.parametrize("k", [0, 1, 3, 64, -1])
def test_selection_matches_numpy(k, dir, base):
    s, t, n = ROWS
    if dir == "out":
        s, t = t, s                                                    # the same rows, now by source
    want = np_sample(s, t, n, None, k, dir, 99)
    deg = np.bincount(t if dir == "in" else s, minlength=n)
    assert want.size == (np.minimum(deg, k).sum() if k >= 0 else s.size)
    if base == 0:
        g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
        same_edges(ng.sample_neighbors(g, None, k, dir=dir, seed=99), g, want)
    else:
        so, to, eid = c_sample(s, t, n, 1, dir, None, k, False, 99)
        assert np.array_equal(eid, want) and np.array_equal(so, s[want] + 1) and np.array_equal(to, t[want] + 1)


def test_bad_ends_and_nodes_are_refused():
    s, t, n = ROWS
    bad = s.copy()
    bad[17] = n
    for base in (0, 1):
        with pytest.raises(ng.DimensionMismatch, match="outside"):
            c_sample(bad, t, n, base, "in", None, 3, False, 1)
        with pytest.raises(ng.DimensionMismatch, match="outside"):
            c_sample(t, bad, n, base, "in", None, 3, True, 1)
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    for nodes in ([0, n], [-1], [2, 5, 2]):
        with pytest.raises(ng.ArgumentError, match="nodes"):
            ng.sample_neighbors(g, nodes, 3, seed=1)


# ---- 3. independence ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dir", ["in", "out"])
def test_a_nodes_sample_does_not_depend_on_the_list(dir):
    s, t, n = ROWS
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    node = t if dir == "in" else s
    k = 3
    full = eids_of(ng.sample_neighbors(g, None, k, dir=dir, seed=4))
    for v in (1, 4, 7, 9, 13, 15, 16):
        same_edges(ng.sample_neighbors(g, [v], k, dir=dir, seed=4), g, full[node[full] == v])
    nodes = [15, 3, 9, 0, 14]
    sub = ng.sample_neighbors(g, torch.as_tensor(nodes), k, dir=dir, seed=4)
    same_edges(sub, g, full[np.isin(node[full], nodes)])
    assert np.array_equal(eids_of(sub), np_sample(s, t, n, nodes, k, dir, 4))
    assert ng.sample_neighbors(g, [], k, dir=dir, seed=4).num_edges == 0


# ---- 4. with replacement --------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("dir", ["in", "out"])
@pytest.mark.parametrize("k", [0, 1, 5])
def test_replacement_matches_numpy(k, dir):
    s, t, n = ROWS
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    node = t if dir == "in" else s
    deg = np.bincount(node, minlength=n)
    for nodes in (None, [15, 0, 3, 16, 9, 1]):
        got = ng.sample_neighbors(g, nodes, k, dir=dir, replace=True, seed=31)
        want = np_sample_replace(s, t, n, nodes, k, dir, 31)
        same_edges(got, g, want)
        listed = list(range(n)) if nodes is None else nodes
        owner = np.repeat([v for v in listed if deg[v] > 0], k)          # exactly k per listed node with an edge, all of them its own
        assert np.array_equal(node[eids_of(got)], owner)
    so, to, eid = c_sample(s, t, n, 1, dir, [9, 2], 5, True, 31)
    want = np_sample_replace(s, t, n, [9, 2], 5, dir, 31)
    assert np.array_equal(eid, want) and np.array_equal(so, s[want] + 1) and np.array_equal(to, t[want] + 1)


# ---- 5. frequencies -------------------------------------------------------------------------------------------------------------------


def test_every_slot_is_chosen_equally_often():
    rng = np.random.default_rng(3)
    n, deg, k = 20000, 8, 3
    g = ng.GNNGraph(rng.integers(0, n, n * deg), np.repeat(np.arange(n), deg), num_nodes=n, index_base=0)
    eid = eids_of(ng.sample_neighbors(g, None, k, seed=12345))
    count = np.bincount(eid % deg, minlength=deg)          # edge v * deg + slot
    mean, sigma = n * k / deg, np.sqrt(n * (k / deg) * (1 - k / deg))
    assert count.sum() == n * k and (np.abs(count - mean) <= 5 * sigma).all(), (count, mean, sigma)

    n, deg, k = 5000, 7, 4
    g = ng.GNNGraph(rng.integers(0, n, n * deg), np.repeat(np.arange(n), deg), num_nodes=n, index_base=0)
    eid = eids_of(ng.sample_neighbors(g, None, k, replace=True, seed=12345))
    count = np.bincount(eid % deg, minlength=deg)
    mean, sigma = n * k / deg, np.sqrt(n * k * (1 / deg) * (1 - 1 / deg))
    assert count.sum() == n * k and (np.abs(count - mean) <= 5 * sigma).all(), (count, mean, sigma)


# ---- 6. reproducibility ---------------------------------------------------------------------------------------------------------------


def test_seeds():
    s, t, n = ROWS
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    for f in (lambda seed: [ng.sample_neighbors(g, None, 3, seed=seed)],
              lambda seed: [ng.sample_neighbors(g, None, 3, replace=True, seed=seed)],
              lambda seed: list(ng.rand_edge_split(g, 0.4, seed=seed))):
        a, b, c = f(7), f(7), f(8)
        assert all(torch.equal(x.edata["EID"], y.edata["EID"]) and x == y for x, y in zip(a, b))
        assert not any(torch.equal(x.edata["EID"], y.edata["EID"]) for x, y in zip(a, c))
        torch.manual_seed(0)
        a = f(None)
        torch.manual_seed(0)
        b = f(None)
        c = f(None)
        assert all(torch.equal(x.edata["EID"], y.edata["EID"]) for x, y in zip(a, b))
        assert not any(torch.equal(x.edata["EID"], y.edata["EID"]) for x, y in zip(a, c))


# ---- 7. features ----------------------------------------------------------------------------------------------------------------------


def featured_graph():
    rng = np.random.default_rng(13)
    n, e = 40, 600
    s, t = rng.integers(0, n, e), rng.integers(0, n - 3, e)          # the last three nodes have no inbound edge
    s[s >= n - 2] = 0                                                  # ... and the last two no edge at all
    xe = torch.randn(5, e, device=DEV, requires_grad=True)
    w = torch.rand(e, device=DEV, requires_grad=True)
    lab = torch.as_tensor(rng.integers(0, 9, (2, e)))                  # int64, on the host
    code = rng.integers(0, 9, e).astype(np.int16)                      # numpy
    dlab = torch.arange(e, device=DEV, dtype=torch.int32)
    xn = torch.randn(3, n, device=DEV, requires_grad=True)
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, ndata={"x": xn, "id": np.arange(n)}, edata={"e": xe, "lab": lab, "code": code, "dlab": dlab},
                    edge_weight=w)
    return g, s, t, n, e, xe, w, lab, code, dlab, xn


@pytest.mark.parametrize("replace", [False, True])
def test_features_and_gradients_follow(replace):
    g, s, t, n, e, xe, w, lab, code, dlab, xn = featured_graph()
    gs = ng.sample_neighbors(g, None, 4, replace=replace, seed=5)
    eid = eids_of(gs)
    assert (np.bincount(eid, minlength=e).max() > 1) == replace
    assert torch.equal(gs.edata["e"], xe.detach()[:, eid]) and torch.equal(gs.edge_weight, w.detach()[eid])
    assert gs.edata["lab"].dtype == torch.int64 and not gs.edata["lab"].is_cuda and torch.equal(gs.edata["lab"], lab[:, eid])
    assert isinstance(gs.edata["code"], np.ndarray) and gs.edata["code"].dtype == np.int16 and np.array_equal(gs.edata["code"], code[eid])
    assert gs.edata["dlab"].dtype == torch.int32 and gs.edata["dlab"].is_cuda and np.array_equal(gs.edata["dlab"].cpu().numpy(), eid)
    assert gs.ndata["x"] is xn and gs.num_nodes == n
    coef = torch.arange(1, 6, device=DEV, dtype=torch.float32)[:, None]
    ((gs.edata["e"] * coef).sum() + 3 * gs.edge_weight.sum()).backward()
    mult = np.bincount(eid, minlength=e).astype(np.float64)          # the 0 / 1 mask, or the number of draws
    assert np.array_equal(xe.grad.cpu().double().numpy(), coef.cpu().double().numpy() * mult[None, :])
    assert np.array_equal(w.grad.cpu().double().numpy(), 3 * mult)


def test_split_gradients_follow():
    g, s, t, n, e, xe, w, *_ = featured_graph()
    g1, g2 = ng.rand_edge_split(g, 0.3, bidirected=False, seed=2)
    e1, e2 = eids_of(g1), eids_of(g2)
    assert torch.equal(g1.edata["e"], xe.detach()[:, e1]) and torch.equal(g2.edge_weight, w.detach()[e2])
    (g1.edata["e"].sum() + 2 * g2.edata["e"].sum() + g1.edge_weight.sum()).backward()
    m1 = np.zeros(e)
    m1[e1] = 1
    assert np.array_equal(xe.grad.cpu().double().numpy(), np.broadcast_to(m1 + 2 * (1 - m1), (5, e)))
    assert np.array_equal(w.grad.cpu().double().numpy(), m1)


@pytest.mark.parametrize("replace", [False, True])
def test_dropnodes(replace):
    g, s, t, n, e, xe, w, lab, code, dlab, xn = featured_graph()
    nodes = [3, 8, 20, n - 1, 11]
    full = ng.sample_neighbors(g, nodes, 2, replace=replace, seed=6)
    gd = ng.sample_neighbors(g, nodes, 2, replace=replace, seed=6, dropnodes=True)
    eid = eids_of(full)
    assert np.array_equal(eids_of(gd), eid) and eid.size == 8
    nid = np.unique(np.concatenate([s[eid], t[eid]]))
    assert gd.ndata["NID"].dtype == torch.int64 and np.array_equal(gd.ndata["NID"].cpu().numpy(), nid) and gd.num_nodes == nid.size
    gs, gt = gd.edge_index(index_base=0)
    assert np.array_equal(nid[gs], s[eid]) and np.array_equal(nid[gt], t[eid])
    assert torch.equal(gd.ndata["x"], xn.detach()[:, nid]) and np.array_equal(gd.ndata["id"], nid)
    assert torch.equal(gd.edata["e"], xe.detach()[:, eid]) and torch.equal(gd.edge_weight, w.detach()[eid])
    gd.ndata["x"].sum().backward()
    assert np.array_equal(xn.grad.cpu().numpy(), np.broadcast_to(np.isin(np.arange(n), nid).astype(np.float32), (3, n)))


# ---- 8. the split ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("frac", [0, 0.3, 0.5, 1])
def test_split_matches_numpy(frac):
    s, t, n = ROWS
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    assert not ng.is_bidirected(g)
    g1, g2 = ng.rand_edge_split(g, frac, seed=77)          # bidirected=None: the graph decides
    e1, e2 = eids_of(g1), eids_of(g2)
    assert e1.size == int(round(frac * s.size)) and e1.size + e2.size == s.size
    assert np.array_equal(np.sort(np.concatenate([e1, e2])), np.arange(s.size))          # disjoint, and together every edge
    assert (np.diff(e1) > 0).all() and (np.diff(e2) > 0).all()
    w1, w2 = np_split(s, t, frac, False, 77)
    same_edges(g1, g, w1)
    same_edges(g2, g, w2)
    assert g1.num_nodes == n and g2.num_nodes == n
    with pytest.raises(ng.ArgumentError, match="bidirected"):
        ng.rand_edge_split(g, frac, bidirected=True, seed=77)


def grid_triangles(k):
    """the k x k grid, every cell cut into two triangles; three directed edges a -> b -> c -> a per triangle"""
    idx = np.arange(k * k).reshape(k, k)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, c], 1), np.stack([b, d, c], 1)])
    return np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]]), np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])


@pytest.mark.parametrize("frac", [0, 0.3, 0.5, 1])
def test_split_of_a_bidirected_mesh_keeps_pairs_together(frac):
    k = 30
    s, t = grid_triangles(k)
    g = ng.to_bidirected(ng.GNNGraph(s, t, num_nodes=k * k, index_base=0))
    assert ng.is_bidirected(g)
    s, t = g.edge_index(index_base=0)
    p = np.count_nonzero(s <= t)
    for bidirected in (None, True):
        g1, g2 = ng.rand_edge_split(g, frac, bidirected=bidirected, seed=9)
        assert ng.is_bidirected(g1) and ng.is_bidirected(g2)
        s1, t1 = g1.edge_index(index_base=0)
        assert np.count_nonzero(s1 <= t1) == int(round(frac * p)) and g1.num_edges + g2.num_edges == s.size
        w1, w2 = np_split(s, t, frac, True, 9)
        same_edges(g1, g, w1)
        same_edges(g2, g, w2)
    g1, _ = ng.rand_edge_split(g, frac, bidirected=False, seed=9)          # the per-edge rule on the same graph
    same_edges(g1, g, np_split(s, t, frac, False, 9)[0])


def test_split_with_parallel_pairs_and_loops():
    """both directions and every parallel copy of a pair share a key, so g1 may hold more than round(frac * P) upper edges"""
    rng = np.random.default_rng(17)
    n = 12
    a, b = rng.integers(0, n, 400), rng.integers(0, n, 400)
    s, t = np.concatenate([a, b]), np.concatenate([b, a])
    p = rng.permutation(s.size)
    s, t = s[p], t[p]
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    assert ng.is_bidirected(g) and ng.has_multi_edges(g) and ng.has_self_loops(g)
    for frac in (0, 0.25, 0.5, 1):
        g1, g2 = ng.rand_edge_split(g, frac, seed=3)
        w1, w2 = np_split(s, t, frac, True, 3)
        same_edges(g1, g, w1)
        same_edges(g2, g, w2)
        assert ng.is_bidirected(g1) and ng.is_bidirected(g2)
        s1, t1 = g1.edge_index(index_base=0)
        assert np.count_nonzero(s1 <= t1) >= int(round(frac * np.count_nonzero(s <= t)))
        pairs1 = set(zip(np.minimum(s1, t1), np.maximum(s1, t1)))
        s2, t2 = g2.edge_index(index_base=0)
        assert not pairs1 & set(zip(np.minimum(s2, t2), np.maximum(s2, t2)))          # no pair is torn


# ---- 9. as a model's graph ------------------------------------------------------------------------------------------------------------


def test_result_as_a_layers_graph():
    rng = np.random.default_rng(4)
    n, e, d = 500, 12000, 16
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    gs = ng.sample_neighbors(g, None, 8, seed=1)
    keep = np_sample(s, t, n, None, 8, "in", 1)
    twin = ng.GNNGraph(s[keep], t[keep], num_nodes=n, index_base=0)          # built on the host from the restatement
    assert gs.num_edges == np.minimum(np.bincount(t, minlength=n), 8).sum()
    assert int(graphops.degree(gs, "in").max()) == 8
    gcn = ng.GCNConv((d, d), "relu", initialgraph=g)
    ps, st = ng.setup(0, gcn)
    ps = ng.to_device(ps, DEV)
    x = torch.randn(d, n, device=DEV)
    y0 = gcn(x, ps, st)[0]
    y1 = gcn(x, ps, ng.updategraph(st, gs))[0]
    y2 = gcn(x, ps, ng.updategraph(st, twin))[0]
    assert torch.equal(y1, y2) and not torch.equal(y0, y1) and bool(y1.abs().sum() > 0)
