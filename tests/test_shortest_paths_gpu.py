"""The weighted shortest paths on the device (traversal.shortest_paths over csrc/graph_paths.hip) against the numpy float32 restatement
of tests/test_shortest_paths_host.py.  The rounds are double-buffered and fp32 addition is monotone, so distances, parents and the
number of rounds are pure functions of the COO list, the weights and the sources: EVERY comparison here is bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from test_shortest_paths_host import FAMILIES, ref_shortest_paths, weights
from test_traversal_gpu import capture
from test_traversal_host import path_edges, random_edges

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(n, e) for n in (1, 2, 300) for e in (0, 1, 255, 256, 257, 1000)] + [(100003, 1000)]
DIRS = ("out", "in", "both")
PATH_N = 4096


def host(x):
    return x.detach().cpu().numpy()


def graph(n, s, t, **kw):
    return ng.GNNGraph(s, t, num_nodes=n, index_base=0, **kw)


def same(sp, want, what=None):
    """dist, parent_eid, parents and rounds, bit for bit"""
    dist, parent_eid, parents, rounds = want
    assert sp.dist.dtype == torch.float32 and sp.dist.is_cuda and tuple(sp.dist.shape) == dist.shape, what
    assert host(sp.dist).tobytes() == dist.tobytes(), what
    if sp.parents is not None:
        assert sp.parent_eid.dtype == torch.int32 and sp.parents.dtype == torch.int32
        assert np.array_equal(host(sp.parent_eid), parent_eid), what
        assert np.array_equal(host(sp.parents), parents), what
    assert sp.rounds == rounds and not sp.unfinished, (what, sp.rounds, rounds)


@functools.lru_cache(maxsize=None)
def edges(n, e):
    return random_edges(n, e, 1000 * n + e) if e else (np.zeros(0, np.int64), np.zeros(0, np.int64))


def sources_of(n):
    several = np.random.default_rng(n).integers(0, n, 5)
    return np.concatenate([several, several[:1]])


# ---- general cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,e", CASES)
def test_general(n, e):
    s, t = edges(n, e)
    g = graph(n, s, t)
    sources = sources_of(n)
    for k, family in enumerate(FAMILIES):
        w = weights(family, e, 31 * k + e)
        for dir in DIRS:
            want = ref_shortest_paths(n, s, t, w, sources, dir)
            same(ng.shortest_paths(g, sources, w, dir=dir, return_parents=True), want, (family, dir))
            sp = ng.shortest_paths(g, torch.as_tensor(sources, device=DEV), torch.as_tensor(w, device=DEV), dir=dir)
            assert sp.parents is None and sp.parent_eid is None
            same(sp, want, (family, dir, "device arguments"))
        one = ref_shortest_paths(n, s, t, w, [n // 2], "out")
        same(ng.shortest_paths(g, n // 2, w, return_parents=True), one, (family, "an int"))
        finite = np.sort(one[0][np.isfinite(one[0])])
        cut = float(finite[len(finite) // 2])                            # a distance that occurs: the boundary of max_dist
        near = ng.shortest_paths(g, n // 2, w, max_dist=cut, return_parents=True)
        same(near, ref_shortest_paths(n, s, t, w, [n // 2], "out", max_dist=cut), (family, "max_dist"))
        assert np.array_equal(host(near.dist), np.where(one[0] <= np.float32(cut), one[0], np.float32(np.inf)))
    none = ng.shortest_paths(g, [], dir="both", return_parents=True)
    same(none, ref_shortest_paths(n, s, t, None, [], "both"), "no sources")
    assert none.rounds == 0 and np.isinf(host(none.dist)).all()
    w = weights("uniform", e, 5)
    same(ng.shortest_paths(graph(n, s, t, edge_weight=w), sources, return_parents=True), ref_shortest_paths(n, s, t, w, sources),
         "the graph's own weights")


@pytest.mark.parametrize("n,e", [(300, 1000), (100003, 1000), (2, 257)])
def test_unit_weights_are_hop_distances(n, e):
    s, t = edges(n, e)
    g = graph(n, s, t)
    sources = sources_of(n)
    for dir in DIRS:
        sp = ng.shortest_paths(g, sources, dir=dir, return_parents=True)
        same(sp, ref_shortest_paths(n, s, t, None, sources, dir), dir)
        hops = host(ng.hop_distance(g, sources, dir=dir))
        assert np.array_equal(host(sp.dist), np.where(hops < 0, np.float32(np.inf), hops.astype(np.float32))), dir
        assert np.array_equal(np.isinf(host(sp.dist)), hops == -1)
    rows = ng.shortest_paths(g, sources, dir="both", separate=True)
    hops = host(ng.hop_distance(g, sources, dir="both", separate=True))
    assert np.array_equal(host(rows.dist), np.where(hops < 0, np.float32(np.inf), hops.astype(np.float32)))


# ---- hub rows, the star, the path -------------------------------------------------------------------------------------------------

def test_rows_at_the_wave_threshold():
    """rows of 63, 64 and 65 entries (nodes 0, 1, 2): the row of 63 is walked by its lane, the others by the whole wave.  With small
    integer weights and every leaf a source the hub sees many EQUAL candidates in round 1: the first in row order has to win"""
    assert _lib.SSSP_WAVE_ROW == 64
    rng = np.random.default_rng(63)
    n = 203
    t = np.concatenate([np.full(63, 0), np.full(64, 1), np.full(65, 2)])
    s = rng.integers(3, n, len(t))
    order = rng.permutation(len(t))
    s, t = s[order], t[order]
    g = graph(n, s, t)
    for family in FAMILIES:
        w = weights(family, len(t), 7)
        leaves = np.arange(3, n)
        for dir in DIRS:
            same(ng.shortest_paths(g, leaves, w, dir=dir, return_parents=True), ref_shortest_paths(n, s, t, w, leaves, dir), (family, dir))
        some = [5, 0, 77, 2, 5]
        same(ng.shortest_paths(g, some, w, dir="both", separate=True, return_parents=True),
             ref_shortest_paths(n, s, t, w, some, "both", separate=True), family)


def test_star():
    """2049 leaves around the centre 2049: a row of 2049 entries, first with the centre as the target, then as the source"""
    leaves = np.arange(2049)
    n, s, t = 2050, leaves, np.full(2049, 2049)
    g = graph(n, s, t)
    for family in FAMILIES:
        w = weights(family, 2049, 11)
        for dir in DIRS:
            for sources in (leaves[5::7], [2049], [7, 2049]):
                same(ng.shortest_paths(g, sources, w, dir=dir, return_parents=True), ref_shortest_paths(n, s, t, w, sources, dir),
                     (family, dir, len(sources)))
    w = weights("ties", 2049, 11)
    same(ng.shortest_paths(g, [7, 2049, 0], w, dir="both", separate=True, return_parents=True),
         ref_shortest_paths(n, s, t, w, [7, 2049, 0], "both", separate=True))


@functools.lru_cache(maxsize=None)
def path_case(name):
    seq = np.arange(PATH_N)
    numbering = {"sequential": seq, "reversed": seq[::-1].copy(), "permuted": np.random.default_rng(4).permutation(PATH_N)}[name]
    s, t = path_edges(numbering)
    w = weights("uniform", PATH_N - 1, 3)
    return s, t, w, int(numbering[0]), ref_shortest_paths(PATH_N, s, t, w, [int(numbering[0])])


@pytest.mark.parametrize("name", ["sequential", "reversed", "permuted"])
def test_long_path(name):
    """4095 rounds that each lower one node, and the confirming one: one launch per round"""
    s, t, w, first, want = path_case(name)
    assert want[3] == PATH_N
    g = graph(PATH_N, s, t)
    for kw in (dict(check_every=1), dict(check_every=8), dict(), dict(check_every=0, max_rounds=PATH_N), dict(check_every=8, max_rounds=PATH_N)):
        same(ng.shortest_paths(g, first, w, return_parents=True, **kw), want, kw)
    back = ng.shortest_paths(g, first, w, dir="in")                          # against the edges the first node reaches only itself
    assert back.rounds == 1 and np.isinf(host(back.dist)).sum() == PATH_N - 1
    # one round short: the status, and with check_every=0 the flag word
    with pytest.raises(ng.NgpdeError, match=f"still changing after max_rounds = {PATH_N - 1}") as err:
        ng.shortest_paths(g, first, w, max_rounds=PATH_N - 1)
    assert err.value.code == _lib.ERR_STATE
    short = ng.shortest_paths(g, first, w, max_rounds=PATH_N - 1, check_every=0)
    assert short.unfinished and short.rounds == PATH_N - 1 and host(short.flags).tolist() == [PATH_N - 1, 1]


# ---- separate sources, batches ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, _lib.SSSP_PASS - 1, _lib.SSSP_PASS, _lib.SSSP_PASS + 1])
def test_separate_sources(count):
    """one below, at and one above a pass; the counts are no multiples of the sources a lane takes"""
    n, e = 300, 1000
    s, t = edges(n, e)
    g = graph(n, s, t)
    sources = np.random.default_rng(count).integers(0, n, count)
    sources[-1] = sources[0]                                             # a source listed twice gives two equal rows
    for family, dir in (("uniform", "out"), ("ties", "both"), ("inf", "in")):
        w = weights(family, e, count)
        sp = ng.shortest_paths(g, sources, w, dir=dir, separate=True, return_parents=True)
        same(sp, ref_shortest_paths(n, s, t, w, sources, dir, separate=True), (family, dir))
        assert torch.equal(sp.dist[-1], sp.dist[0]) and torch.equal(sp.parent_eid[-1], sp.parent_eid[0])
        for i in (0, count // 2, count - 1):
            alone = ng.shortest_paths(g, [int(sources[i])], w, dir=dir, return_parents=True)
            assert torch.equal(sp.dist[i], alone.dist) and torch.equal(sp.parents[i], alone.parents), i
        cut = float(np.median(host(sp.dist)[np.isfinite(host(sp.dist))]))
        same(ng.shortest_paths(g, sources, w, dir=dir, separate=True, max_dist=cut, return_parents=True),
             ref_shortest_paths(n, s, t, w, sources, dir, max_dist=cut, separate=True), (family, dir, "max_dist"))
    empty = ng.shortest_paths(g, [], separate=True, return_parents=True)
    assert tuple(empty.dist.shape) == (0, n) and tuple(empty.parents.shape) == (0, n) and empty.rounds == 0


def test_a_source_reaches_only_its_own_graph():
    ring = lambda k: (k, np.arange(k), (np.arange(k) + 1) % k)
    gb = ng.batch([graph(*ring(5)), graph(6, [0, 1, 3], [1, 2, 4]), graph(*ring(7))])
    s, t = gb.edge_index(0)
    n, w = gb.num_nodes, weights("uniform", gb.num_edges, 2)
    assert gb.num_graphs == 3 and n == 18
    for sources in ([12], [6, 12]):
        sp = ng.shortest_paths(gb, sources, w, dir="both", return_parents=True)
        same(sp, ref_shortest_paths(n, s, t, w, sources, "both"), sources)
        d = host(sp.dist)
        assert np.isinf(d[:5]).all() and np.isfinite(d[11:]).all() and np.isfinite(d[5:8]).all() == (6 in sources) and np.isinf(d[8:11]).all()
    rows = ng.shortest_paths(gb, [0, 12], w, dir="both", separate=True)
    assert np.isfinite(host(rows.dist)).sum(1).tolist() == [5, 7]


def test_path_to():
    n, e = 300, 1000
    s, t = edges(n, e)
    w = weights("uniform", e, 1)
    sp = ng.shortest_paths(graph(n, s, t), [3, 150], w, separate=True, return_parents=True)
    dist = host(sp.dist)
    for row, source in enumerate((3, 150)):
        assert sp.path_to(source, row) == [source]
        far = int(np.argmax(np.where(np.isfinite(dist[row]), dist[row], -1)))
        path = sp.path_to(far, row)
        assert path[0] == source and path[-1] == far and len(path) >= 2
        total = np.float32(0)
        for a, b in zip(path[:-1], path[1:]):                                # every link is an edge; the lengths add up to dist, in float32
            total = np.float32(total + w[(s == a) & (t == b)].min())
        assert total == dist[row, far]
        lost = np.flatnonzero(np.isinf(dist[row]))
        if len(lost):
            assert sp.path_to(int(lost[0]), row) == []
    with pytest.raises(ng.ArgumentError, match="row must be"):
        sp.path_to(0, 2)
    with pytest.raises(ng.ArgumentError, match="v must be"):
        sp.path_to(n)


# ---- purity -----------------------------------------------------------------------------------------------------------------------

def test_purity_two_runs_and_a_permuted_list():
    n, e = 300, 1000
    s, t = edges(n, e)
    sources = sources_of(n)
    perm = np.random.default_rng(12).permutation(e)
    for family in FAMILIES:
        w = weights(family, e, 21)
        for dir in DIRS:
            first = ng.shortest_paths(graph(n, s, t), sources, w, dir=dir, return_parents=True)
            again = ng.shortest_paths(graph(n, s, t), sources, w, dir=dir, return_parents=True)
            assert torch.equal(first.dist, again.dist) and torch.equal(first.parent_eid, again.parent_eid) and first.rounds == again.rounds
            moved = ng.shortest_paths(graph(n, s[perm], t[perm]), sources, w[perm], dir=dir, return_parents=True)
            assert host(moved.dist).tobytes() == host(first.dist).tobytes() and moved.rounds == first.rounds, (family, dir)
            # the parents may differ, through the row-order rule alone: they are the restatement's on the permuted list
            same(moved, ref_shortest_paths(n, s[perm], t[perm], w[perm], sources, dir), (family, dir))


# ---- the C entry: index_base 1, plan reuse ----------------------------------------------------------------------------------------

def test_index_base_one_at_the_c_entry():
    n, e = 300, 257
    s, t = edges(n, e)
    w = weights("ties", e, 8)
    sources = sources_of(n)
    lib = _lib.load()
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.int32), device=DEV)
    sd, td, wd = i32(s + 1), i32(t + 1), torch.as_tensor(w, device=DEV)
    src = torch.as_tensor(sources + 1, device=DEV)
    plans = []
    for code in (1, 0):
        ptr, other, eid = torch.empty(n + 1, dtype=torch.int32, device=DEV), i32(np.zeros(e)), i32(np.zeros(e))
        _lib.check(lib.ngpde_coo_rows_eid(n, e, _lib.ptr(sd), _lib.ptr(td), 1, code, _lib.ptr(ptr), _lib.ptr(other), _lib.ptr(eid), None))
        plans.append((ptr, other, eid))
    (pa, oa, ea), (pb, ob, eb) = plans
    s_of, t_of = host(sd).astype(np.int64) - 1, host(td).astype(np.int64) - 1
    assert np.array_equal(t_of[host(ea)], np.repeat(np.arange(n), np.diff(host(pa)))) and np.array_equal(s_of[host(ea)], host(oa))
    assert np.array_equal(s_of[host(eb)], np.repeat(np.arange(n), np.diff(host(pb)))) and np.array_equal(t_of[host(eb)], host(ob))
    dist = torch.empty(n, dtype=torch.float32, device=DEV)
    parent_eid, parents = torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV)
    flags = torch.empty(2, dtype=torch.int32, device=DEV)
    nbytes = lib.ngpde_csr_shortest_paths_workspace_bytes(n, e, e, len(sources), 0)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    _lib.check(lib.ngpde_csr_shortest_paths(n, e, _lib.ptr(pa), _lib.ptr(oa), _lib.ptr(ea), e, _lib.ptr(pb), _lib.ptr(ob), _lib.ptr(eb),
                                            len(sources), _lib.ptr(src), 1, 0, _lib.ptr(wd), np.inf, 0, 8, _lib.ptr(dist), _lib.ptr(parent_eid),
                                            _lib.ptr(parents), _lib.ptr(flags), _lib.ptr(ws), nbytes, _lib.current_stream()))
    torch.cuda.synchronize()
    same(ng.ShortestPaths(dist, parent_eid, parents, flags), ref_shortest_paths(n, s, t, w, sources, "both"))
    # a source named with index_base 1: 301 is node 300
    bad = torch.as_tensor(np.array([5, 301, 0], np.int64), device=DEV)
    st = lib.ngpde_csr_shortest_paths(n, e, _lib.ptr(pa), _lib.ptr(oa), _lib.ptr(ea), 0, None, None, None, 3, _lib.ptr(bad), 1, 0, _lib.ptr(wd),
                                      np.inf, 0, 8, _lib.ptr(dist), None, None, None, _lib.ptr(ws), nbytes, _lib.current_stream())
    assert st == _lib.ERR_DIMENSION_MISMATCH and b"sources lists node -1, outside the 300 nodes" in lib.ngpde_last_error()


def test_errors_and_plan_reuse():
    n, e = 300, 257
    s, t = edges(n, e)
    g = graph(n, s, t)
    w = weights("uniform", e, 9)
    for value in (-1.0, np.nan, -np.inf):
        bad = w.copy()
        bad[[200, 17, 99]] = value
        bad[40] = np.inf                                                 # (valid)
        for kw in (dict(), dict(separate=True), dict(dir="both", check_every=1)):
            with pytest.raises(ng.ArgumentError, match=r"the weight at COO position 17 is negative or NaN"):
                ng.shortest_paths(g, [0, 5], bad, **kw)
    for bad, named in (([5, 300, 1000], 300), ([5, -2, 300, -9], -9)):
        for kw in (dict(), dict(separate=True)):
            with pytest.raises(ng.DimensionMismatch, match=rf"sources lists node {named}, outside the 300 nodes"):
                ng.shortest_paths(g, bad, w, **kw)
    with pytest.raises(ng.NgpdeError, match="still changing after max_rounds = 1") as err:
        ng.shortest_paths(g, sources_of(n), w, dir="both", max_rounds=1)
    assert err.value.code == _lib.ERR_STATE
    assert ng.shortest_paths(g, sources_of(n), w, dir="both", max_rounds=1, check_every=0).unfinished
    plans = lambda: {k: v for k, v in g._shared.items() if k[0] == "rows_eid"}
    first = plans()
    assert sorted(k[1] for k in first) == [0, 1]                         # dir="both" sorted both; nothing is sorted twice
    for dir in DIRS:
        ng.shortest_paths(ng.GNNGraph(g), [1], w, dir=dir)                # a copy shares the structure's plans
    assert len(plans()) == 2 and all(plans()[k] is v for k, v in first.items())
    assert not [k for k in g._shared if k[0] == "rows"]                  # (hop_distance's plans have a key of their own)


def test_capture_and_replay():
    n, e = 300, 1000
    s, t = edges(n, e)
    g = graph(n, s, t)
    w = weights("magnitudes", e, 13)
    sources = torch.as_tensor(np.array([3, 150, 3, 299], np.int64), device=DEV)
    wd = torch.as_tensor(w, device=DEV)
    rounds = ng.shortest_paths(g, sources, wd, dir="both", separate=True).rounds          # (the rows plans are sorted here, outside the capture)
    kw = dict(dir="both", max_rounds=rounds + 3, check_every=0, return_parents=True)
    step = lambda: [x for sp in (ng.shortest_paths(g, sources, wd, **kw), ng.shortest_paths(g, sources, wd, separate=True, **kw))
                    for x in (sp.dist, sp.parent_eid, sp.parents, sp.flags)]
    eager, outs, gr = capture(step)
    for k, separate in ((0, False), (4, True)):
        want = ref_shortest_paths(n, s, t, w, host(sources), "both", separate=separate)
        same(ng.ShortestPaths(*eager[k:k + 4]), want, separate)
    for _ in range(2):
        for x in outs:
            x.fill_(-7)
        gr.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(outs, eager))
