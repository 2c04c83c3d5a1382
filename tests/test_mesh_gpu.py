"""Delaunay graphs and triangles on the device (include/ngpde_mesh.h, ngpde_amd.mesh) against the float64 brute-force restatement of
tests/mesh_spec.py and against Qhull.

Edges and triangles are compared EXACTLY (index lists, no tolerance).  That is a fair demand only where no decision of the cloud is
inside the device's doubt zone, so every random cloud first asserts its precondition on the reference alone: the smallest
normalised in-circle margin of Qhull's triangulation (mesh_spec.min_margin) is at least 1024 x NGPDE_DELAUNAY_TIE_BOUND.  The
lattices are the opposite regime: integer coordinates, every in-circle determinant computed exactly, every tie exactly 0, and the
result must be the 8-neighbour stencil.  The five small clouds are the ones tests/test_mesh_host.py checks the restatement on.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
from scipy.spatial import ConvexHull, Delaunay

import ngpde_amd as ng
from ngpde_amd import _lib

import mesh_spec as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = ng.mesh


def directed(g):
    """the graph's directed pairs (point, neighbour) in list order: dir='in' writes the neighbour to s, the point to t"""
    return np.stack([g._t0, g._s0], 1).astype(np.int64)


def graph_and_triangles(p, **kw):
    """both calls on a [n][2] cloud; symmetry and row order are asserted on every graph that passes through here"""
    g = M.delaunay_graph(p.T, **kw)
    assert_symmetric_rows(directed(g))
    tri = M.delaunay_triangles(p.T, **kw)
    assert tri.dtype == torch.int32 and tri.is_cuda and tri.dim() == 2 and tri.shape[1] == 3
    return g, tri.cpu().numpy().astype(np.int64)


def assert_symmetric_rows(e):
    """both directions of every edge, ordered by point, the neighbours of a point ascending, no loops, no duplicates"""
    if len(e) == 0:
        return
    assert (e[:, 0] != e[:, 1]).all()
    code = e[:, 0] * (1 << 32) + e[:, 1]
    assert (np.diff(code) > 0).all()
    assert set(map(tuple, e.tolist())) == set(map(tuple, e[:, ::-1].tolist()))


def qhull(p):
    d = Delaunay(p.astype(np.float64))
    assert S.min_margin(p, d.simplices) >= 1024 * S.TIE_BOUND          # the precondition, on the reference alone
    return S.edges_of_simplices(d.simplices), S.canonical_triangles(p, d.simplices), len(ConvexHull(p.astype(np.float64)).vertices)


_SMALL = {}


def small(name):
    """the five host-checked clouds with the restatement's edges and triangles, computed once"""
    if name not in _SMALL:
        p = {"uniform": lambda: S.cloud("uniform", 0), "clustered": lambda: S.cloud("clustered", 0), "circle": lambda: S.cloud("circle", 0),
             "lattice5x4": lambda: S.lattice(5, 4), "lattice7x7": lambda: S.lattice(7, 7)}[name]()
        e = S.edges_brute(p)
        _SMALL[name] = (p, e, S.triangles_from_rows(p, e))
    return _SMALL[name]


SMALL = ["uniform", "clustered", "circle", "lattice5x4", "lattice7x7"]


@pytest.mark.parametrize("name", SMALL)
def test_edges_and_triangles_equal_the_restatement(name):
    p, e_ref, t_ref = small(name)
    g, tri = graph_and_triangles(p)
    e = directed(g)
    assert_symmetric_rows(e)
    assert np.array_equal(e, e_ref)
    assert np.array_equal(tri, t_ref)
    assert g.num_nodes == len(p) and g.num_graphs == 1
    if name.startswith("lattice"):
        nx, ny = (5, 4) if name == "lattice5x4" else (7, 7)
        assert np.array_equal(e, S.stencil8(nx, ny))
    if name == "circle":
        assert np.bincount(e[:, 0])[-1] == len(p) - 1                    # the hub: over the first pass's vertex budget


@pytest.mark.parametrize("kind", ["uniform", "clustered"])
def test_larger_clouds_equal_qhull(kind):
    n = 3000
    p = S.cloud(kind, 7, n)
    e_ref, t_ref, h = qhull(p)
    g, tri = graph_and_triangles(p)
    e = directed(g)
    assert_symmetric_rows(e)
    assert np.array_equal(e, e_ref) and np.array_equal(tri, t_ref)
    assert len(e) == 2 * (3 * n - 3 - h) and len(tri) == 2 * n - 2 - h


def passes():
    a, b = C.c_int64(-1), C.c_int64(-1)
    assert _lib.load().ngpde_delaunay_last_passes(C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def test_both_passes_run():
    p = S.cloud("uniform", 3, 200)
    e_ref, t_ref, h = qhull(p)
    g = M.delaunay_graph(p.T)
    lane, wave = passes()
    assert lane + wave == 200 and lane > 0 and wave >= h                # every hull point has an unbounded cell: the wave pass
    assert np.array_equal(directed(g), e_ref)
    p, e_ref, _ = small("circle")
    g = M.delaunay_graph(p.T)
    lane, wave = passes()
    assert wave >= 1 and np.array_equal(directed(g), e_ref)              # the centre's 149 neighbours do not fit 24 vertices


def test_a_batch_equals_its_graphs_shifted():
    parts = [S.cloud("uniform", 11, 40), np.array([[0.3, 0.3]], np.float32), S.cloud("clustered", 12, 300)]
    # the clouds overlap in space: an edge across graphs would be found if anything crossed
    p = np.concatenate(parts)
    sizes = [len(q) for q in parts]
    gi = np.repeat(np.arange(1, 4), sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    es, ts = [], []
    for q, o in zip(parts, off):
        g, tri = graph_and_triangles(q)
        es.append(directed(g) + o)
        ts.append(tri + o)
    e_ref, t_ref = np.concatenate(es), np.concatenate(ts)
    assert len(es[1]) == 0 and len(ts[1]) == 0
    g, tri = graph_and_triangles(p, graph_indicator=gi)
    assert g.num_graphs == 3
    assert np.array_equal(directed(g), e_ref) and np.array_equal(tri, t_ref)
    # the C entries with both id bases and both index bases
    lib = _lib.load()
    pts = torch.as_tensor(p, device=DEV).contiguous()
    for id_base in (0, 1):
        for index_base in (0, 1):
            ids = torch.as_tensor((gi - 1 + id_base).astype(np.int32), device=DEV)
            cnt = C.c_int64(0)
            head = (len(p), _lib.ptr(pts), _lib.ptr(ids), 3, id_base, math.inf)
            assert lib.ngpde_delaunay_graph(*head, 0, index_base, 0, None, None, C.byref(cnt), None) == 0
            assert cnt.value == len(e_ref)
            s = torch.empty(cnt.value, dtype=torch.int32, device=DEV)
            t = torch.empty(cnt.value, dtype=torch.int32, device=DEV)
            assert lib.ngpde_delaunay_graph(*head, 0, index_base, cnt.value, _lib.ptr(s), _lib.ptr(t), C.byref(cnt), None) == 0
            assert np.array_equal(np.stack([t.cpu().numpy(), s.cpu().numpy()], 1), e_ref + index_base)
            assert lib.ngpde_delaunay_triangles(*head, index_base, 0, None, C.byref(cnt), None) == 0
            assert cnt.value == len(t_ref)
            tri = torch.empty((cnt.value, 3), dtype=torch.int32, device=DEV)
            assert lib.ngpde_delaunay_triangles(*head, index_base, cnt.value, _lib.ptr(tri), C.byref(cnt), None) == 0
            assert np.array_equal(tri.cpu().numpy(), t_ref + index_base)
    ids = torch.as_tensor(gi.astype(np.int32), device=DEV)
    cnt = C.c_int64(0)
    assert lib.ngpde_delaunay_graph(len(p), _lib.ptr(pts), _lib.ptr(ids), 3, 0, math.inf, 0, 0, 0, None, None, C.byref(cnt),
                                    None) == _lib.ERR_INVALID_ARGUMENT and b"outside" in lib.ngpde_last_error()


def test_dir_swaps_s_and_t():
    p, e_ref, _ = small("uniform")
    a, b = M.delaunay_graph(p.T), M.delaunay_graph(p.T, dir="out")
    assert np.array_equal(a._s0, b._t0) and np.array_equal(a._t0, b._s0)
    assert np.array_equal(np.stack([b._s0, b._t0], 1), e_ref)


@pytest.mark.parametrize("name", ["uniform", "clustered", "lattice7x7"])
def test_max_edge_length_filters_by_the_float_rule(name):
    p, e_ref, t_ref = small(name)
    lengths = np.sqrt(((p[e_ref[:, 0]] - p[e_ref[:, 1]]).astype(np.float64) ** 2).sum(1))
    radii = (1.0, 1.2) if name == "lattice7x7" else (float(np.median(lengths)), float(np.float32(lengths[len(lengths) // 3])), 0.0)
    for r in radii:                                                      # (one of them is an edge's own length rounded to float)
        e_want, t_want = S.filter_edges(p, e_ref, r), S.filter_triangles(p, t_ref, r)
        g, tri = graph_and_triangles(p, max_edge_length=r)
        e = directed(g)
        assert np.array_equal(e, e_want) and np.array_equal(tri, t_want)
        assert len(e_want) < len(e_ref)
    g, tri = graph_and_triangles(p, max_edge_length=math.inf)
    assert np.array_equal(directed(g), e_ref) and np.array_equal(tri, t_ref)
    g, tri = graph_and_triangles(p, max_edge_length=1e30)                   # r * r = inf in float: no limit either
    assert np.array_equal(directed(g), e_ref) and np.array_equal(tri, t_ref)


def test_two_runs_give_the_same_bits():
    p = S.cloud("clustered", 5, 3000)
    a, ta = graph_and_triangles(p)
    b, tb = graph_and_triangles(p)
    assert a._s0.tobytes() == b._s0.tobytes() and a._t0.tobytes() == b._t0.tobytes() and ta.tobytes() == tb.tobytes()


def test_a_capacity_too_small_is_refused_before_anything_is_written():
    lib = _lib.load()
    p, e_ref, t_ref = small("uniform")
    pts = torch.as_tensor(p, device=DEV).contiguous()
    cnt = C.c_int64(0)
    s = torch.full((len(e_ref),), -7, dtype=torch.int32, device=DEV)
    t = torch.full((len(e_ref),), -7, dtype=torch.int32, device=DEV)
    st = lib.ngpde_delaunay_graph(len(p), _lib.ptr(pts), None, 1, 1, math.inf, 0, 0, len(e_ref) - 1, _lib.ptr(s), _lib.ptr(t),
                                  C.byref(cnt), None)
    assert st == _lib.ERR_INVALID_ARGUMENT and b"output arrays hold" in lib.ngpde_last_error()
    assert cnt.value == len(e_ref) and (s == -7).all() and (t == -7).all()
    tri = torch.full((len(t_ref), 3), -7, dtype=torch.int32, device=DEV)
    st = lib.ngpde_delaunay_triangles(len(p), _lib.ptr(pts), None, 1, 1, math.inf, 0, len(t_ref) - 1, _lib.ptr(tri), C.byref(cnt), None)
    assert st == _lib.ERR_INVALID_ARGUMENT and b"output array holds" in lib.ngpde_last_error()
    assert cnt.value == len(t_ref) and (tri == -7).all()


def test_coincident_points_are_refused_naming_the_smallest_pair():
    p = S.cloud("uniform", 9, 120).copy()
    p[77] = p[13]
    p[101] = p[40]
    with pytest.raises(ng.ArgumentError, match=r"points 13 and 77 coincide"):
        M.delaunay_graph(p.T)
    with pytest.raises(ng.ArgumentError, match=r"points 13 and 77 coincide"):
        M.delaunay_triangles(p.T)
    gi = np.ones(120, np.int64)                                       # in different graphs they are no pair
    gi[77] = gi[101] = 2
    M.delaunay_graph(p.T, graph_indicator=gi)


def test_a_hub_over_the_cap_is_refused_naming_the_point():
    """2 050 points on a circle and its centre: the circle alone is a valid cloud, the centre's star is over the cap, and the
    refusal is a clean status"""
    k = 2050
    a = np.arange(k) * (2 * np.pi / k)
    ring = np.stack([np.cos(a), np.sin(a)], 1).astype(np.float32)
    g = M.delaunay_graph(ring.T)
    assert g.num_edges >= 2 * k
    with pytest.raises(ng.ArgumentError, match=rf"star of point {k} exceeds NGPDE_DELAUNAY_MAX_DEGREE = 2048"):
        M.delaunay_graph(np.concatenate([ring, np.zeros((1, 2), np.float32)]).T)


def test_degenerate_clouds():
    empty = M.delaunay_graph(np.zeros((2, 0), np.float32))
    assert empty.num_nodes == 0 and empty.num_edges == 0 and M.delaunay_triangles(np.zeros((2, 0), np.float32)).shape == (0, 3)
    one = M.delaunay_graph(np.array([[0.5], [0.25]], np.float32))
    assert one.num_nodes == 1 and one.num_edges == 0
    two = np.array([[0.0, 1.0], [3.0, -2.0]], np.float32)
    g, tri = graph_and_triangles(two)
    assert directed(g).tolist() == [[0, 1], [1, 0]] and len(tri) == 0
    for line in (np.stack([np.arange(9.0), np.zeros(9)], 1), np.stack([np.zeros(9), np.arange(9.0) ** 2], 1),
                 np.stack([np.arange(70.0) * 3 - 40, 2 * (np.arange(70.0) * 3 - 40) + 7], 1)):
        perm = np.random.default_rng(4).permutation(len(line))
        p = line[perm].astype(np.float32)
        g, tri = graph_and_triangles(p)
        rank = np.argsort(perm)                                          # point rank[k] is the k-th along the line
        want = sorted([(int(rank[k]), int(rank[k + 1])) for k in range(len(p) - 1)] + [(int(rank[k + 1]), int(rank[k])) for k in range(len(p) - 1)])
        assert directed(g).tolist() == [list(w) for w in want] and len(tri) == 0


def test_input_forms_give_the_same_graph():
    p, e_ref, t_ref = small("clustered")
    wide = torch.zeros((4, 2 * len(p) + 1), dtype=torch.float32, device=DEV)
    wide[1:3, 1::2] = torch.as_tensor(p.T, device=DEV)
    forms = {"float64 numpy": p.T.astype(np.float64), "strided offset view": wide[1:3, 1::2], "cpu tensor": torch.as_tensor(p.T.copy()),
             "row-major transpose": torch.as_tensor(p, device=DEV).T}
    for name, pts in forms.items():
        assert np.array_equal(directed(M.delaunay_graph(pts)), e_ref), name
        assert np.array_equal(M.delaunay_triangles(pts).cpu().numpy(), t_ref), name


def test_a_call_on_a_side_stream_with_the_null_stream_busy():
    p, e_ref, t_ref = small("uniform")
    real = torch.as_tensor(p.T.copy(), device=DEV)
    side = torch.cuda.Stream()
    for null_busy in (True, False):
        stale = torch.full_like(real, float("nan"))
        torch.cuda.synchronize()
        if null_busy:
            torch.cuda._sleep(200_000_000)                               # the NULL stream has work queued while the side stream runs
        with torch.cuda.stream(side):
            torch.cuda._sleep(20_000_000)
            stale.copy_(real)                                            # the points arrive on the side stream, behind a delay: with
            g = M.delaunay_graph(stale)                                  # an idle NULL stream a launch or copy put there instead
            tri = M.delaunay_triangles(stale)                            # reads NaN, which is refused by name
        side.synchronize()
        torch.cuda.synchronize()
        assert np.array_equal(directed(g), e_ref) and np.array_equal(tri.cpu().numpy(), t_ref)


def test_a_gcn_layer_on_the_graph_equals_the_layer_on_qhulls_triangles():
    p = S.cloud("uniform", 21, 500)
    d = Delaunay(p.astype(np.float64))
    assert S.min_margin(p, d.simplices) >= 1024 * S.TIE_BOUND
    tri = d.simplices
    s = np.concatenate([tri[:, 0], tri[:, 1], tri[:, 2]])
    t = np.concatenate([tri[:, 1], tri[:, 2], tri[:, 0]])
    ref = ng.to_bidirected(ng.remove_multi_edges(ng.GNNGraph(s, t, num_nodes=len(p), index_base=0)))
    g = M.delaunay_graph(p.T)
    assert g.num_edges == ref.num_edges
    x = torch.randn(8, len(p), device=DEV)
    ys = []
    for gg in (g, ref):
        layer = ng.GCNConv((8, 6), "relu", initialgraph=gg)
        ps, st = ng.setup(0, layer)
        ps = ng.to_device(ps, DEV)
        y, _ = layer(x, ps, st)
        ys.append(y.cpu().numpy())
    # the two lists hold the same edges in another order (by target here, by source there): every output entry is a sum of at most
    # 8 products and a point's <= 32 neighbour terms with positive coefficients, each rounded once, so two orders differ by at most
    # 2 * 40 * 2^-24 of the largest entry's scale
    assert np.bincount(g._t0).max() <= 32
    assert np.abs(ys[0] - ys[1]).max() <= 80 * 2.0 ** -24 * max(1.0, float(np.abs(ys[1]).max()))
