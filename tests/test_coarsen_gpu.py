"""The coarsening block on the device (ngpde_amd.coarsen; include/ngpde_coarsen.h) against the numpy restatements of
tests/coarsen_spec.py.  Farthest-point sampling equals the brute force BIT FOR BIT on both paths (forced through the C entry's `path`)
and the two paths equal each other, across the sizes at which the kernels change behaviour (1, 2, around a wave, around the tile
workgroup W, more than one point per thread, the cap and the cap + 1) and in the regimes where the float rule decides (ties,
coincident points, squares that round to 0, to denormals, to inf).  grid_cluster equals the brute force exactly.  Pooling: max / min
bitwise, "+" / mean within the rounding bound (m + 2) 2^-24 sum|x| of a cluster of m members (one rounding per addition, one for the
division, one spare; for the mean the sum's bound divided by m).  Then the harness properties: HIP-graph replay, side streams, and
every array argument over dtype, stride, offset and numpy.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

import coarsen_spec as S

pytestmark = pytest.mark.gpu

K = ng.coarsen
DEV = "cuda"
W = S.TILE_THREADS
CAP = S.TILE_MAX_POINTS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = _lib.ptr


def dev(a):
    return a.to(DEV) if isinstance(a, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_path(pts, ptr, ks, starts, path):
    idx, d2, info = K._run_fps(dev(pts), np.asarray(ptr, np.int64), np.asarray(ks, np.int64), starts, path)
    torch.cuda.synchronize()
    return host(idx), host(d2), info


def assert_fps(pts, ptr, ks, starts=None, ref=None):
    """both paths equal the brute force and each other, bit for bit; the reference is returned"""
    ref = S.fps_brute(pts, ptr, ks, starts) if ref is None else ref
    ti, td, tinfo = run_path(pts, ptr, ks, starts, "tile")
    ri, rd, rinfo = run_path(pts, ptr, ks, starts, "round")
    work = int(np.sum(np.asarray(ks) > 0))
    assert tinfo[2:5] == [work, 0, 0] and rinfo[2:4] == [0, work] and rinfo[4] == max(list(ks) + [0])
    assert same_bits(ti, ref[0]) and same_bits(td, ref[1]), "tile path"
    assert same_bits(ri, ref[0]) and same_bits(rd, ref[1]), "round path"
    return ref


# ---- FPS equals the brute force on both paths ------------------------------------------------------------------------------------
SIZES = [1, 2, 63, 64, 65, W - 1, W, W + 1, 2 * W + 1]


@pytest.mark.parametrize("kind", ["none", "one", "two", "all"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_fps_equals_the_brute_force_across_sizes(dim, kind):
    """every n_g of SIZES as one graph of a batch (each graph is sampled by itself), k_g = 0, 1, 2 or n_g"""
    rng = np.random.default_rng(100 * dim + len(kind))
    ptr = np.concatenate(([0], np.cumsum(SIZES)))
    pts = rng.random((int(ptr[-1]), dim)).astype(np.float32)
    ks = [dict(none=0, one=1, two=min(2, n), all=n)[kind] for n in SIZES]
    idx, d2 = assert_fps(pts, ptr, ks)
    assert len(idx) == sum(ks)
    if kind == "all":
        for g, n in enumerate(SIZES):
            assert sorted(idx[ptr[g]:ptr[g + 1]].tolist()) == list(range(ptr[g], ptr[g + 1]))      # a point is never selected twice


def test_a_batch_of_unequal_graphs_equals_each_graph_alone():
    rng = np.random.default_rng(5)
    sizes, ks = [700, 0, 2 * W + 300], [50, 0, 333]
    ptr = np.concatenate(([0], np.cumsum(sizes)))
    pts = rng.random((int(ptr[-1]), 3)).astype(np.float32)
    starts = np.array([13, 700, 700 + 2000], dtype=np.int32)
    idx, d2 = assert_fps(pts, ptr, ks, starts)
    for g in (0, 2):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        for path in ("tile", "round", "auto"):
            ai, ad, _ = run_path(pts[lo:hi], [0, hi - lo], [ks[g]], np.array([starts[g] - lo], np.int32), path)
            at = sum(ks[:g])
            assert same_bits(ai + lo, idx[at:at + ks[g]]) and same_bits(ad, d2[at:at + ks[g]])
    # through the public function, with the indicator on the device
    gi = dev(np.repeat([1, 3], [sizes[0], sizes[2]]))
    pi, pd = K.fps(dev(pts).T, num=[50, 0, 333], graph_indicator=gi, start=starts, return_d2=True)
    assert pi.dtype == torch.int32 and pd.dtype == torch.float32 and same_bits(host(pi), idx) and same_bits(host(pd), d2)
    assert same_bits(host(K.fps(dev(pts).T, num=[50, 0, 333], graph_indicator=gi, start=starts)), idx)


def test_the_cap_takes_the_tile_path_and_one_point_more_the_round_path():
    rng = np.random.default_rng(6)
    pts = rng.random((CAP + 1, 2)).astype(np.float32)
    ref = S.fps_brute(pts, [0, CAP + 1], [8])
    idx, d2, info = run_path(pts, [0, CAP + 1], [8], None, "auto")
    assert info == [CAP + 1, 8, 0, 1, 8, 0]                                  # auto: the round path, 8 launches
    assert same_bits(idx, ref[0]) and same_bits(d2, ref[1])
    lib = _lib.load()
    plan = C.c_void_p()
    gp, sp = np.array([0, CAP + 1], np.int64), np.array([0, 8], np.int64)
    assert lib.ngpde_fps_plan_create(1, P(gp), P(sp), 2, 1, None, C.byref(plan)) == _lib.ERR_INVALID_ARGUMENT
    msg = lib.ngpde_last_error().decode()
    assert "graph 0" in msg and "FPS_TILE_MAX_POINTS = " in msg and plan.value is None
    ref = S.fps_brute(pts[:CAP], [0, CAP], [8])
    idx, d2, info = run_path(pts[:CAP], [0, CAP], [8], None, "auto")
    assert info == [CAP, 8, 1, 0, 0, 1]                                      # exactly the cap: the tile path
    assert same_bits(idx, ref[0]) and same_bits(d2, ref[1])
    assert_fps(pts[:CAP], [0, CAP], [8], ref=ref)


# ---- named regimes: each asserted on the reference before the device output is looked at -----------------------------------------------
def test_a_lattice_ties_and_the_smallest_index_wins():
    rng = np.random.default_rng(7)
    perm = rng.permutation(81)
    pts = np.stack([perm % 9, perm // 9], axis=1).astype(np.float32)
    corner = int(np.flatnonzero(perm == 0)[0])
    ties = []
    ref = S.fps_graph(pts, 81, corner, ties)
    assert ties[1] == 2 and max(ties[2:]) >= 2 and sum(t >= 2 for t in ties) > 10       # round 2 is a two-way tie, later rounds tie further
    assert sorted(ref[0].tolist()) == list(range(81))
    assert_fps(pts, [0, 81], [81], np.array([corner], np.int32), ref=ref)


def test_coincident_points_are_taken_once_each():
    rng = np.random.default_rng(8)
    pts = rng.random((47, 3)).astype(np.float32)
    pts[rng.choice(47, 10, replace=False)] = np.float32([0.25, 0.5, 0.75])
    ref = S.fps_brute(pts, [0, 47], [47])
    assert sorted(ref[0].tolist()) == list(range(47)) and int(np.sum(ref[1] == 0)) == 9
    assert_fps(pts, [0, 47], [47], ref=ref)


@pytest.mark.parametrize("regime", ["zero", "denormal", "inf"])
def test_squares_that_round_to_zero_denormals_and_inf(regime):
    rng = np.random.default_rng(9)
    n, start = 150, 17
    if regime == "inf":
        cells = rng.permutation(400)[:n]
        pts = (np.stack([cells % 20, cells // 20], axis=1) * 2).astype(np.float32) * np.float32(1e19)      # distinct; differences 0 or >= 2e19
    else:
        pts = rng.random((n, 2)).astype(np.float32) * np.float32(1e-24 if regime == "zero" else 1e-20)
    ref = S.fps_brute(pts, [0, n], [n], [start])
    rest = [i for i in range(n) if i != start]
    if regime == "zero":                                                     # every square rounds to 0: the start, then ascending indices
        assert ref[0].tolist() == [start] + rest and np.all(ref[1][1:] == 0)
    elif regime == "inf":                                                    # every distance is inf: ties go by index
        assert ref[0].tolist() == [start] + rest and np.all(np.isinf(ref[1]))
    else:
        tiny = np.finfo(np.float32).tiny
        assert np.all(ref[1][1:] < tiny) and int(np.sum(ref[1][1:] > 0)) > n // 2 and ref[0].tolist() != [start] + rest
    assert_fps(pts, [0, n], [n], np.array([start], np.int32), ref=ref)


def test_prefix_start_random_start_and_the_distances():
    rng = np.random.default_rng(10)
    sizes = [900, 1500]
    pts = dev(rng.random((2, sum(sizes))).astype(np.float32))
    gi = dev(np.repeat([1, 2], sizes))
    big, d2 = K.fps(pts, num=[200, 300], graph_indicator=gi, return_d2=True)
    small = K.fps(pts, num=[60, 7], graph_indicator=gi)
    big, d2, small = host(big), host(d2), host(small)
    assert same_bits(small, np.concatenate([big[:60], big[200:207]]))           # nested: fps(num=a) is a prefix of fps(num=b)
    assert big[0] == 0 and big[200] == 900                                    # the default start: each graph's first point
    for lo, hi in ((0, 200), (200, 500)):
        assert np.isinf(d2[lo]) and np.all(np.diff(d2[lo + 1:hi]) <= 0) and d2[hi - 1] > 0
    ref = S.fps_brute(host(pts).T.copy(), [0, 900, 2400], [200, 300])
    assert same_bits(big, ref[0]) and same_bits(d2, ref[1])
    by_ratio = host(K.fps(pts, ratio=0.1, graph_indicator=gi))
    assert same_bits(by_ratio, np.concatenate([big[:90], big[200:350]]))       # ceil(0.1 * 900) = 90, ceil(0.1 * 1500) = 150
    started = host(K.fps(pts, num=5, graph_indicator=gi, start=[450, 901]))
    assert started[0] == 450 and started[5] == 901
    assert same_bits(started, S.fps_brute(host(pts).T.copy(), [0, 900, 2400], [5, 5], [450, 901])[0])
    gen = torch.Generator()
    gen.manual_seed(123)
    drawn = [int(torch.randint(900, (1,), generator=gen)), 900 + int(torch.randint(1500, (1,), generator=gen))]
    a = host(K.fps(pts, num=9, graph_indicator=gi, random_start=True, seed=123))
    assert [a[0], a[9]] == drawn
    assert same_bits(a, host(K.fps(pts, num=9, graph_indicator=gi, start=drawn)))
    assert same_bits(a, host(K.fps(pts, num=9, graph_indicator=gi, random_start=True, seed=123)))
    torch.manual_seed(77)
    b = host(K.fps(pts, num=3, graph_indicator=gi, random_start=True))
    torch.manual_seed(77)
    assert same_bits(b, host(K.fps(pts, num=3, graph_indicator=gi, random_start=True)))      # seed=None: torch's CPU generator governs
    empty = K.fps(pts, num=0, graph_indicator=gi)
    assert empty.numel() == 0 and empty.dtype == torch.int32


# ---- grid_cluster equals the brute force exactly -----------------------------------------------------------------------------------------
def assert_clusters(cl, ref):
    assert isinstance(ref, dict), ref
    assert cl.count == ref["count"] and cl.num_points == len(ref["labels"])
    for name in ("labels", "ptr", "order", "graph_indicator"):
        got = host(getattr(cl, name))
        assert got.dtype == np.int32 and np.array_equal(got, ref[name]), name
    assert np.array_equal(host(cl.sizes), np.diff(ref["ptr"]))


def indicator_of(ptr):
    return np.repeat(np.arange(1, len(ptr)), np.diff(ptr))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_grid_cluster_equals_the_brute_force(dim):
    rng = np.random.default_rng(20 + dim)
    ptr = np.array([0, 400, 400, 1000, 1001])                                # an empty graph and a graph of one point
    pts = (rng.random((1001, dim)) * 6 - 3).astype(np.float32)               # negative coordinates
    size = [0.5, 0.25, 1.5][:dim]
    cl = K.grid_cluster(dev(pts).T, size, graph_indicator=dev(indicator_of(ptr)))
    ref = S.grid_cluster_brute(pts, size, ptr)
    assert_clusters(cl, ref)
    assert cl.num_graphs == 4 and ref["count"] > 20 and np.all(np.diff(ref["graph_indicator"]) >= 0)
    # the per-graph origin against an explicit one
    origin = [-3.0, -3.5, -4.0][:dim]
    cl2 = K.grid_cluster(dev(pts).T, 0.5, graph_indicator=dev(indicator_of(ptr)), origin=origin)
    assert_clusters(cl2, S.grid_cluster_brute(pts, [0.5] * dim, ptr, origin=origin))
    # a graph alone against inside the batch
    alone = K.grid_cluster(dev(pts[400:1000]).T, size)
    inside = host(cl.labels)[400:1000]
    assert np.array_equal(host(alone.labels), inside - inside.min()) and alone.num_graphs == 1
    # a size so large that every graph is one cluster
    one = K.grid_cluster(dev(pts).T, 1e6, graph_indicator=dev(indicator_of(ptr)))
    assert one.count == 3 and host(one.graph_indicator).tolist() == [1, 3, 4] and host(one.ptr).tolist() == [0, 400, 1000, 1001]


def test_grid_cluster_lattice_points_on_cell_edges():
    xs, ys = np.meshgrid(np.arange(-4, 7), np.arange(-3, 6))
    pts = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float32)
    pts = pts[np.random.default_rng(3).permutation(len(pts))]
    ref = S.grid_cluster_brute(pts, 2.0, [0, len(pts)])
    assert ref["count"] == 6 * 5 and np.bincount(ref["labels"]).max() == 4   # a point on an edge belongs to the upper cell: 2 x 2 blocks
    assert_clusters(K.grid_cluster(dev(pts).T, 2.0), ref)
    assert_clusters(K.grid_cluster(dev(pts).T, 2.0, origin=[-5.0, -3.0]), S.grid_cluster_brute(pts, 2.0, [0, len(pts)], origin=[-5.0, -3.0]))


def test_grid_cluster_refusals_by_name():
    rng = np.random.default_rng(4)
    pts = rng.random((300, 3)).astype(np.float32)
    wide = pts * np.float32(1e5)
    assert S.grid_cluster_brute(wide, 1e-2, [0, 300]) == "too small"          # 3 x 24 bits
    with pytest.raises(ng.ArgumentError, match="cell size too small for the cloud's extent.*bits"):
        K.grid_cluster(dev(wide).T, 1e-2)
    assert S.grid_cluster_brute(wide, 1e-6, [0, 300]) == "too small"          # a cell beyond int32
    with pytest.raises(ng.ArgumentError, match="cell size too small for the cloud's extent"):
        K.grid_cluster(dev(wide).T, 1e-6)
    assert isinstance(S.grid_cluster_brute(wide, 1.0, [0, 300]), dict)        # 3 x 17 bits: fine
    assert_clusters(K.grid_cluster(dev(wide).T, 1.0), S.grid_cluster_brute(wide, 1.0, [0, 300]))
    low = pts.copy()
    low[[70, 200], 1] = -0.5
    assert S.grid_cluster_brute(low, 0.1, [0, 300], origin=[0, 0, 0]) == "below"
    with pytest.raises(ng.ArgumentError, match="point 70 lies below the origin"):
        K.grid_cluster(dev(low).T, 0.1, origin=[0.0, 0.0, 0.0])
    assert isinstance(S.grid_cluster_brute(low, 0.1, [0, 300]), dict)         # its own minimum as origin: fine
    K.grid_cluster(dev(low).T, 0.1)
    for bad in (np.nan, np.inf, -np.inf):
        broken = pts.copy()
        broken[[123, 250], 2] = bad
        assert S.grid_cluster_brute(broken, 0.1, [0, 300]) == "non-finite"
        with pytest.raises(ng.ArgumentError, match="point 123 has a non-finite coordinate"):
            K.grid_cluster(dev(broken).T, 0.1)


# ---- pooling -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def parts():
    """700 points in 3 graphs: a cluster of 250 scattered points, 40 singletons, the rest in clusters of a handful"""
    rng = np.random.default_rng(30)
    sizes = [300, 150, 250]
    gi = indicator_of(np.concatenate(([0], np.cumsum(sizes))))
    labels = np.zeros(700, np.int64)
    labels[:300] = 1 + rng.integers(0, 30, 300)                              # graph 1: clusters 1 .. 30
    labels[rng.choice(300, 250, replace=False)] = 0                          # ... and the large cluster 0
    labels[300:340] = 31 + np.arange(40)                                     # graph 2: 40 singletons, then clusters 71 .. 80
    labels[340:450] = 71 + rng.integers(0, 10, 110)
    labels[450:] = 81 + rng.integers(0, 20, 250)                             # graph 3
    labels = np.unique(labels, return_inverse=True)[1]                       # every label occurs, the order is kept
    cl = K.Clusters.from_labels(dev(labels), graph_indicator=dev(gi))
    sizes_c = np.bincount(labels)
    assert sizes_c.max() >= 200 and int(np.sum(sizes_c == 1)) >= 40
    order = np.argsort(labels, kind="stable")
    assert np.array_equal(host(cl.labels), labels) and np.array_equal(host(cl.order), order) and cl.count == len(sizes_c)
    assert np.array_equal(host(cl.ptr), np.concatenate(([0], np.cumsum(sizes_c)))) and np.array_equal(host(cl.sizes), sizes_c)
    assert np.array_equal(host(cl.graph_indicator), gi[order[np.cumsum(sizes_c) - 1]]) and cl.num_graphs == 3
    return dict(cl=cl, labels=labels, sizes=sizes_c, n=700)


@pytest.mark.parametrize("d", [1, 3, 64, 65, 130])
def test_pool_against_float64_and_bitwise_extrema(parts, d):
    f, lib = parts, _lib.load()
    cl, n, c = f["cl"], f["n"], f["cl"].count
    x = np.random.default_rng(31 + d).standard_normal((n, d)).astype(np.float32)
    xd = dev(x)
    for aggr in ("+", "mean", "max", "min"):
        out = torch.full((c, d), float("nan"), device=DEV)                   # pre-filled with NaN: every entry is written
        assert lib.ngpde_cluster_pool_forward(n, c, d, _lib.AGGR[aggr], P(cl.ptr), P(cl.order), P(xd), P(out), _lib.current_stream()) == 0
        got = host(out)
        assert same_bits(host(K.pool(cl, xd.T, aggr)).T, got)
        ref, mag, sizes = S.pool_ref(x, f["labels"], c, aggr)
        if aggr in ("max", "min"):
            assert same_bits(got, ref.astype(np.float32))
        else:
            bound = (sizes[:, None] + 2) * 2.0 ** -24 * mag
            err = np.abs(got.astype(np.float64) - ref)
            print(f"pool {aggr!r} d = {d}: reached {float((err / bound).max()):.3f} of the bound")
            assert np.all(err <= bound)
    again = torch.full((c, d), float("nan"), device=DEV)
    assert lib.ngpde_cluster_pool_forward(n, c, d, 0, P(cl.ptr), P(cl.order), P(xd), P(again), _lib.current_stream()) == 0
    assert same_bits(host(again), host(K.pool(cl, xd.T, "+")).T)              # the same bits every run


@pytest.mark.parametrize("aggr", ["+", "mean", "max", "min"])
def test_autograd_equals_the_backward_entry(parts, aggr):
    f, lib = parts, _lib.load()
    cl, n, c, d = f["cl"], f["n"], f["cl"].count, 5
    rng = np.random.default_rng(40)
    x = rng.integers(-3, 4, (n, d)).astype(np.float32)                       # small integers: every large cluster has tied extrema
    dout = rng.standard_normal((c, d)).astype(np.float32)
    xt = dev(x).T.clone().requires_grad_(True)
    out = K.pool(cl, xt, aggr)
    out.backward(dev(dout).T)
    dx = torch.full((n, d), float("nan"), device=DEV)
    outr = out.detach().T.contiguous()
    assert lib.ngpde_cluster_pool_backward(n, c, d, _lib.AGGR[aggr], P(cl.labels), P(cl.ptr), P(dev(x)), P(outr), P(dev(dout)), P(dx),
                                           _lib.current_stream()) == 0
    assert same_bits(host(xt.grad).T, host(dx))
    want = S.pool_backward_ref(x, host(outr), dout, f["labels"], f["sizes"], aggr)
    assert same_bits(host(dx), want)
    if aggr in ("max", "min"):
        tied = (x == host(outr)[f["labels"]]).sum(axis=0)
        assert np.all(tied > c)                                              # more entries receive a gradient than there are clusters: ties


def test_unpool_is_a_gather_and_its_pullback_the_sum_pool(parts):
    cl, c, n = parts["cl"], parts["cl"].count, parts["n"]
    rng = np.random.default_rng(41)
    xc = dev(rng.standard_normal((4, c)).astype(np.float32)).requires_grad_(True)
    w = dev(rng.standard_normal((4, n)).astype(np.float32))
    y = cl.unpool(xc)
    assert same_bits(host(y), host(xc)[:, parts["labels"]])
    y.backward(w)
    assert same_bits(host(xc.grad), host(K.pool(cl, w, "+")))
    pos = dev(rng.random((2, n)).astype(np.float32))
    assert same_bits(host(K.pool_positions(cl, pos)), host(K.pool(cl, pos, "mean")))


def test_pool_graph_equals_relabel_drop_loops_and_unique_with_sum(parts):
    cl, labels, n = parts["cl"], parts["labels"], parts["n"]
    rng = np.random.default_rng(42)
    e = 5000
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    w = rng.integers(1, 9, e).astype(np.float32)                             # integer weights: the sums are exact in float32
    wd = dev(w).requires_grad_(True)
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=wd)
    coarse = K.pool_graph(g, cl)
    rs, rt, rw = S.pool_graph_ref(s, t, w, labels, cl.count)
    cs, ct = coarse.edge_index(index_base=0)
    assert coarse.num_nodes == cl.count and coarse.num_graphs == 3 and len(rs) < e
    assert np.array_equal(cs, rs) and np.array_equal(ct, rt)                  # by source, then target; no loops, no duplicates
    assert np.array_equal(host(coarse.edge_weight).astype(np.float64), rw)
    assert np.array_equal(coarse.graph_indicator, host(cl.graph_indicator) - 1)
    coarse.edge_weight.sum().backward()
    keep = labels[s] != labels[t]
    assert np.array_equal(host(wd.grad), keep.astype(np.float32))             # the gradient reaches every edge that was not a loop


# ---- HIP graph: fps, pool forward and pool backward replay to the eager bits ------------------------------------------------------------
def test_fps_and_pooling_replay_from_one_hip_graph(parts):
    lib = _lib.load()
    cl, n, c, d = parts["cl"], parts["n"], parts["cl"].count, 33
    rng = np.random.default_rng(50)
    sizes = [300, 150, 250]
    gp = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    ks = np.array([40, 150, 9], np.int64)
    sp = np.concatenate(([0], np.cumsum(ks))).astype(np.int64)
    pts = dev(rng.random((n, 2)).astype(np.float32))
    x, dout = dev(rng.standard_normal((n, d)).astype(np.float32)), dev(rng.standard_normal((c, d)).astype(np.float32))
    plans = []
    for path in (1, 2):                                                      # both paths inside the one graph; made ahead: a create allocates
        plan = C.c_void_p()
        assert lib.ngpde_fps_plan_create(3, P(gp), P(sp), 2, path, None, C.byref(plan)) == 0
        nbytes = int(lib.ngpde_fps_workspace_bytes(plan))
        plans.append((plan, torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV), nbytes))
    K_ = int(sp[-1])
    idx = [torch.empty(K_, dtype=torch.int32, device=DEV) for _ in plans]
    d2 = [torch.empty(K_, dtype=torch.float32, device=DEV) for _ in plans]
    out, dx = torch.empty((c, d), device=DEV), torch.empty((n, d), device=DEV)

    def all_three():
        s = _lib.current_stream()
        for (plan, ws, nbytes), i, dd in zip(plans, idx, d2):
            assert lib.ngpde_fps(plan, P(pts), None, 0, P(i), P(dd), P(ws), nbytes, s) == 0
        assert lib.ngpde_cluster_pool_forward(n, c, d, 2, P(cl.ptr), P(cl.order), P(x), P(out), s) == 0
        assert lib.ngpde_cluster_pool_backward(n, c, d, 2, P(cl.labels), P(cl.ptr), P(x), P(out), P(dout), P(dx), s) == 0

    all_three()
    torch.cuda.synchronize()
    outs = idx + d2 + [out, dx]
    eager = [host(t).copy() for t in outs]
    ref = S.fps_brute(host(pts), gp, ks)
    assert same_bits(eager[0], ref[0]) and same_bits(eager[1], ref[0]) and same_bits(eager[2], ref[1]) and same_bits(eager[3], ref[1])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                            # a single stream, no parallel branches
        all_three()
    for t in outs:
        t.fill_(-1) if t.dtype == torch.int32 else t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for t, e in zip(outs, eager):
        assert same_bits(host(t), e)
    for plan, _, _ in plans:
        assert lib.ngpde_fps_plan_destroy(plan) == 0


# ---- streams: every stream-taking entry behind still-running producer work ---------------------------------------------------------------
def header_stream_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngpde_coarsen.h")).read(), flags=re.S)
    return sorted(name for name, args in re.findall(r"\b(ngpde_[a-z0-9_]+)\s*\(([^)]*)\)", src) if "ngpde_stream_t" in args)


def stream_cases():
    """name -> (inputs, call): call(inputs, stream) runs the entry on `stream` and returns (statuses, outputs)"""
    lib = _lib.load()
    rng = np.random.default_rng(60)
    sizes = [2 * S.TILE_THREADS + 5, 600]
    n, d = sum(sizes), 48
    gp = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    sp = np.array([0, 30, 50], np.int64)
    pts = rng.random((n, 2)).astype(np.float32)
    start = np.array([7, sizes[0] + 3], np.int32)
    ref = S.grid_cluster_brute(pts, 0.125, gp)
    c = ref["count"]
    x, dout = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((c, d)).astype(np.float32)
    pooled = S.pool_ref(x, ref["labels"], c, "max")[0].astype(np.float32)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=DEV)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)

    def fps_on(path, create_on_stream):
        def call(a, s):
            if getattr(call, "keep", None):
                lib.ngpde_fps_plan_destroy(call.keep[0])
            plan = C.c_void_p()
            st = [lib.ngpde_fps_plan_create(2, P(gp), P(sp), 2, path, s if create_on_stream else None, C.byref(plan))]
            nbytes = int(lib.ngpde_fps_workspace_bytes(plan))
            ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=DEV)
            oi, od = i32(50), f32(50)
            st.append(lib.ngpde_fps(plan, P(a["pts"]), P(a["start"]), 0, P(oi), P(od), P(ws), nbytes, s))
            call.keep = (plan, ws)                                           # destroyed by the next call: the launches here may still be queued
            return st, [oi, od]
        return call

    def grid(a, s):
        size = np.array([0.125, 0.125], np.float32)
        ol, op, oo, og = i32(n), i32(n + 1), i32(n), i32(n)
        cnt = C.c_int64(0)
        st = [lib.ngpde_grid_cluster(n, 2, P(a["pts"]), 2, P(gp), P(size), None, P(ol), P(op), P(oo), P(og), C.byref(cnt), s)]
        k = int(cnt.value)
        return st, [ol, op[:k + 1], oo, og[:k], torch.tensor([k])]

    def forward(a, s):
        o = f32(c, d)
        return [lib.ngpde_cluster_pool_forward(n, c, d, 1, P(a["ptr"]), P(a["order"]), P(a["x"]), P(o), s)], [o]

    def backward(a, s):
        o = f32(n, d)
        return [lib.ngpde_cluster_pool_backward(n, c, d, 2, P(a["labels"]), P(a["ptr"]), P(a["x"]), P(a["out"]), P(a["dout"]), P(o), s)], [o]

    sets = dict(pts=pts, start=start)
    return {
        "ngpde_fps": (sets, fps_on(1, False)),
        "ngpde_fps round path": (sets, fps_on(2, False)),
        "ngpde_fps_plan_create": (sets, fps_on(0, True)),
        "ngpde_grid_cluster": (dict(pts=pts), grid),
        "ngpde_cluster_pool_forward": (dict(ptr=ref["ptr"], order=ref["order"], x=x), forward),
        "ngpde_cluster_pool_backward": (dict(labels=ref["labels"], ptr=ref["ptr"], x=x, out=pooled, dout=dout), backward),
    }


CASES = None


def case(name):
    global CASES
    if CASES is None:
        CASES = stream_cases()
    return CASES[name]


class Side:
    """a side stream that does not run in order with the NULL stream, and a calibrated delay (torch.cuda._sleep)"""

    def __init__(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
        torch.cuda.synchronize()
        self.cycles_per_ms = 20_000_000 / a.elapsed_time(b)
        assert 1e3 < self.cycles_per_ms < 1e8
        self.stream = None

    def run(self, inputs, call, stream, ms=20.0):
        """the inputs arrive on the side stream behind a delay, in buffers that hold NaN / zeros until then; `call` gets `stream`"""
        real = {k: dev(v) for k, v in inputs.items()}
        stale = {k: (torch.full_like(v, float("nan")) if v.is_floating_point() else torch.zeros_like(v)) for k, v in real.items()}
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
            for k in stale:
                stale[k].copy_(real[k])
            st, out = call(stale, self.stream.cuda_stream if stream == "side" else None)
        self.stream.synchronize()
        torch.cuda.synchronize()
        return st, [host(o).copy() for o in out]


def expected(name):
    inputs, call = case(name)
    st, out = call({k: dev(v) for k, v in inputs.items()}, None)
    torch.cuda.synchronize()
    assert st == [0] * len(st), (name, _lib.load().ngpde_last_error())
    return [host(o).copy() for o in out]


@pytest.fixture(scope="module")
def side():
    """the control: ONE deliberately mis-streamed call (stream = NULL while its inputs arrive on the side stream) must differ from the
    expected result; up to 8 streams are tried for one that does not share the NULL stream's order"""
    s = Side()
    name = "ngpde_cluster_pool_forward"
    want = expected(name)
    for _ in range(8):
        s.stream = torch.cuda.Stream()
        st, got = s.run(*case(name), stream="null")
        if not all(same_bits(g, w) for g, w in zip(got, want)):
            return s
    pytest.fail("no side stream out of order with the NULL stream: the stream cases could not fail")


def test_the_stream_cases_cover_the_header():
    assert sorted(k for k in stream_cases() if " " not in k) == header_stream_entries() and len(header_stream_entries()) == 5


@pytest.mark.parametrize("name", ["ngpde_fps", "ngpde_fps round path", "ngpde_fps_plan_create", "ngpde_grid_cluster",
                                  "ngpde_cluster_pool_forward", "ngpde_cluster_pool_backward"])
def test_entry_runs_on_the_stream_it_is_given(side, name):
    want = expected(name)
    if name.startswith("ngpde_fps"):
        ref = S.fps_brute(case(name)[0]["pts"], [0, 2 * S.TILE_THREADS + 5, 2 * S.TILE_THREADS + 605], [30, 20], case(name)[0]["start"])
        assert same_bits(want[0], ref[0]) and same_bits(want[1], ref[1])
    st, got = side.run(*case(name), stream="side")
    assert st == [0] * len(st), (name, _lib.load().ngpde_last_error())
    assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)), name


# ---- every array argument over dtype, stride, offset and numpy ------------------------------------------------------------------------------
def variants(t):
    """the same values as float64, with stride 2, at storage offset 1 and as a numpy array"""
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    shifted = flat[1:].view(t.shape)
    assert wide[..., ::2].stride(-1) == 2 and shifted.storage_offset() == 1
    return {"float64": t.double(), "stride 2": wide[..., ::2], "offset 1": shifted, "numpy": t.cpu().numpy()}


def sweep_inputs():
    rng = np.random.default_rng(70)
    n = 90
    pts = torch.as_tensor(rng.integers(0, 64, (2, n)) / 8.0, dtype=torch.float32, device=DEV)
    gi = torch.as_tensor(np.repeat([1, 2, 4], [40, 30, 20]), dtype=torch.int64, device=DEV)
    start = torch.as_tensor([5, 41, 0, 88], dtype=torch.int64, device=DEV)
    x = torch.as_tensor(rng.integers(-8, 9, (5, n)) / 4.0, dtype=torch.float32, device=DEV)
    labels = torch.as_tensor(np.sort(rng.integers(0, 12, n)), dtype=torch.int64, device=DEV)
    return dict(points=pts, graph_indicator=gi, start=start, x=x, labels=labels)


SWEPT = {"fps": ("points", "graph_indicator", "start"), "grid_cluster": ("points", "graph_indicator"),
         "from_labels": ("labels", "graph_indicator"), "pool": ("x",), "pool_positions": ("points",), "unpool": ("x",)}


def outputs_of(fn, a):
    if fn == "fps":
        return list(K.fps(a["points"], ratio=0.3, graph_indicator=a["graph_indicator"], start=a["start"], return_d2=True))
    if fn == "grid_cluster":
        cl = K.grid_cluster(a["points"], 1.5, graph_indicator=a["graph_indicator"])
        return [cl.labels, cl.ptr, cl.order, cl.graph_indicator]
    if fn == "from_labels":
        gi = a["graph_indicator"]
        cl = K.Clusters.from_labels(a["labels"], graph_indicator=(gi if isinstance(gi, np.ndarray) else gi.clone()).clip(1, 1))
        return [cl.labels, cl.ptr, cl.order, cl.graph_indicator]
    cl = K.Clusters.from_labels(sweep_inputs()["labels"])
    if fn == "pool":
        return [K.pool(cl, a["x"], "+"), K.pool(cl, a["x"], "max")]
    if fn == "pool_positions":
        return [K.pool_positions(cl, a["points"])]
    xc = a["x"][..., :cl.count]
    return [cl.unpool(xc)]


@pytest.mark.parametrize("fn", sorted(SWEPT))
def test_every_array_argument_in_every_form(fn):
    base = sweep_inputs()
    want = outputs_of(fn, base)
    assert all(w.numel() > 0 for w in want)
    for name in SWEPT[fn]:
        for form, value in variants(base[name]).items():
            got = outputs_of(fn, dict(base, **{name: value}))
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and torch.equal(g, w), (fn, name, form)
