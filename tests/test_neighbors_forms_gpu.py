"""Neighbour search on the device across the cell grid's unusual forms: ngpde_radius_graph / ngpde_knn_graph / ngpde_spatial_order at
the C entries against the brute-force float32 restatement (oracle.ngpde_oracle.radius_graph / knn_graph / spatial_order).  Every
comparison is exact -- the same list in the same order -- or the call is refused by name; no tolerance occurs.

tests/test_neighbors_gpu.py compares at one comfortable geometry (thousands of points in the unit box, an ordinary grid).  Here the
grid itself is the subject: the 8192-cells-per-dimension cap, the coarsening loop under the cell budget, flat and coincident boxes,
coordinates far from the origin, one outlier that inflates the box, batches whose members sit far apart, clouds smaller than a
workgroup, a k-NN ring walk across a hundred empty rings, and magnitudes at which r*r or (p_i - p_j)^2 leave the float range (there
the float rule accepts every pair, and the grid has to be one cell: csrc/neighbor_grid.h).

grid_np() restates neighbor_grid.h's make_grid in numpy float32.  Its only use is that each named case asserts the regime it is named
for, so a case that drifts out of its regime fails instead of passing vacuously.  Each case also asserts, on the oracle's output and
before the device's is looked at, that it is not empty (n/2 edges, or the planted pairs where the case is named sparse) and, where it
is about ties, that some point's k-th and (k+1)-th distances are equal.  tests/host/neighbor_grid_check.cpp checks the grid's
properties themselves on the host.
"""
import ctypes as C
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from oracle import ngpde_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
FLT_MAX = np.finfo(np.float32).max
FLT_MIN = np.finfo(np.float32).tiny
K_MIN_CELL = F(2.0 ** -69)
CAP = 8192


# ---- the grid, restated ----------------------------------------------------------------------------------------------------------
Grid = namedtuple("Grid", "lo cell inv nc cells steps")


def cell_budget(n):
    return min(max(4 * n, 1 << 16), 1 << 30)


def radius_want(r):
    with np.errstate(all="ignore"):
        return F(r) * F(1.01) if np.isfinite(F(r) * F(r)) else F(np.inf)


def knn_want(P, k, n_graphs=1):
    ext = P.max(axis=1).astype(np.float64) - P.min(axis=1).astype(np.float64)
    vol = float(np.prod(np.maximum(ext, 1e-30)))
    want = (vol * max(1.0, 0.5 * k) / max(1.0, P.shape[1] / n_graphs)) ** (1.0 / P.shape[0])
    return F(want) if want < float(FLT_MAX) else F(np.inf)


def grid_np(P, want, n_graphs=1):
    """neighbor_grid.h's make_grid over the bounding box of P (dim x n), float32 operation by operation"""
    with np.errstate(all="ignore"):
        lo, hi = P.min(axis=1), P.max(axis=1)
        ext = (hi - lo).astype(F)
        assert np.all(np.isfinite(ext))
        ext_max = max(F(0), ext.max())
        budget, cell, steps, nc = cell_budget(P.shape[1]), F(want), 0, [1, 1, 1]
        one = not np.isfinite(cell)
        if not one:
            if not cell > 0:
                cell = ext_max / F(CAP) if ext_max > 0 else F(1)
            cell = max(cell, ext_max / F(CAP), K_MIN_CELL)
            while True:
                nc = [int(min(float(CAP), np.floor(float(e) / float(cell)) + 1.0)) for e in ext] + [1] * (3 - len(ext))
                if nc[0] * nc[1] * nc[2] * n_graphs <= budget or nc == [1, 1, 1]:
                    break
                if not cell < FLT_MAX / F(1.26):
                    one = True
                    break
                cell, steps = F(cell * F(1.26)), steps + 1
        if one:
            cell, nc = min(max(max(ext_max, F(1)) * F(2), K_MIN_CELL), F(2.0 ** 126)), [1, 1, 1]
        return Grid(lo, cell, F(1) / cell, nc, nc[0] * nc[1] * nc[2], steps)


def cells_of(P, g):
    with np.errstate(all="ignore"):
        c = ((P - g.lo[:, None]).astype(F) * g.inv).astype(F)
    return np.clip(c.astype(np.int64), 0, np.array(g.nc[:P.shape[0]])[:, None] - 1)


def ordinary(g):
    return g.steps == 0 and g.cells > 1 and max(g.nc) < CAP


# ---- device calls at the C entries ------------------------------------------------------------------------------------------------
def to_dev(P, gi):
    pts = torch.as_tensor(np.array(P.T, dtype=F, order="C"), device=DEV)           # [n][dim], a writable copy
    gd = None if gi is None else torch.as_tensor(np.asarray(gi, np.int32), device=DEV)
    return pts, gd


def dev_radius(P, r, gi=None, n_graphs=1, id_base=0, self_loops=False, dir_out=0, index_base=0):
    """(status, s, t) as int64 arrays"""
    lib = _lib.load()
    dim, n = P.shape
    pts, gd = to_dev(P, gi)
    ne = C.c_int64(-1)
    st = lib.ngpde_radius_graph(n, dim, pts.data_ptr(), float(r), _lib.ptr(gd), n_graphs, id_base, int(self_loops), dir_out, index_base, 0,
                                None, None, C.byref(ne), None)
    if st != _lib.OK:
        return st, None, None
    m = ne.value
    s = torch.full((max(m, 1),), -7, dtype=torch.int32, device=DEV)
    t = torch.full((max(m, 1),), -7, dtype=torch.int32, device=DEV)
    st = lib.ngpde_radius_graph(n, dim, pts.data_ptr(), float(r), _lib.ptr(gd), n_graphs, id_base, int(self_loops), dir_out, index_base, m,
                                s.data_ptr(), t.data_ptr(), C.byref(ne), None)
    assert st == _lib.OK and ne.value == m, lib.ngpde_last_error()
    return st, s[:m].cpu().numpy().astype(np.int64), t[:m].cpu().numpy().astype(np.int64)


def dev_knn(P, k, gi=None, n_graphs=1, id_base=0, self_loops=False, dir_out=0, index_base=0):
    lib = _lib.load()
    dim, n = P.shape
    pts, gd = to_dev(P, gi)
    s = torch.full((n * k,), -7, dtype=torch.int32, device=DEV)
    t = torch.full((n * k,), -7, dtype=torch.int32, device=DEV)
    st = lib.ngpde_knn_graph(n, dim, pts.data_ptr(), k, _lib.ptr(gd), n_graphs, id_base, int(self_loops), dir_out, index_base, s.data_ptr(),
                             t.data_ptr(), None)
    return st, s.cpu().numpy().astype(np.int64), t.cpu().numpy().astype(np.int64)


def dev_order(P, gi=None, n_graphs=1, id_base=0):
    lib = _lib.load()
    dim, n = P.shape
    pts, gd = to_dev(P, gi)
    out = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    st = lib.ngpde_spatial_order(n, dim, pts.data_ptr(), _lib.ptr(gd), n_graphs, id_base, out.data_ptr(), None)
    return st, out.cpu().numpy()


def refused(st, word):
    return st == _lib.ERR_INVALID_ARGUMENT and word in _lib.load().ngpde_last_error()


# ---- the oracle, once per input ---------------------------------------------------------------------------------------------------
def pair_d2(P):
    with np.errstate(all="ignore"):
        return O._pair_d2_f32(np.ascontiguousarray(P.T), np.ascontiguousarray(P.T))


@functools.lru_cache(maxsize=None)
def oracle_radius(name, self_loops):
    c = case(name)
    with np.errstate(all="ignore"):
        s, t = O.radius_graph(c.P, c.r, self_loops=self_loops)
    s.setflags(write=False)
    t.setflags(write=False)
    return s, t


@functools.lru_cache(maxsize=None)
def oracle_knn(name, k):
    c = case(name)
    with np.errstate(all="ignore"):
        s, t = O.knn_graph(c.P, k)
    s.setflags(write=False)
    t.setflags(write=False)
    return s, t


def has_tie_at_k(P, k):
    """some point's k-th and (k+1)-th smallest distances to the others are equal"""
    d2 = pair_d2(P).astype(np.float64)
    d2[np.isinf(d2)] = 1e300
    np.fill_diagonal(d2, np.inf)
    d = np.sort(d2, axis=1)
    return P.shape[1] >= k + 2 and bool(np.any(d[:, k - 1] == d[:, k]))


# ---- geometry cases ---------------------------------------------------------------------------------------------------------------
# P (dim x n) float32, r, sparse: the oracle's radius list may be short (then the case plants ten pairs), ties: the k-NN is decided by
# index for some point, regime(P, r): asserts that the case is where its name says
Case = namedtuple("Case", "P r sparse ties regime")
CASES = {}


def geometry(name, sparse=False, ties=False):
    def deco(fn):
        CASES[name] = (fn, sparse, ties)
        return fn
    return deco


@functools.lru_cache(maxsize=None)
def case(name):
    fn, sparse, ties = CASES[name]
    P, r, regime = fn(np.random.default_rng(sum(map(ord, name))))
    P = np.ascontiguousarray(P, dtype=F)
    P.setflags(write=False)
    return Case(P, r, sparse, ties, regime)


def plant(P, r):
    """ten pairs at distance r/2 along the first coordinate: the last ten points beside the first ten"""
    P[:, -10:] = P[:, :10]
    P[0, -10:] += F(r) / F(2)
    return P


def _sweep(n, knn_groups, radius_blocks):
    def build(rng):
        P = rng.random((2, n)).astype(F)

        def regime(P, r):
            assert (P.shape[1] + 63) // 64 == knn_groups and (P.shape[1] + 255) // 256 == radius_blocks
        return P, (2.0 if n <= 2 else 0.15), regime
    return build


for _n, _g, _b in ((1, 1, 1), (2, 1, 1), (63, 1, 1), (64, 1, 1), (65, 2, 1), (255, 4, 1), (256, 4, 1), (257, 5, 2)):
    geometry(f"n{_n}")(_sweep(_n, _g, _b))


@geometry("capped_1d", sparse=True)
def _capped_1d(rng):
    P = rng.random((1, 600)).astype(F)
    P[0, 10], P[0, 11] = 0.0, 1.0
    r = 1e-6

    def regime(P, r):
        g = grid_np(P, radius_want(r))
        assert g.nc == [CAP, 1, 1] and g.steps == 0 and g.cell > F(1.01) * F(r)
    return plant(P, r), r, regime


def _clumps(rng, dim, n=600):
    """box 1e4 x 1e-3 (x 1): 60 sites along the long side, ten points within +-0.4 of each, the corners of the box among them"""
    x = np.repeat(rng.random(n // 10) * 9998 + 1, 10) + rng.random(n) * 0.8 - 0.4
    P = np.stack([x] + [rng.random(n) * s for s in (1e-3, 1.0)[:dim - 1]]).astype(F)
    P[:, 0] = 0
    P[:, 1] = (1e4, 1e-3, 1.0)[:dim]
    return P


def _aniso(dim, frac, capped):
    def build(rng):
        P = _clumps(rng, dim)

        def regime(P, r):
            g = grid_np(P, radius_want(r))
            assert g.steps == 0 and g.nc[1:] == [1, 1]
            if capped:
                assert g.nc[0] == CAP and g.cell > F(1.01) * F(r)
            else:
                assert 1000 < g.nc[0] < CAP
        return P, frac * 1e4, regime
    return build


# r = 2e-4 of the long side leaves 4951 cells along it (1e4 / 2.02): anisotropic but under the cap; r = 1e-4 of it reaches the cap
geometry("aniso_2d")(_aniso(2, 2e-4, False))
geometry("aniso_3d")(_aniso(3, 2e-4, False))
geometry("capped_aniso_2d")(_aniso(2, 1e-4, True))
geometry("capped_aniso_3d")(_aniso(3, 1e-4, True))


def _coarsened(dim):
    def build(rng):
        P = rng.random((dim, 600)).astype(F)
        P[:, 10], P[:, 11] = 0.0, 1.0
        r = 1e-5

        def regime(P, r):
            g = grid_np(P, radius_want(r))
            assert g.steps >= 1 and 1 < g.cells <= cell_budget(P.shape[1]) and g.cell > F(1.01) * F(r)
        return plant(P, r), r, regime
    return build


geometry("coarsened_2d", sparse=True)(_coarsened(2))
geometry("coarsened_3d", sparse=True)(_coarsened(3))


def _offset(shift, quantum):
    def build(rng):
        P = (rng.random((2, 500)) + shift).astype(F)

        def regime(P, r):
            assert ordinary(grid_np(P, radius_want(r)))
            assert np.all(P / F(quantum) == np.round(P / F(quantum)))           # the offset has eaten the low bits
        return P, 0.1, regime
    return build


geometry("offset_1e6", ties=True)(_offset(1e6, 1 / 16))          # coordinates on a 1/16 lattice
geometry("offset_m1e3")(_offset(-1e3, 2.0 ** -14))
geometry("offset_1p6e7", ties=True)(_offset(1.6e7, 1.0))          # coordinates quantised to whole numbers: four sites


@geometry("outlier")
def _outlier(rng):
    P = (rng.random((2, 501)) * 1e-3).astype(F)
    P[:, 250] = 1e6

    def regime(P, r):
        g = grid_np(P, radius_want(r))
        c = cells_of(P, g)
        lin = c[0] * g.nc[1] + c[1]
        assert g.cells > 1 and np.sum(lin == lin[0]) == P.shape[1] - 1 and lin[250] != lin[0]
    return P, 1e-4, regime


def _flat(kind):
    def build(rng):
        n = 100 if kind == "coincident" else 600
        P = rng.random((3, n))
        if kind == "collinear":
            P[1], P[2] = 0.5, -2.0
        elif kind == "coplanar":
            P[2] = 3.0
        else:
            P[:] = 1.0
        flat = {"collinear": [1, 2], "coplanar": [2], "coincident": [0, 1, 2]}[kind]

        def regime(P, r):
            g = grid_np(P, radius_want(r))
            assert all(g.nc[d] == 1 for d in flat) and all(g.nc[d] > 1 for d in range(3) if d not in flat)
        return P.astype(F), {"collinear": 0.01, "coplanar": 0.05, "coincident": 0.0}[kind], regime
    return build


geometry("collinear_3d")(_flat("collinear"))
geometry("coplanar_3d")(_flat("coplanar"))
geometry("coincident_3d", ties=True)(_flat("coincident"))


def _lattice(shift):
    def build(rng):
        ax = np.arange(24, dtype=F) * F(0.125)
        P = np.stack([a.reshape(-1) for a in np.meshgrid(ax, ax, indexing="ij")]).astype(F) + np.array(shift, F)[:, None]

        def regime(P, r):
            d2, r2 = pair_d2(P), F(r) * F(r)
            assert np.sum(np.abs(d2 - r2) <= 4 * np.spacing(r2)) >= 2 * P.shape[1]     # pairs at the threshold, to the last bits
            assert ordinary(grid_np(P, radius_want(r)))
        return P.astype(F), 0.125, regime
    return build


geometry("lattice", ties=True)(_lattice((0.0, 0.0)))
geometry("lattice_shifted", ties=True)(_lattice((0.3, -7.7)))


@geometry("duplicates", ties=True)
def _duplicates(rng):
    P = np.repeat(rng.random((2, 40)), 8, axis=1)[:, rng.permutation(320)].astype(F)

    def regime(P, r):
        assert np.unique(P.T, axis=0).shape[0] == 40 and r == 0.0
    return P, 0.0, regime


def _magnitude(dim, sx, sy, r, what):
    def build(rng):
        P = (rng.random((dim, 200)) * np.array([sx, sy, sx][:dim])[:, None]).astype(F)

        def regime(P, r):
            with np.errstate(all="ignore"):
                g, r2, d2 = grid_np(P, radius_want(r)), F(r) * F(r), pair_d2(P)
            if what == "underflow":        # r*r and every square round to 0: the float rule accepts every pair
                assert r2 == 0 and np.all(d2 == 0) and g.cells == 1 and g.cell == K_MIN_CELL
            elif what == "denormal":       # the box itself is denormal
                assert 0 < (P.max() - P.min()) < FLT_MIN and np.all(d2 == 0) and g.cells == 1 and np.isfinite(g.inv)
            elif what == "finite":         # squares up to 1e38: still inside the float range, an ordinary grid
                assert np.isfinite(r2) and np.all(np.isfinite(d2)) and d2.max() > 1e37 and ordinary(g)
            else:                          # r*r = inf: d2 <= inf accepts every pair, most d2 are inf themselves
                assert np.isinf(r2) and np.isfinite(F(r)) and np.mean(np.isinf(d2)) > 0.5 and g.cells == 1 and g.inv > 0
        return P, r, regime
    return build


geometry("mag_1em30", ties=True)(_magnitude(2, 1e-30, 1e-30, 1e-31, "underflow"))
geometry("mag_1em40", ties=True)(_magnitude(2, 1e-40, 1e-40, 0.0, "denormal"))
geometry("mag_1e19")(_magnitude(2, 1e19, 1e19, 1e18, "finite"))
geometry("mag_1e30", ties=True)(_magnitude(2, 1e30, 1e30, 1e29, "overflow"))
geometry("mag_1e30_3d", ties=True)(_magnitude(3, 1e30, 1e30, 1e29, "overflow"))
geometry("mag_3e38_x_1", ties=True)(_magnitude(2, 3e38, 1.0, 1e37, "overflow"))

NAMES = sorted(CASES)


# ---- radius, k-NN and order on every geometry case ----------------------------------------------------------------------------------
@pytest.mark.parametrize("self_loops", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_radius_graph_matches_brute_force(name, self_loops):
    c = case(name)
    n = c.P.shape[1]
    c.regime(c.P, c.r)
    so, to = oracle_radius(name, self_loops)
    if n == 1 and not self_loops:
        assert so.size == 0
    elif c.sparse:
        assert so.size >= 20                      # the ten planted pairs, both ways
    else:
        assert so.size >= max(n // 2, 1)
    st, s, t = dev_radius(c.P, c.r, self_loops=self_loops)
    assert st == _lib.OK, _lib.load().ngpde_last_error()
    assert s.size == so.size
    assert np.array_equal(t, to) and np.array_equal(s, so)


@pytest.mark.parametrize("k", [1, 6])
@pytest.mark.parametrize("name", NAMES)
def test_knn_graph_matches_brute_force(name, k):
    c = case(name)
    n = c.P.shape[1]
    if n < k + 1:                                 # refused by name, nothing else
        st, _, _ = dev_knn(c.P, k)
        assert refused(st, b"fewer than k")
        return
    so, to = oracle_knn(name, k)
    if c.ties:
        assert has_tie_at_k(c.P, k)
    st, s, t = dev_knn(c.P, k)
    assert st == _lib.OK, _lib.load().ngpde_last_error()
    assert np.array_equal(t, to) and np.array_equal(s, so)


@pytest.mark.parametrize("batched", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_spatial_order_matches_brute_force(name, batched):
    c = case(name)
    n = c.P.shape[1]
    gi = np.random.default_rng(n).integers(1, 4, n).astype(np.int32) if batched else None
    with np.errstate(all="ignore"):
        want = O.spatial_order(c.P, gi, id_base=1)
    assert np.array_equal(np.sort(want), np.arange(n))
    st, got = dev_order(c.P, gi, 3 if batched else 1, 1)
    assert st == _lib.OK, _lib.load().ngpde_last_error()
    assert np.array_equal(got, want)


# ---- the ring walk ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 6, 33])
def test_knn_ring_walk_crosses_every_empty_ring(k):
    """k points near the origin and one more than a hundred cells away in a thin box: the lone point's walk (and every other point's:
    with k + 1 points all the others are neighbours) passes every ring up to the last before it has k candidates."""
    rng = np.random.default_rng(50 + k)
    P = (rng.random((2, k + 1)) * np.array([[1e-3], [1e-4]])).astype(F)
    P[:, 0] = 0.0
    P[:, k] = (1.0, 1e-4)
    g = grid_np(P, knn_want(P, k))
    c = cells_of(P, g)
    assert g.steps == 0 and g.nc[0] >= 100 and np.all(c[0, :k] == 0) and c[0, k] == g.nc[0] - 1     # max_ring = nc[0] - 1, all of them empty
    with np.errstate(all="ignore"):
        so, to = O.knn_graph(P, k)
    st, s, t = dev_knn(P, k)
    assert st == _lib.OK, _lib.load().ngpde_last_error()
    assert np.array_equal(t, to) and np.array_equal(s, so)
    assert set(s[t == k].tolist()) == set(range(k))


# ---- magnitudes the library refuses -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wide", ["last", "all"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_span_above_the_float_range_is_refused_by_name(dim, wide):
    """finite coordinates whose hi - lo is inf, in the last coordinate or in all of them (with two such coordinates the grid sizing
    used to coarsen for ever): refused before the grid is sized"""
    P = np.random.default_rng(dim).random((dim, 50)).astype(F)
    for d in range(dim - 1 if wide == "last" else 0, dim):
        P[d, 3], P[d, 17] = -3e38, 3e38
    with np.errstate(all="ignore"):
        assert np.all(np.isfinite(P)) and np.isinf(P.max(axis=1) - P.min(axis=1)).sum() == (1 if wide == "last" else dim)
    st, _, _ = dev_radius(P, 1.0)
    assert refused(st, b"span")
    st, _, _ = dev_knn(P, 3)
    assert refused(st, b"span")
    st, _ = dev_order(P)
    assert refused(st, b"span")


# ---- batches ----------------------------------------------------------------------------------------------------------------------
def far_members(k):
    """three graphs of k + 1, 500 and 7 points in unit boxes 1e3 apart"""
    rng = np.random.default_rng(70 + k)
    sizes = (k + 1, 500, 7)
    at = np.array([[0.0, 1e3, 2e3], [0.0, 1e3, 0.0]])
    P = np.concatenate([rng.random((2, m)) + at[:, [j]] for j, m in enumerate(sizes)], axis=1).astype(F)
    gi = np.repeat(np.arange(3), sizes).astype(np.int32)
    return P, gi, sizes


@pytest.mark.parametrize("index_base", [0, 1])
@pytest.mark.parametrize("id_base", [0, 1])
@pytest.mark.parametrize("k", [1, 6])
def test_batch_of_far_members(k, id_base, index_base):
    P, gi, sizes = far_members(k)
    n = P.shape[1]
    g = grid_np(P, knn_want(P, k, 3), 3)
    c = cells_of(P, g)
    occupied = np.unique(c[0] * g.nc[1] + c[1]).size
    assert g.cells >= 16 and occupied * 4 <= g.cells             # the global box is mostly empty cells
    with np.errstate(all="ignore"):
        so, to = O.knn_graph(P, k, graph_indicator=gi)
        parts = [O.knn_graph(P[:, gi == j], k) for j in range(3)]
    off = np.cumsum((0,) + sizes)
    assert np.array_equal(so, np.concatenate([p[0] + off[j] for j, p in enumerate(parts)]))   # the members searched alone, offset
    st, s, t = dev_knn(P, k, gi + id_base, 3, id_base, index_base=index_base)
    assert st == _lib.OK, _lib.load().ngpde_last_error()
    assert np.array_equal(t, to + index_base) and np.array_equal(s, so + index_base)
    r = 0.06
    with np.errstate(all="ignore"):
        so, to = O.radius_graph(P, r, graph_indicator=gi)
    assert so.size >= n // 2
    st, s, t = dev_radius(P, r, gi + id_base, 3, id_base, index_base=index_base)
    assert st == _lib.OK, _lib.load().ngpde_last_error()
    assert np.array_equal(t, to + index_base) and np.array_equal(s, so + index_base)


def test_batch_with_a_member_too_small_is_refused_by_name():
    P, gi, _ = far_members(6)                                     # graph three has 7 points: k = 7 needs 8
    st, _, _ = dev_knn(P, 7, gi, 3, 0)
    assert refused(st, b"fewer than k")
    st, s, t = dev_knn(P, 7, gi, 3, 0, self_loops=True)           # with self loops 7 points are enough
    with np.errstate(all="ignore"):
        so, to = O.knn_graph(P, 7, graph_indicator=gi, self_loops=True)
    assert st == _lib.OK and np.array_equal(s, so) and np.array_equal(t, to)


@pytest.mark.parametrize("index_base", [0, 1])
@pytest.mark.parametrize("id_base", [0, 1])
def test_batch_of_interleaved_members_with_unsorted_ids(id_base, index_base):
    rng = np.random.default_rng(81)
    n = 600
    P = rng.random((2, n)).astype(F)
    gi = rng.integers(0, 4, n).astype(np.int32)
    assert np.any(np.diff(gi) < 0) and np.bincount(gi).min() >= 100
    with np.errstate(all="ignore"):
        so, to = O.radius_graph(P, 0.08, graph_indicator=gi)
        ko, kt = O.knn_graph(P, 6, graph_indicator=gi)
        oo = O.spatial_order(P, gi + id_base, id_base=id_base)
    assert so.size >= n // 2 and np.array_equal(gi[so], gi[to])
    st, s, t = dev_radius(P, 0.08, gi + id_base, 4, id_base, index_base=index_base)
    assert st == _lib.OK and np.array_equal(t, to + index_base) and np.array_equal(s, so + index_base)
    st, s, t = dev_knn(P, 6, gi + id_base, 4, id_base, index_base=index_base)
    assert st == _lib.OK and np.array_equal(t, kt + index_base) and np.array_equal(s, ko + index_base)
    st, got = dev_order(P, gi + id_base, 4, id_base)
    assert st == _lib.OK and np.array_equal(got, oo)


# ---- direction, the largest k -----------------------------------------------------------------------------------------------------
def test_dir_out_is_the_swap_of_dir_in():
    c = case("lattice_shifted")
    so, to = oracle_radius("lattice_shifted", False)
    st, s, t = dev_radius(c.P, c.r, dir_out=1)
    assert st == _lib.OK and np.array_equal(s, to) and np.array_equal(t, so)
    ko, kt = oracle_knn("duplicates", 6)
    st, s, t = dev_knn(case("duplicates").P, 6, dir_out=1)
    assert st == _lib.OK and np.array_equal(s, kt) and np.array_equal(t, ko)


@pytest.mark.parametrize("which", ["clustered_3d", "duplicates"])
def test_knn_at_the_largest_k(which):
    """k = NGPDE_KNN_MAX_K = 128: the running lists fill the 64 KiB of LDS"""
    if which == "duplicates":
        P = case("duplicates").P
        assert has_tie_at_k(P, 128)
    else:
        rng = np.random.default_rng(90)
        centres = rng.random((3, 5))
        P = (centres[:, rng.integers(0, 5, 200)] + 0.01 * rng.standard_normal((3, 200))).astype(F)
    with np.errstate(all="ignore"):
        so, to = O.knn_graph(P, 128)
    st, s, t = dev_knn(P, 128)
    assert st == _lib.OK, _lib.load().ngpde_last_error()
    assert np.array_equal(t, to) and np.array_equal(s, so)
