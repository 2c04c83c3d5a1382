"""GPU tests of the graph matrices (matrices.py over csrc/graph_matrix.hip; src/NeuralGraphPDE.jl:4 of the reference re-exports
adjacency_matrix, laplacian_matrix, normalized_laplacian, scaled_laplacian, laplacian_lambda_max, khop_adj and has_isolated_nodes from
GNNGraphs).

Every reference is a numpy float64 restatement written here.  Structure and order are compared exactly.  Values are compared under
bounds derived where they are made, all in units of u2 = 2^-23 (twice the float32 unit roundoff, which covers the second-order terms):
a float32 sum of m terms taken in any fixed order is within (m - 1) * u2 * sum |terms| of the exact sum, a product or quotient within
u2 * |result|.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
U2 = 2.0 ** -23

SIZES = [(n, e) for n in (1, 2, 300) for e in (0, 1, 255, 256, 257, 1000)] + [(100003, 1000)]          # the last: row * n + col needs 64 bits


# ---- graphs ---------------------------------------------------------------------------------------------------------------------

def random_edges(n, e, seed):
    """e random ends with duplicates (the first eighth repeated at the end) and self loops (every seventh edge)"""
    rng = np.random.default_rng(seed)
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    k = e // 8
    if k:
        s[-k:], t[-k:] = s[:k], t[:k]
    t[::7] = s[::7]
    return s.astype(np.int64), t.astype(np.int64)


def weights(e, seed, signed=False):
    rng = np.random.default_rng(seed + 1000)
    w = (0.5 + rng.random(e)).astype(np.float32)
    if signed:                                       # +-[0.25, 1.75)
        w = ((0.25 + 1.5 * rng.random(e)) * rng.choice([-1.0, 1.0], e)).astype(np.float32)
    return w


def graph(n, s, t, w=None, **kw):
    return ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=None if w is None else torch.as_tensor(w, device=DEV), **kw)


def host(x):
    return x.detach().cpu().numpy()


# ---- the float64 restatement ----------------------------------------------------------------------------------------------------

def ref_matrix(kind, n, s, t, w, dir="out", add_self_loops=False, lam=None, graph_of=None):
    """(rows, cols, values, bound) of the matrix, entries sorted by (row, col); values float64, bound = the float32 rounding bound per
    entry.  kind: "adj" | "lap" | "norm"; lam (per graph) selects the scaled form of "norm"."""
    e = len(s)
    w = np.ones(e) if w is None else w.astype(np.float64)
    r, c = (s, t) if dir == "out" else (t, s)
    key, wv, one = r * n + c, w, np.ones(e)
    if kind != "adj":
        key = np.concatenate([key, np.arange(n, dtype=np.int64) * (n + 1)])
        wv, one = np.concatenate([w, np.zeros(n)]), np.concatenate([one, np.zeros(n)])
    uk, inv = np.unique(key, return_inverse=True)
    rows, cols = uk // n, uk % n
    a = np.bincount(inv, wv, len(uk))
    ab = np.bincount(inv, np.abs(wv), len(uk))
    m = np.bincount(inv, one, len(uk))
    e_a = np.maximum(m - 1, 0) * U2 * ab                     # the entry's m weights added in COO order
    if kind == "adj":
        return rows, cols, a, e_a
    diag = rows == cols
    if add_self_loops:
        e_a = e_a + diag * U2 * (np.abs(a) + 1.0)            # ... and the loop's 1 last
        a, ab = a + diag, ab + diag
    d = np.bincount(rows, a, n)
    rlen = np.bincount(rows, minlength=n)
    # a row sum: its r entries front to back, each with its own error
    e_d = np.bincount(rows, e_a, n) + np.maximum(rlen - 1, 0) * U2 * np.bincount(rows, ab, n)
    if kind == "lap":
        vals = np.where(diag, d[rows] - a, -a)
        bound = np.where(diag, e_d[rows] + e_a + U2 * (np.abs(d[rows]) + np.abs(a)), e_a)   # d - a: both errors and the subtraction
        return rows, cols, vals, bound
    with np.errstate(divide="ignore", invalid="ignore"):
        ci = 1.0 / np.sqrt(d)
        rel_c = 0.5 * e_d / np.abs(d) + 2 * U2               # c = 1 / sqrt(d): half the relative error of d, a root and a quotient
        p = ci[rows] * a * ci[cols]
        vals = diag - p
        # (c_i a) c_j: the relative errors of the three factors and two products; then the subtraction from (i == j)
        bound = np.abs(p) * (rel_c[rows] + rel_c[cols] + 2 * U2) + e_a * ci[rows] * ci[cols] + U2 * np.abs(vals)
        if lam is not None:
            sc = 2.0 / np.asarray(lam, dtype=np.float64)[graph_of[rows] if graph_of is not None else np.zeros(len(rows), np.int64)]
            scaled = sc * vals - diag
            bound = sc * bound + 3 * U2 * (np.abs(sc * vals) + np.abs(scaled))          # 2 / lam, the product, the subtraction
            vals = scaled
    return rows, cols, vals, bound


def row_sums_ok(n, s, t, w, dir, add_self_loops):
    d = np.bincount(s if dir == "out" else t, np.ones(len(s)) if w is None else w.astype(np.float64), n) + (1.0 if add_self_loops else 0.0)
    return bool(np.all(d > 0))


def dense(n, rows, cols, vals):
    out = np.zeros((n, n))
    out[rows, cols] = vals
    return out


def check_matrix(m, ref, exact=False):
    rows, cols, vals, bound = ref
    assert m.nnz == len(rows) and m.rows.dtype == torch.int32 and m.cols.dtype == torch.int32 and m.values.dtype == torch.float32
    assert np.array_equal(host(m.rows), rows) and np.array_equal(host(m.cols), cols)          # structure AND order, exactly
    rp = host(m.row_ptr)
    assert np.array_equal(rp, np.searchsorted(rows, np.arange(m.shape[0] + 1)))
    got = host(m.values).astype(np.float64)
    if exact:
        assert np.array_equal(got, vals)
    else:
        err = np.abs(got - vals)
        assert np.all(err <= bound), (float(err.max()), float((err - bound).max()))


# ---- assembly -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dir", ["out", "in"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n,e", SIZES)
def test_assembly(n, e, weighted, dir):
    s, t = random_edges(n, e, seed=n + e)
    w = weights(e, seed=e) if weighted else None
    g = graph(n, s, t, w)
    a = ng.adjacency_matrix(g, dir=dir)
    check_matrix(a, ref_matrix("adj", n, s, t, w, dir), exact=not weighted)          # multiplicities are exact
    check_matrix(ng.adjacency_matrix(g, dir=dir, weighted=False), ref_matrix("adj", n, s, t, None, dir), exact=True)
    lap = ng.laplacian_matrix(g, dir=dir)
    check_matrix(lap, ref_matrix("lap", n, s, t, w, dir))
    assert np.array_equal(host(lap.rows)[host(lap.rows) == host(lap.cols)], np.arange(n))          # every diagonal position is stored
    for loops in (True, False):
        if row_sums_ok(n, s, t, w, dir, loops):
            check_matrix(ng.normalized_laplacian(g, add_self_loops=loops, dir=dir), ref_matrix("norm", n, s, t, w, dir, loops))
        else:
            with pytest.raises(ng.ArgumentError, match="row sum"):
                ng.normalized_laplacian(g, add_self_loops=loops, dir=dir)
    assert ng.has_isolated_nodes(g, dir=dir) == bool(np.any(np.bincount(s if dir == "out" else t, minlength=n) == 0))
    if n <= 300:
        assert np.array_equal(host(a.to_dense()).astype(np.float64)[host(a.rows), host(a.cols)], host(a.values).astype(np.float64))
        assert a.to_dense().shape == (n, n) and int((a.to_dense() != 0).sum()) <= a.nnz
    # the same call twice gives the same bits
    for f in (lambda: ng.adjacency_matrix(g, dir=dir), lambda: ng.laplacian_matrix(g, dir=dir),
              lambda: ng.normalized_laplacian(g, add_self_loops=True, dir=dir)):
        x, y = f(), f()
        assert torch.equal(x.rows, y.rows) and torch.equal(x.cols, y.cols) and torch.equal(x.values, y.values)


def batch_of_three():
    parts, ss, tt, off = [(7, 20, 1), (40, 150, 2), (13, 30, 3)], [], [], 0
    for n, e, seed in parts:
        s, t = random_edges(n, e, seed)
        ss.append(s + off)
        tt.append(t + off)
        off += n
    gi = np.repeat(np.arange(3), [p[0] for p in parts])
    return off, np.concatenate(ss), np.concatenate(tt), gi


@pytest.mark.parametrize("dir", ["out", "in"])
def test_assembly_batch_of_three_unequal_graphs(dir):
    n, s, t, gi = batch_of_three()
    w = weights(len(s), seed=5)
    g = graph(n, s, t, w, graph_indicator=gi)
    check_matrix(ng.adjacency_matrix(g, dir=dir), ref_matrix("adj", n, s, t, w, dir))
    check_matrix(ng.laplacian_matrix(g, dir=dir), ref_matrix("lap", n, s, t, w, dir))
    check_matrix(ng.normalized_laplacian(g, add_self_loops=True, dir=dir), ref_matrix("norm", n, s, t, w, dir, True))
    # the scaled form: every block by its own graph's lambda_max (self loops make every row sum positive here)
    gl = ng.add_self_loops(g)
    sl, tl = np.concatenate([s, np.arange(n)]), np.concatenate([t, np.arange(n)])
    wl = np.concatenate([w, np.ones(n, np.float32)])
    lam = np.array([1.25, 2.0, 1.5], np.float32)
    m = ng.scaled_laplacian(gl, dir=dir, lambda_max=lam)
    check_matrix(m, ref_matrix("norm", n, sl, tl, wl, dir, False, lam=lam, graph_of=gi))
    assert m.as_graph().num_graphs == 3 and np.array_equal(m.as_graph().graph_indicator, gi)


def test_isolated_node():
    s, t = np.array([0, 1, 1, 3]), np.array([1, 0, 3, 1])          # node 2 has no edge; node 4 only a self loop
    s, t = np.concatenate([s, [4]]), np.concatenate([t, [4]])
    g = graph(5, s, t)
    lap = ng.laplacian_matrix(g)
    check_matrix(lap, ref_matrix("lap", 5, s, t, None))
    d = dense(5, host(lap.rows), host(lap.cols), host(lap.values))
    at = {(int(r), int(c)) for r, c in zip(host(lap.rows), host(lap.cols))}
    assert (2, 2) in at and (4, 4) in at and d[2, 2] == 0.0 and d[4, 4] == 0.0          # stored zeros
    with pytest.raises(ng.ArgumentError, match="node 2"):
        ng.normalized_laplacian(g)
    check_matrix(ng.normalized_laplacian(g, add_self_loops=True), ref_matrix("norm", 5, s, t, None, "out", True))
    assert ng.has_isolated_nodes(g) and ng.has_isolated_nodes(g, dir="in")
    assert not ng.has_isolated_nodes(graph(2, np.array([0, 1]), np.array([1, 0])))
    assert ng.has_isolated_nodes(graph(2, np.array([0]), np.array([1]))) and ng.has_isolated_nodes(graph(2, np.array([0]), np.array([1])), dir="in")


# ---- apply ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D", [1, 3, 64])
def test_apply(D):
    n, e = 300, 1000
    s, t = random_edges(n, e, seed=11)
    w = weights(e, seed=12, signed=True)
    g = graph(n, s, t, w)
    m = ng.laplacian_matrix(g)
    rows, cols, vals = host(m.rows), host(m.cols), host(m.values).astype(np.float64)
    M = dense(n, rows, cols, vals)                                  # the float32 matrix the device holds, in float64
    rlen, clen = np.bincount(rows, minlength=n).max(), np.bincount(cols, minlength=n).max()
    X = torch.randn(D, n, device=DEV, requires_grad=True)
    R = torch.randn(D, n, device=DEV)
    X64, R64 = host(X).astype(np.float64), host(R).astype(np.float64)
    y = m.matmul(X)
    ref, scale = X64 @ M.T, np.abs(X64) @ np.abs(M).T
    assert y.shape == (D, n)
    assert np.all(np.abs(host(y) - ref) <= rlen * U2 * scale)      # a row of r products added in a fixed order
    y2 = ng.propagate(ng.w_mul_xj, m.as_graph(), "+", xj=X.detach())
    assert np.all(np.abs(host(y2) - ref) <= rlen * U2 * scale)
    assert m.as_graph() is m.as_graph()
    (y * R).sum().backward()
    assert np.all(np.abs(host(X.grad) - R64 @ M) <= clen * U2 * (np.abs(R64) @ np.abs(M)))          # the transpose product
    # ... and the values: dM[i, j] = sum_d R[d, i] X[d, j]
    mv = ng.GraphMatrix(n, m.rows, m.cols, m.values.detach().clone().requires_grad_(True), m.row_ptr)
    (mv.matmul(X.detach()) * R).sum().backward()
    assert np.all(np.abs(host(mv.values.grad) - (R64[:, rows] * X64[:, cols]).sum(0)) <= D * U2 * (np.abs(R64[:, rows]) * np.abs(X64[:, cols])).sum(0))


# ---- gradients ------------------------------------------------------------------------------------------------------------------

def dense64(kind, n, s, t, w, dir, loops, lam):
    """the dense float64 restatement in torch, differentiable in w"""
    r, c = (s, t) if dir == "out" else (t, s)
    a = torch.zeros(n * n, dtype=torch.float64).index_add(0, torch.as_tensor(r * n + c), w).reshape(n, n)
    eye = torch.eye(n, dtype=torch.float64)
    if kind == "adj":
        return a
    if kind == "lap":
        return torch.diag(a.sum(1)) - a
    a = a + eye if loops else a
    c = a.sum(1).rsqrt()
    l = eye - c[:, None] * a * c[None, :]
    return l if kind == "norm" else 2.0 / lam * l - eye


@pytest.mark.parametrize("dir", ["out", "in"])
@pytest.mark.parametrize("kind,loops", [("adj", False), ("lap", False), ("norm", False), ("norm", True), ("scaled", False)])
def test_gradients(kind, loops, dir):
    n = 40
    s, t = random_edges(n, 160, seed=21)
    s, t = np.concatenate([s, np.arange(n)]), np.concatenate([t, (np.arange(n) + 1) % n])          # a ring: no zero row sum in either dir
    w0 = weights(len(s), seed=22)
    lam = 1.75
    fn = {"adj": lambda g: ng.adjacency_matrix(g, dir=dir), "lap": lambda g: ng.laplacian_matrix(g, dir=dir),
          "norm": lambda g: ng.normalized_laplacian(g, add_self_loops=loops, dir=dir),
          "scaled": lambda g: ng.scaled_laplacian(g, dir=dir, lambda_max=lam)}[kind]
    grads = []
    for _ in range(2):
        w = torch.as_tensor(w0, device=DEV).requires_grad_(True)
        m = fn(ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=w))
        assert m.values.requires_grad
        if not grads:
            R = torch.randn(m.nnz, device=DEV)
        (m.values * R).sum().backward()
        grads.append(w.grad.clone())
    assert torch.equal(grads[0], grads[1])                          # the backward run twice gives the same bits
    rows, cols = host(m.rows), host(m.cols)
    R64 = torch.as_tensor(host(R).astype(np.float64))
    w64 = torch.as_tensor(w0.astype(np.float64)).requires_grad_(True)
    (dense64(kind, n, s, t, w64, dir, loops, lam)[rows, cols] * R64).sum().backward()
    ref = w64.grad.numpy()
    # The tolerance: one gradient entry is a sum over a row and a column of the matrix (at most 2 * rmax terms, each a product of a
    # handful of rounded factors: 16 covers them).  `mag` restates that sum with every term's magnitude, so that
    # (2 * rmax + 16) * u2 * |mag|_inf bounds its rounding; relative to |grad|_inf the factor is (2 * rmax + 16) * |mag|_inf / |grad|_inf.
    rmax = max(np.bincount(rows, minlength=n).max(), np.bincount(cols, minlength=n).max())
    absR = np.abs(R64.numpy())
    if kind == "adj":
        mag = absR
    elif kind == "lap":
        mag = absR + absR[np.flatnonzero(rows == cols)][rows]
    else:
        at = ref_matrix("adj", n, np.concatenate([s, np.arange(n)]), np.concatenate([t, np.arange(n)]),
                        np.concatenate([w0, np.full(n, 1.0 if loops else 0.0, np.float32)]), dir)[2]          # a~ on the matrix's structure
        d = np.bincount(rows, at, n)
        q = (2.0 / lam if kind == "scaled" else 1.0) * absR / np.sqrt(d[rows] * d[cols])
        mag = q + 0.5 / d[rows] * (np.bincount(rows, q * at, n) + np.bincount(cols, q * at, n))[rows]
    tol = (2 * rmax + 16) * U2 * mag.max()
    err = np.abs(host(grads[0]).astype(np.float64) - ref).max()
    assert np.abs(ref).max() > 0 and err <= tol, (err, tol, float(np.abs(ref).max()))


# ---- khop_adj -------------------------------------------------------------------------------------------------------------------

def hub_graph():
    n = 120
    s, t = random_edges(n, 600, seed=31)
    rng = np.random.default_rng(32)
    s = np.concatenate([s, np.zeros(100, np.int64), rng.integers(0, n, 100)])          # node 0: 100 more out-edges and 100 more in-edges
    t = np.concatenate([t, rng.integers(0, n, 100), np.zeros(100, np.int64)])
    return n, s, t


def khop_reference(n, s, t, w, k, dir):
    r, c, a, _ = ref_matrix("adj", n, s, t, w, dir)
    A = dense(n, r, c, a)
    B = (dense(n, r, c, np.ones(len(r))) != 0).astype(np.int64)
    P, absP, S, m_max = A, np.abs(A), B, 1
    for _ in range(k - 1):
        terms = S @ B                                               # the number of terms added into every entry of this product
        m_max = max(m_max, int(terms.max()))
        P, absP, S = P @ A, absP @ np.abs(A), (terms > 0).astype(np.int64)
    return P, absP, S, m_max


@pytest.mark.parametrize("dir", ["out", "in"])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("family", ["n40", "hub"])
def test_khop_adj(family, k, dir):
    n, s, t = (40,) + random_edges(40, 150, seed=33) if family == "n40" else hub_graph()
    w = weights(len(s), seed=34, signed=True)
    g = graph(n, s, t, w)
    m = ng.khop_adj(g, k, dir=dir)
    P, absP, S, m_max = khop_reference(n, s, t, w, k, dir)
    rows, cols = np.nonzero(S)                                      # (row-major: sorted by row, then column)
    assert np.array_equal(host(m.rows), rows) and np.array_equal(host(m.cols), cols)          # the boolean power, exactly
    assert np.array_equal(host(m.row_ptr), np.searchsorted(rows, np.arange(n + 1)))
    err = np.abs(host(m.values).astype(np.float64) - P[rows, cols])
    assert np.all(err <= k * (m_max + 2) * U2 * absP[rows, cols]), float((err / np.maximum(absP[rows, cols], 1e-300)).max() / U2)
    assert not m.values.requires_grad
    m2 = ng.khop_adj(g, k, dir=dir)
    assert torch.equal(m.rows, m2.rows) and torch.equal(m.cols, m2.cols) and torch.equal(m.values, m2.values)
    if k == 1:
        a = ng.adjacency_matrix(g, dir=dir)
        assert torch.equal(m.rows, a.rows) and torch.equal(m.cols, a.cols) and torch.equal(m.values, a.values)          # bitwise
    mu = ng.khop_adj(g, k, dir=dir, weighted=False)                 # path counts: exact
    assert np.array_equal(host(mu.values).astype(np.int64), np.linalg.matrix_power((dense(n, *ref_matrix("adj", n, s, t, None, dir)[:3])).astype(np.int64), k)[rows, cols])


def test_khop_adj_rows_without_entries_cancellation_and_no_gradient():
    s, t = np.array([0, 0, 1, 2, 5]), np.array([1, 2, 3, 3, 5])          # 0 -> {1, 2} -> 3; nodes 3, 4 have no out-edge
    w = np.array([1.0, 1.0, 1.0, -1.0, 2.0], np.float32)
    wt = torch.as_tensor(w, device=DEV).requires_grad_(True)
    m = ng.khop_adj(ng.GNNGraph(s, t, num_nodes=6, index_base=0, edge_weight=wt), 2)
    assert host(m.rows).tolist() == [0, 5] and host(m.cols).tolist() == [3, 5]
    assert host(m.values).tolist() == [0.0, 4.0]                    # 1 * 1 + 1 * -1 cancels to 0.0 and stays an entry
    assert host(m.row_ptr).tolist() == [0, 1, 1, 1, 1, 1, 2]
    assert not m.values.requires_grad and not ng.khop_adj(ng.GNNGraph(s, t, num_nodes=6, index_base=0, edge_weight=wt), 1).values.requires_grad
    m3 = ng.khop_adj(graph(6, s, t, w), 3)
    assert host(m3.rows).tolist() == [5] and host(m3.values).tolist() == [8.0]
    empty = ng.khop_adj(graph(4, np.array([0]), np.array([1])), 2)
    assert empty.nnz == 0 and host(empty.row_ptr).tolist() == [0] * 5


def test_khop_adj_64_bit_keys():
    n, e = 100003, 1000
    s, t = random_edges(n, e, seed=35)
    t[:400] = s[200:600]                                            # chain some edges so that two-hop paths exist
    w = weights(e, seed=36, signed=True)
    m = ng.khop_adj(graph(n, s, t, w), 2)
    r, c, a, _ = ref_matrix("adj", n, s, t, w)
    by_row = {}
    for i, j, v in zip(r.tolist(), c.tolist(), a.tolist()):
        by_row.setdefault(i, []).append((j, v))
    val, mag, cnt = {}, {}, {}
    for i, j, v in zip(r.tolist(), c.tolist(), a.tolist()):
        for c2, v2 in by_row.get(j, ()):
            key = i * n + c2
            val[key], mag[key], cnt[key] = val.get(key, 0.0) + v * v2, mag.get(key, 0.0) + abs(v * v2), cnt.get(key, 0) + 1
    keys = np.array(sorted(val), dtype=np.int64)
    assert len(keys) > 100 and keys.max() > 2 ** 32
    assert np.array_equal(host(m.rows).astype(np.int64) * n + host(m.cols), keys)
    err = np.abs(host(m.values).astype(np.float64) - np.array([val[k] for k in keys.tolist()]))
    assert np.all(err <= 2 * (max(cnt.values()) + 2) * U2 * np.array([mag[k] for k in keys.tolist()]))


def test_spgemm_refuses_a_product_too_dense_to_expand():
    n = 8
    s, t = np.nonzero(1 - np.eye(n, dtype=np.int64))               # the complete graph: 56 entries, every row 7 long: 392 terms
    a = ng.adjacency_matrix(graph(n, s, t))
    lib = _lib.load()
    total = C.c_int64(-1)
    args = (n, a.nnz, _lib.ptr(a.cols), a.nnz, _lib.ptr(a.row_ptr))
    st = lib.ngpde_csr_spgemm_count(*args, 391, None, C.byref(total), _lib.current_stream())
    assert st == _lib.ERR_INVALID_ARGUMENT and total.value == 0
    assert b"too dense" in lib.ngpde_last_error() and b"392" in lib.ngpde_last_error()
    off = torch.empty(a.nnz + 1, dtype=torch.int64, device=DEV)
    assert lib.ngpde_csr_spgemm_count(*args, 392, _lib.ptr(off), C.byref(total), _lib.current_stream()) == 0 and total.value == 392
    assert host(off).tolist() == list(range(0, 393, 7))
    # the product takes those offsets; ones that do not fit the matrices are refused by the expanding launch, nothing is read through them
    rows, cols = (torch.empty(392, dtype=torch.int32, device=DEV) for _ in range(2))
    vals, row_ptr, nnz = torch.empty(392, device=DEV), torch.empty(n + 1, dtype=torch.int32, device=DEV), C.c_int64(-1)

    def product(offsets, count):
        return lib.ngpde_csr_spgemm(n, a.nnz, _lib.ptr(a.rows), _lib.ptr(a.cols), _lib.ptr(a.values), a.nnz, _lib.ptr(a.row_ptr), _lib.ptr(a.cols),
                                    _lib.ptr(a.values), _lib.ptr(offsets), count, _lib.ptr(rows), _lib.ptr(cols), _lib.ptr(vals), _lib.ptr(row_ptr),
                                    C.byref(nnz), _lib.current_stream())

    assert product(off, 392) == 0 and nnz.value == n * n and np.array_equal(host(vals)[:n * n].reshape(n, n), 6 + np.eye(n))
    for wrong, count in ((off * 2, 392), (off, 385), (off // 2, 392)):
        assert product(wrong.contiguous(), count) == _lib.ERR_INVALID_ARGUMENT and nnz.value == 0 and b"offsets" in lib.ngpde_last_error()
    m = ng.khop_adj(graph(n, s, t), 2)
    assert m.nnz == n * n and np.array_equal(host(m.values).reshape(n, n), 6 + np.eye(n))          # n - 2 two-hop paths, n - 1 round trips


# ---- lambda_max -----------------------------------------------------------------------------------------------------------------

def bidirected(n, a, b, wpair=None):
    s, t = np.concatenate([a, b]), np.concatenate([b, a])
    return n, s.astype(np.int64), t.astype(np.int64), None if wpair is None else np.concatenate([wpair, wpair])


def ring(n):
    return bidirected(n, np.arange(n), (np.arange(n) + 1) % n)


def grid(k):
    idx = np.arange(k * k).reshape(k, k)
    return bidirected(k * k, np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]), np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]))


def random_over_ring(n, pairs, seed, weighted):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, pairs), rng.integers(0, n, pairs)
    keep = a != b
    a, b = np.concatenate([np.arange(n), a[keep]]), np.concatenate([(np.arange(n) + 1) % n, b[keep]])
    return bidirected(n, a, b, (0.5 + rng.random(len(a))).astype(np.float32) if weighted else None)


FAMILIES = {
    "pair": lambda: bidirected(2, np.array([0]), np.array([1])),
    "ring300": lambda: ring(300), "ring301": lambda: ring(301), "grid20": lambda: grid(20),
    "rand64": lambda: random_over_ring(64, 200, 41, False), "rand300": lambda: random_over_ring(300, 1200, 42, False),
    "rand1000": lambda: random_over_ring(1000, 4000, 43, False),
    "rand64w": lambda: random_over_ring(64, 200, 44, True), "rand300w": lambda: random_over_ring(300, 1200, 45, True),
    "rand1000w": lambda: random_over_ring(1000, 4000, 46, True),
}


def lambda_reference(n, s, t, w, loops):
    rows, cols, vals, _ = ref_matrix("norm", n, s, t, w, "out", loops)
    L = dense(n, rows, cols, vals)
    return float(np.linalg.eigvalsh(L)[-1]), L, int(np.bincount(rows, minlength=n).max())


def check_lambda(value, residual, iterations, vector, ref, L, dmax, size, max_iter=64):
    slack = (dmax + 16) * U2 * ref
    print(f"value {value:.9g} ref {ref:.9g} residual {residual:.3g} iterations {iterations} slack {slack:.3g}")
    # a Ritz value never exceeds lambda_max beyond rounding, and an eigenvalue lies within `residual` of it
    assert ref - residual - slack <= value <= ref + slack
    y = vector.astype(np.float64)
    assert abs(np.linalg.norm(y) - 1.0) <= 16 * U2
    assert abs(residual - np.linalg.norm(L @ y - value * y)) <= slack
    assert residual <= 0.01 * ref                                   # so that a wide residual cannot hide a wrong value
    assert 1 <= iterations <= min(max_iter, size)


@pytest.mark.parametrize("loops", [False, True])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_lambda_max(family, loops):
    n, s, t, w = FAMILIES[family]()
    g = graph(n, s, t, w)
    ref, L, dmax = lambda_reference(n, s, t, w, loops)
    value, info = ng.laplacian_lambda_max(g, add_self_loops=loops, return_info=True)
    assert isinstance(value, float) and isinstance(info.residual, float) and isinstance(info.iterations, int)
    check_lambda(value, info.residual, info.iterations, host(info.vector), ref, L, dmax, n)
    if family == "pair":
        assert info.iterations == 2                                 # the Krylov space ends there: the value is exact
    again, info2 = ng.laplacian_lambda_max(g, add_self_loops=loops, return_info=True)
    assert again == value and info2.residual == info.residual and torch.equal(info2.vector, info.vector)          # the same bits
    assert ng.laplacian_lambda_max(g, add_self_loops=loops) == value


@pytest.mark.parametrize("loops", [False, True])
def test_lambda_max_per_graph_of_a_batch(loops):
    members = [FAMILIES["pair"](), ring(37), FAMILIES["rand64"]()]
    gb = ng.batch([graph(*m) for m in members])
    value, info = ng.laplacian_lambda_max(gb, add_self_loops=loops, return_info=True)
    assert value.shape == (3,) and value.dtype == torch.float32 and info.residual.shape == (3,) and info.iterations.shape == (3,)
    off = 0
    for k, (n, s, t, w) in enumerate(members):
        ref, L, dmax = lambda_reference(n, s, t, w, loops)
        check_lambda(float(value[k]), float(info.residual[k]), int(info.iterations[k]), host(info.vector)[off:off + n], ref, L, dmax, n)
        alone = ng.laplacian_lambda_max(graph(n, s, t, w), add_self_loops=loops)
        assert abs(alone - float(value[k])) <= 2 * (dmax + 16) * U2 * ref          # a member starts as it would alone
        off += n
    again = ng.laplacian_lambda_max(gb, add_self_loops=loops)
    assert torch.equal(again, value)


def test_lambda_max_refuses_what_is_not_symmetric():
    n, s, t, _ = ring(12)
    with pytest.raises(ng.ArgumentError, match=r"not symmetric: entry \(3, 7\)"):
        ng.laplacian_lambda_max(graph(n, np.concatenate([s, [3]]), np.concatenate([t, [7]])))          # a directed edge
    w = np.ones(len(s), np.float32)
    w[5] = np.float32(1.0 + 2.0 ** -20)                              # edge 5 -> 6 heavier than 6 -> 5: single copies must match exactly
    with pytest.raises(ng.ArgumentError, match=r"not symmetric: entry \(5, 6\)"):
        ng.laplacian_lambda_max(graph(n, s, t, w))
    # duplicates added in two orders differ by rounding only: accepted
    s2, t2 = np.concatenate([s, [0, 0, 1, 1]]), np.concatenate([t, [1, 1, 0, 0]])
    w2 = np.concatenate([np.ones(len(s), np.float32), np.float32([1e-4, 3.0, 3.0, 1e-4])])
    assert abs(ng.laplacian_lambda_max(graph(n, s2, t2, w2)) - lambda_reference(n, s2, t2, w2, False)[0]) <= 1e-4
    with pytest.raises(ng.ArgumentError, match="row sum"):
        ng.laplacian_lambda_max(graph(n + 1, s, t))                  # an isolated node
    gi = np.array([0] * 6 + [1] * 6)
    sb, tb = np.concatenate([s[:5], s[6:11]]), np.concatenate([t[:5], t[6:11]])          # two paths of six nodes
    sb, tb = np.concatenate([sb, tb]), np.concatenate([tb, sb])
    assert ng.laplacian_lambda_max(graph(n, sb, tb, graph_indicator=gi)).shape == (2,)
    with pytest.raises(ng.ArgumentError, match="non-decreasing"):
        ng.laplacian_lambda_max(graph(n, sb, tb, graph_indicator=gi[::-1].copy()))


def test_scaled_laplacian_takes_its_scale_from_lambda_max():
    n, s, t, w = FAMILIES["rand300w"]()
    g = graph(n, s, t, w)
    lam = ng.laplacian_lambda_max(g)
    lhat, m = ng.normalized_laplacian(g), ng.scaled_laplacian(g)
    assert torch.equal(m.rows, lhat.rows) and torch.equal(m.cols, lhat.cols)          # bitwise in structure
    eye = (host(m.rows) == host(m.cols)).astype(np.float32)
    scl = (np.float32(2.0) / np.float32(lam)) * host(lhat.values)
    want = scl - eye
    assert np.all(np.abs(host(m.values) - want) <= 2 * np.spacing(np.maximum(np.abs(scl), np.abs(want))))          # 2 ulp
    # lambda_max given: no eigen solve; the launch path by value
    m2 = ng.scaled_laplacian(g, lambda_max=1.5)
    check_matrix(m2, ref_matrix("norm", n, s, t, w, "out", False, lam=np.array([1.5], np.float32)))
    # on a batch every block takes its own graph's value
    members = [FAMILIES["pair"](), ring(37), FAMILIES["rand64"]()]
    gb = ng.batch([graph(*mm) for mm in members])
    lams = host(ng.laplacian_lambda_max(gb))
    nb = sum(mm[0] for mm in members)
    sb = np.concatenate([mm[1] + o for mm, o in zip(members, np.cumsum([0] + [mm[0] for mm in members[:-1]]))])
    tb = np.concatenate([mm[2] + o for mm, o in zip(members, np.cumsum([0] + [mm[0] for mm in members[:-1]]))])
    check_matrix(ng.scaled_laplacian(gb), ref_matrix("norm", nb, sb, tb, None, "out", False, lam=lams, graph_of=np.repeat(np.arange(3), [2, 37, 64])))


def test_lambda_max_entry_checks_its_lists_on_the_device():
    """the C entry alone: laplacian_lambda_max refuses a decreasing graph_indicator on the host, so the device-side checks of
    ngpde_csr_lambda_max (graph ids, their order, the CSR lists) are reached here"""
    n, s, t, _ = ring(12)
    m = ng.normalized_laplacian(graph(n, s, t))
    lib = _lib.load()
    nbytes = lib.ngpde_csr_lambda_max_workspace_bytes(n, 2, 16)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    lam = torch.full((2,), -1.0, device=DEV)

    def call(graph_of, cols=m.cols, row_ptr=m.row_ptr):
        gi = torch.as_tensor(np.asarray(graph_of, np.int32), device=DEV)
        return lib.ngpde_csr_lambda_max(n, m.nnz, _lib.ptr(row_ptr), _lib.ptr(cols), _lib.ptr(m.values), 2, _lib.ptr(gi), 16, 1e-5, 0, _lib.ptr(lam),
                                        None, None, None, _lib.ptr(ws), nbytes, _lib.current_stream())

    assert call([1] * 6 + [0] * 6) == _lib.ERR_INVALID_ARGUMENT and b"non-decreasing" in lib.ngpde_last_error()
    for ids in ([0] * 6 + [2] * 6, [-1] + [0] * 11):
        assert call(ids) == _lib.ERR_INVALID_ARGUMENT and b"outside 0:1" in lib.ngpde_last_error()
    bad_cols = m.cols.clone()
    bad_cols[5] = n
    assert call([0] * 12, cols=bad_cols) == _lib.ERR_DIMENSION_MISMATCH
    bad_ptr = m.row_ptr.clone()
    bad_ptr[3] = m.nnz + 7
    assert call([0] * 12, row_ptr=bad_ptr) == _lib.ERR_DIMENSION_MISMATCH
    assert torch.equal(lam, torch.full((2,), -1.0, device=DEV))          # nothing was computed
    assert call([0] * 12) == 0 and abs(float(lam[0]) - 2.0) <= 1e-5 and float(lam[1]) == 0.0          # the ring alone; graph 1 is empty


def test_lambda_max_of_a_batch_with_an_empty_graph():
    n, s, t, _ = ring(12)
    g = graph(n, s, t, num_graphs=3, graph_indicator=np.array([0] * 12))          # graphs 1 and 2 hold no node
    value, info = ng.laplacian_lambda_max(g, return_info=True)
    assert abs(float(value[0]) - 2.0) <= 1e-5 and host(value)[1:].tolist() == [0.0, 0.0]
    assert host(info.iterations)[1:].tolist() == [0, 0] and host(info.residual)[1:].tolist() == [0.0, 0.0] and 1 <= int(info.iterations[0]) <= 12
