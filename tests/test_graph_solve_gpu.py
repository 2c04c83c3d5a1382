"""GPU tests of the conjugate-gradient solve on graph matrices (linsolve.py over csrc/graph_solve.hip; upstream the same matrix is a
SparseMatrixCSC and `A \\ b` / IterativeSolvers.cg are one line): cg_solve, GraphMatrix.solve, GraphMatrix.diagonal, their pullback and
the C entry ngpde_csr_cg under a HIP-graph capture.

Every reference is float64 numpy (float64 torch autograd on the CPU for the gradients) written here.  The operator of the tests is
A = I + b L with L = laplacian_matrix(g) and b = 9 / lambda_max(L) (numpy), so its spectrum lies in [1, 10]: condition number <= 10,
|A^-1|_2 <= 1 / shift = 1.  A32 is that operator built from the LIBRARY's float32 values cast to float64.  The bounds:

  residual   |b - A32 x|_2 <= 2 rtol |b|_2 per (graph, column): a float32 numpy restatement of Jacobi-CG on these shapes stays within
             0.98 rtol for rtol = 1e-4 and 1e-6 in at most 20 iterations; the factor 2 is the margin for another summation order
  solution   |x - x*|_2 <= |A32^-1|_2 |b - A32 x|_2 <= 2 rtol |b|_2 / shift
  steps      at most 40 per (graph, column); the residual test passes max_iter = 40 (the default, the node count of the largest graph, is
             the exact-arithmetic count: in float32 a 2-node graph can need a third step to reach 1e-6)
"""

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
U2 = 2.0 ** -23
SHIFT = 1.0
DS = (1, 3, 64, 65)


# ---- graphs ---------------------------------------------------------------------------------------------------------------------

def knn_pairs(n, k, seed):
    """the undirected pairs {i, j} of the k nearest neighbours of n random points in the plane"""
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 2))
    pairs = set()
    for i in range(n):
        d = ((pts - pts[i]) ** 2).sum(1)
        d[i] = np.inf
        for j in np.argsort(d, kind="stable")[:min(k, n - 1)]:
            pairs.add((min(i, int(j)), max(i, int(j))))
    return sorted(pairs)


def both_directions(pairs, seed):
    """s, t, w: every pair in both directions with the same float32 weight of [0.5, 1.5)"""
    rng = np.random.default_rng(seed + 500)
    a = np.array([p[0] for p in pairs], dtype=np.int64)
    b = np.array([p[1] for p in pairs], dtype=np.int64)
    w = (0.5 + rng.random(len(pairs))).astype(np.float32)
    return np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([w, w])


def knn_case(n, seed=0):
    return (n,) + both_directions(knn_pairs(n, 6, seed + n), seed + n) + (np.zeros(n, np.int32),)


def hub_case():
    """300 nodes: 6 nearest neighbours among nodes 0 .. 298, node 0 joined to 80 more (a hub of degree > 64), node 299 isolated"""
    pairs = set(knn_pairs(299, 6, 77))
    for j in range(100, 180):
        pairs.add((0, j))
    return (300,) + both_directions(sorted(pairs), 77) + (np.zeros(300, np.int32),)


def batch_case(sizes=(65, 1, 300)):
    ss, ts, ws, gis, off = [], [], [], [], 0
    for k, n in enumerate(sizes):
        _, s, t, w, _ = knn_case(n)
        ss.append(s + off), ts.append(t + off), ws.append(w), gis.append(np.full(n, k, np.int32))
        off += n
    return off, np.concatenate(ss), np.concatenate(ts), np.concatenate(ws), np.concatenate(gis)


CASES = {f"knn{n}": (lambda n=n: knn_case(n)) for n in (1, 2, 63, 64, 65, 257, 300)}
CASES["hub300"] = hub_case
CASES["batch"] = batch_case
_built = {}


def host(x):
    return x.detach().cpu().numpy()


class Problem:
    """a case's graph, its Laplacian on the device, b, A32 and the node ranges of its graphs -- built once, shared, never changed"""

    def __init__(self, name):
        n, s, t, w, gi = CASES[name]()
        self.n, self.s, self.t, self.w, self.gi = n, s, t, w, gi
        kw = dict(graph_indicator=gi) if gi.max(initial=0) > 0 else {}
        self.g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=torch.as_tensor(w, device=DEV), **kw)
        self.M = ng.laplacian_matrix(self.g)
        L32 = host(self.M.to_dense()).astype(np.float64)
        lam = float(np.linalg.eigvalsh(L32).max())
        self.b = float(np.float32(9.0 / lam)) if lam > 0 else 1.0
        self.A32 = SHIFT * np.eye(n) + self.b * L32
        self.blocks = [np.flatnonzero(gi == k) for k in range(int(gi.max(initial=0)) + 1)]

    def rhs(self, D, seed=0):
        return np.random.default_rng(1000 * D + seed).standard_normal((D, self.n)).astype(np.float32)

    def solve(self, B, **kw):
        kw = {"shift": SHIFT, "scale": self.b, **kw}
        return ng.cg_solve(self.M, torch.as_tensor(B, device=DEV), **kw)


def problem(name):
    if name not in _built:
        _built[name] = Problem(name)
    return _built[name]


# ---- 1. residual and solution ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_residual_and_solution_within_twice_rtol(name):
    P = problem(name)
    for D in DS:
        B = P.rhs(D)
        ref = np.linalg.solve(P.A32, B.astype(np.float64).T).T
        for rtol in (1e-4, 1e-6):
            X, info = P.solve(B, rtol=rtol, max_iter=40, return_info=True)
            assert X.shape == (D, P.n) and X.dtype == torch.float32
            x = host(X).astype(np.float64)
            status, its = host(info.status), host(info.iterations)
            assert status.shape == (len(P.blocks), D) and its.shape == status.shape and info.residual.shape == status.shape
            for k, blk in enumerate(P.blocks):
                A = P.A32[np.ix_(blk, blk)]
                for c in range(D):
                    bn = np.linalg.norm(B[c, blk].astype(np.float64))
                    res = np.linalg.norm(B[c, blk] - A @ x[c, blk])
                    err = np.linalg.norm(x[c, blk] - ref[c, blk])
                    print(f"{name} D={D} rtol={rtol:g} graph {k} col {c}: res/|b| {res / max(bn, 1e-300):.3e} err/|b| "
                          f"{err / max(bn, 1e-300):.3e} its {its[k, c]}")
                    assert status[k, c] == 0, (D, rtol, k, c, status[k, c])
                    assert its[k, c] <= 40, (D, rtol, k, c, its[k, c])
                    assert res <= 2 * rtol * bn, (D, rtol, k, c, res, bn)
                    assert err <= 2 * rtol * bn / SHIFT, (D, rtol, k, c, err, bn)
                    assert float(info.residual[k, c]) <= rtol * bn * (1 + 1e-5)          # the stop's own test (float32 norms)


def test_method_and_diagonal():
    P = problem("hub300")
    B = torch.as_tensor(P.rhs(3), device=DEV)
    assert torch.equal(P.M.solve(B, shift=SHIFT, scale=P.b), ng.cg_solve(P.M, B, shift=SHIFT, scale=P.b))
    d = P.M.diagonal()
    assert d.shape == (P.n,) and d.dtype == torch.float32
    assert torch.equal(d, torch.diagonal(P.M.to_dense()))
    adj = ng.adjacency_matrix(P.g)          # no diagonal position is an entry
    assert torch.equal(adj.diagonal(), torch.zeros(P.n, device=DEV))
    w = torch.as_tensor(P.w, device=DEV).requires_grad_(True)
    g = ng.GNNGraph(P.s, P.t, num_nodes=P.n, index_base=0, edge_weight=w)
    r = torch.as_tensor(np.random.default_rng(5).standard_normal(P.n).astype(np.float32), device=DEV)
    (ng.laplacian_matrix(g).diagonal() * r).sum().backward()          # d_ii = the sum of the weights of i's out-edges
    assert torch.equal(w.grad, r[torch.as_tensor(P.s, device=DEV)])


# ---- 2. invariances, all bitwise --------------------------------------------------------------------------------------------------

def test_the_same_call_twice_gives_the_same_bits():
    P = problem("batch")
    B = P.rhs(65)
    X1, i1 = P.solve(B, return_info=True)
    X2, i2 = P.solve(B, return_info=True)
    assert torch.equal(X1, X2) and torch.equal(i1.iterations, i2.iterations) and torch.equal(i1.residual, i2.residual)


@pytest.mark.parametrize("name", ["knn300", "hub300", "batch"])
def test_columns_do_not_depend_on_their_company(name):
    P = problem(name)
    for D, parts in ((5, [slice(c, c + 1) for c in range(5)]), (65, [slice(0, 64), slice(64, 65)])):
        B = P.rhs(D)
        X, info = P.solve(B, rtol=1e-6, return_info=True)
        for sl in parts:
            Xs, infos = P.solve(B[sl], rtol=1e-6, return_info=True)
            assert torch.equal(X[sl], Xs), (D, sl)
            assert torch.equal(info.iterations[:, sl], infos.iterations) and torch.equal(info.residual[:, sl], infos.residual)


def test_the_batch_equals_its_members_solved_alone():
    P = problem("batch")
    for D in (3, 65):
        B = P.rhs(D)
        X, info = P.solve(B, rtol=1e-6, return_info=True)
        for k, (blk, n) in enumerate(zip(P.blocks, (65, 1, 300))):
            _, s, t, w, _ = knn_case(n)
            g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=torch.as_tensor(w, device=DEV))
            Xk, ik = ng.cg_solve(ng.laplacian_matrix(g), torch.as_tensor(np.ascontiguousarray(B[:, blk]), device=DEV), shift=SHIFT, scale=P.b,
                                 rtol=1e-6, return_info=True)
            assert torch.equal(X[:, blk[0]:blk[-1] + 1], Xk), (D, k)
            assert torch.equal(info.iterations[k], ik.iterations[0]) and torch.equal(info.residual[k], ik.residual[0])


@pytest.mark.parametrize("name", ["knn257", "batch"])
def test_check_every_changes_nothing(name):
    P = problem(name)
    B = P.rhs(65)
    X1, i1 = P.solve(B, rtol=1e-6, check_every=1, return_info=True)
    top = int(i1.iterations.max())
    for check_every, max_iter in ((16, None), (0, top), (0, top + 7), (16, top)):
        X, info = P.solve(B, rtol=1e-6, check_every=check_every, max_iter=max_iter, return_info=True)
        assert torch.equal(X, X1), (check_every, max_iter)
        assert torch.equal(info.iterations, i1.iterations) and torch.equal(info.status, i1.status), (check_every, max_iter)


def test_plain_cg_converges_to_the_same_answer():
    P = problem("hub300")
    B = P.rhs(3)
    rtol = 1e-6
    Xj = host(P.solve(B, rtol=rtol, check_every=1)).astype(np.float64)
    Xn, info = P.solve(B, rtol=rtol, check_every=1, precondition=None, return_info=True)
    assert int(info.status.max()) == 0 and int(info.iterations.max()) <= 40
    xn = host(Xn).astype(np.float64)
    for c in range(3):
        bn = np.linalg.norm(B[c].astype(np.float64))
        assert np.linalg.norm(B[c] - P.A32 @ xn[c]) <= 2 * rtol * bn
        assert np.linalg.norm(xn[c] - Xj[c]) <= 4 * rtol * bn / SHIFT          # each within 2 rtol |b| / shift of the one solution


def test_a_start_that_solves_the_system_takes_no_iteration():
    P = problem("batch")
    B = P.rhs(65)
    X1 = P.solve(B, rtol=1e-6)
    X2, info = P.solve(B, rtol=1e-4, x0=X1, return_info=True)
    assert torch.equal(X2, X1) and int(info.iterations.max()) == 0 and int(info.status.max()) == 0
    X3, info3 = P.solve(B, rtol=1e-6, x0=torch.zeros_like(X1), return_info=True)          # x0 = 0 is the default start
    assert torch.equal(X3, X1)


# ---- 3. stops -------------------------------------------------------------------------------------------------------------------

def test_max_iter_is_a_status_not_an_error():
    P = problem("knn300")
    X, info = P.solve(P.rhs(3), rtol=1e-6, max_iter=2, return_info=True)
    assert torch.equal(info.status, torch.ones_like(info.status)) and torch.equal(info.iterations, torch.full_like(info.iterations, 2))
    assert bool(torch.isfinite(X).all())


def test_breakdown_names_graph_and_column():
    P = problem("knn300")
    for check_every in (16, 0):
        with pytest.raises(ng.ArgumentError, match=r"not positive definite: graph 0, column 0"):
            ng.cg_solve(P.M, torch.as_tensor(P.rhs(3), device=DEV), shift=-1.0, scale=0.0, precondition=None, check_every=check_every,
                        max_iter=5)


def test_a_zero_diagonal_names_the_node():
    P = problem("knn300")
    adj = ng.adjacency_matrix(P.g)
    B = torch.as_tensor(P.rhs(1), device=DEV)
    for check_every in (16, 0):
        with pytest.raises(ng.ArgumentError, match=r"diagonal .* of node 0 is not positive"):
            ng.cg_solve(adj, B, shift=0.0, scale=1.0, check_every=check_every)
    with pytest.raises(ng.ArgumentError, match=r"of node 299 is not positive"):          # only the isolated node's diagonal is 0
        ng.cg_solve(problem("hub300").M, B, shift=0.0, scale=1.0)


def test_a_directed_edge_is_refused():
    g = ng.GNNGraph([0, 1, 2], [1, 0, 0], num_nodes=3, index_base=0)
    with pytest.raises(ng.ArgumentError, match=r"ngpde_csr_check_symmetric: the matrix is not symmetric: entry \(2, 0\)"):
        ng.cg_solve(ng.laplacian_matrix(g), torch.ones(1, 3, device=DEV), shift=1.0)


def test_refused_by_name_on_the_device():
    P = problem("knn64")
    B = torch.as_tensor(P.rhs(2), device=DEV)
    with pytest.raises(ng.DimensionMismatch, match="B has shape"):
        P.solve(B[:, :63])
    with pytest.raises(ng.DimensionMismatch, match="x0 has shape"):
        P.solve(B, x0=B[:1])
    with pytest.raises(ng.ArgumentError, match="B must hold float32"):
        P.solve(B.double())
    with pytest.raises(ng.ArgumentError, match="must live on"):
        ng.cg_solve(P.M, B.cpu(), shift=SHIFT, scale=P.b)
    # the C entry: a workspace one byte short, and an indicator that the device finds unordered
    lib, M = _lib.load(), P.M
    need = int(lib.ngpde_csr_cg_workspace_bytes(P.n, 1, 2))
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    X = torch.empty_like(B)
    st, it = (torch.empty((2, 2), dtype=torch.int32, device=DEV) for _ in range(2))
    res = torch.empty((2, 2), dtype=torch.float32, device=DEV)

    def call(n_graphs, graph_of, nbytes):
        return lib.ngpde_csr_cg(P.n, M.nnz, _lib.ptr(M.row_ptr), _lib.ptr(M.cols), _lib.ptr(M.values.detach()), n_graphs, _lib.ptr(graph_of), 1.0,
                                P.b, 2, _lib.ptr(B), None, _lib.ptr(X), 1, 1e-5, 0.0, 10, 16, _lib.ptr(st), _lib.ptr(it), _lib.ptr(res), _lib.ptr(ws),
                                nbytes, _lib.current_stream())

    assert call(1, None, need - 1) == _lib.ERR_WORKSPACE and b"needed" in lib.ngpde_last_error()
    gi = torch.zeros(P.n, dtype=torch.int32, device=DEV)
    gi[:8] = 1
    ws2 = torch.empty(int(lib.ngpde_csr_cg_workspace_bytes(P.n, 2, 2)), dtype=torch.uint8, device=DEV)
    ws, need2 = ws2, ws2.numel()
    assert call(2, gi, need2) == _lib.ERR_INVALID_ARGUMENT and b"not non-decreasing" in lib.ngpde_last_error()


# ---- 4. gradients ---------------------------------------------------------------------------------------------------------------

def test_gradients_against_float64_autograd_through_a_dense_solve():
    """loss = (X . R).sum() at rtol = 1e-6 on the hub graph, D = 5; the float64 reference solves with A32 (the assembly's float32
    rounding carried as a constant, so the forward operator is the library's) and differentiates the exact assembly.

    With G = dloss/dX = R: dB* = A32^-1 G, and the library's dB is a CG solve of G with the same settings, so by check 1
        eB_d = |dB_d - dB*_d|_2 <= 2 rtol |G_d|_2 / shift,          eX_d = |X_d - X*_d|_2 <= 2 rtol |B_d|_2 / shift.
    dvalues[(i, j)] = -scale sum_d dB[d, i] X[d, j] is bilinear; every component of an error vector is at most its 2-norm, so
        |dvalues - dvalues*|[(i, j)] <= scale sum_d (eB_d |X*[d, j]| + |dB*[d, i]| eX_d + eB_d eX_d) + D 2^-23 scale sum_d |dB[d, i] X[d, j]|
    (the last term: the float32 dot product of D terms and the product with scale).  The Laplacian's pullback to an edge s -> t is
    dw = dvalues[(s, s)] - dvalues[(s, t)]: the two entries' bounds and the rounding of the subtraction, 2^-23 (|.| + |.|)."""
    P = problem("hub300")
    D, rtol = 5, 1e-6
    B, R = P.rhs(D), P.rhs(D, seed=1)
    w = torch.as_tensor(P.w, device=DEV).requires_grad_(True)
    g = ng.GNNGraph(P.s, P.t, num_nodes=P.n, index_base=0, edge_weight=w)
    M = ng.laplacian_matrix(g)
    M.values.retain_grad()
    Bt = torch.as_tensor(B, device=DEV).requires_grad_(True)
    X = ng.cg_solve(M, Bt, shift=SHIFT, scale=P.b, rtol=rtol)
    (X * torch.as_tensor(R, device=DEV)).sum().backward()
    rows, cols = host(M.rows).astype(np.int64), host(M.cols).astype(np.int64)

    # the reference
    w64 = torch.tensor(P.w.astype(np.float64), requires_grad=True)
    B64 = torch.tensor(B.astype(np.float64), requires_grad=True)
    s, t = torch.as_tensor(P.s), torch.as_tensor(P.t)
    adj = torch.zeros(P.n, P.n, dtype=torch.float64).index_put((s, t), w64, accumulate=True)
    lap = torch.diag(adj.sum(1)) - adj
    exact = lap[torch.as_tensor(rows), torch.as_tensor(cols)]
    v64 = exact + (torch.tensor(host(M.values).astype(np.float64)) - exact).detach()          # = the library's float32 values
    v64.retain_grad()
    A = SHIFT * torch.eye(P.n, dtype=torch.float64) + P.b * torch.zeros(P.n, P.n, dtype=torch.float64).index_put(
        (torch.as_tensor(rows), torch.as_tensor(cols)), v64)
    assert np.allclose(A.detach().numpy(), P.A32, rtol=1e-14, atol=0)
    Xs = torch.linalg.solve(A, B64.T).T
    (Xs * torch.tensor(R.astype(np.float64))).sum().backward()
    dBs, dvs, dws, Xs = B64.grad.numpy(), v64.grad.numpy(), w64.grad.numpy(), Xs.detach().numpy()

    eB = 2 * rtol * np.linalg.norm(R.astype(np.float64), axis=1) / SHIFT
    eX = 2 * rtol * np.linalg.norm(B.astype(np.float64), axis=1) / SHIFT
    dB, dv, dw = (host(v).astype(np.float64) for v in (Bt.grad, M.values.grad, w.grad))
    for c in range(D):
        got = np.linalg.norm(dB[c] - dBs[c])
        print(f"dB col {c}: {got:.3e} <= {eB[c]:.3e}")
        assert got <= eB[c]
    terms = np.abs(dB[:, rows] * host(X).astype(np.float64)[:, cols]).sum(0)
    bound_v = P.b * ((eB[:, None] * np.abs(Xs[:, cols])).sum(0) + (np.abs(dBs[:, rows]) * eX[:, None]).sum(0) + float(eB @ eX)) + D * U2 * P.b * terms
    print(f"dvalues: worst error / bound {np.max(np.abs(dv - dvs) / bound_v):.3f}")
    assert np.all(np.abs(dv - dvs) <= bound_v)
    at = {(int(r), int(c)): k for k, (r, c) in enumerate(zip(rows, cols))}
    diag = np.array([at[(int(a), int(a))] for a in P.s])
    ent = np.array([at[(int(a), int(b))] for a, b in zip(P.s, P.t)])
    bound_w = bound_v[diag] + bound_v[ent] + U2 * (np.abs(dvs[diag]) + np.abs(dvs[ent]))
    print(f"dw: worst error / bound {np.max(np.abs(dw - dws) / bound_w):.3f}")
    assert np.all(np.abs(dw - dws) <= bound_w)
    # the pullback has no atomics: the same bits again
    w.grad = None
    M2 = ng.laplacian_matrix(g)
    Bt2 = torch.as_tensor(B, device=DEV).requires_grad_(True)
    (ng.cg_solve(M2, Bt2, shift=SHIFT, scale=P.b, rtol=rtol) * torch.as_tensor(R, device=DEV)).sum().backward()
    assert torch.equal(Bt2.grad, Bt.grad) and torch.equal(w.grad, torch.as_tensor(dw.astype(np.float32), device=DEV))


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------

def test_the_entry_is_captured_and_replayed_bitwise():
    P = problem("batch")
    D, max_iter, rtol = 65, 30, 1e-6
    lib, M, ng_ = _lib.load(), P.M, len(P.blocks)
    graph_of = torch.as_tensor(P.gi, device=DEV)
    values = M.values.detach()
    B = torch.zeros((D, P.n), dtype=torch.float32, device=DEV)
    X = torch.empty_like(B)
    st, it = (torch.empty((ng_, D), dtype=torch.int32, device=DEV) for _ in range(2))
    res = torch.empty((ng_, D), dtype=torch.float32, device=DEV)
    nbytes = int(lib.ngpde_csr_cg_workspace_bytes(P.n, ng_, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

    def entry():
        return lib.ngpde_csr_cg(P.n, M.nnz, _lib.ptr(M.row_ptr), _lib.ptr(M.cols), _lib.ptr(values), ng_, _lib.ptr(graph_of), SHIFT, P.b, D,
                                _lib.ptr(B), None, _lib.ptr(X), 1, rtol, 0.0, max_iter, 0, _lib.ptr(st), _lib.ptr(it), _lib.ptr(res),
                                _lib.ptr(ws), nbytes, _lib.current_stream())

    assert entry() == 0, lib.ngpde_last_error()          # (eager once: the kernels are loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):          # one stream, a linear chain of launches
        code = entry()
    assert code == 0, lib.ngpde_last_error()
    for seed in (1, 2):
        Bk = torch.as_tensor(P.rhs(D, seed=seed), device=DEV)
        B.copy_(Bk)
        graph.replay()
        torch.cuda.synchronize()
        Xe, info = P.solve(Bk, rtol=rtol, max_iter=max_iter, check_every=0, return_info=True)
        assert int(info.status.max()) == 0
        assert torch.equal(X, Xe) and torch.equal(it, info.iterations) and torch.equal(st, info.status) and torch.equal(res, info.residual)
