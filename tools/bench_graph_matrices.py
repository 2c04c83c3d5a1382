"""Time the graph matrices (ngpde_amd.adjacency_matrix / laplacian_matrix / normalized_laplacian / laplacian_lambda_max / khop_adj and
GraphMatrix.matmul) next to two baselines:

    torch   the same operation composed from torch ops on the GPU: torch.sparse_coo_tensor(...).coalesce() and index_add for the
            assemblies, torch.sparse.mm for the products, and for lambda_max torch.lobpcg on the sparse matrix (one graph) or the batched
            torch.linalg.eigvalsh of the dense blocks (a batch: lobpcg gives one value, not one per graph)
    numpy   the same on the host with numpy / scipy.sparse (scipy.sparse.linalg.eigsh for lambda_max), INCLUDING the transfers: the
            device COO lists and weights down, the result up

on two workloads, both with float32 edge weights that are equal in the two directions of a pair:

    graph   bench.py's graph size, 16 384 nodes / 131 072 edges (the closest-pairs graph, bidirected by construction)
    batch   24 clouds of 3 000 points, 8 nearest neighbours each, made bidirected: 72 000 nodes, one block per graph

    python tools/bench_graph_matrices.py [--reps 20]

The normalised Laplacian and lambda_max run with add_self_loops=True (the closest-pairs graph has isolated nodes).  The library's
entries return counts through the host and synchronise, so nothing here is captured into a HIP graph: every figure is the wall-clock
time of one call between device synchronisations, the median of `reps` after warm-up; the eigenvalue baselines, which take seconds, run
3 times.  A baseline that this torch build cannot run is reported as null.  One JSON line at the end holds every result.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ngpde_amd as ng                       # noqa: E402
from ngpde_amd import graphops               # noqa: E402
from ngpde_amd import synth as S             # noqa: E402

try:
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
except ImportError:          # the numpy column then holds only what numpy alone does
    sp = spl = None

D = 64


def wall_ms(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def workloads(dev):
    n = 16384
    _, s0, t0 = S.closest_pairs_graph(n, 65536, seed=1)
    rng = np.random.default_rng(0)
    pair_w = {}
    w = np.array([pair_w.setdefault((min(a, b), max(a, b)), 0.5 + rng.random()) for a, b in zip(s0.tolist(), t0.tolist())], np.float32)
    yield "graph", ng.GNNGraph(s0, t0, num_nodes=n, index_base=0, edge_weight=torch.as_tensor(w, device=dev)), None
    pts = torch.rand(3, 24 * 3000, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    gi = torch.arange(24, device=dev).repeat_interleave(3000) + 1
    gk = ng.to_bidirected(ng.knn_graph(pts, 8, graph_indicator=gi))
    s, t = gk.edge_index(index_base=0)
    w = (0.5 + ((np.minimum(s, t) * 7919 + np.maximum(s, t) * 104729) % 1000) / 1000.0).astype(np.float32)          # one weight per pair
    yield "batch", ng.GNNGraph(gk, edge_weight=torch.as_tensor(w, device=dev)), gk.graph_indicator


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_graph_matrices.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    results = {}
    for name, g, gi in workloads(dev):
        n, e = g.num_nodes, g.num_edges
        s32, t32 = graphops._coo(g, dev)
        s, t, w = s32.long(), t32.long(), g.edge_weight
        eye = torch.arange(n, device=dev)
        X = torch.randn(D, n, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        lap = ng.laplacian_matrix(g)

        # ---- torch compositions
        def coo(rows, cols, vals):
            return torch.sparse_coo_tensor(torch.stack([rows, cols]), vals, (n, n)).coalesce()

        def adj_torch():
            return coo(s, t, w)

        def lap_torch():
            d = torch.zeros(n, device=dev).index_add(0, s, w)
            return coo(torch.cat([s, eye]), torch.cat([t, eye]), torch.cat([-w, d]))

        def norm_torch():
            c = (torch.zeros(n, device=dev).index_add(0, s, w) + 1.0).rsqrt()
            return coo(torch.cat([s, eye]), torch.cat([t, eye]), torch.cat([-c[s] * w * c[t], 1.0 - c * c]))

        def lam_torch():
            m = norm_torch()
            if gi is None:
                return torch.lobpcg(m, k=1, largest=True, niter=64, tol=1e-5)[0]
            r, c = m.indices()
            blocks = torch.zeros(24, 3000, 3000, device=dev).index_put((r // 3000, r % 3000, c % 3000), m.values())
            return torch.linalg.eigvalsh(blocks)[:, -1]

        a_t = adj_torch()
        lap_t = lap_torch()

        def khop_torch(k):
            p = a_t
            for _ in range(k - 1):
                p = torch.sparse.mm(p, a_t)
            return p

        # ---- numpy / scipy on the host, transfers included
        def down():
            return s32.cpu().numpy(), t32.cpu().numpy(), w.cpu().numpy()

        def up(m):
            m = m.tocoo()
            return [torch.as_tensor(v, device=dev) for v in (m.row, m.col, m.data)]

        def adj_host():
            hs, ht, hw = down()
            return sp.csr_matrix((hw, (hs, ht)), shape=(n, n))

        def lap_host():
            a = adj_host()
            return sp.diags(np.asarray(a.sum(1)).ravel()) - a

        def norm_host():
            a = adj_host() + sp.identity(n, dtype=np.float32, format="csr")
            c = sp.diags(1.0 / np.sqrt(np.asarray(a.sum(1)).ravel()))
            return sp.identity(n, format="csr") - c @ a @ c

        def lam_host():
            m = norm_host()
            if gi is None:
                return spl.eigsh(m, k=1, which="LA", tol=1e-5, return_eigenvectors=False)
            return [spl.eigsh(m[k * 3000:(k + 1) * 3000, k * 3000:(k + 1) * 3000], k=1, which="LA", tol=1e-5, return_eigenvectors=False)
                    for k in range(24)]

        def khop_host(k):
            a = adj_host()
            p = a
            for _ in range(k - 1):
                p = p @ a
            return up(p)

        def matmul_host():
            m = adj_host()
            return torch.as_tensor(np.ascontiguousarray((m @ X.cpu().numpy().T).T), device=dev)

        ops = {
            "adjacency_matrix": (lambda: ng.adjacency_matrix(g), adj_torch, lambda: up(adj_host()), args.reps),
            "laplacian_matrix": (lambda: ng.laplacian_matrix(g), lap_torch, lambda: up(lap_host()), args.reps),
            "normalized_laplacian": (lambda: ng.normalized_laplacian(g, add_self_loops=True), norm_torch, lambda: up(norm_host()), args.reps),
            "laplacian_lambda_max": (lambda: ng.laplacian_lambda_max(g, add_self_loops=True), lam_torch, lam_host, 3),
            "khop_adj k=2": (lambda: ng.khop_adj(g, 2), lambda: khop_torch(2), lambda: khop_host(2), args.reps),
            "khop_adj k=3": (lambda: ng.khop_adj(g, 3), lambda: khop_torch(3), lambda: khop_host(3), args.reps),
            "matmul D=64": (lambda: lap.matmul(X), lambda: torch.sparse.mm(lap_t, X.T), matmul_host, args.reps),
        }
        # the compositions do the library's work
        assert ng.adjacency_matrix(g).nnz == a_t._nnz() and ng.khop_adj(g, 2).nnz == khop_torch(2)._nnz()
        assert torch.allclose(lap.matmul(X), torch.sparse.mm(lap_t, X.T).T, rtol=1e-4, atol=1e-4)
        results[name] = {"nodes": n, "edges": e}
        for op, (f_ours, f_torch, f_host, reps) in ops.items():
            row = {}
            for col, f in (("ms", f_ours), ("torch_ms", f_torch), ("numpy_ms", f_host)):
                try:
                    if col == "numpy_ms" and sp is None:
                        raise ImportError("scipy")
                    row[col] = round(wall_ms(f, reps if col == "ms" else min(reps, args.reps), warm=3 if reps > 3 else 1), 4)
                except Exception as err:          # (a baseline this build cannot run; the library's own column never lands here silently)
                    if col == "ms":
                        raise
                    row[col] = None
                    print(f"  {name} {op} {col}: {type(err).__name__}: {str(err)[:120]}", flush=True)
            for col in ("torch_ms", "numpy_ms"):
                row["speedup_vs_" + col[:-3]] = None if row[col] is None else round(row[col] / row["ms"], 3)
            results[name][op] = row
            fmt = lambda v: "     n/a" if v is None else f"{v:8.3f}"
            print(f"{name:6s} {op:22s} ours {row['ms']:9.3f} ms   torch {fmt(row['torch_ms'])} ms (x{fmt(row['speedup_vs_torch'])})   "
                  f"numpy + transfers {fmt(row['numpy_ms'])} ms (x{fmt(row['speedup_vs_numpy'])})", flush=True)
    print(json.dumps({"d": D, "results": results}))


if __name__ == "__main__":
    main()
