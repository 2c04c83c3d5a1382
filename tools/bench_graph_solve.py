"""Time one implicit diffusion step (I + dt L)^-1 u with ngpde_amd.cg_solve next to three baselines:

    torch   the same Jacobi-preconditioned CG composed from torch ops on the GPU: the product through torch.sparse (CSR) @ dense, the
            inner products per graph by index_add over the graph indicator, per-(graph, column) stops as masks, one read-back of "all
            stopped" every 16 steps, as the library does
    scipy   scipy.sparse.linalg.cg on the host, column by column and graph by graph, INCLUDING the transfers (the matrix's device lists
            and B down, X up)
    dense   GraphMatrix.to_dense() + torch.linalg.solve on the GPU, where the N x N matrix fits (the single graph; the batch's 72 000 x
            72 000 does not)

on two workloads, both with float32 edge weights, at D = 1 and D = 64 columns:

    graph   bench.py's graph size, 16 384 nodes / 131 072 edges (the closest-pairs graph, bidirected by construction)
    batch   24 clouds of 3 000 points, 8 nearest neighbours each, made bidirected: 72 000 nodes, one block per graph

    python tools/bench_graph_solve.py [--reps 10] [--rtol 1e-5] [--stiff 20]

dt = stiff * 2 / lambda_max(L) per workload (Gershgorin bound: 2 * the largest diagonal), i.e. `stiff` times the explicit step
bound.  Every figure is the wall-clock time of one call between device synchronisations, the median of `reps` after warm-up (the host
baseline runs once).  A baseline that this build cannot run is reported as null.  One JSON line at the end holds every result.
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
from ngpde_amd import synth as S             # noqa: E402

try:
    import scipy.sparse as sp
    import scipy.sparse.linalg as spla
except ImportError:          # the scipy column is then null
    sp = spla = None


def wall_ms(fn, reps, warm=2):
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
    w = (0.5 + ((s0.astype(np.int64) + t0.astype(np.int64)) * 7919 % 1000) / 1000.0).astype(np.float32)          # symmetric in (s, t)
    yield "graph", ng.GNNGraph(s0, t0, num_nodes=n, index_base=0, edge_weight=torch.as_tensor(w, device=dev))
    pts = torch.rand(3, 24 * 3000, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    gi = torch.arange(24, device=dev).repeat_interleave(3000) + 1
    gk = ng.to_bidirected(ng.knn_graph(pts, 8, graph_indicator=gi))
    s, t = gk.edge_index(index_base=0)
    w = (0.5 + ((s.astype(np.int64) + t.astype(np.int64)) * 7919 % 1000) / 1000.0).astype(np.float32)
    yield "batch", ng.GNNGraph(gk, edge_weight=torch.as_tensor(w, device=dev))


def torch_cg(A, dinv, graph_of, n_graphs, B, rtol, max_iter, check_every=16):
    """Jacobi-CG on X (N x D) with per-(graph, column) scalars and stops; A: torch sparse CSR (N x N)"""
    def dots(a, b):
        return torch.zeros(n_graphs, a.shape[1], device=a.device).index_add_(0, graph_of, a * b)

    x = torch.zeros_like(B)
    r = B.clone()
    z = r * dinv
    p = z.clone()
    rho = dots(r, z)
    tol = rtol * dots(B, B).sqrt()
    run = dots(r, r).sqrt() > tol
    for it in range(1, max_iter + 1):
        q = A @ p
        alpha = torch.where(run, rho / dots(p, q), torch.zeros_like(rho))
        x = x + alpha[graph_of] * p
        r = r - alpha[graph_of] * q
        z = r * dinv
        rho_new = dots(r, z)
        beta = torch.where(run, rho_new / rho, torch.zeros_like(rho))
        rho = torch.where(run, rho_new, rho)
        run = run & (dots(r, r).sqrt() > tol)
        p = z + beta[graph_of] * p
        if it % check_every == 0 and not bool(run.any()):
            break
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rtol", type=float, default=1e-5)
    ap.add_argument("--stiff", type=float, default=20.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_graph_solve.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    results = {}
    for name, g in workloads(dev):
        n, ng_ = g.num_nodes, g.num_graphs
        L = ng.laplacian_matrix(g)
        diag = L.diagonal()
        dt = float(args.stiff * 2.0 / (2.0 * float(diag.max())))
        graph_of = torch.zeros(n, dtype=torch.int64, device=dev) if g.graph_indicator is None else torch.as_tensor(g.graph_indicator, device=dev).long()
        vals = dt * L.values + (L.rows == L.cols).float()          # every diagonal position of a Laplacian is an entry
        A = torch.sparse_csr_tensor(L.row_ptr.long(), L.cols.long(), vals, size=(n, n))
        dinv = (1.0 / (1.0 + dt * diag)).reshape(-1, 1)
        results[name] = {"nodes": n, "edges": g.num_edges, "graphs": ng_, "dt": dt, "rtol": args.rtol}
        for D in (1, 64):
            B = torch.randn(D, n, device=dev, generator=torch.Generator(device=dev).manual_seed(D))
            Bt = B.T.contiguous()
            X, info = ng.cg_solve(L, B, shift=1.0, scale=dt, rtol=args.rtol, return_info=True)
            its = int(info.iterations.max())
            assert int(info.status.max()) == 0

            def ours():
                return ng.cg_solve(L, B, shift=1.0, scale=dt, rtol=args.rtol, check_symmetric=False)

            def ours_checked():
                return ng.cg_solve(L, B, shift=1.0, scale=dt, rtol=args.rtol)

            def composed():
                return torch_cg(A, dinv, graph_of, ng_, Bt, args.rtol, 1000)

            def dense():
                if n > 20000:
                    raise MemoryError("the dense matrix does not fit")
                a = torch.eye(n, device=dev) + dt * L.to_dense()
                return torch.linalg.solve(a, Bt).T

            def host():
                if sp is None:
                    raise ImportError("scipy")
                m = sp.csr_matrix((L.values.cpu().numpy().astype(np.float64) * dt, L.cols.cpu().numpy(), L.row_ptr.cpu().numpy()), shape=(n, n))
                m = (m + sp.identity(n, format="csr")).tocsr()
                b = B.cpu().numpy().astype(np.float64)
                gof = graph_of.cpu().numpy()
                out = np.zeros_like(b)
                for k in range(ng_):
                    idx = np.flatnonzero(gof == k)
                    mk = m[idx[0]:idx[-1] + 1, idx[0]:idx[-1] + 1]
                    pre = sp.diags(1.0 / mk.diagonal())
                    for c in range(D):
                        out[c, idx], _ = spla.cg(mk, b[c, idx], rtol=args.rtol, atol=0.0, M=pre)
                return torch.as_tensor(out.astype(np.float32), device=dev)

            # the baselines solve the same system
            try:
                ref = composed().T
                assert float((X - ref).abs().max()) <= 100 * args.rtol * float(X.abs().max()), float((X - ref).abs().max())
            except RuntimeError as err:          # (torch.sparse is not in every build: its column is then null)
                print(f"  {name} D={D} torch CG: {str(err)[:120]}", flush=True)
            row = {"iterations": its}
            for col, f, reps in (("ms", ours, args.reps), ("checked_ms", ours_checked, args.reps), ("torch_ms", composed, args.reps),
                                 ("dense_ms", dense, 3), ("scipy_ms", host, 1)):
                try:
                    row[col] = round(wall_ms(f, reps, warm=0 if col == "scipy_ms" else 2), 4)
                except Exception as err:          # (a baseline this build cannot run; the library's own columns never land here silently)
                    if col in ("ms", "checked_ms"):
                        raise
                    row[col] = None
                    print(f"  {name} D={D} {col}: {type(err).__name__}: {str(err)[:120]}", flush=True)
            for col in ("torch_ms", "dense_ms", "scipy_ms"):
                row["speedup_vs_" + col[:-3]] = None if row[col] is None else round(row[col] / row["ms"], 3)
            results[name][f"D={D}"] = row
            fmt = lambda v: "     n/a" if v is None else f"{v:9.3f}"
            print(f"{name:6s} D={D:3d} its {its:3d}  ours {row['ms']:9.3f} ms (with the symmetry check {row['checked_ms']:9.3f})   torch CG "
                  f"{fmt(row['torch_ms'])} ms (x{fmt(row['speedup_vs_torch'])})   dense solve {fmt(row['dense_ms'])} ms   scipy + transfers "
                  f"{fmt(row['scipy_ms'])} ms", flush=True)
    print(json.dumps({"results": results}))


if __name__ == "__main__":
    main()
