"""Time the queries by node and by pair (ngpde_amd.has_edge / adjacency_list / neighbors / intersect / random_walk_pe) next to two
baselines:

    torch   the same operation composed from torch ops on the GPU: torch.isin on the 64-bit keys for has_edge, a stable argsort and
            bincount for adjacency_list, a mask for one node's neighbours, torch.unique + scatter_reduce + isin for intersect, and for
            random_walk_pe (a) the dense matrix power upstream uses -- the N x N matrix for one graph, the 24 dense blocks (bmm) for the
            batch -- and (b) repeated GraphMatrix.matmul of RW on blocks of 256 rows of the identity, the diagonal read off each product
    numpy   the same on the host with numpy (scipy.sparse for the walk: csr @ dense blocks of 256 seed columns, per graph on the batch),
            INCLUDING the transfers: the device COO lists and weights down, the result up

on two workloads, both with float32 edge weights:

    graph   bench.py's graph size, 16 384 nodes / 131 072 edges (the closest-pairs graph, bidirected by construction)
    batch   24 clouds of 3 000 points, 8 nearest neighbours each, made bidirected: 72 000 nodes, one block per graph

    python tools/bench_graph_queries.py [--reps 20] [--walk 8]

has_edge asks for every edge and as many random pairs; intersect pairs the graph with one that shares half of its edges.  The
library's sorted-key plan is cached with the structure, so `has_edge` and `intersect` are timed warm and the sort itself has a row of
its own ("key plan").  Most entries return counts through the host and synchronise, so nothing here is captured into a HIP graph: every
figure is the wall-clock time of one call between device synchronisations, the median of `reps` after warm-up; the walk baselines, which
take seconds, run twice (the host one once).  A baseline that this build cannot run is reported as null.  One JSON line at the end
holds every result.
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
from ngpde_amd import graphops, queries      # noqa: E402
from ngpde_amd import synth as S             # noqa: E402

try:
    import scipy.sparse as sp
except ImportError:          # the numpy column of the walk is then null
    sp = None

B = 256          # seed columns per block in the two blocked walk baselines


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
    w = (0.5 + rng.random(len(s0))).astype(np.float32)
    yield "graph", ng.GNNGraph(s0, t0, num_nodes=n, index_base=0, edge_weight=torch.as_tensor(w, device=dev)), None
    pts = torch.rand(3, 24 * 3000, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    gi = torch.arange(24, device=dev).repeat_interleave(3000) + 1
    gk = ng.to_bidirected(ng.knn_graph(pts, 8, graph_indicator=gi))
    s, t = gk.edge_index(index_base=0)
    w = (0.5 + ((s * 7919 + t * 104729) % 1000) / 1000.0).astype(np.float32)
    yield "batch", ng.GNNGraph(gk, edge_weight=torch.as_tensor(w, device=dev)), gk.graph_indicator


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--walk", type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_graph_queries.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    K = args.walk
    results = {}
    for name, g, gi in workloads(dev):
        n, e = g.num_nodes, g.num_edges
        s32, t32 = graphops._coo(g, dev)
        s, t, w = s32.long(), t32.long(), g.edge_weight
        gen = torch.Generator(device=dev).manual_seed(3)
        qs = torch.cat([s, torch.randint(0, n, (e,), device=dev, generator=gen)])
        qt = torch.cat([t, torch.randint(0, n, (e,), device=dev, generator=gen)])
        half = torch.randperm(e, device=dev, generator=gen)[:e // 2]
        s2 = torch.cat([s[half], torch.randint(0, n, (e // 2,), device=dev, generator=gen)])
        t2 = torch.cat([t[half], torch.randint(0, n, (e // 2,), device=dev, generator=gen)])
        g2 = ng.GNNGraph(s2.cpu().numpy(), t2.cpu().numpy(), num_nodes=n, index_base=0)
        hub = int(torch.bincount(s, minlength=n).argmax())
        a = ng.adjacency_matrix(g)
        n_blocks = 24 if gi is not None else 1
        size = n // n_blocks

        # ---- torch compositions
        keys = s * n + t
        keys2 = s2 * n + t2

        def has_torch():
            return torch.isin(qs * n + qt, keys)

        def adj_torch():
            order = torch.argsort(s, stable=True)
            return torch.cumsum(torch.bincount(s, minlength=n), 0), t[order], order

        def nb_torch():
            return t[s == hub]

        def inter_torch():
            _, inverse = torch.unique(keys, return_inverse=True)
            pos = torch.arange(e, device=dev)
            first = torch.full((int(inverse.max()) + 1,), e, device=dev).scatter_reduce(0, inverse, pos, "amin")
            keep = (first[inverse] == pos) & torch.isin(keys, keys2)
            return s[keep], t[keep], pos[keep]

        def rw_values():
            d = torch.zeros(n, device=dev).index_add(0, a.rows.long(), a.values)
            inv = torch.where(d == 0, torch.zeros_like(d), 1.0 / d)
            return a.values * inv[a.cols.long()]

        def rw_dense():
            vals = rw_values()
            if gi is None:
                m = torch.zeros(n, n, device=dev).index_put((a.rows.long(), a.cols.long()), vals)
                p, out = m, []
                for k in range(K):
                    p = m if k == 0 else m @ p
                    out.append(torch.diagonal(p))
                return torch.stack(out)
            r, c = a.rows.long(), a.cols.long()
            m = torch.zeros(n_blocks, size, size, device=dev).index_put((r // size, r % size, c % size), vals)
            p, out = m, []
            for k in range(K):
                p = m if k == 0 else torch.bmm(m, p)
                out.append(torch.diagonal(p, dim1=1, dim2=2).reshape(-1))
            return torch.stack(out)

        rw = ng.GraphMatrix(n, a.rows, a.cols, rw_values(), a.row_ptr, g.num_graphs, g.graph_indicator)
        rw.as_graph()

        def rw_matmul():
            out = torch.empty(K, n, device=dev)
            idx = torch.arange(B, device=dev)
            for b0 in range(0, n, B):
                width = min(B, n - b0)
                x = torch.zeros(width, n, device=dev)
                x[idx[:width], b0 + idx[:width]] = 1.0
                for k in range(K):
                    x = rw.matmul(x)
                    out[k, b0:b0 + width] = x[idx[:width], b0 + idx[:width]]
            return out

        # ---- numpy on the host, transfers included
        def down():
            return s32.cpu().numpy().astype(np.int64), t32.cpu().numpy().astype(np.int64)

        def up(*arrays):
            return [torch.as_tensor(np.ascontiguousarray(v), device=dev) for v in arrays]

        def has_host():
            hs, ht = down()
            return up(np.isin(qs.cpu().numpy() * n + qt.cpu().numpy(), hs * n + ht))

        def adj_host():
            hs, ht = down()
            order = np.argsort(hs, kind="stable")
            return up(np.cumsum(np.bincount(hs, minlength=n)), ht[order], order)

        def nb_host():
            hs, ht = down()
            return up(ht[hs == hub])

        def inter_host():
            hs, ht = down()
            k1, first = np.unique(hs * n + ht, return_index=True)
            eid = np.sort(first[np.isin(k1, s2.cpu().numpy() * n + t2.cpu().numpy())])
            return up(hs[eid], ht[eid], eid)

        def rw_host():
            if sp is None:
                raise ImportError("scipy")
            hs, ht = down()
            m = sp.csr_matrix((w.cpu().numpy(), (hs, ht)), shape=(n, n))
            d = np.asarray(m.sum(1)).ravel()
            inv = np.where(d == 0, 0.0, 1.0 / np.where(d == 0, 1.0, d)).astype(np.float32)
            m = (m @ sp.diags(inv)).tocsr()
            out = np.zeros((K, n), np.float32)
            for gb in range(n_blocks):
                lo = gb * size
                mg = m[lo:lo + size, lo:lo + size]
                for b0 in range(0, size, B):
                    width = min(B, size - b0)
                    x = np.zeros((size, width), np.float32)
                    x[b0 + np.arange(width), np.arange(width)] = 1.0
                    for k in range(K):
                        x = mg @ x
                        out[k, lo + b0:lo + b0 + width] = x[b0 + np.arange(width), np.arange(width)]
            return up(out)

        def plan():
            return queries._KeyPlan(g, dev)

        ops = {
            "key plan (the sort)": (plan, lambda: torch.sort(keys, stable=True), None, args.reps),
            "has_edge 2E queries": (lambda: ng.has_edge(g, qs, qt), has_torch, has_host, args.reps),
            "adjacency_list": (lambda: ng.adjacency_list(g), adj_torch, adj_host, args.reps),
            "neighbors(hub)": (lambda: ng.neighbors(g, hub), nb_torch, nb_host, args.reps),
            "intersect": (lambda: ng.intersect(g, g2, return_eid=True), inter_torch, inter_host, args.reps),
            f"random_walk_pe K={K}": (lambda: ng.random_walk_pe(g, K), rw_dense, rw_host, 2),
            f"random_walk_pe K={K} (torch: matmul blocks)": (lambda: ng.random_walk_pe(g, K), rw_matmul, None, 2),
        }
        # the compositions do the library's work
        assert torch.equal(ng.has_edge(g, qs, qt), has_torch())
        assert torch.equal(ng.adjacency_list(g).neighbors.long(), adj_torch()[1]) and torch.equal(ng.neighbors(g, hub).long(), nb_torch())
        assert torch.equal(ng.intersect(g, g2, return_eid=True).edata["EID"], inter_torch()[2])
        pe = ng.random_walk_pe(g, K)
        for other in (rw_dense(), rw_matmul()):
            assert torch.allclose(pe, other, rtol=1e-3, atol=1e-5), float((pe - other).abs().max())
        results[name] = {"nodes": n, "edges": e, "hub_degree": int(ng.neighbors(g, hub).numel())}
        for op, (f_ours, f_torch, f_host, reps) in ops.items():
            row = {}
            for col, f in (("ms", f_ours), ("torch_ms", f_torch), ("numpy_ms", f_host)):
                try:
                    if f is None:
                        raise NotImplementedError("no such baseline")
                    slow = reps <= 2
                    row[col] = round(wall_ms(f, 1 if (slow and col == "numpy_ms") else reps, warm=0 if (slow and col == "numpy_ms") else (1 if slow else 3)), 4)
                except Exception as err:          # (a baseline this build cannot run; the library's own column never lands here silently)
                    if col == "ms":
                        raise
                    row[col] = None
                    if f is not None:
                        print(f"  {name} {op} {col}: {type(err).__name__}: {str(err)[:120]}", flush=True)
            for col in ("torch_ms", "numpy_ms"):
                row["speedup_vs_" + col[:-3]] = None if row[col] is None else round(row[col] / row["ms"], 3)
            results[name][op] = row
            fmt = lambda v: "     n/a" if v is None else f"{v:8.3f}"
            print(f"{name:6s} {op:46s} ours {row['ms']:9.3f} ms   torch {fmt(row['torch_ms'])} ms (x{fmt(row['speedup_vs_torch'])})   "
                  f"numpy + transfers {fmt(row['numpy_ms'])} ms (x{fmt(row['speedup_vs_numpy'])})", flush=True)
    print(json.dumps({"walk_length": K, "results": results}))


if __name__ == "__main__":
    main()
