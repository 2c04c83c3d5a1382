"""Time the weighted shortest paths (ngpde_amd.shortest_paths) next to three baselines:

    torch   the same synchronous rounds composed from torch ops on the GPU: the distances of the other ends gathered with
            `index_select`, the weights added, `scatter_reduce(amin)` into the nodes, one host read per round (as the stop needs);
            the 64 separate sources as one (64 x N) array.  It computes the same float32 fixed point: the results are compared bitwise.
    scipy   `scipy.sparse.csgraph.dijkstra(indices=)` in float64 on the host, INCLUDING the transfers: the device COO lists and
            weights down, the result up (null if scipy does not import)
    hops    for the rows with unit weights: `hop_distance`, the level loop on bit masks that answers the same question there

on three workloads:

    graph   bench.py's graph size, 16 384 nodes / 131 072 edges (the closest-pairs graph, bidirected by construction), the edge
            lengths |x_s - x_t|
    batch   24 clouds of 3 000 points, 8 nearest neighbours each, made bidirected: 72 000 nodes, the edge lengths |x_s - x_t|
    path    the directed path 0 -> 1 -> ... of 16 384 nodes with weights in [0.5, 1.5], the deep case: 16 384 rounds from node 0,
            one launch each

from one source and from 64 separate sources.

    python tools/bench_shortest_paths.py [--reps 10]

The rows plan is cached with the structure, so the calls are timed warm (its sort is `bench_traversal.py`'s "rows plan" row plus one
more output).  The calls read a word back per group of rounds, so nothing here is captured into a HIP graph: every figure is the
wall-clock time of one call between device synchronisations, the median of `reps` after warm-up; what takes seconds (the deep case's
baselines) runs twice.  A baseline that this build cannot run is reported as null.  One JSON line at the end holds every result.
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
    from scipy.sparse import csgraph
except ImportError:          # the scipy column is then null
    sp = csgraph = None


def wall_ms(fn, reps, warm):
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


def lengths(pts, g, dev):
    """|x_s - x_t| of every edge, float32 on the device; pts is (dim x N)"""
    s, t = graphops._coo(g, dev)
    return (pts.index_select(1, s.long()) - pts.index_select(1, t.long())).norm(dim=0).float().contiguous()


def workloads(dev):
    n = 16384
    pts, s0, t0 = S.closest_pairs_graph(n, 65536, seed=1)
    g = ng.GNNGraph(s0, t0, num_nodes=n, index_base=0)
    yield "graph", g, lengths(torch.as_tensor(np.ascontiguousarray(pts.T), dtype=torch.float32, device=dev), g, dev), False
    pts = torch.rand(3, 24 * 3000, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    gi = torch.arange(24, device=dev).repeat_interleave(3000) + 1
    g = ng.to_bidirected(ng.knn_graph(pts, 8, graph_indicator=gi))
    yield "batch", g, lengths(pts, g, dev), False
    g = ng.GNNGraph(np.arange(n - 1), np.arange(1, n), num_nodes=n, index_base=0)
    w = 0.5 + torch.rand(n - 1, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    yield "path", g, w.float().contiguous(), True


def paths_torch(s, t, w, n, sources):
    """(S x N): row i from sources[i] alone, following s -> t; the rounds of the library, one host read each"""
    k = len(sources)
    dist = torch.full((k, n), float("inf"), dtype=torch.float32, device=s.device)
    dist[torch.arange(k, device=s.device), sources] = 0
    tt = t.expand(k, -1)
    while True:
        lower = dist.scatter_reduce(1, tt, dist.index_select(1, s) + w, "amin", include_self=True)
        if torch.equal(lower, dist):
            return dist
        dist = lower


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_shortest_paths.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    results = {}
    for name, g, w, deep in workloads(dev):
        n, e = g.num_nodes, g.num_edges
        s32, t32 = graphops._coo(g, dev)
        s, t = s32.long(), t32.long()
        unit = torch.ones(e, dtype=torch.float32, device=dev)
        one = torch.zeros(1, dtype=torch.int64, device=dev)
        many = (torch.arange(64, device=dev) * (n // 64)).long()
        many[0] = 0

        def dijkstra_host(sources, weights):
            if sp is None:
                raise ImportError("scipy")
            m = sp.csr_matrix((weights.cpu().numpy().astype(np.float64), (s32.cpu().numpy(), t32.cpu().numpy())), shape=(n, n))
            return torch.as_tensor(csgraph.dijkstra(m, directed=True, indices=sources.cpu().numpy()).astype(np.float32), device=dev)

        reps = 2 if deep else args.reps
        ours = lambda sources, weights: lambda: ng.shortest_paths(g, sources, weights, separate=True)
        composed = lambda sources, weights: lambda: paths_torch(s, t, weights, n, sources)
        host = lambda sources, weights: lambda: dijkstra_host(sources, weights)
        hops = lambda sources: lambda: ng.hop_distance(g, sources, separate=True)
        ops = {
            "1 source": (ours(one, w), composed(one, w), host(one, w), None),
            "64 separate": (ours(many, w), composed(many, w), host(many, w), None),
            "1 source, unit weights": (ours(one, unit), composed(one, unit), host(one, unit), hops(one)),
            "64 separate, unit weights": (ours(many, unit), composed(many, unit), host(many, unit), hops(many)),
        }
        # the compositions do the library's work, bit for bit
        sep = ng.shortest_paths(g, many, w, separate=True, return_parents=True)
        assert torch.equal(sep.dist, paths_torch(s, t, w, n, many))
        assert torch.equal(ng.shortest_paths(g, one, w).dist, sep.dist[0])
        flat = ng.shortest_paths(g, many, unit, separate=True).dist
        level = ng.hop_distance(g, many, separate=True)
        assert torch.equal(flat, torch.where(level < 0, torch.full_like(flat, float("inf")), level.float()))
        reached = torch.isfinite(sep.dist)
        results[name] = {"nodes": n, "edges": e, "rounds": sep.rounds, "reached": round(float(reached.float().mean()), 4),
                         "longest": round(float(sep.dist[reached].max()), 4)}
        for op, (f_ours, f_torch, f_host, f_hops) in ops.items():
            row = {}
            for col, f in (("ms", f_ours), ("torch_ms", f_torch), ("scipy_ms", f_host), ("hops_ms", f_hops)):
                try:
                    if f is None:
                        raise NotImplementedError("no such baseline")
                    slow = deep and col in ("torch_ms", "scipy_ms")
                    row[col] = round(wall_ms(f, min(reps, 2) if slow else reps, warm=1 if slow else 2), 4)
                except Exception as err:          # (a baseline this build cannot run; the library's own column never lands here silently)
                    if col == "ms":
                        raise
                    row[col] = None
                    if f is not None:
                        print(f"  {name} {op} {col}: {type(err).__name__}: {str(err)[:120]}", flush=True)
            for col in ("torch_ms", "scipy_ms", "hops_ms"):
                row["speedup_vs_" + col[:-3]] = None if row[col] is None else round(row[col] / row["ms"], 3)
            results[name][op] = row
            fmt = lambda v: "     n/a" if v is None else f"{v:9.3f}"
            print(f"{name:6s} shortest_paths, {op:26s} ours {row['ms']:9.3f} ms   torch {fmt(row['torch_ms'])} ms (x{fmt(row['speedup_vs_torch'])})   "
                  f"scipy + transfers {fmt(row['scipy_ms'])} ms (x{fmt(row['speedup_vs_scipy'])})   "
                  f"hop_distance {fmt(row['hops_ms'])} ms (x{fmt(row['speedup_vs_hops'])})", flush=True)
        print(f"{name:6s} {results[name]['rounds']} rounds; {results[name]['reached']} of the (source, node) pairs reached, the longest "
              f"distance {results[name]['longest']}", flush=True)
    print(json.dumps({"results": results}))


if __name__ == "__main__":
    main()
