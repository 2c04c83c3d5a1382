"""Time the graph traversal (ngpde_amd.connected_components / hop_distance) next to three baselines:

    torch   the same algorithms composed from torch ops on the GPU: min-hooking with `scatter_reduce(amin)` and pointer jumping by
            `index_select` for the components (one host read per round and per jump, as the stop needs), and a level loop -- the
            frontier gathered with `index_select`, scattered with `scatter_reduce(amax)` -- for the hop distances; the 64 separate
            sources as one (64 x N) frontier
    scipy   `scipy.sparse.csgraph.connected_components(connection="weak")` and `shortest_path(unweighted=True, indices=)` on the host,
            INCLUDING the transfers: the device COO lists down, the result up (null if scipy does not import)
    x64     for the 64 separate sources: 64 single-source calls of the library

on three workloads:

    graph   bench.py's graph size, 16 384 nodes / 131 072 edges (the closest-pairs graph, bidirected by construction)
    batch   24 clouds of 3 000 points, 8 nearest neighbours each, made bidirected: 72 000 nodes, one block per graph
    path    the directed path 0 -> 1 -> ... of 16 384 nodes, the deep case: 16 383 levels from node 0, one launch each, and for the
            components the chain of depth N after the first hook round

    python tools/bench_traversal.py [--reps 10]

The rows plan of hop_distance is cached with the structure, so the calls are timed warm and the sort has a row of its own ("rows
plan").  The calls read a word back per group of rounds / levels, so nothing here is captured into a HIP graph: every figure is the
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
from ngpde_amd import graphops, traversal    # noqa: E402
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


def workloads(dev):
    n = 16384
    _, s0, t0 = S.closest_pairs_graph(n, 65536, seed=1)
    yield "graph", ng.GNNGraph(s0, t0, num_nodes=n, index_base=0), False
    pts = torch.rand(3, 24 * 3000, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    gi = torch.arange(24, device=dev).repeat_interleave(3000) + 1
    yield "batch", ng.to_bidirected(ng.knn_graph(pts, 8, graph_indicator=gi)), False
    yield "path", ng.GNNGraph(np.arange(n - 1), np.arange(1, n), num_nodes=n, index_base=0), True


def components_torch(s, t, n):
    parent = torch.arange(n, device=s.device)
    while True:
        ra, rb = parent.index_select(0, s), parent.index_select(0, t)
        differ = ra != rb
        if not bool(differ.any()):
            return parent
        parent = parent.scatter_reduce(0, torch.maximum(ra, rb)[differ], torch.minimum(ra, rb)[differ], "amin")
        while True:
            up = parent.index_select(0, parent)
            if torch.equal(up, parent):
                break
            parent = up


def hop_torch(s, t, n, sources):
    """(S x N): row i from sources[i] alone, following s -> t"""
    k = len(sources)
    rows = torch.arange(k, device=s.device)
    dist = torch.full((k, n), -1, dtype=torch.int32, device=s.device)
    dist[rows, sources] = 0
    frontier = dist == 0
    tt = t.expand(k, -1)
    level = 0
    while True:
        level += 1
        reach = torch.zeros((k, n), dtype=torch.int32, device=s.device).scatter_reduce(1, tt, frontier.index_select(1, s).int(), "amax")
        frontier = (reach > 0) & (dist < 0)
        if not bool(frontier.any()):
            return dist
        dist[frontier] = level


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_traversal.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    results = {}
    for name, g, deep in workloads(dev):
        n, e = g.num_nodes, g.num_edges
        s32, t32 = graphops._coo(g, dev)
        s, t = s32.long(), t32.long()
        one = torch.zeros(1, dtype=torch.int64, device=dev)
        many = (torch.arange(64, device=dev) * (n // 64)).long()
        many[0] = 0

        def down():
            hs, ht = s32.cpu().numpy(), t32.cpu().numpy()
            return sp.csr_matrix((np.ones(e, np.int8), (hs, ht)), shape=(n, n))

        def cc_host():
            if sp is None:
                raise ImportError("scipy")
            return torch.as_tensor(csgraph.connected_components(down(), directed=True, connection="weak")[1], device=dev)

        def hop_host(sources):
            if sp is None:
                raise ImportError("scipy")
            d = csgraph.shortest_path(down(), unweighted=True, indices=sources.cpu().numpy())
            return torch.as_tensor(np.where(np.isinf(d), -1, d).astype(np.int32), device=dev)

        def x64():
            return torch.stack([ng.hop_distance(g, many[i:i + 1]) for i in range(64)])

        slow = 2 if deep else args.reps
        ops = {
            "rows plan (the sort)": (lambda: traversal._RowsPlan(g, 1, dev), lambda: torch.sort(t, stable=True), None, None, args.reps),
            "connected_components": (lambda: ng.connected_components(g), lambda: components_torch(s, t, n), cc_host, None, args.reps),
            "hop_distance, 1 source": (lambda: ng.hop_distance(g, one), lambda: hop_torch(s, t, n, one), lambda: hop_host(one), None, slow),
            "hop_distance, 64 separate": (lambda: ng.hop_distance(g, many, separate=True), lambda: hop_torch(s, t, n, many),
                                          lambda: hop_host(many), x64, slow),
        }
        # the compositions do the library's work
        comps = ng.connected_components(g)
        assert torch.equal(comps.smallest.long(), components_torch(s, t, n))
        assert torch.equal(ng.hop_distance(g, one), hop_torch(s, t, n, one)[0])
        sep = ng.hop_distance(g, many, separate=True)
        assert torch.equal(sep, hop_torch(s, t, n, many))
        results[name] = {"nodes": n, "edges": e, "components": comps.count, "rounds": comps.rounds, "levels": int(sep.max())}
        for op, (f_ours, f_torch, f_host, f_x64, reps) in ops.items():
            row = {}
            for col, f in (("ms", f_ours), ("torch_ms", f_torch), ("scipy_ms", f_host), ("x64_ms", f_x64)):
                try:
                    if f is None:
                        raise NotImplementedError("no such baseline")
                    row[col] = round(wall_ms(f, reps if col == "ms" or not deep else min(reps, 2), warm=1 if (deep and col != "ms") else 2), 4)
                except Exception as err:          # (a baseline this build cannot run; the library's own column never lands here silently)
                    if col == "ms":
                        raise
                    row[col] = None
                    if f is not None:
                        print(f"  {name} {op} {col}: {type(err).__name__}: {str(err)[:120]}", flush=True)
            for col in ("torch_ms", "scipy_ms", "x64_ms"):
                row["speedup_vs_" + col[:-3]] = None if row[col] is None else round(row[col] / row["ms"], 3)
            results[name][op] = row
            fmt = lambda v: "     n/a" if v is None else f"{v:9.3f}"
            print(f"{name:6s} {op:28s} ours {row['ms']:9.3f} ms   torch {fmt(row['torch_ms'])} ms (x{fmt(row['speedup_vs_torch'])})   "
                  f"scipy + transfers {fmt(row['scipy_ms'])} ms (x{fmt(row['speedup_vs_scipy'])})   "
                  f"64 calls {fmt(row['x64_ms'])} ms (x{fmt(row['speedup_vs_x64'])})", flush=True)
        print(f"{name:6s} {results[name]['components']} components in {results[name]['rounds']} rounds; {results[name]['levels']} levels",
              flush=True)
    print(json.dumps({"results": results}))


if __name__ == "__main__":
    main()
