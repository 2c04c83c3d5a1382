"""Time the graph transforms (ngpde_amd.remove_multi_edges / to_bidirected / remove_self_loops / getgraph / degree) next to two baselines:

    torch   the same operation composed from torch ops on the GPU (torch.unique / sort / index_add_ / boolean masks / bincount)
    numpy   the same operation in numpy on the host, INCLUDING the transfers: the device COO lists and features down, the result up

on two graphs, each with a 16-row float32 edge feature:

    bench   bench.py's graph size: 16 384 nodes / 131 072 edges (the closest-pairs graph), as one graph
    vmh     a batch of 24 clouds of 3 000 points, 6 nearest neighbours each (the README's VMH minibatch): 72 000 nodes / 432 000 edges

    python tools/bench_graph_ops.py [--reps 30]

The library's transforms return a count through the host and synchronise, so nothing here is captured into a HIP graph: every figure
is the wall-clock time of one call between device synchronisations, the median of `reps` after warm-up.  `ours` is the public Python
function, which ends in a GNNGraph (its host copy of the edge list included); the torch and numpy columns stop at device tensors of the
result, so the comparison is biased against the library.  `ok` says the library was no slower than the torch composition.  One JSON line
at the end holds every result.
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

D = 16


def wall_ms(fn, reps):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def make_graphs(dev):
    _, s, t = S.closest_pairs_graph(16384, 65536, seed=1)
    bench = ng.GNNGraph(s, t, num_nodes=16384, index_base=0)
    gen = torch.Generator(device=dev).manual_seed(0)
    pts = torch.rand(2, 24 * 3000, device=dev, generator=gen)
    gi = torch.arange(24, device=dev).repeat_interleave(3000) + 1
    vmh = ng.knn_graph(pts, 6, graph_indicator=gi)
    return {"bench": bench, "vmh": vmh}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_graph_ops.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    results = {}
    for name, g0 in make_graphs(dev).items():
        n, e = g0.num_nodes, g0.num_edges
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(D, e, device=dev, generator=gen)
        g = ng.GNNGraph(g0, edata={"e": x})
        s32, t32 = graphops._coo(g, dev)
        s, t = s32.long(), t32.long()
        xr = x.T.contiguous()
        gid = None if g.graph_indicator is None else torch.as_tensor(g.graph_indicator.astype(np.int64), device=dev)
        member = 0 if gid is None else 11

        def coalesce_torch(sym):
            ss, tt, rows = (torch.cat([s, t]), torch.cat([t, s]), torch.cat([xr, xr])) if sym else (s, t, xr)
            uniq, inv = torch.unique(ss * n + tt, return_inverse=True)
            out = torch.zeros(uniq.numel(), D, device=dev).index_add_(0, inv, rows)
            if sym:
                out = out / torch.bincount(inv, minlength=uniq.numel())[:, None]
            return uniq // n, uniq % n, out.T

        def coalesce_numpy(sym):
            hs, ht, hx = s32.cpu().numpy().astype(np.int64), t32.cpu().numpy().astype(np.int64), x.cpu().numpy()
            if sym:
                hs, ht, hx = np.concatenate([hs, ht]), np.concatenate([ht, hs]), np.concatenate([hx, hx], axis=1)
            uniq, inv = np.unique(hs * n + ht, return_inverse=True)
            out = np.zeros((uniq.size, D), dtype=np.float32)
            np.add.at(out, inv.reshape(-1), hx.T)
            if sym:
                out /= np.bincount(inv.reshape(-1), minlength=uniq.size)[:, None]
            return torch.as_tensor(uniq // n, device=dev), torch.as_tensor(uniq % n, device=dev), torch.as_tensor(out.T, device=dev)

        def loops_torch():
            keep = s != t
            return s[keep], t[keep], x[:, keep]

        def loops_numpy():
            hs, ht, hx = s32.cpu().numpy(), t32.cpu().numpy(), x.cpu().numpy()
            keep = hs != ht
            return torch.as_tensor(hs[keep], device=dev), torch.as_tensor(ht[keep], device=dev), torch.as_tensor(hx[:, keep], device=dev)

        def getgraph_torch():
            mask = torch.ones(n, dtype=torch.bool, device=dev) if gid is None else gid == member
            relabel = torch.cumsum(mask, 0) - 1
            keep = mask[s] & mask[t]
            return relabel[s[keep]], relabel[t[keep]], x[:, keep]

        def getgraph_numpy():
            hs, ht, hx = s32.cpu().numpy(), t32.cpu().numpy(), x.cpu().numpy()
            mask = np.ones(n, dtype=bool) if gid is None else g.graph_indicator == member
            relabel = np.cumsum(mask) - 1
            keep = mask[hs] & mask[ht]
            return (torch.as_tensor(relabel[hs[keep]], device=dev), torch.as_tensor(relabel[ht[keep]], device=dev),
                    torch.as_tensor(hx[:, keep], device=dev))

        ops = {
            "remove_multi_edges": (lambda: ng.remove_multi_edges(g), lambda: coalesce_torch(False), lambda: coalesce_numpy(False)),
            "to_bidirected": (lambda: ng.to_bidirected(g), lambda: coalesce_torch(True), lambda: coalesce_numpy(True)),
            "remove_self_loops": (lambda: ng.remove_self_loops(g), loops_torch, loops_numpy),
            "getgraph": (lambda: ng.getgraph(g, member), getgraph_torch, getgraph_numpy),
            "degree": (lambda: ng.degree(g, "in"), lambda: torch.bincount(t, minlength=n),
                       lambda: torch.as_tensor(np.bincount(t32.cpu().numpy(), minlength=n), device=dev)),
        }
        # the compositions compute what the library computes
        ours, ref = ng.to_bidirected(g), coalesce_torch(True)
        so, to = ours.edge_index(index_base=0)
        assert np.array_equal(so, ref[0].cpu().numpy()) and np.array_equal(to, ref[1].cpu().numpy())
        assert torch.allclose(ours.edata["e"], ref[2], rtol=1e-5, atol=1e-6)
        assert torch.equal(ng.degree(g, "in").long(), torch.bincount(t, minlength=n))
        for op, (f_ours, f_torch, f_numpy) in ops.items():
            a, b, c = wall_ms(f_ours, args.reps), wall_ms(f_torch, args.reps), wall_ms(f_numpy, args.reps)
            key = f"{name} {op}"
            results[key] = dict(ms=round(a, 4), torch_ms=round(b, 4), numpy_ms=round(c, 4), speedup_vs_torch=round(b / a, 3),
                                speedup_vs_numpy=round(c / a, 3), ok=bool(a <= b))
            print(f"{key:28s} ours {a:8.3f} ms   torch {b:8.3f} ms (x{b / a:6.2f})   numpy + transfers {c:8.3f} ms (x{c / a:6.2f})", flush=True)
    print(json.dumps({"d": D, "graphs": {"bench": [16384, 131072], "vmh": [72000, 432000]}, "results": results}))


if __name__ == "__main__":
    main()
