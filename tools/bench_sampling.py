"""Time the random graph sampling (ngpde_amd.sample_neighbors / rand_edge_split) next to two baselines:

    torch   the same kind of sample composed from torch ops on the GPU: torch.rand keys, a sort by (row, key), a rank mask
    numpy   the same in numpy on the host, INCLUDING the transfers: the device COO lists and the feature down, the result up

on two graphs, each with a 16-row float32 edge feature:

    bench   bench.py's graph size: 16 384 nodes / 131 072 edges (the closest-pairs graph)
    radius  a radius graph of 20 000 uniform points in the unit square, r = 0.03: ~56 neighbours per node, the row lengths the
            selection kernel is built for

    python tools/bench_sampling.py [--reps 30]

The baselines draw other random numbers than the library (torch.rand / numpy's generator against Philox keyed by edge), so they time
the same work, not the same sample.  The library's entries return a count through the host and synchronise, so nothing here is
captured into a HIP graph: every figure is the wall-clock time of one call between device synchronisations, the median of `reps` after
warm-up.  `ours` is the public Python function, which ends in GNNGraphs (their host copies of the edge lists included); the torch and
numpy columns stop at device tensors of the result, so the comparison is biased against the library.  `c_entry` times the C entry alone
(ngpde_coo_sample_neighbors / ngpde_coo_rand_split on device lists, outputs preallocated).  One JSON line at the end holds every result.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ngpde_amd as ng                       # noqa: E402
from ngpde_amd import _lib, graphops         # noqa: E402
from ngpde_amd import synth as S             # noqa: E402

D, K, FRAC = 16, 8, 0.8


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
    pts = torch.rand(2, 20000, device=dev, generator=gen)
    return {"bench": bench, "radius": ng.radius_graph(pts, 0.03)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sampling.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    results, shapes = {}, {}
    for name, g0 in make_graphs(dev).items():
        n, e = g0.num_nodes, g0.num_edges
        shapes[name] = [n, e]
        gen = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(D, e, device=dev, generator=gen)
        g = ng.GNNGraph(g0, edata={"e": x})
        s32, t32 = graphops._coo(g, dev)
        s, t = s32.long(), t32.long()
        n_first = int(round(FRAC * e))
        so, to = torch.empty(e, dtype=torch.int32, device=dev), torch.empty(e, dtype=torch.int32, device=dev)
        eid, side = torch.empty((2, e), dtype=torch.int64, device=dev), torch.empty(e, dtype=torch.int32, device=dev)
        count = C.c_int64(0)

        def sample_c():
            _lib.check(lib.ngpde_coo_sample_neighbors(n, e, _lib.ptr(s32), _lib.ptr(t32), 0, 1, 0, None, K, 0, 7, _lib.ptr(so), _lib.ptr(to),
                                                      _lib.ptr(eid[0]), C.byref(count), _lib.current_stream()))

        def split_c():
            _lib.check(lib.ngpde_coo_rand_split(n, e, _lib.ptr(s32), _lib.ptr(t32), 0, n_first, 0, 7, _lib.ptr(side), _lib.ptr(eid[0]),
                                                _lib.ptr(eid[1]), C.byref(count), _lib.current_stream()))

        def sample_torch():
            key = torch.rand(e, device=dev)
            order = torch.argsort(key)
            order = order[torch.argsort(t[order], stable=True)]                       # by row, then key
            rows = t[order]
            start = torch.searchsorted(rows, torch.arange(n, device=dev))
            keep = torch.zeros(e, dtype=torch.bool, device=dev)
            keep[order] = torch.arange(e, device=dev) - start[rows] < K
            return s[keep], t[keep], x[:, keep]

        def sample_numpy():
            hs, ht, hx = s32.cpu().numpy(), t32.cpu().numpy(), x.cpu().numpy()
            order = np.lexsort((np.random.default_rng(7).random(e), ht))
            start = np.searchsorted(ht[order], np.arange(n))
            keep = np.zeros(e, dtype=bool)
            keep[order] = np.arange(e) - start[ht[order]] < K
            return torch.as_tensor(hs[keep], device=dev), torch.as_tensor(ht[keep], device=dev), torch.as_tensor(hx[:, keep], device=dev)

        def split_torch():
            first = torch.zeros(e, dtype=torch.bool, device=dev)
            first[torch.argsort(torch.rand(e, device=dev))[:n_first]] = True
            return s[first], t[first], x[:, first], s[~first], t[~first], x[:, ~first]

        def split_numpy():
            hs, ht, hx = s32.cpu().numpy(), t32.cpu().numpy(), x.cpu().numpy()
            first = np.zeros(e, dtype=bool)
            first[np.argsort(np.random.default_rng(7).random(e))[:n_first]] = True
            return [torch.as_tensor(a, device=dev) for a in (hs[first], ht[first], hx[:, first], hs[~first], ht[~first], hx[:, ~first])]

        ops = {
            "sample_neighbors": (lambda: ng.sample_neighbors(g, None, K, seed=7), sample_c, sample_torch, sample_numpy),
            "rand_edge_split": (lambda: ng.rand_edge_split(g, FRAC, bidirected=False, seed=7), split_c, split_torch, split_numpy),
        }
        # the compositions do the library's work: the same number of edges per row, the same split sizes
        ours, ref = ng.sample_neighbors(g, None, K, seed=7), sample_torch()
        assert torch.equal(torch.bincount(torch.as_tensor(ours.edge_index(index_base=0)[1], device=dev), minlength=n), torch.bincount(ref[1], minlength=n))
        assert ng.rand_edge_split(g, FRAC, bidirected=False, seed=7)[0].num_edges == split_torch()[0].numel()
        for op, (f_ours, f_c, f_torch, f_numpy) in ops.items():
            a, c, b, h = (wall_ms(f, args.reps) for f in (f_ours, f_c, f_torch, f_numpy))
            key = f"{name} {op}"
            results[key] = dict(ms=round(a, 4), c_entry_ms=round(c, 4), torch_ms=round(b, 4), numpy_ms=round(h, 4), speedup_vs_torch=round(b / a, 3),
                                speedup_vs_numpy=round(h / a, 3))
            print(f"{key:28s} ours {a:8.3f} ms (C entry {c:7.3f} ms)   torch {b:8.3f} ms (x{b / a:6.2f})   numpy + transfers {h:8.3f} ms "
                  f"(x{h / a:6.2f})", flush=True)
    print(json.dumps({"d": D, "k": K, "frac": FRAC, "graphs": shapes, "results": results}))


if __name__ == "__main__":
    main()
