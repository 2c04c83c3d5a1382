"""Time the graph editing and negative sampling (ngpde_amd.remove_edges / remove_nodes / add_edges / negative_sample) next to two baselines:

    torch   the same operation composed from torch ops on the GPU: torch.isin on the 64-bit keys s * n + t, a cumsum relabel, torch.cat,
            torch.randint + torch.unique
    numpy   the same in numpy on the host, INCLUDING the transfers: the device COO lists and the feature down, the result up

on bench.py's graph size, 16 384 nodes / 131 072 edges (the closest-pairs graph), with a 16-row float32 edge feature:

    remove_edges     by pairs, the pairs of 10 % of the edges
    remove_nodes     10 % of the nodes
    add_edges        10 % more edges, with their features
    negative_sample  the default count (as many negatives as the graph has edges), directed

    python tools/bench_graph_edit.py [--reps 30]

The library's entries return counts or errors through the host and synchronise, so nothing here is captured into a HIP graph: every
figure is the wall-clock time of one call between device synchronisations, the median of `reps` after warm-up.  `ours` is the public
Python function, which ends in a GNNGraph (its host copy of the edge list included); the torch and numpy columns stop at device tensors
of the result, so the comparison is biased against the library.  `c_entry` times the C entries alone on device lists with the outputs
preallocated (no features).  The negative-sampling baselines draw other random numbers than the library and return their sample in
another order (torch.unique sorts; a random permutation picks the count), so they time the same kind of work, not the same sample.
One JSON line at the end holds every result.
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

D, FRAC = 16, 0.1


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_graph_edit.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    n = 16384
    _, s0, t0 = S.closest_pairs_graph(n, 65536, seed=1)
    g0 = ng.GNNGraph(s0, t0, num_nodes=n, index_base=0)
    e = g0.num_edges
    gen = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(D, e, device=dev, generator=gen)
    g = ng.GNNGraph(g0, edata={"e": x})
    s32, t32 = graphops._coo(g, dev)
    s, t = s32.long(), t32.long()
    rng = np.random.default_rng(0)
    k = int(round(FRAC * e))
    picked = torch.as_tensor(rng.permutation(e)[:k], device=dev)
    ls32, lt32 = s32[picked].contiguous(), t32[picked].contiguous()
    ls, lt = ls32.long(), lt32.long()
    nodes = torch.as_tensor(rng.permutation(n)[:int(round(FRAC * n))], device=dev)
    s_new, t_new = (torch.as_tensor(rng.integers(0, n, k).astype(np.int32), device=dev) for _ in range(2))
    x_new = torch.randn(D, k, device=dev, generator=gen)
    so, to = torch.empty(2 * e, dtype=torch.int32, device=dev), torch.empty(2 * e, dtype=torch.int32, device=dev)
    kept, rest = torch.empty(e, dtype=torch.int64, device=dev), torch.empty(n, dtype=torch.int64, device=dev)
    count = C.c_int64(0)
    stream = _lib.current_stream

    # ---- remove_edges by pairs
    def remove_edges_c():
        _lib.check(lib.ngpde_coo_remove_edges(n, e, _lib.ptr(s32), _lib.ptr(t32), 0, k, None, _lib.ptr(ls32), _lib.ptr(lt32), _lib.ptr(so), _lib.ptr(to),
                                              _lib.ptr(kept), C.byref(count), stream()))

    def remove_edges_torch():
        keep = ~torch.isin(s * n + t, ls * n + lt)
        return s[keep], t[keep], x[:, keep]

    def remove_edges_numpy():
        hs, ht, hx = s32.cpu().numpy().astype(np.int64), t32.cpu().numpy().astype(np.int64), x.cpu().numpy()
        hl = ls.cpu().numpy() * n + lt.cpu().numpy()
        keep = ~np.isin(hs * n + ht, hl)
        return [torch.as_tensor(a, device=dev) for a in (hs[keep], ht[keep], hx[:, keep])]

    # ---- remove_nodes
    def remove_nodes_c():
        _lib.check(lib.ngpde_coo_complement_nodes(n, nodes.numel(), _lib.ptr(nodes), _lib.ptr(rest), C.byref(count), stream()))
        _lib.check(lib.ngpde_coo_compact(n, e, _lib.ptr(s32), _lib.ptr(t32), 0, count.value, _lib.ptr(rest), 0, _lib.ptr(so), _lib.ptr(to),
                                         _lib.ptr(kept), C.byref(count), stream()))

    def remove_nodes_torch():
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        alive[nodes] = False
        relabel = torch.cumsum(alive, 0) - 1
        keep = alive[s] & alive[t]
        return relabel[s[keep]], relabel[t[keep]], x[:, keep]

    def remove_nodes_numpy():
        hs, ht, hx = s32.cpu().numpy(), t32.cpu().numpy(), x.cpu().numpy()
        alive = np.ones(n, dtype=bool)
        alive[nodes.cpu().numpy()] = False
        relabel = np.cumsum(alive) - 1
        keep = alive[hs] & alive[ht]
        return [torch.as_tensor(a, device=dev) for a in (relabel[hs[keep]], relabel[ht[keep]], hx[:, keep])]

    # ---- add_edges
    def add_edges_c():
        _lib.check(lib.ngpde_coo_append(n, e, _lib.ptr(s32), _lib.ptr(t32), 0, k, _lib.ptr(s_new), _lib.ptr(t_new), None, _lib.ptr(so), _lib.ptr(to),
                                        stream()))

    def add_edges_torch():
        if bool(((s_new < 0) | (s_new >= n) | (t_new < 0) | (t_new >= n)).any()):          # the range check the library reads back
            raise ValueError
        return torch.cat([s32, s_new]), torch.cat([t32, t_new]), torch.cat([x, x_new], dim=1)

    def add_edges_numpy():
        hs, ht, hx = s32.cpu().numpy(), t32.cpu().numpy(), x.cpu().numpy()
        a, b, c = s_new.cpu().numpy(), t_new.cpu().numpy(), x_new.cpu().numpy()
        return [torch.as_tensor(v, device=dev) for v in (np.concatenate([hs, a]), np.concatenate([ht, b]), np.concatenate([hx, c], axis=1))]

    # ---- negative_sample
    u = n * (n - 1)

    def negative_c():
        _lib.check(lib.ngpde_coo_negative_sample(n, e, _lib.ptr(s32), _lib.ptr(t32), 0, e, 0, 7, 0, _lib.ptr(so), _lib.ptr(to), C.byref(count), stream()))

    def negative_torch():
        code = torch.randint(0, u, (int(1.25 * e) + 64,), device=dev)
        a, b = code // (n - 1), code % (n - 1)
        key = torch.unique(a * n + b + (b >= a))
        key = key[~torch.isin(key, s * n + t)]
        assert key.numel() >= e
        key = key[torch.randperm(key.numel(), device=dev)[:e]]
        return key // n, key % n

    def negative_numpy():
        hs, ht = s32.cpu().numpy().astype(np.int64), t32.cpu().numpy().astype(np.int64)
        code = np.random.default_rng(7).integers(0, u, int(1.25 * e) + 64)
        a, b = code // (n - 1), code % (n - 1)
        key = np.unique(a * n + b + (b >= a))
        key = key[~np.isin(key, hs * n + ht)]
        key = np.random.default_rng(8).permutation(key)[:e]
        return torch.as_tensor(key // n, device=dev), torch.as_tensor(key % n, device=dev)

    ops = {
        "remove_edges (pairs, 10 %)": (lambda: ng.remove_edges(g, ls, lt), remove_edges_c, remove_edges_torch, remove_edges_numpy),
        "remove_nodes (10 %)": (lambda: ng.remove_nodes(g, nodes), remove_nodes_c, remove_nodes_torch, remove_nodes_numpy),
        "add_edges (10 %)": (lambda: ng.add_edges(g, s_new, t_new, x_new), add_edges_c, add_edges_torch, add_edges_numpy),
        "negative_sample (E)": (lambda: ng.negative_sample(g0, bidirected=False, seed=7), negative_c, negative_torch, negative_numpy),
    }
    # the compositions do the library's work: the same edges, features included
    for name, torch_fn in (("remove_edges (pairs, 10 %)", remove_edges_torch), ("remove_nodes (10 %)", remove_nodes_torch), ("add_edges (10 %)", add_edges_torch)):
        ours, ref = ops[name][0](), torch_fn()
        gs, gt = ours.edge_index(index_base=0)
        assert np.array_equal(gs, ref[0].cpu().numpy()) and np.array_equal(gt, ref[1].cpu().numpy()) and torch.equal(ours.edata["e"], ref[2]), name
    assert ng.negative_sample(g0, bidirected=False, seed=7).num_edges == negative_torch()[0].numel() == e
    results = {}
    for op, (f_ours, f_c, f_torch, f_numpy) in ops.items():
        a, c, b, h = (wall_ms(f, args.reps) for f in (f_ours, f_c, f_torch, f_numpy))
        results[op] = dict(ms=round(a, 4), c_entry_ms=round(c, 4), torch_ms=round(b, 4), numpy_ms=round(h, 4), speedup_vs_torch=round(b / a, 3),
                           speedup_vs_numpy=round(h / a, 3))
        print(f"{op:28s} ours {a:8.3f} ms (C entry {c:7.3f} ms)   torch {b:8.3f} ms (x{b / a:6.2f})   numpy + transfers {h:8.3f} ms "
              f"(x{h / a:6.2f})", flush=True)
    print(json.dumps({"d": D, "frac": FRAC, "graph": [n, e], "results": results}))


if __name__ == "__main__":
    main()
