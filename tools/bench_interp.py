"""Time the two-set search and the k-NN interpolation (ngpde_amd.interp: knn, KNNInterpolator) next to two baselines:

    torch   the composition users write today on the GPU: torch.cdist + topk for the search (an M x N matrix; per graph for the
            batch), inverse-squared-distance weights and a gather x[:, idx] for the interpolation, autograd for its pullback
    scipy   scipy.spatial.cKDTree on the host (one tree per graph), INCLUDING the transfers: points and queries down, idx and d2 up;
            the interpolation with numpy on the host, x down and y up

on two workloads with D = 64 features and k = 3:

    grid    the bench cloud, 16 384 scattered points in the unit square, onto a regular 256 x 256 grid (65 536 queries)
    batch   24 clouds of 3 000 points onto 24 x 4 096 queries, every query searched in its own cloud

    python tools/bench_interp.py [--reps 20]

Three figures per workload: the search (wall clock between device synchronisations: the entry reads its counts back), one
interpolation y = itp(x), and forward plus backward.  The library's interpolation launches allocate nothing and read nothing back, so
they are ALSO timed as HIP-graph replays (`graph_ms`: 20 launches captured into one graph, per launch), as the other tools do; the torch
columns are eager wall-clock.  The median of `reps` after warm-up.  A baseline this build cannot run is reported as null.  One JSON line
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
from ngpde_amd import _lib                   # noqa: E402

try:
    from scipy.spatial import cKDTree
except ImportError:
    cKDTree = None

D, K = 64, 3


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


def graph_ms(fn, reps, per_graph=20):
    """per-launch time of `fn` replayed from a HIP graph that holds it `per_graph` times"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per_graph):
            fn()
    return wall_ms(g.replay, reps) / per_graph


def workloads(dev):
    gen = torch.Generator(device=dev).manual_seed(1)
    pts = torch.rand(2, 16384, device=dev, generator=gen)
    c = (torch.arange(256, device=dev, dtype=torch.float32) + 0.5) / 256
    qs = torch.stack(torch.meshgrid(c, c, indexing="ij")).reshape(2, -1)
    yield "grid", pts, qs, None, None, 1
    pts = torch.rand(2, 24 * 3000, device=dev, generator=gen)
    qs = torch.rand(2, 24 * 4096, device=dev, generator=gen)
    yield "batch", pts, qs, torch.arange(24, device=dev).repeat_interleave(3000) + 1, torch.arange(24, device=dev).repeat_interleave(4096) + 1, 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_interp.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    results = {}
    for name, pts, qs, gp, gq, n_graphs in workloads(dev):
        n, m = pts.shape[1], qs.shape[1]
        kw = {} if gp is None else dict(graph_indicator=gp, query_graph_indicator=gq)
        x = torch.randn(D, n, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        ybar = torch.randn(D, m, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
        itp = ng.interp.KNNInterpolator(pts, qs, K, **kw)
        ptr, slot = itp.transpose()

        # ---- torch: cdist + topk (+ gather)
        P, Q = pts.T.reshape(n_graphs, n // n_graphs, 2), qs.T.reshape(n_graphs, m // n_graphs, 2)
        base = (torch.arange(n_graphs, device=dev) * (n // n_graphs)).view(-1, 1, 1)

        def search_torch():
            d, i = torch.cdist(Q, P).topk(K, dim=2, largest=False)
            return (i + base).reshape(m, K), (d * d).reshape(m, K)

        # (the lists the torch and host interpolations use come from differences squared and summed directly, a block of queries at a
        # time: cdist's default forms large problems from a matrix product, whose distances are too coarse to compare with, and its exact
        # mode's launch does not take these sizes; the timed search is the default a user would call)
        rows = max(1, (1 << 24) // n)
        parts = [((Q[:, a:a + rows, None, :] - P[:, None, :, :]) ** 2).sum(-1).topk(K, dim=2, largest=False) for a in range(0, Q.shape[1], rows)]
        d2, i = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
        t_idx, t_d2 = (i + base).reshape(m, K), d2.reshape(m, K)
        del d2, i, parts

        def weights_torch():
            w = 1.0 / t_d2.clamp(min=1e-16)
            return w / w.sum(1, keepdim=True)

        t_w = weights_torch()

        def interp_torch(xx):
            return (xx[:, t_idx] * t_w).sum(2)

        def both_torch():
            xx = x.detach().requires_grad_(True)
            interp_torch(xx).backward(ybar)
            return xx.grad

        # ---- scipy on the host, transfers included
        def search_host():
            hp, hq = pts.T.cpu().numpy(), qs.T.cpu().numpy()
            idx, d2 = np.empty((m, K), np.int64), np.empty((m, K), np.float32)
            for g in range(n_graphs):
                a, b = slice(g * (n // n_graphs), (g + 1) * (n // n_graphs)), slice(g * (m // n_graphs), (g + 1) * (m // n_graphs))
                d, i = cKDTree(hp[a]).query(hq[b], k=K)
                idx[b], d2[b] = i.reshape(-1, K) + a.start, (d * d).reshape(-1, K)
            return torch.as_tensor(idx, device=dev), torch.as_tensor(d2, device=dev)

        h_idx, h_w = t_idx.cpu().numpy(), t_w.cpu().numpy()

        def interp_host():
            hx = x.cpu().numpy()
            return torch.as_tensor((hx[:, h_idx] * h_w).sum(2), device=dev)

        def both_host():
            y = interp_host()
            hy = ybar.cpu().numpy()
            xb = np.zeros((D, n), np.float32)
            for j in range(K):
                np.add.at(xb.T, h_idx[:, j], (hy * h_w[:, j]).T)
            return y, torch.as_tensor(xb, device=dev)

        # ---- the library's launches on fixed buffers, for the graph replays
        xr, yb = x.T.contiguous(), ybar.T.contiguous()
        y_out, xbar_out = torch.empty(m, D, device=dev), torch.empty(n, D, device=dev)
        P_ = _lib.ptr

        def fwd_launch():
            _lib.check(lib.ngpde_knn_interp_forward(n, m, K, D, P_(itp._idx), P_(itp._w), P_(xr), P_(y_out), _lib.current_stream()))

        def both_launch():
            fwd_launch()
            _lib.check(lib.ngpde_knn_interp_backward(n, m, K, D, P_(ptr), P_(slot), P_(itp._w), P_(yb), P_(xbar_out), _lib.current_stream()))

        def both_ours():
            xx = x.detach().requires_grad_(True)
            itp(xx).backward(ybar)
            return xx.grad

        # the compositions do the library's work (ties may be cut differently: compare distances and values, not positions)
        assert torch.allclose(itp.d2.T, t_d2, rtol=1e-3, atol=1e-7)
        assert torch.allclose(itp(x), interp_torch(x), rtol=1e-3, atol=1e-3)

        ops = {
            "search": (lambda: ng.interp.knn(pts, qs, K, **kw), None, search_torch, search_host),
            "interpolate": (lambda: itp(x), fwd_launch, lambda: interp_torch(x), interp_host),
            "forward + backward": (both_ours, both_launch, both_torch, both_host),
        }
        results[name] = {"points": n, "queries": m, "graphs": n_graphs}
        for op, (f_ours, f_launch, f_torch, f_host) in ops.items():
            row = {"ms": round(wall_ms(f_ours, args.reps), 4), "graph_ms": None if f_launch is None else round(graph_ms(f_launch, args.reps), 4)}
            for col, f in (("torch_ms", f_torch), ("scipy_ms", f_host)):
                try:
                    if col == "scipy_ms" and cKDTree is None and op == "search":
                        raise ImportError("scipy")
                    row[col] = round(wall_ms(f, min(args.reps, 5) if col == "scipy_ms" else args.reps, warm=1), 4)
                except Exception as err:          # (a baseline this build cannot run)
                    row[col] = None
                    print(f"  {name} {op} {col}: {type(err).__name__}: {str(err)[:120]}", flush=True)
            results[name][op] = row
            fmt = lambda v: "     n/a" if v is None else f"{v:9.4f}"
            print(f"{name:6s} {op:20s} ours {fmt(row['ms'])} ms (graph replay {fmt(row['graph_ms'])} ms)   torch {fmt(row['torch_ms'])} ms   "
                  f"scipy + transfers {fmt(row['scipy_ms'])} ms", flush=True)
    print(json.dumps({"d": D, "k": K, "results": results}))


if __name__ == "__main__":
    main()
