"""Time the coarsening block (ngpde_amd.coarsen: fps, grid_cluster, pool) next to what a user composes today.

Farthest-point sampling at ratio 0.25, on two workloads in the unit square:

    cloud   the bench cloud, one graph of 16 384 points (4 096 rounds)
    batch   24 clouds of 3 000 points (750 rounds each, side by side)

    tile        the library's tile path (one workgroup per graph, every round inside one launch): the ngpde_fps call on a plan made once
    round       the library's round path on the same input (one launch per round), forced through the C entry's `path`
    public      ng.coarsen.fps(...) as a user calls it: indicator read-back, plan, workspace and the launches
    torch       the same rounds composed from torch ops on the GPU (min-distance update + argmax, the batch as one [24][3000] array)
    numpy       the same rounds in numpy on the host, INCLUDING the transfers (points down, idx up)
    torch_cluster   torch_cluster.fps if this build has it (random_start=False); null otherwise -- it is never installed from here

grid_cluster + pool (D = 64, "mean") on the same two workloads with cells of 1 / 32, against torch.unique(return_inverse) of the cell
keys + index_reduce_("mean") on the GPU.

    python tools/bench_coarsen.py [--reps 10]

Wall clock between device synchronisations, the median of `reps` after warm-up of every shape (the slow baselines take min(reps, 3)).
The two library paths are also compared for equal bits, and the torch composition for equal positions.  One JSON line at the end
holds every result.
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
from ngpde_amd import _lib                   # noqa: E402

try:
    from torch_cluster import fps as cluster_fps
except Exception:                            # (not on this box)
    cluster_fps = None

D, RATIO, CELL = 64, 0.25, 1.0 / 32


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


class Plan:
    """an ngpde_fps plan on fixed buffers: what a training loop that samples every step would hold"""

    def __init__(self, pts_rows, ptr, ks, path):
        self.lib = lib = _lib.load()
        self.pts = pts_rows
        gp, sp = np.asarray(ptr, np.int64), np.concatenate(([0], np.cumsum(ks))).astype(np.int64)
        self.plan = C.c_void_p()
        _lib.check(lib.ngpde_fps_plan_create(len(ks), _lib.ptr(gp), _lib.ptr(sp), 2, path, _lib.current_stream(), C.byref(self.plan)))
        self.nbytes = int(lib.ngpde_fps_workspace_bytes(self.plan))
        self.ws = torch.empty(max(self.nbytes, 1), dtype=torch.uint8, device=pts_rows.device)
        self.idx = torch.empty(int(sp[-1]), dtype=torch.int32, device=pts_rows.device)
        self.d2 = torch.empty(int(sp[-1]), dtype=torch.float32, device=pts_rows.device)
        info = (C.c_int64 * 6)()
        _lib.check(lib.ngpde_fps_plan_info(self.plan, info))
        self.info = list(info)

    def __call__(self):
        P = _lib.ptr
        _lib.check(self.lib.ngpde_fps(self.plan, P(self.pts), None, 0, P(self.idx), P(self.d2), P(self.ws), self.nbytes, _lib.current_stream()))
        return self.idx

    def close(self):
        self.lib.ngpde_fps_plan_destroy(self.plan)


def fps_torch(P, k):
    """P [G][n][2] on the device, k samples per graph: the rounds as torch ops"""
    G, n, _ = P.shape
    key = torch.full((G, n), float("inf"), device=P.device)
    idx = torch.empty((G, k), dtype=torch.int64, device=P.device)
    s = torch.zeros(G, dtype=torch.int64, device=P.device)
    rows = torch.arange(G, device=P.device)
    for r in range(k):
        idx[:, r] = s
        d = ((P - P[rows, s].unsqueeze(1)) ** 2).sum(-1)
        key = torch.minimum(key, d)
        key[rows, s] = -1.0
        s = key.argmax(dim=1)
    return idx


def fps_numpy(pts_dev, G, n, k, dev):
    hp = pts_dev.cpu().numpy().reshape(G, n, 2)
    out = np.empty((G, k), np.int64)
    for g in range(G):
        p = hp[g]
        key = np.full(n, np.inf, np.float32)
        s = 0
        for r in range(k):
            out[g, r] = s + g * n
            d = ((p - p[s]) ** 2).sum(-1)
            np.minimum(key, d, out=key)
            key[s] = -1
            s = int(key.argmax())
    return torch.as_tensor(out.reshape(-1), device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_coarsen.py measures on the MI355X"
    dev = torch.device("cuda", torch.cuda.current_device())
    slow = min(args.reps, 3)
    results = {}
    gen = torch.Generator(device=dev).manual_seed(1)
    for name, G, n in (("cloud", 1, 16384), ("batch", 24, 3000)):
        pts = torch.rand(2, G * n, device=dev, generator=gen)
        rows = pts.T.contiguous()
        gi = torch.arange(G, device=dev).repeat_interleave(n) + 1
        k = int(np.ceil(RATIO * n))
        ptr, ks = np.arange(G + 1) * n, [k] * G
        tile, rnd = Plan(rows, ptr, ks, 1), Plan(rows, ptr, ks, 2)
        a, b = tile().clone(), rnd().clone()
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(tile.d2, rnd.d2), "the two paths differ"
        t_idx = (fps_torch(rows.reshape(G, n, 2), k) + (torch.arange(G, device=dev) * n).unsqueeze(1)).reshape(-1)
        agree = float((t_idx == a).float().mean())                 # (torch's sum of squares may round a tie the other way)
        row = {"points": G * n, "graphs": G, "samples": G * k, "rounds": k, "tile_launches": tile.info[5], "round_launches": rnd.info[4],
               "torch_agrees": round(agree, 4)}
        row["tile_ms"] = round(wall_ms(tile, args.reps), 4)
        row["round_ms"] = round(wall_ms(rnd, args.reps), 4)
        row["public_ms"] = round(wall_ms(lambda: ng.coarsen.fps(pts, ratio=RATIO, graph_indicator=gi), args.reps), 4)
        row["torch_ms"] = round(wall_ms(lambda: fps_torch(rows.reshape(G, n, 2), k), slow, warm=1), 4)
        row["numpy_ms"] = round(wall_ms(lambda: fps_numpy(rows, G, n, k, dev), slow, warm=1), 4)
        row["torch_cluster_ms"] = None
        if cluster_fps is not None:
            try:
                row["torch_cluster_ms"] = round(wall_ms(lambda: cluster_fps(rows, gi - 1, ratio=RATIO, random_start=False), args.reps), 4)
            except Exception as err:
                print(f"  {name} torch_cluster: {type(err).__name__}: {str(err)[:120]}", flush=True)
        tile.close()
        rnd.close()
        fmt = lambda v: "     n/a" if v is None else f"{v:10.4f}"
        print(f"{name:6s} fps {G} x {n} -> {k} each: tile {fmt(row['tile_ms'])} ms   round {fmt(row['round_ms'])} ms   public {fmt(row['public_ms'])} ms   "
              f"torch {fmt(row['torch_ms'])} ms   numpy + transfers {fmt(row['numpy_ms'])} ms   torch_cluster {fmt(row['torch_cluster_ms'])} ms", flush=True)

        # ---- grid_cluster + pool against torch.unique + index_reduce_
        x = torch.randn(D, G * n, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        xr = x.T.contiguous()
        side = int(round(1 / CELL)) + 1

        def ours():
            cl = ng.coarsen.grid_cluster(pts, CELL, graph_indicator=gi, origin=[0.0, 0.0])
            return ng.coarsen.pool(cl, x, "mean")

        def composed():
            c = torch.floor(rows / CELL).long()
            key = ((gi - 1) * side + c[:, 1]) * side + c[:, 0]
            uniq, inv = torch.unique(key, return_inverse=True)
            out = torch.zeros(uniq.numel(), D, device=dev)
            return out.index_reduce_(0, inv, xr, "mean", include_self=False)

        mine, theirs = ours(), composed()
        assert mine.shape[1] == theirs.shape[0] and torch.allclose(mine.T, theirs, rtol=1e-4, atol=1e-5)
        cl = ng.coarsen.grid_cluster(pts, CELL, graph_indicator=gi, origin=[0.0, 0.0])
        row["clusters"] = cl.count
        row["cluster_pool_ms"] = round(wall_ms(ours, args.reps), 4)
        row["cluster_only_ms"] = round(wall_ms(lambda: ng.coarsen.grid_cluster(pts, CELL, graph_indicator=gi, origin=[0.0, 0.0]), args.reps), 4)
        row["pool_only_ms"] = round(wall_ms(lambda: ng.coarsen.pool(cl, x, "mean"), args.reps), 4)
        row["torch_unique_reduce_ms"] = round(wall_ms(composed, args.reps), 4)
        print(f"{name:6s} grid_cluster + pool ({cl.count} clusters, D = {D}): ours {fmt(row['cluster_pool_ms'])} ms (clusters {fmt(row['cluster_only_ms'])}, "
              f"pool {fmt(row['pool_only_ms'])})   torch.unique + index_reduce_ {fmt(row['torch_unique_reduce_ms'])} ms", flush=True)
        results[name] = row
    # ---- the two paths over the tile path's range: one graph of n points, n / 4 samples (where would auto have to switch?)
    sweep = []
    for n in (64, 256, 1024, 2048, 4096, 8192, 12288, 16384):
        rows = torch.rand(n, 2, device=dev, generator=gen)
        tile, rnd = Plan(rows, [0, n], [n // 4], 1), Plan(rows, [0, n], [n // 4], 2)
        sweep.append({"points": n, "samples": n // 4, "tile_ms": round(wall_ms(tile, args.reps), 4), "round_ms": round(wall_ms(rnd, args.reps), 4)})
        tile.close()
        rnd.close()
        print(f"one graph of {n:6d} points, {n // 4:5d} samples: tile {sweep[-1]['tile_ms']:9.4f} ms   round {sweep[-1]['round_ms']:9.4f} ms", flush=True)
    print(json.dumps({"d": D, "ratio": RATIO, "cell": CELL, "results": results, "paths": sweep}))


if __name__ == "__main__":
    main()
