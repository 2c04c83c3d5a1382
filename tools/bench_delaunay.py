"""Time the Delaunay builder (ngpde_amd.mesh: delaunay_graph, delaunay_triangles) next to the way users get the tutorial's kind of
graph today:

    scipy   scipy.spatial.Delaunay on the host (one triangulation per graph), INCLUDING the transfers: points down, then the
            bidirected edge list (edges of the simplices, both directions, unique) or the simplices up

on two workloads:

    cloud   the bench cloud, 16 384 scattered points in the unit square
    batch   24 clouds of 3 000 points, every cloud triangulated by itself

    python tools/bench_delaunay.py [--reps 10]

Two figures per workload, wall clock between device synchronisations (both entries read their counts back and cannot be replayed
from a HIP graph): the graph and the triangles.  The median of `reps` after warm-up.  Also printed: the share of points that take
the second pass (ngpde_delaunay_last_passes), the degree histogram, and whether the edge set equals scipy's.  One JSON line at the
end holds every result.
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
    from scipy.spatial import Delaunay
except ImportError:
    Delaunay = None


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
    gen = torch.Generator(device=dev).manual_seed(1)
    cloud = torch.rand(2, 16384, device=dev, generator=gen)
    batch = torch.rand(2, 24 * 3000, device=dev, generator=gen)
    gi = torch.arange(1, 25, device=dev).repeat_interleave(3000)
    return {"cloud": (cloud, None, 1), "batch": (batch, gi, 24)}


def scipy_edges(pts, gi, graphs, dev, triangles):
    """host triangulation with its transfers; returns the device result"""
    p = pts.T.cpu().numpy().astype(np.float64)
    ids = None if gi is None else gi.cpu().numpy()
    out = []
    for g in range(graphs):
        sel = np.arange(len(p)) if ids is None else np.flatnonzero(ids == g + 1)
        s = sel[Delaunay(p[sel]).simplices]
        if triangles:
            out.append(s)
        else:
            e = np.concatenate([s[:, [0, 1]], s[:, [1, 2]], s[:, [2, 0]]])
            out.append(np.unique(np.concatenate([e, e[:, ::-1]]), axis=0))
    return torch.as_tensor(np.concatenate(out), device=dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = _lib.load()
    results = {}
    for name, (pts, gi, graphs) in workloads(dev).items():
        n = pts.shape[1]
        graph = lambda: ng.mesh.delaunay_graph(pts, graph_indicator=gi)
        tris = lambda: ng.mesh.delaunay_triangles(pts, graph_indicator=gi)
        g = graph()
        lane, wave = C.c_int64(0), C.c_int64(0)
        lib.ngpde_delaunay_last_passes(C.byref(lane), C.byref(wave))
        deg = np.bincount(g._t0, minlength=n)
        row = {"points": n, "graphs": graphs, "edges": int(g.num_edges), "triangles": int(tris().shape[0]),
               "second_pass_share": wave.value / n, "max_degree": int(deg.max()), "degree_histogram": np.bincount(deg).tolist()}
        # the entry alone, without the host copy of the lists that a GNNGraph keeps
        p32 = pts.T.contiguous()
        ids = None if gi is None else gi.to(torch.int32)
        cap = 6 * n + 64
        s, t = torch.empty(cap, dtype=torch.int32, device=dev), torch.empty(cap, dtype=torch.int32, device=dev)
        cnt = C.c_int64(0)
        entry = lambda: _lib.check(lib.ngpde_delaunay_graph(n, _lib.ptr(p32), _lib.ptr(ids), graphs, 1, float("inf"), 0, 0, cap, _lib.ptr(s),
                                                            _lib.ptr(t), C.byref(cnt), None))
        row["graph"] = {"entry_ms": round(wall_ms(entry, args.reps), 4), "ms": round(wall_ms(graph, args.reps), 4), "scipy_ms": None}
        row["triangles_"] = {"ms": round(wall_ms(tris, args.reps), 4), "scipy_ms": None}
        if Delaunay is not None:
            row["graph"]["scipy_ms"] = round(wall_ms(lambda: scipy_edges(pts, gi, graphs, dev, False), max(2, args.reps // 3), 1), 4)
            row["triangles_"]["scipy_ms"] = round(wall_ms(lambda: scipy_edges(pts, gi, graphs, dev, True), max(2, args.reps // 3), 1), 4)
            ref = scipy_edges(pts, gi, graphs, dev, False).cpu().numpy()
            ours = np.stack([g._t0, g._s0], 1)
            row["equals_scipy"] = bool(ref.shape == ours.shape and (ref == ours).all())
        results[name] = row
        fmt = lambda v: "     n/a" if v is None else f"{v:8.4f}"
        print(f"{name:6s} {n} points, {graphs} graph(s): {row['edges']} directed edges, {row['triangles']} triangles, "
              f"second pass {100 * row['second_pass_share']:.2f} % of the points, largest degree {row['max_degree']}, equals scipy: "
              f"{row.get('equals_scipy')}")
        print(f"{name:6s} graph       ours {fmt(row['graph']['ms'])} ms (entry alone {fmt(row['graph']['entry_ms'])} ms)   "
              f"scipy + transfers {fmt(row['graph']['scipy_ms'])} ms")
        print(f"{name:6s} triangles   ours {fmt(row['triangles_']['ms'])} ms                                 "
              f"scipy + transfers {fmt(row['triangles_']['scipy_ms'])} ms")
    print(json.dumps({"results": results}))


if __name__ == "__main__":
    main()
