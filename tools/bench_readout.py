"""Time the per-graph readouts (ngpde_amd.reduce_nodes("mean") / softmax_nodes / broadcast_nodes), forward and forward + backward,
next to the same operation composed from torch ops (index_add_ / scatter_reduce / index_select / exp / div), on four shapes at d = 64:

    bench    one graph of 16 384 nodes (bench.py's C2 graph size)
    vmh      a batch of 24 graphs of 3 000 nodes (the README's VMH minibatch)
    small    a batch of 256 graphs of 64 nodes
    hbm      one graph of 4 194 304 nodes: 1 GiB per array, past the 256 MiB Infinity Cache

    python tools/bench_readout.py [--reps 200] [--shapes bench,vmh,small,hbm]

Every figure is device time per call from events around replays of a captured HIP graph (no Python / autograd dispatch in the
window), after warm-up.  `bytes` is the least traffic the operation needs (each array read or written once, the int32 segment ids
of the item-wise passes included); `frac_hbm` = bytes / 8 TB/s over the measured time (the spec peak, as bench_propagate.py), and
`frac_copy` = the same against the ~6.3 TB/s a float4 copy reaches.
`launches` counts the library's kernel launches per call.  The torch composition is timed the same way in the same process; `ok` says
the library was no slower.  One JSON line at the end holds every result.
"""
import argparse
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ngpde_amd as ng                       # noqa: E402
from ngpde_amd import readout as RO          # noqa: E402

D = 64
HBM_PEAK = 8.0e12
COPY_PEAK = 6.3e12
SHAPES = {"bench": (1, 16384), "vmh": (24, 3000), "small": (256, 64), "hbm": (1, 4194304)}


def time_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def graph_ms(fn, reps):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    gc_was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(gr):
            fn()
    finally:
        if gc_was:
            gc.enable()
    return time_ms(gr.replay, reps)


def edgeless_batch(n_graphs, n_nodes):
    """the readouts of nodes need no edges: a batch of edgeless members (the indicator is what batch() records)"""
    n = n_graphs * n_nodes
    gi = np.repeat(np.arange(n_graphs, dtype=np.int32), n_nodes)
    return ng.GNNGraph([], [], num_nodes=n, index_base=0, graph_indicator=gi if n_graphs > 1 else None, num_graphs=n_graphs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--shapes", default="bench,vmh,small,hbm")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_readout.py measures on the MI355X"
    dev = "cuda"
    results, plans = {}, {}

    for shape in args.shapes.split(","):
        S, per = SHAPES[shape]
        g = edgeless_batch(S, per)
        N = g.num_nodes
        reps = max(10, args.reps // 10) if shape == "hbm" else args.reps
        gen = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(N, D, device=dev, generator=gen).T.detach().requires_grad_(True)       # (D x N) views of [N][D] rows
        u = torch.randn(S, D, device=dev, generator=gen).T.detach().requires_grad_(True)
        dS = torch.randn(S, D, device=dev, generator=gen).T
        dN = torch.randn(N, D, device=dev, generator=gen).T
        gi = torch.zeros(N, dtype=torch.int64, device=dev) if S == 1 else torch.as_tensor(g.graph_indicator.astype(np.int64), device=dev)
        gi2 = gi[:, None].expand(N, D)
        count = torch.bincount(gi, minlength=S).clamp(min=1).to(torch.float32)[:, None]
        info = RO._plan(g, "nodes", x.device).info()
        single = all(0 < c <= info["chunk_rows"] for c in np.bincount(gi.cpu().numpy(), minlength=S))
        plans[shape] = dict(info, single_chunk_segments=single)
        rows, stat = 4 * N * D, 4 * S * D

        def report(name, ours, torch_ms, nbytes, launches):
            key = f"{shape} {name}"
            results[key] = dict(ms=round(ours, 5), torch_ms=round(torch_ms, 5), speedup_vs_torch=round(torch_ms / ours, 3),
                                ok=bool(ours <= torch_ms), bytes=int(nbytes), frac_hbm=round(nbytes / HBM_PEAK / (ours * 1e-3), 3),
                                frac_copy=round(nbytes / COPY_PEAK / (ours * 1e-3), 3), launches=launches)
            print(f"{key:34s} ours {ours * 1e3:9.2f} us   torch {torch_ms * 1e3:9.2f} us   x{torch_ms / ours:7.2f}   "
                  f"{nbytes / 1e6:8.1f} MB  {results[key]['frac_hbm']:.3f} of HBM peak, {results[key]['frac_copy']:.3f} of a copy   {launches} launches", flush=True)

        # ---- reduce_nodes("mean") -----------------------------------------------------------------------------------------
        def mean_torch(xr):
            return torch.zeros(S, D, device=dev).index_add(0, gi, xr) / count

        def red_fwd():
            with torch.no_grad():
                return ng.reduce_nodes("mean", g, x)

        def red_fwd_torch():
            with torch.no_grad():
                return mean_torch(x.T).T

        def red_fb():
            torch.autograd.backward([ng.reduce_nodes("mean", g, x)], [dS], inputs=[x])

        def red_fb_torch():
            torch.autograd.backward([mean_torch(x.T).T], [dS], inputs=[x])

        ref, ours = red_fwd_torch(), red_fwd()
        assert torch.allclose(ours, ref, rtol=1e-3, atol=1e-4), float((ours - ref).abs().max())
        n_red = 1 if single else 2
        report("mean fwd", graph_ms(red_fwd, reps), graph_ms(red_fwd_torch, reps), rows + stat, n_red)
        report("mean fwd+bwd", graph_ms(red_fb, reps), graph_ms(red_fb_torch, reps), (rows + stat) + (stat + rows + 4 * N), n_red + 1)

        # ---- softmax_nodes ----------------------------------------------------------------------------------------------------
        def softmax_torch(xr):
            mx = torch.full((S, D), -float("inf"), device=dev).scatter_reduce(0, gi2, xr, "amax", include_self=True)
            z = torch.exp(xr - mx.index_select(0, gi))
            return z / torch.zeros(S, D, device=dev).index_add(0, gi, z).index_select(0, gi)

        def soft_fwd():
            with torch.no_grad():
                return ng.softmax_nodes(g, x)

        def soft_fwd_torch():
            with torch.no_grad():
                return softmax_torch(x.T).T

        def soft_fb():
            torch.autograd.backward([ng.softmax_nodes(g, x)], [dN], inputs=[x])

        def soft_fb_torch():
            torch.autograd.backward([softmax_torch(x.T).T], [dN], inputs=[x])

        ref, ours = soft_fwd_torch(), soft_fwd()
        assert torch.allclose(ours, ref, rtol=1e-3, atol=1e-7), float((ours - ref).abs().max())
        n_soft = 2 if single else 3
        soft_fwd_bytes = 3 * rows + 4 * N            # x read twice, y written, the segment ids
        report("softmax fwd", graph_ms(soft_fwd, reps), graph_ms(soft_fwd_torch, reps), soft_fwd_bytes, n_soft)
        report("softmax fwd+bwd", graph_ms(soft_fb, reps), graph_ms(soft_fb_torch, reps), soft_fwd_bytes + 5 * rows + 4 * N, 2 * n_soft)

        # ---- broadcast_nodes ----------------------------------------------------------------------------------------------------
        def bc_fwd():
            with torch.no_grad():
                return ng.broadcast_nodes(g, u)

        def bc_fwd_torch():
            with torch.no_grad():
                return u.T.index_select(0, gi).T

        def bc_fb():
            torch.autograd.backward([ng.broadcast_nodes(g, u)], [dN], inputs=[u])

        def bc_fb_torch():
            torch.autograd.backward([u.T.index_select(0, gi).T], [dN], inputs=[u])

        assert torch.equal(bc_fwd(), bc_fwd_torch())
        report("broadcast fwd", graph_ms(bc_fwd, reps), graph_ms(bc_fwd_torch, reps), rows + stat + 4 * N, 1)
        report("broadcast fwd+bwd", graph_ms(bc_fb, reps), graph_ms(bc_fb_torch, reps), 2 * rows + 2 * stat + 4 * N, 1 + n_red)

        del x, u, dS, dN, gi, gi2, g
        gc.collect()
        torch.cuda.empty_cache()

    print(json.dumps({"d": D, "hbm_peak_Bps": HBM_PEAK, "copy_Bps": COPY_PEAK, "plans": plans, "gate_ok": all(r["ok"] for r in results.values()),
                      "results": results}))


if __name__ == "__main__":
    main()
