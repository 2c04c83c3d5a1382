"""Time the public message-passing kernels (ngpde_amd.propagate / softmax_edge_neighbors and the gather under a user message) on the
benchmark graph -- bench.py's C2 graph: 16 384 nodes, 131 072 edges (65 536 closest pairs, both directions), d = 64 -- next to the same
operation composed from torch ops, and next to the HBM-bound fraction of a stated byte count.

    python tools/bench_propagate.py [--reps 200]

Every figure is device time per call from events around replays of a captured HIP graph (no Python / autograd dispatch in the
window), after warm-up.  `bytes` is the least traffic the operation needs (each array read or written once, the int32 index arrays
included); `frac_hbm` = bytes / 8 TB/s over the measured time (the spec peak; a float4 copy reaches ~6.3 TB/s).  One JSON line at
the end holds every result.
"""
import argparse
import gc
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ngpde_amd as ng                       # noqa: E402
from ngpde_amd import msgpass as MP          # noqa: E402
from ngpde_amd import synth as S             # noqa: E402

N_NODES, N_PAIRS, D, GRAPH_SEED = 16384, 65536, 64, 2
HBM_PEAK = 8.0e12


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_propagate.py measures on the MI355X"
    dev = "cuda"
    _, s, t = S.closest_pairs_graph(N_NODES, N_PAIRS, seed=GRAPH_SEED)
    g = ng.GNNGraph(s, t, num_nodes=N_NODES, index_base=0)
    N, E = g.num_nodes, g.num_edges
    si = torch.as_tensor(s, dtype=torch.int64, device=dev)
    ti = torch.as_tensor(t, dtype=torch.int64, device=dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(N, D, device=dev, generator=gen).T.detach().requires_grad_(True)   # (D x N) views of [N][D] rows, as the layers take
    eD = torch.randn(E, D, device=dev, generator=gen).T.detach().requires_grad_(True)
    dout = torch.randn(N, D, device=dev, generator=gen).T
    dxe = torch.randn(E, D, device=dev, generator=gen).T
    idx_bytes = 4 * (N + 1) + 8 * E                                            # rowptr + col + eid of one direction
    results = {}

    def report(name, ours, torch_ms, nbytes):
        results[name] = dict(ms=round(ours, 5), torch_ms=round(torch_ms, 5), speedup_vs_torch=round(torch_ms / ours, 3),
                             bytes=int(nbytes), frac_hbm=round(nbytes / HBM_PEAK / (ours * 1e-3), 3))
        print(f"{name:34s} ours {ours * 1e3:9.2f} us   torch {torch_ms * 1e3:9.2f} us   x{torch_ms / ours:6.2f}   "
              f"{nbytes / 1e6:7.1f} MB  {results[name]['frac_hbm']:.3f} of HBM peak", flush=True)

    # ---- K2: propagate(e_mul_xj, g, +; xj = x, e) with e of width D --------------------------------------------------------
    def k2_fwd():
        with torch.no_grad():
            return ng.propagate(ng.e_mul_xj, g, "+", xj=x, e=eD)

    def k2_fwd_torch():
        with torch.no_grad():
            return torch.zeros(N, D, device=dev).index_add_(0, ti, eD.T * x.T.index_select(0, si)).T

    ref, ours = k2_fwd_torch(), k2_fwd()
    assert torch.allclose(ours, ref, rtol=1e-4, atol=1e-4), float((ours - ref).abs().max())
    fwd_bytes = 4 * E * D + 2 * 4 * N * D + idx_bytes
    report("K2 e_mul_xj + fwd", graph_ms(k2_fwd, args.reps), graph_ms(k2_fwd_torch, args.reps), fwd_bytes)

    def k2_fb():
        y = ng.propagate(ng.e_mul_xj, g, "+", xj=x, e=eD)
        torch.autograd.backward([y], [dout], inputs=[x, eD])

    def k2_fb_torch():
        y = torch.zeros(N, D, device=dev).index_add(0, ti, eD.T * x.T.index_select(0, si)).T
        torch.autograd.backward([y], [dout], inputs=[x, eD])

    # pullback: e, dout, x read and dx, de written, plus the by-source index arrays and the targets' row pointers
    bwd_bytes = 2 * 4 * E * D + 3 * 4 * N * D + idx_bytes + 4 * (N + 1)
    report("K2 e_mul_xj + fwd+bwd", graph_ms(k2_fb, args.reps), graph_ms(k2_fb_torch, args.reps), fwd_bytes + bwd_bytes)

    # ---- K1: the gather of a user message (xi = x at the targets, xj = x at the sources) and its pullback ---------------------
    def k1_fb():
        xi, xj = MP._gather(g, g.handle(), x, x)
        torch.autograd.backward([xi, xj], [dxe, dxe], inputs=[x])

    def k1_fb_torch():
        xr = x.T
        xi, xj = xr.index_select(0, ti).T, xr.index_select(0, si).T
        torch.autograd.backward([xi, xj], [dxe, dxe], inputs=[x])

    k1_bytes = (4 * N * D + 2 * 4 * E * D + idx_bytes) + (2 * 4 * E * D + 4 * N * D + 4 * (2 * N + 2) + 4 * E)
    report("K1 gather xi,xj fwd+bwd", graph_ms(k1_fb, args.reps), graph_ms(k1_fb_torch, args.reps), k1_bytes)

    # ---- K4: softmax_edge_neighbors with H heads ------------------------------------------------------------------------------
    for H in (4, 64):
        e = torch.randn(E, H, device=dev, generator=gen).T.detach().requires_grad_(True)
        dy = torch.randn(E, H, device=dev, generator=gen).T

        def k4_fb():
            y = ng.softmax_edge_neighbors(g, e)
            torch.autograd.backward([y], [dy], inputs=[e])

        def k4_torch(er):
            mx = torch.full((N, H), -float("inf"), device=dev).scatter_reduce(0, ti[:, None].expand(E, H), er, "amax", include_self=True)
            z = torch.exp(er - mx.index_select(0, ti))
            return z / torch.zeros(N, H, device=dev).index_add(0, ti, z).index_select(0, ti)

        def k4_fb_torch():
            y = k4_torch(e.T).T
            torch.autograd.backward([y], [dy], inputs=[e])

        with torch.no_grad():
            ref, ours = k4_torch(e.T).T, ng.softmax_edge_neighbors(g, e)
        assert torch.allclose(ours, ref, rtol=1e-4, atol=1e-6), float((ours - ref).abs().max())
        k4_bytes = 5 * 4 * E * H + 2 * (4 * (N + 1) + 4 * E)
        report(f"K4 softmax H={H} fwd+bwd", graph_ms(k4_fb, args.reps), graph_ms(k4_fb_torch, args.reps), k4_bytes)

    print(json.dumps({"graph": dict(nodes=N, edges=E, d=D), "hbm_peak_Bps": HBM_PEAK, "results": results}))


if __name__ == "__main__":
    main()
