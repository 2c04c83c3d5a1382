"""saveat in adaptive Tsit5: landing on the save points (the scalar default) against Tsit5's dense output (interpolate_saveat=True),
on the generic path.  Two shapes: the Cora tutorial's right-hand side (2 x GCNConv(16 => 16, relu) on 2 708 nodes, reltol = abstol =
1e-3) with 100 save points, and a VMHConv cloud of the VMH tutorial's shape (VMH.md:75-87: 3 000 points, reltol = 1e-9, abstol = 1e-3)
with saveat = 0.005.  Per case and mode: naccept, nf, wall ms of the solve and of solve + backward.  One JSON line each.

    python tools/time_dense_output.py [--reps 5]
    python tools/time_dense_output.py --kernels      # the kernels alone, for `rocprofv3 --kernel-trace --stats`: per (count, M)
                                                     # one ngpde_rk_dense_output, one pullback and M rk_combine_kernel launches
Needs the MI355X.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ngpde_amd as ng  # noqa: E402
from ngpde_amd import node as NODE, synth as S  # noqa: E402
from time_adaptive_node import DEV, leaves, timed  # noqa: E402


def case(name, model, ps, st, u0, tspan, saveat, reltol, abstol, reps):
    for mode in ("landing", "interpolating"):
        node = ng.NeuralODE(model, tspan=tspan, adaptive=True, saveat=saveat, reltol=reltol, abstol=abstol,
                            interpolate_saveat=(mode == "interpolating"))

        def solve():
            with torch.no_grad():
                node(u0, ps, st)

        def solve_backward():
            u = u0.clone().requires_grad_(True)
            y, _ = node(u, ps, st)
            y.sum().backward()
        ms_s = timed(solve, reps)
        ms_b = timed(solve_backward, reps)
        s = node.stats
        print(json.dumps(dict(case=name, mode=mode, saves=int(round((tspan[1] - tspan[0]) / saveat)) + 1, naccept=s["naccept"],
                              nreject=s["nreject"], nf=s["nf"], ninterp=s.get("ninterp", 0), solve_ms=round(ms_s, 3),
                              solve_backward_ms=round(ms_b, 3))), flush=True)


def kernels():
    gen = torch.Generator().manual_seed(0)
    for count in (2708 * 16, 1 << 22):
        u = torch.randn(count, generator=gen).to(DEV)
        ks = [torch.randn(count, generator=gen).to(DEV) for _ in range(7)]
        for m in (1, 4, 8, 16):
            rows = [[0.01 * (i + j + 1) for i in range(7)] for j in range(m)]
            outs = [torch.empty_like(u) for _ in range(m)]
            for _ in range(20):
                NODE._dense_output(u, ks, rows, outs)
                NODE._dense_output_pullback(outs, rows, 7, u)
                for j in range(m):
                    NODE._combine(u, 1.0, ks, rows[j], out=outs[j])
            torch.cuda.synchronize()
            print(json.dumps(dict(count=count, m=m, forward_bytes=(8 + m) * 4 * count, pullback_bytes=(m + 9) * 4 * count,
                                  combines_bytes=9 * m * 4 * count)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    if args.kernels:
        kernels()
        return
    torch.manual_seed(0)
    N, D = 2708, 16
    s, t = S.preferential_pairs_graph(N, 5278, seed=1)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    model = ng.Chain(ng.GCNConv((D, D), "relu", initialgraph=g), ng.GCNConv((D, D), "relu", initialgraph=g))
    ps, st = ng.setup(1, model)
    ps = ng.to_device(ps, DEV)
    for v in leaves(ps):
        v.requires_grad_(True)
    u0 = torch.as_tensor(S.normal(2, D * N).reshape(D, N).astype(np.float32), device=DEV)
    case("cora_gcn2_16", model, ps, st, u0, (0.0, 1.0), 0.01, 1e-3, 1e-3, args.reps)
    nv = 3000
    pts = torch.as_tensor(S.uniform01(41, 2 * nv).reshape(2, nv).astype(np.float32), device=DEV)
    gv = ng.GNNGraph(ng.knn_graph(pts, 6), ndata={"x": pts})
    phi = ng.Chain(ng.Dense(4, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 40))
    gam = ng.Chain(ng.Dense(41, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 1))
    vm = ng.VMHConv(phi, gam, initialgraph=gv)
    ps, st = ng.setup(4, vm)
    ps = ng.to_device(ps, DEV)
    for v in leaves(ps):
        v.requires_grad_(True)
    u0 = torch.as_tensor(S.normal(42, nv).reshape(1, nv).astype(np.float32), device=DEV)
    case("vmh_3000", vm, ps, st, u0, (0.0, 0.5), 0.005, 1e-9, 1e-3, args.reps)


if __name__ == "__main__":
    main()
