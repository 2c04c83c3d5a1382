"""Wall time of an adaptive Tsit5 solve + backward on the generic path (NeuralODE(..., adaptive=True)) against the same model stepped
at a fixed size, with the same step count, through the same path -- the difference is the price of the per-attempt error pass and
read-back.  Two shapes: the Cora tutorial's right-hand side (docs/src/tutorials/graph_node.md:78-81: 2 x GCNConv(16 => 16, relu) on a
2 708-node graph, reltol = abstol = 1e-3) and a VMHConv cloud (VMH.md:75-87: 3 000 points, saveat, reltol = 1e-9, abstol = 1e-3).
Prints one JSON line per case.  Needs the MI355X.

    python tools/time_adaptive_node.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ngpde_amd as ng  # noqa: E402
from ngpde_amd import node as NODE, synth as S  # noqa: E402

DEV = "cuda:0"


def timed(fn, reps):
    fn()                                    # warm-up: workspaces, graph handles, code objects
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out)) * 1e3


def leaves(ps):
    out = []
    for v in ps.values():
        out += leaves(v) if isinstance(v, dict) else [v]
    return out


def case(name, model, ps, st, u0, tspan, saveat, reltol, abstol, reps):
    node = ng.NeuralODE(model, tspan=tspan, adaptive=True, saveat=saveat, reltol=reltol, abstol=abstol)

    def adaptive():
        u = u0.clone().requires_grad_(True)
        y, _ = node(u, ps, st)
        y.sum().backward()
    ms_a = timed(adaptive, reps)
    stats = dict(node.stats)
    n = stats["naccept"]
    fixed = ng.NeuralODE(model, tspan=tspan, n_steps=n)       # (u(T) only: copying the saved states out costs one launch per state)

    def fixed_step():                       # the generic path itself (the persistent plans would take the GCN chain otherwise)
        u = u0.clone().requires_grad_(True)
        y = NODE._NodeGenericFn.apply(ng.layers.rows_of(u), fixed, ps, st, *leaves(ps))
        y.sum().backward()
    ms_f = timed(fixed_step, reps)
    print(json.dumps(dict(case=name, adaptive_ms=round(ms_a, 3), fixed_same_steps_ms=round(ms_f, 3), naccept=n, nreject=stats["nreject"],
                          nf=stats["nf"], dt_min=min(stats["dts"]), dt_max=max(stats["dts"]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    torch.manual_seed(0)
    # Cora-shaped: 2 x GCNConv(16 => 16, relu)
    N, D = 2708, 16
    s, t = S.preferential_pairs_graph(N, 5278, seed=1)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    model = ng.Chain(ng.GCNConv((D, D), "relu", initialgraph=g), ng.GCNConv((D, D), "relu", initialgraph=g))
    ps, st = ng.setup(1, model)
    ps = ng.to_device(ps, DEV)
    for v in leaves(ps):
        v.requires_grad_(True)
    u0 = torch.as_tensor(S.normal(2, D * N).reshape(D, N).astype(np.float32), device=DEV)
    case("cora_gcn2_16", model, ps, st, u0, (0.0, 1.0), None, 1e-3, 1e-3, args.reps)
    # VMH-shaped: 3 000 points, 6 neighbours, the tutorial's phi / gamma
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
    case("vmh_3000", vm, ps, st, u0, (0.0, 0.5), 0.1, 1e-9, 1e-3, args.reps)


if __name__ == "__main__":
    main()
