"""In-kernel phase timestamps of the diagnostic build: where the cycles of a kernel's phases go.

    make -C neuralgraphpde.jl_amd/csrc diag [STAMPED="<sources>"]
    python3 tools/stamps.py FAMILY [args]

FAMILY (the source it needs stamped):
  gcn          fused GCN forward, one launch                          gcn_fused
  node         every GCN launch of two Tsit5 steps, forward + adjoint  gcn_fused
  persistent   persistent GCN solver, first PH phases (env GRAPH=cora)  node_persistent
               DUMP=1 saves the per-tile segments for tile_work.py as stamps_{fwd,bwd}.npy in the current directory
  interleaved  persistent solver, two members per workgroup            node_persistent
  tile-rounds  a turn of the pipelined tile-round forward (env N)      node_persistent
  vmh          device-resident VMH solver (env N, K, STEPS)             node_vmh
  gat          one-launch GAT layer forward                            gat_fused
  gat-node     device-resident GAT solver, last phase (env STEPS)      gat_fused
  pair         pair Dense forward, one steady-state tile               dense_mfma
  pair-bwd     pair Dense pullback, one steady-state tile, CU sharing   dense_stream_bwd
  small-dense  one-launch small Dense pullback (100 MHz wall clock)    dense_small_bwd
  edge         fused edge-MLP forward [traj] [act]                     edge_mlp_fused
  edge64       pipelined 64-wide message kernel [traj] [act]           edge_mlp64

Thread 0 of every workgroup stamps; shader-clock (s_memtime) cycles unless a table says otherwise.  The buffer's capacity goes to the
library with it (ngpde_debug_set_stamps), and the kernels write nothing past it.  The family numbers are stamps.h's StampFamily."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ngpde_amd as ng  # noqa: E402
from ngpde_amd import _lib, synth as S  # noqa: E402

_lib.LIB_PATH = os.path.join(ROOT, "neuralgraphpde.jl_amd", "libngpde_diag.so")
FAMILIES = ["gcn", "persistent", "vmh", "gat", "pair", "pair_bwd", "small_dense", "edge", "edge64"]
DEV = "cuda:0"
lib = None
p = _lib.ptr


class Stamps:
    """A device buffer of `words` 64-bit stamps for one family."""

    def __init__(self, family, words):
        self.family, self.buf = FAMILIES.index(family), torch.zeros(words, dtype=torch.int64, device=DEV)

    def on(self, n=0):   # n: launches to record (gcn) or phases per workgroup (persistent, vmh)
        self.buf.zero_()
        _lib.check(lib.ngpde_debug_set_stamps(self.family, p(self.buf), self.buf.numel(), n))

    def off(self):
        _lib.check(lib.ngpde_debug_set_stamps(self.family, None, 0, 0))

    def read(self, *shape):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy().reshape(*shape).astype(np.float64)


def table(title, d, names, unit="cycles"):
    """d[..., k]: phase k's samples; prints mean / median / p90 / max per phase."""
    d = d.reshape(-1, d.shape[-1])
    print(f"{title}: {d.shape[0]} samples, {unit} mean / median / p90 / max")
    for k, nm in enumerate(names):
        x = d[:, k]
        print(f"  {nm:52s} {x.mean():9.0f} {np.median(x):9.0f} {np.percentile(x, 90):9.0f} {x.max():9.0f}")


def used(a, k=0):
    """rows (workgroups) that wrote stamp k"""
    return a[a[..., k] > 0]


def c2_graph(n=16384, pairs=65536, seed=2):
    _, s, t = S.closest_pairs_graph(n, pairs, seed=seed)
    return ng.GNNGraph(s, t, num_nodes=n, index_base=0)


# ---- GCN: [launch][block][16], clock / wall pairs at 2k, 2k + 1, the forward's halo sub-phases at 10 .. 14

def gcn():
    N, D = 16384, 64
    h = c2_graph().handle((True, None, False))
    x = torch.randn(N, D, device=DEV); w = torch.randn(D, D, device=DEV) * 0.1; b = torch.zeros(D, device=DEV)
    y, agg = torch.empty_like(x), torch.empty_like(x)
    ws = torch.empty(1024, dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    fwd = lambda: _lib.check(lib.ngpde_gcn_forward(h.ptr, D, D, 1, p(x), p(w), p(b), p(y), p(agg), None, p(ws), ws.numel(), st))
    for _ in range(10):
        fwd()
    nb = (N + 31) // 32
    sb = Stamps("gcn", nb * 16)
    sb.on(1)
    fwd()
    a = sb.read(nb, 8, 2)
    clk, wall = a[:, :5, 0], a[:, :5, 1]
    table("fused forward, per workgroup", np.concatenate([np.diff(clk, axis=1), (clk[:, 4] - clk[:, 0])[:, None]], axis=1),
          ["W-issue+aggregate", "LDS stage+sync", "MFMA+sync", "epilogue", "WG total"])
    w0 = wall[:, 0].min()
    print("wall (100 MHz ticks = 10 ns): first WG start 0; last WG start", wall[:, 0].max() - w0, "; last WG end", wall[:, 4].max() - w0)
    for nm, v in (("start", wall[:, 0]), ("end  ", wall[:, 4])):
        v = np.sort(v - w0)
        print(f"WG {nm} quantiles (x10ns):", [int(v[int(q * (nb - 1))]) for q in (0, .25, .5, .75, .9, 1)])
    print("cycles per 10ns tick ~", np.median((clk[:, 4] - clk[:, 0]) / np.maximum(wall[:, 4] - wall[:, 0], 1)))


def node():
    N, D, STEPS = 16384, 64, 2
    from ngpde_amd.node import _Plan
    plan = _Plan(c2_graph().handle((True, None, False)), D, 1, "tsit5", STEPS, 0.02, True)
    u0 = torch.randn(N, D, device=DEV); w1 = torch.randn(D, D, device=DEV) * 0.1; w2 = torch.randn(D, D, device=DEV) * 0.1
    b1 = torch.zeros(D, device=DEV); b2 = torch.zeros(D, device=DEV)
    uT, du0, seed = torch.empty_like(u0), torch.empty_like(u0), torch.ones_like(u0)
    dw1, dw2, db1, db2 = torch.empty_like(w1), torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(b1)
    st = torch.cuda.current_stream().cuda_stream

    def solve():
        _lib.check(lib.ngpde_node_gcn2_forward(plan.ptr, p(u0), p(w1), p(b1), p(w2), p(b2), p(uT), st))
        _lib.check(lib.ngpde_node_gcn2_backward(plan.ptr, p(seed), p(du0), p(dw1), p(db1), p(dw2), p(db2), st))
    for _ in range(3):
        solve()
    nb = (N + 31) // 32
    nf = 2 * 6 * STEPS
    nl = nf + 1 + nf
    sb = Stamps("gcn", nl * nb * 16)
    sb.on(nl)
    solve()
    raw = sb.read(nl, nb, 16)
    a = raw.reshape(nl, nb, 8, 2)

    def report(name, idx, nph, labels):
        clk, wall = a[idx][:, :, :nph + 1, 0], a[idx][:, :, :nph + 1, 1]
        live = wall[0, :, 0] > 0                       # paired backward workgroups stamp only n_tiles / 2 slots
        clk, wall = clk[:, live], wall[:, live]
        dur = (wall[:, :, nph].max(axis=1) - wall[:, :, 0].min(axis=1)) * 10.0   # ns, kernel span by wall clock
        tot = clk[:, :, nph] - clk[:, :, 0]
        table(f"{name}: kernel span (first WG start -> last WG end) median {np.median(dur) / 1000:.2f} us over {len(idx)} launches",
              np.concatenate([np.diff(clk, axis=2), tot[:, :, None]], axis=2), labels + ["WG total"])
        print(f"  WG total {np.median((wall[:, :, nph] - wall[:, :, 0]) * 10.0):.0f} ns;  start skew "
              f"{np.median((wall[:, :, 0].max(axis=1) - wall[:, :, 0].min(axis=1)) * 10):.0f} ns")
    fwd1 = list(range(0, nf, 2))
    table("fwd layer1 halo aggregation sub-phases, cycles since WG start", raw[fwd1][:, :, 10:15] - raw[fwd1][:, :, :1],
          ["round-1 data arrived", "halo rows arrived", "LDS written", "barrier passed", "LDS aggregation done"])
    fl = ["sched+W issue+aggregate", "LDS stage+sync", "MFMA+sync", "epilogue"]
    report("fwd layer1", fwd1, 4, fl)
    report("fwd layer2+stage", list(range(1, nf, 2)), 4, fl)
    bl = ["sched+W issue+aggregate", "comb+mask+LDS stage+sync", "G MFMA+sync", "G rows out", "dW MFMA+db", "fold+slab store"]
    report("bwd layer1", list(range(nf + 1, nl - 1, 2)), 6, bl)
    report("bwd stage+layer2", list(range(nf + 2, nl - 1, 2)), 6, bl)


# ---- persistent solvers: [block][phase][8]

def gcn2_plan(n, pairs, members=1, steps=50, cora=False, seed=2):
    from ngpde_amd.node import _Plan
    D = 64
    if cora:
        s, t = S.preferential_pairs_graph(n, pairs, seed=1)
        g = ng.GNNGraph(s, t, num_nodes=n, index_base=0)
    else:
        g = c2_graph(n, pairs, seed)
    dv = lambda a: torch.as_tensor(np.ascontiguousarray(a, np.float32), device=DEV)
    u0 = dv(S.normal(1000, D * n * members).reshape(n * members, D))
    w1, w2 = dv(S.glorot_uniform(11, D, D).T), dv(S.glorot_uniform(12, D, D).T)
    b1, b2 = dv(np.zeros(D)), dv(np.zeros(D))
    plan = _Plan(g.handle((True, None, False)), D, _lib.ACT["relu"], "tsit5", steps, 1.0 / 50, True, members=members)
    outs = [torch.empty_like(u0), torch.empty_like(u0), torch.empty_like(w1), torch.empty_like(b1), torch.empty_like(w2), torch.empty_like(b2)]
    seed_ = torch.ones_like(u0)
    stream = torch.cuda.current_stream().cuda_stream

    def launch(which):
        if which == "fwd":
            _lib.check(lib.ngpde_node_gcn2_forward(plan.ptr, p(u0), p(w1), p(b1), p(w2), p(b2), p(outs[0]), stream))
        else:
            _lib.check(lib.ngpde_node_gcn2_backward(plan.ptr, p(seed_), p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]), p(outs[5]), stream))
    return plan, launch


def stamped_solve(launch, sb, ph, which, reps=3, kinds=("fwd", "bwd")):
    """the last of `reps` solves stamps the `which` launch"""
    for rep in range(reps):
        for k in kinds:
            if rep == reps - 1 and k == which:
                sb.on(ph)
            else:
                sb.off()
            launch(k)
        torch.cuda.synchronize()
    sb.off()


def persistent():
    cora = os.environ.get("GRAPH", "c2") == "cora"     # BASELINE config 1's shape (2 708 nodes with hubs: the hub geometry)
    N, PAIRS, STEPS, PH = (2708, 5278, 10, 100) if cora else (16384, 65536, 50, 240)
    plan, launch = gcn2_plan(N, PAIRS, steps=STEPS, cora=cora)
    NT = (N + 31) // 32
    sb = Stamps("persistent", NT * PH * 8)
    names = dict(fwd=["wait for the neighbours' flags", "gather foreign rows (LDS-DMA) + barrier", "LDS aggregation, tile write, barrier",
                      "MFMA + barrier", "epilogue + row stores issued", "drain + barrier + flag"],
                 bwd=["prefetch + wait for the flags", "gather foreign rows + barrier", "LDS aggregation, stage terms, tile writes, barrier",
                      "MFMA (G) + barrier", "row stores issued", "drain + barrier + flag", "dW / db products"])
    for which in ("fwd", "bwd"):
        stamped_solve(launch, sb, PH, which)
        st = sb.read(NT, PH, 8)
        nm = names[which]
        for parity, label in ((0, "odd phases (layer 1)"), (1, "even phases (layer 2 + stage terms)")):
            sel = st[:, 8 + parity:PH:2, :]
            table(f"{which} {label}", np.diff(sel[:, :, :len(nm) + 1], axis=2), nm)
            print(f"  two consecutive phases start-to-start: {(sel[:, 1:, 0] - sel[:, :-1, 0]).mean():.0f} cycles")
        per_tile = (st[:, PH - 1, 0] - st[:, 8, 0]) / (PH - 9)          # mean cycles per phase, tile by tile
        waits = np.diff(st[:, 8:, :2], axis=2)[:, :, 0].mean(axis=1)    # mean wait per tile
        order = np.argsort(waits)
        print(f"{which}: cycles per phase {per_tile.mean():.0f}; tiles waiting least (the ones waited for): " +
              ", ".join(f"tile {k}: wait {waits[k]:.0f}" for k in order[:6]))
        if os.environ.get("DUMP"):     # for tools/tile_work.py, in the current directory
            np.save(f"stamps_{which}.npy", np.diff(st[:, 8:, :len(nm) + 1], axis=2).mean(axis=1))
        k0 = int(order[0])
        d0 = np.diff(st[k0, 8:, :len(nm) + 1], axis=1).mean(axis=0)
        print(f"{which}: workgroup {k0} (waits least), mean cycles per step of a phase: " + "; ".join(f"{n}: {d0[k]:.0f}" for k, n in enumerate(nm)))
    print("flags", sorted(plan.flags()), "fault", plan.fault())


def interleaved():
    """Both slots stamp the same phase index, so what survives is slot 1's slot-phase: 0 top, 2 halo complete (T0: drain + barrier,
    or the blocking path), 3 operand tile written + T2 barrier, 4 matrix products + T4 (flags of the next slot-phase + barrier),
    5 epilogue, ahead-gather issued, row stores issued, 6 end.  Start-to-start of consecutive phases of one slot = two slot-phases."""
    N, PH, K = 16384, 240, 2
    plan, launch = gcn2_plan(N, 65536, members=K)
    NT = N // 32
    sb = Stamps("persistent", NT * PH * 8)
    pts = [(0, 2, "T0: drain + barrier (or blocking path)"), (2, 3, "aggregate + operand tile + T2"), (3, 4, "products + T4 (next flags, barrier)"),
           (4, 5, "epilogue + ahead-gather + stores issued"), (5, 6, "tail"), (0, 6, "whole slot-phase")]
    for which in ("fwd", "bwd"):
        stamped_solve(launch, sb, PH, which)
        st = sb.read(NT, PH, 8)
        for parity, label in ((0, "odd phases (layer 1)"), (1, "even phases (layer 2)")):
            sel = st[:, 8 + parity:PH:2, :]
            table(f"{which} slot 1, {label}", np.stack([sel[:, :, b] - sel[:, :, a] for a, b, _ in pts], axis=2), [n for _, _, n in pts])
            print(f"  four slot-phases start-to-start {(sel[:, 1:, 0] - sel[:, :-1, 0]).mean():.0f} cycles")
    print("flags", sorted(plan.flags()), "fault", plan.fault())


def tile_rounds():
    N = int(os.environ.get("N", 65536))
    TURNS, NW = 400, 512
    plan, launch = gcn2_plan(N, 4 * N, steps=10, seed=4)
    assert "tile_rounds" in plan.flags(), plan.flags()
    sb = Stamps("persistent", NW * TURNS * 8)
    stamped_solve(launch, sb, TURNS, "fwd", kinds=("fwd",))
    st = sb.read(NW, TURNS, 8)
    sel, nxt = st[:, 16:TURNS - 1, :], st[:, 17:TURNS, 0]
    d = np.diff(np.concatenate([sel[:, :, :7], nxt[:, :, None]], axis=2), axis=2)
    print(f"nodes {N}, flags {sorted(plan.flags())}")
    table("a turn of the tile-round forward", d, ["T0: vmcnt(0) + barrier (gather landed, stores drained)",
                                                  "publish + blocking path if the gather was not ahead", "poll issue + aggregation + barrier",
                                                  "next turn's DMA issue", "product + barrier", "epilogue, stores, next state loads",
                                                  "(loop overhead to the next turn)"])
    print(f"  turn start-to-start: {(nxt - sel[:, :, 0]).mean():.0f} cycles")


def vmh():
    nv, kv, steps = int(os.environ.get("N", 3000)), int(os.environ.get("K", 6)), int(os.environ.get("STEPS", 20))
    pts = torch.as_tensor(S.uniform01(41, 2 * nv).reshape(2, nv).astype(np.float32), device=DEV)
    gv = ng.GNNGraph(ng.knn_graph(pts, kv), ndata={"x": pts})
    phi = ng.Chain(ng.Dense(4, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 40))
    gam = ng.Chain(ng.Dense(41, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 60, "tanh"), ng.Dense(60, 1))
    u0 = torch.as_tensor(S.normal(42, nv).reshape(1, nv).astype(np.float32), device=DEV)
    nde = ng.NeuralODE(ng.VMHConv(phi, gam, initialgraph=gv), solver="tsit5", n_steps=steps, dt=0.2 / steps, capture=False)
    ps, st = ng.setup(4, nde)
    ps = ng.to_device(ps, DEV)

    def leaves(t):
        for v in t.values():
            yield from (leaves(v) if isinstance(v, dict) else (v,))
    for v in leaves(ps):
        v.requires_grad_(True)
    PH, NW = 6 * steps, 512
    sb = Stamps("vmh", NW * PH * 8)
    u = u0.clone().requires_grad_(True)
    for rep in range(3):
        sb.on(PH) if rep == 2 else sb.off()
        uT, _ = nde(u, ps, st)
        fw = sb.read(NW, PH, 8)
        sb.on(PH) if rep == 2 else sb.off()
        uT.sum().backward()
        bw = sb.read(NW, PH, 8)
    sb.off()
    print("plans", [sorted(q.flags()) for pool in nde._plans.values() for q in pool])

    def report(title, s, names):
        s = s[s[:, 0, 0] > 0]
        sel, nxt = s[:, 8:PH - 1, :7], s[:, 9:PH, 0]
        table(f"{title}: {s.shape[0]} workgroups, phase start-to-start {(nxt - sel[:, :, 0]).mean():.0f}",
              np.diff(np.concatenate([sel, nxt[:, :, None]], axis=2), axis=2), names)
    report("forward", fw, ["wait for the neighbours' flags", "halo values + barrier", "message MLP of the wave's 16 edges", "staging + per-target sums",
                           "node MLP (4 layers, a barrier each)", "stage update + drain + flag", "tape rows issued, loop overhead"])
    if (fw[:, 8:PH - 1, 7] > 0).any():      # the forward's staging step, split at its first barrier (stamp 7)
        f = fw[fw[:, 0, 0] > 0][:, 8:PH - 1, :]
        print(f"   staging, split: message MLP end of wave 0 -> all waves staged {np.mean(f[:, :, 7] - f[:, :, 3]):.0f}, "
              f"-> sums done {np.mean(f[:, :, 4] - f[:, :, 7]):.0f}")
    report("adjoint", bw, ["K-bar + node MLP backwards", "message MLP backwards of the wave's 16 edges", "barrier (the slowest wave)",
                           "own-row sums + drain + flag", "dz rows issued", "wait for the neighbours' flags", "by-source gather + stage adjoint"])
    if nv > 4096:      # tile rounds: a turn of the adjoint = tables, second half of the phase before, first half of this one
        b = bw[bw[:, 0, 0] > 0][:, 8:PH - 1, :]
        seq = [7, 5, 6, 0, 1, 2, 3, 4]
        table("adjoint, last turn of a sweep (tile rounds)", np.stack([b[:, :, seq[k + 1]] - b[:, :, seq[k]] for k in range(7)], axis=2),
              ["tables, by-source positions, state, tape rows asked for", "wait for the phase before (published a sweep ago)",
               "by-source gather + stage adjoint", "K-bar + node MLP backwards", "message MLP backwards (both rounds)", "barrier",
               "own-row sums + drain + flag"])


# ---- GAT: [block][16], wall clock at 11 / 12 (the layer's first and last stamps)

def gat_layer(g):
    layer = ng.GATConv((64, 16), "relu", heads=4, initialgraph=g)
    return layer


def gat():
    g = c2_graph()
    layer = gat_layer(g)
    ps, st = ng.setup(3, layer)
    ps = ng.to_device(ps, DEV)
    x = torch.randn(16384, 64, device=DEV).T
    sb = Stamps("gat", 2048 * 16)
    with torch.no_grad():
        for rep in range(4):
            sb.on() if rep == 3 else sb.off()
            layer(x, ps, st)
            raw = sb.read(2048, 16)
    sb.off()
    raw = used(raw, 10)
    st_, w0, w1 = raw[:, :11], raw[:, 11], raw[:, 12]
    table("one-launch GAT layer forward", np.concatenate([np.diff(st_, axis=1), (st_[:, 10] - st_[:, 0])[:, None]], axis=1),
          ["metadata + W loads + DMA issue + v vectors", "barrier (DMA data lands)", "score halves (ar of staged rows, al)", "barrier",
           "softmax + coefficient table", "per-head aggregation", "barrier", "MFMA + tile store", "barrier", "epilogue store", "workgroup total"])
    print(f"workgroup total {(w1 - w0).mean() * 0.01:.2f} us; first start -> last end {(w1.max() - w0.min()) * 0.01:.2f} us; start spread "
          f"{(w0.max() - w0.min()) * 0.01:.2f} us; end spread {(w1.max() - w1.min()) * 0.01:.2f} us")
    order = np.argsort(w0)
    print("start times (us, sorted, every 64th):", np.round((w0[order][::64] - w0.min()) * 0.01, 2).tolist())


def gat_node():
    g = c2_graph()
    nde = ng.NeuralODE(gat_layer(g), solver="tsit5", n_steps=int(os.environ.get("STEPS", 10)), dt=0.02)
    ps, st = ng.setup(3, nde)
    ps = ng.to_device(ps, DEV)
    for v in ps.values():
        v.requires_grad_(True)
    u = torch.randn(16384, 64, device=DEV).T.requires_grad_(True)
    sb = Stamps("gat", 2048 * 16)
    for rep in range(3):
        sb.on() if rep == 2 else sb.off()
        uT, _ = nde(u, ps, st)
        fw = sb.read(2048, 16)
        sb.on() if rep == 2 else sb.off()
        uT.sum().backward()
        bw = sb.read(2048, 16)
    sb.off()

    def steps(raw, order):
        raw = used(raw, order[-1])
        return np.stack([raw[:, b] - raw[:, a] for a, b in zip(order[:-1], order[1:])] + [raw[:, order[-1]] - raw[:, order[0]]], axis=1)
    # forward: 0 phase start, 13 after the wait, 1..5, 9 inside the layer code (gat_fwd_compute), 14 stores issued, 15 published
    table("forward, last phase", steps(fw, [0, 13, 1, 2, 3, 4, 5, 9, 14, 15]),
          ["wait for the neighbours", "DMA issue, a_l / a_r loads", "barrier (rows land)", "W x of the staged rows (MFMA)", "barrier",
           "score halves, barrier, softmax + coefficients", "aggregation", "activation, tape, combination, row store", "drain + barrier + flag",
           "phase"])
    table("adjoint, last phase", steps(bw, [0, 1, 7, 8, 9, 2, 3, 4, 5, 10, 11, 12, 13, 14, 6]),
          ["by-target metadata, DMA issue, K-bar, dz store", "T: W / alpha loads, dz tile, barrier (rows land)", "T: db partial, MFMA, barrier",
           "T: d alpha loop", "T: softmax pullback, dscore / dal stores", "drain + barrier + flag", "by-source metadata + W copy",
           "wait for the neighbours", "S: DMA issue, alpha / dscore / x loads", "S: barrier (rows land)", "S: aggregation, tiles", "S: barrier",
           "S: dx and dW products", "S: u accumulators, barrier, dx read, barrier", "T + S"])


# ---- Dense: the pair forward / pullback ([block][16], the workgroup's 4th tile), the small pullback ([block][8], wall clock)

def pair_inputs(grad):
    n = 524288
    mk = lambda *s, scale=1.0, g=grad: (torch.randn(*s, device=DEV) * scale).requires_grad_(g)
    return n, mk(n, 64), mk(n, 2, g=False), mk(64, 2, g=False), mk(68, 64, scale=0.1), mk(66, 64, scale=0.1), mk(64)


def pair():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import composed as F      # the primitives' autograd wrappers (tests/composed.py)
    n, h, d, th, wp, wq, bp = pair_inputs(False)
    run = lambda: F.dense_pair([h, d, th], wp, bp, 0, [h, d], wq, None, 0, row_divs_a=[1, 1, n // 64], n=n)
    sb = Stamps("pair", 2048 * 16)
    with torch.no_grad():
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        sb.on()
        run()
        a = used(sb.read(2048, 16), 8)
    sb.off()
    table("pair Dense forward, one tile per workgroup", np.concatenate([np.diff(a[:, :9], axis=1), (a[:, 8] - a[:, 0])[:, None]], axis=1),
          ["top barrier", "narrow loads + DMA issue + products", "collect next image (vmcnt)", "xn write + barrier", "stage a + barrier",
           "epilogue a", "barrier + stage b + barrier", "epilogue b", "tile total"])


def pair_bwd():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import composed as F
    n, h, d, th, wp, wq, bp = pair_inputs(True)
    gp, gq = torch.randn(n, 64, device=DEV), torch.randn(n, 64, device=DEV)

    def once():
        ya, yb = F.dense_pair([h, d, th], wp, bp, 0, [h, d], wq, None, 0, row_divs_a=[1, 1, n // 64], n=n)
        torch.autograd.backward([ya, yb], [gp, gq])
        h.grad = wp.grad = wq.grad = bp.grad = None
    for _ in range(3):
        once()
    torch.cuda.synchronize()
    nb = 2048
    sb = Stamps("pair_bwd", nb * 16)
    sb.on()
    once()
    raw = sb.read(nb, 16)
    sb.off()
    blocks = np.arange(nb)[raw[:, 9] > 0]
    a = raw[blocks]
    table("pair Dense pullback, one tile per workgroup", np.concatenate([np.diff(a[:, :10], axis=1), (a[:, 9] - a[:, 0])[:, None]], axis=1),
          ["top barrier", "dy rows -> LDS + barrier", "issue the next tile's loads", "X DMA issue + products (256 MFMAs per wave)",
           "collect the next tile's loads (vmcnt)", "addend loads issued + barrier", "stage dX + barrier", "addend wait", "dX stores issued",
           "tile total"])
    table("inside the products phase (wave 0)", np.stack([a[:, 12] - a[:, 3], a[:, 13] - a[:, 12], a[:, 4] - a[:, 13]], axis=1),
          ["X DMA issue", "dW (160 MFMAs)", "dX (128 MFMAs)"])
    # who shares a CU: HW_ID bits 8..11 = CU, 13..15 = SE (gfx9 layout), XCC_ID bits 0..3
    hw, xcc = a[:, 10].astype(np.int64), a[:, 11].astype(np.int64) & 15
    cu = ((hw >> 8) & 15) | (((hw >> 13) & 7) << 4) | (xcc << 8)
    groups = {}
    for b_, c_ in zip(blocks, cu):
        groups.setdefault(int(c_), []).append(int(b_))
    sizes = np.bincount([len(v) for v in groups.values()])
    print("workgroups per (XCD, SE, CU):", {k: int(v) for k, v in enumerate(sizes) if v})
    pairs = [v for v in groups.values() if len(v) == 2]
    print("first pairs sharing a CU (block ids):", pairs[:8])
    print("block-id distance within a pair: ", dict(zip(*np.unique([b2 - b1 for b1, b2 in (sorted(v) for v in pairs)], return_counts=True))))
    row = {int(b_): k for k, b_ in enumerate(blocks)}
    off = np.array([abs(a[row[v[0]], 3] - a[row[v[1]], 3]) for v in pairs])   # start of the products phase of the stamped tile
    if len(off):
        print(f"|offset| between the products-phase starts of a CU's two workgroups: median {np.median(off):.0f}, p10 {np.percentile(off, 10):.0f}, "
              f"p90 {np.percentile(off, 90):.0f} cycles (tile {np.median(a[:, 9] - a[:, 0]):.0f})")


def small_dense():
    from ngpde_amd import functional as F
    names = ["W + tile loads, dz", "barrier, LDS writes, barrier", "dX product + stores", "dW product", "slab", "in-kernel total"]
    for n, widths, dout, act in [(3000, [60], 60, "tanh"), (18000, [60], 60, "tanh"), (3000, [2], 60, "identity")]:
        blocks = [torch.randn(n, w, device=DEV, requires_grad=True) for w in widths]
        wt = torch.randn(sum(widths), dout, device=DEV, requires_grad=True)
        b = torch.randn(dout, device=DEV, requires_grad=True)
        R = torch.randn(n, dout, device=DEV)
        nb = min((n + 63) // 64, 1024, n // (sum(widths) + 1))   # the kernel's grid
        sb = Stamps("small_dense", nb * 8)
        for rep in range(4):
            y = F.dense(blocks, wt, b, _lib.ACT[act])
            torch.cuda.synchronize()
            sb.on() if rep == 3 else sb.off()
            y.backward(R)
            st = sb.read(nb, 8)[:, :6] * 0.01       # us
        sb.off()
        table(f"n={n} {widths}=>{dout} {act}, {nb} workgroups", np.concatenate([np.diff(st, axis=1), (st[:, 5] - st[:, 0])[:, None]], axis=1),
              names, unit="us")
        print(f"  first start -> last end {st[:, 5].max() - st[:, 0].min():.2f} us; start spread {st[:, 0].max() - st[:, 0].min():.2f} us")


# ---- edge kernels: [block][16], one steady-state tile per persistent workgroup, on the C4 shard; wall clock at the first and last stamps

def c4_layer_run():
    n, h = 8192, 64
    traj = int(sys.argv[2]) if len(sys.argv) > 2 else 64
    act = sys.argv[3] if len(sys.argv) > 3 else "swish"
    idx = np.arange(n)
    s = np.concatenate([idx for k in (-3, -2, -1, 1, 2, 3)]); t = np.concatenate([(idx + k) % n for k in (-3, -2, -1, 1, 2, 3)])
    S_, T_ = np.concatenate([s + i * n for i in range(traj)]), np.concatenate([t + i * n for i in range(traj)])
    N = n * traj
    g = ng.GNNGraph(S_, T_, num_nodes=N, index_base=0, num_graphs=traj,
                    ndata={"u": torch.rand(1, N), "x": torch.as_tensor(np.tile(idx / n, traj)[None, :].astype(np.float32))},
                    gdata={"θ": torch.rand(2, traj)})
    layer = ng.MPPDEConv(ng.Chain(ng.Dense(132, 64, act), ng.Dense(64, 64, act)), ng.Chain(ng.Dense(130, 64, act), ng.Dense(64, 64)),
                         initialgraph=g)
    ps, st = ng.setup(4, layer)
    ps = ng.to_device(ps, DEV)
    x = torch.randn(N, h, device=DEV).T
    return lambda: layer(x, ps, st)


def edge_family(family, last, wall, names):
    run = c4_layer_run()
    sb = Stamps(family, 2048 * 16)
    with torch.no_grad():
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        sb.on()
        run()
        a = used(sb.read(2048, 16), last)
    sb.off()
    tot = a[:, last] - a[:, 0]
    table(f"{family} forward, one tile per workgroup", np.concatenate([np.diff(a[:, :last + 1], axis=1), tot[:, None]], axis=1), names + ["tile total"])
    r = np.median(tot / np.maximum(a[:, wall + 1] - a[:, wall], 1))
    print("shader cycles per 10 ns wall tick:", r, " => clock GHz ~", r / 10)


def edge():
    edge_family("edge", 7, 8, ["stage + prefix + rowOf (3 syncs)", "chunk0 assemble + sync", "chunk0 MFMA + sync", "chunk0 epilogue + sync",
                               "chunk0 reduce + sync", "chunks 1..", "output store"])


def edge64():
    edge_family("edge64", 13, 14, ["stage + prefix + edge words (3 syncs)", "a1 of slice 0", "products 0 | a1 of slice 1",
                                   "issue next tile's row loads", "steady block (it = 1)", "barrier", "reduce", "barrier",
                                   "steady block (it = 2) + reduce + 2 barriers", "(loop exit)", "messages of the last slice",
                                   "barrier + reduce + barrier", "output store"])


COMMANDS = {"gcn": gcn, "node": node, "persistent": persistent, "interleaved": interleaved, "tile-rounds": tile_rounds, "vmh": vmh,
            "gat": gat, "gat-node": gat_node, "pair": pair, "pair-bwd": pair_bwd, "small-dense": small_dense, "edge": edge, "edge64": edge64}

if __name__ == "__main__":
    if len(sys.argv) < 2 or sys.argv[1] not in COMMANDS:
        sys.exit(__doc__)
    lib = _lib.load()
    lib.ngpde_debug_set_stamps.argtypes = [C.c_int32, C.c_void_p, C.c_int64, C.c_int32]
    lib.ngpde_debug_set_stamps.restype = C.c_int32
    COMMANDS[sys.argv[1]]()
