"""Dense output for saveat in adaptive Tsit5 (NeuralODE(..., adaptive=True, saveat=<vector>) or interpolate_saveat=True; DiffEq's
saveat, as docs/src/tutorials/VMH.md:87 solves): the two kernels against the stage-combine calls they must equal bit for bit, the
step sequence against the same solve without saveat, a linear right-hand side against expm, the gradients against float64 autograd
through an explicit restatement of the accepted steps and the interpolant, and the tutorials' right-hand sides against a float64
replay of the device's accepted steps extended with the interpolant (values and the discrete adjoint)."""
import ctypes as C

import numpy as np
import pytest
import scipy.linalg
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from ngpde_amd import node as NODE
from oracle import ngpde_oracle as O
from test_mp_gpu import close, mlp_grad_pairs, omlp, prep
from test_node_adaptive_gpu import cora_case, offset_tensor
from test_node_vmh_gpu import spatial, tutorial_mlps
from test_rk_dense_output import interp_b

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A, B = O.TSIT5["a"], O.TSIT5["b"]


# ---- the kernels against the stage-combine calls they restate ---------------------------------------------------------------------

def dense_output(u, ks, rows, outs):
    NODE._dense_output(u, ks, rows, outs)


@pytest.mark.parametrize("count", [1, 4099, 1 << 20, 777_777])
@pytest.mark.parametrize("m", [1, 2, 8, 16, 17, 40])
def test_dense_output_kernels_are_the_combines_bit_for_bit(count, m):
    gen = torch.Generator().manual_seed(count + 1000 * m)
    rng = np.random.default_rng(count + m)
    for off in ((0, 1) if count % 4 == 0 else (0,)):
        u = offset_tensor(count, off, gen)
        ks = [offset_tensor(count, off, gen) for _ in range(7)]
        rows = [[float(np.float32(c)) for c in rng.normal(size=7) * 0.3] for _ in range(m)]
        outs = [offset_tensor(count, off, gen) for _ in range(m)]
        dense_output(u, ks, rows, outs)
        for j in range(m):
            ref = NODE._combine(u, 1.0, ks, rows[j])
            assert torch.equal(outs[j], ref), (off, j)
        # the pullback: kbar_i = sum_j rows[j][i] dout_j (written), ubar += sum_j dout_j, as chained combines of up to 8 terms
        douts = outs
        ubar = offset_tensor(count, off, gen)
        ubar0 = ubar.clone()
        darr = (C.c_void_p * m)(*[d.data_ptr() for d in douts])
        kbar = [offset_tensor(count, off, gen) for _ in range(7)]
        cf = (C.c_float * (7 * m))(*[c for r in rows for c in r])
        karr = (C.c_void_p * 7)(*[k.data_ptr() for k in kbar])
        _lib.check(_lib.load().ngpde_rk_dense_output_pullback(count, m, darr, 7, cf, ubar.data_ptr(), karr, _lib.current_stream()))
        for i in range(7):
            ref = None
            for c0 in range(0, m, 8):
                ref = NODE._combine(ref, 1.0, douts[c0:c0 + 8], [rows[j][i] for j in range(c0, min(m, c0 + 8))])
            assert torch.equal(kbar[i], ref), (off, i)
        ref = ubar0
        for c0 in range(0, m, 8):
            ref = NODE._combine(ref, 1.0, douts[c0:c0 + 8], [1.0] * len(douts[c0:c0 + 8]))
        assert torch.equal(ubar, ref), off


# ---- float64 restatement of an interpolating solve and its discrete adjoint --------------------------------------------------------

def step_ends(dts, t0, t1):
    """the controller's t after every accepted step of an interpolating solve: t + dt, the last one landing on t_end itself"""
    ends, t = [], t0
    for n, dt in enumerate(dts):
        t = t1 if n == len(dts) - 1 else t + dt
        ends.append(t)
    return ends


def placement(times, dts, t0, t1):
    """(slot of t0, per step: slot of its end, interior [(slot, theta)]) -- NODE.saves_in_step over the steps"""
    j, t0_slot = 0, None
    if times and times[0] == t0:
        j, t0_slot = 1, 0
    ends, inter, t = [], [], t0
    for dt, te in zip(dts, step_ends(dts, t0, t1)):
        interior, end, j = NODE.saves_in_step(times, j, t, te, dt)
        ends.append(end)
        inter.append(interior)
        t = te
    assert j == len(times)
    return t0_slot, ends, inter


def replay_dense(rhs, vjp, u0, dts, times, t0, t1, dout, accumulate):
    """float64 solve over the given steps with the saves at `times` (Tsit5's interpolant inside a step, restated from the table in
    test_rk_dense_output) and, when dout (the cotangents of the saves) is given, its discrete adjoint.  Returns (saves, du0)."""
    t0_slot, ends, inter = placement(times, dts, t0, t1)
    out = [None] * len(times)
    if t0_slot is not None:
        out[t0_slot] = u0
    u, tape = u0, []
    for n, dt in enumerate(dts):
        ks, caches = [], []
        for i in range(6):
            U = u
            for j in range(i):
                if A[i][j] != 0.0:
                    U = U + (dt * A[i][j]) * ks[j]
            k, c = rhs(U)
            ks.append(k)
            caches.append(c)
        un = u
        for i in range(6):
            un = un + (dt * B[i]) * ks[i]
        k7, c7 = rhs(un)
        rows = []
        for sl, th in inter[n]:
            r = dt * interp_b(th)
            rows.append(r)
            out[sl] = u + sum(r[i] * kk for i, kk in enumerate(ks + [k7]))
        if ends[n] is not None:
            out[ends[n]] = un
        tape.append((caches, c7, rows))
        u = un
    if dout is None:
        return out, None
    zero = np.zeros_like(u0)

    def pull(n):
        rows = tape[n][2]
        if not rows:
            return None
        slots = [sl for sl, _ in inter[n]]
        return [sum(rows[q][i] * dout[sl] for q, sl in enumerate(slots)) for i in range(7)], sum(dout[sl] for sl in slots)
    lam = dout[ends[-1]] if ends[-1] is not None else zero
    pulled = {len(dts) - 1: pull(len(dts) - 1)}
    if pulled[len(dts) - 1] is not None:
        ub, pg = vjp(tape[-1][1], pulled[len(dts) - 1][0][6])
        accumulate(pg)
        lam = lam + ub
    start = [t0_slot] + ends[:-1]
    for n in reversed(range(len(dts))):
        dt, ubars = dts[n], [None] * 6
        pulled[n - 1] = pull(n - 1) if n >= 1 else None
        for i in reversed(range(6)):
            kbar = (dt * B[i]) * lam
            for j in range(i + 1, 6):
                if A[j][i] != 0.0:
                    kbar = kbar + (dt * A[j][i]) * ubars[j]
            if pulled[n] is not None:
                kbar = kbar + pulled[n][0][i]
            if i == 0 and pulled[n - 1] is not None:
                kbar = kbar + pulled[n - 1][0][6]
            ubars[i], pg = vjp(tape[n][0][i], kbar)
            accumulate(pg)
        for i in range(6):
            lam = lam + ubars[i]
        if start[n] is not None:
            lam = lam + dout[start[n]]
        if pulled[n] is not None:
            lam = lam + pulled[n][1]
    return out, lam


# ---- the step sequence does not depend on the saves ----------------------------------------------------------------------------------

def cora_node(node, **kw):
    return ng.NeuralODE(node.model, adaptive=True, reltol=node.reltol, abstol=node.abstol, save_start=False, dt=node.dt,
                        maxiters=node.maxiters, **kw)


def test_same_steps_with_and_without_interpolated_saves():
    node, ps, st, u, params, og, R = cora_case()
    plain, _ = node(u, ps, st)
    s0 = dict(node.stats)
    times = list(np.linspace(0.005, 0.995, 100)) + [1.0]
    nd = cora_node(node, saveat=times)
    us, _ = nd(u, ps, st)
    s1 = nd.stats
    assert tuple(us.shape) == (16, 2708, 101)
    assert s1["dts"] == s0["dts"] and s1["nf"] == s0["nf"] and s1["naccept"] == s0["naccept"], (s0["dts"], s1["dts"])
    assert s1["ninterp"] == 100 and s1["save_times"] == times
    assert torch.equal(us[:, :, -1], plain)                       # the t_end slot is the plain solve's u(T), bit for bit
    land = cora_node(node, saveat=0.01)                            # the same 100 intervals, steps cut to land on every save point
    land(u, ps, st)
    scalar = cora_node(node, saveat=0.01, interpolate_saveat=True)
    us2, _ = scalar(u, ps, st)
    assert scalar.stats["dts"] == s0["dts"] and tuple(us2.shape) == (16, 2708, 100)
    assert land.stats["naccept"] > s0["naccept"], (land.stats["naccept"], s0["naccept"])
    print(f"cora, 100 save points: interpolating naccept={s1['naccept']} nf={s1['nf']}; landing naccept={land.stats['naccept']} "
          f"nf={land.stats['nf']}")


# ---- a linear right-hand side against expm -----------------------------------------------------------------------------------------

def linear_case(T=2.0):
    d, N = 8, 64
    rng = np.random.default_rng(5)
    W = (-0.3 * np.eye(d) + 0.8 * rng.normal(size=(d, d)) / np.sqrt(d)).astype(np.float32)
    b = (0.1 * rng.normal(size=(d, 1))).astype(np.float32)
    u0 = rng.normal(size=(d, N)).astype(np.float32)
    ps = {"weight": torch.as_tensor(W, device=DEV), "bias": torch.as_tensor(b, device=DEV)}
    return d, N, W.astype(np.float64), b.astype(np.float64), u0, ps


def irregular_times(dts, t0, t1, n_final=20, n_rest=20, seed=3):
    """t0 and t1, n_rest random times over the solve and n_final inside its final step"""
    rng = np.random.default_rng(seed)
    ends = step_ends(dts, t0, t1)
    last0 = ends[-2] if len(ends) > 1 else t0
    inner = list(rng.uniform(t0, last0, size=n_rest)) + list(np.linspace(last0, t1, n_final + 2)[1:-1])
    return [t0] + sorted(set(float(x) for x in inner)) + [t1]


def test_linear_rhs_against_expm():
    d, N, W, b, u0, ps = linear_case()
    T = 2.0
    M = np.zeros((d + 1, d + 1))
    M[:d, :d], M[:d, d:] = W, b
    reltol, abstol = 1e-3, 1e-6
    base = ng.NeuralODE(ng.Dense(d, d), tspan=(0.0, T), adaptive=True, reltol=reltol, abstol=abstol)
    _, st = ng.setup(0, base)
    ut = torch.as_tensor(u0, device=DEV)
    base(ut, ps, st)
    times = irregular_times(base.stats["dts"], 0.0, T)
    node = ng.NeuralODE(ng.Dense(d, d), tspan=(0.0, T), adaptive=True, reltol=reltol, abstol=abstol, saveat=times)
    us, _ = node(ut, ps, st)
    s = node.stats
    assert s["dts"] == base.stats["dts"] and s["ninterp"] == len(times) - 2 and tuple(us.shape) == (d, N, len(times))
    rep, _ = replay_dense(lambda x: (W @ x + b, None), None, u0.astype(np.float64), s["dts"], times, 0.0, T, None, None)
    close(us, np.stack(rep, axis=2), 2e-4, 1e-5, "saves against the float64 replay")
    exact = [(scipy.linalg.expm(t * M) @ np.vstack([u0.astype(np.float64), np.ones((1, N))]))[:d] for t in times]
    err = max(np.abs(r - e).max() for r, e in zip(rep, exact))
    scale = reltol * max(np.abs(e).max() for e in exact) + abstol
    # float64 rehearsal of this case (the restated controller fed float64 EEst, 8 steps, the interpolant at 39 points inside every
    # step and the step ends): the worst error against expm is 8.6e-4 of reltol max|u| + abstol.  A factor 0.05 leaves room for the
    # device's float32-driven step sizes; an interpolant of the wrong order or with a wrong coefficient misses it by far.
    assert err <= 0.05 * scale, (err, scale)
    print(f"linear: naccept={s['naccept']} interpolant err / (reltol max|u| + abstol) = {err / scale:.3g}")


# ---- gradients against float64 autograd through the restated steps and interpolant ---------------------------------------------------

def test_gradients_against_float64_autograd():
    d, N, W, b, u0, ps = linear_case(T=1.5)
    T = 1.5
    rhs = ng.Dense(d, d, "tanh")
    base = ng.NeuralODE(rhs, tspan=(0.0, T), adaptive=True, reltol=1e-4, abstol=1e-6)
    _, st = ng.setup(0, base)
    base(torch.as_tensor(u0, device=DEV), ps, st)
    times = irregular_times(base.stats["dts"], 0.0, T, n_final=18, n_rest=12, seed=9)[1:]      # t0 not listed, t_end listed
    node = ng.NeuralODE(rhs, tspan=(0.0, T), adaptive=True, reltol=1e-4, abstol=1e-6, saveat=times)
    psg = {k: v.clone().requires_grad_(True) for k, v in ps.items()}
    u = torch.as_tensor(u0, device=DEV).requires_grad_(True)
    us, _ = node(u, psg, st)
    R = np.random.default_rng(4).normal(size=tuple(us.shape))
    (us * torch.as_tensor(R.astype(np.float32), device=DEV)).sum().backward()
    dts = node.stats["dts"]
    assert dts == base.stats["dts"] and len(dts) >= 3

    Wt = torch.tensor(W, dtype=torch.float64, requires_grad=True)
    bt = torch.tensor(b, dtype=torch.float64, requires_grad=True)
    ut = torch.tensor(u0.astype(np.float64), requires_grad=True)
    f = lambda x: torch.tanh(Wt @ x + bt)
    _, ends, inter = placement(times, dts, 0.0, T)
    x, outs = ut, [None] * len(times)
    for n, dt in enumerate(dts):
        ks = []
        for i in range(6):
            U = x
            for j in range(i):
                if A[i][j] != 0.0:
                    U = U + (dt * A[i][j]) * ks[j]
            ks.append(f(U))
        xn = x
        for i in range(6):
            xn = xn + (dt * B[i]) * ks[i]
        k7 = f(xn)
        for sl, th in inter[n]:
            r = dt * interp_b(th)
            outs[sl] = x + sum(float(r[i]) * kk for i, kk in enumerate(ks + [k7]))
        if ends[n] is not None:
            outs[ends[n]] = xn
        x = xn
    loss = sum((o * torch.as_tensor(R[:, :, j])).sum() for j, o in enumerate(outs))
    loss.backward()
    close(us, torch.stack(outs, dim=2).detach().numpy(), 2e-4, 1e-5, "saves")
    close(u.grad, ut.grad.numpy(), 5e-4, 1e-4, "du0")
    close(psg["weight"].grad, Wt.grad.numpy(), 5e-4, 1e-3, "dW")
    close(psg["bias"].grad, bt.grad.numpy(), 5e-4, 1e-3, "db")


# ---- the tutorials' right-hand sides against the float64 replay --------------------------------------------------------------------

def check_cora_dense(node, ps, u, us, params, og, R, times):
    rhs, vjp = O.gcn2_rhs([{k: v.astype(np.float32).astype(np.float64) for k, v in p.items()} for p in params], og, "relu")
    acc = [dict(weight=np.zeros_like(p["weight"]), bias=np.zeros_like(p["bias"])) for p in params]

    def accumulate(pg):
        for a_, g_ in zip(acc, pg):
            a_["weight"] += g_["weight"]
            a_["bias"] += g_["bias"].reshape(a_["bias"].shape)
    rep, du0 = replay_dense(rhs, vjp, u.detach().cpu().double().numpy(), node.stats["dts"], times, 0.0, 1.0,
                            [R[:, :, j] for j in range(len(times))], accumulate)
    close(us, np.stack(rep, axis=2), 2e-4, 1e-5, "saves")
    close(u.grad, du0, 5e-4, 1e-4, "du0")
    for k in range(2):
        close(ps[f"layer_{k + 1}"]["weight"].grad, acc[k]["weight"], 5e-4, 1e-3, f"dW{k + 1}")
        close(ps[f"layer_{k + 1}"]["bias"].grad, acc[k]["bias"], 5e-4, 1e-3, f"db{k + 1}")


def run_dense(node, ps, st, u, seed=21):
    us, _ = node(u, ps, st)
    R = np.random.default_rng(seed).normal(size=tuple(us.shape))
    (us * torch.as_tensor(R.astype(np.float32), device=DEV)).sum().backward()
    return us, R


CORA_TIMES = [0.0, 0.013, 0.05, 0.11, 0.2, 0.21, 0.37, 0.5, 0.61, 0.74, 0.8, 0.93, 0.999]


def test_cora_rhs_with_vector_saveat_against_the_float64_replay():
    node, ps, st, u, params, og, R = cora_case()
    nd = cora_node(node, saveat=CORA_TIMES)
    us, R = run_dense(nd, ps, st, u)
    assert tuple(us.shape) == (16, 2708, len(CORA_TIMES) - 1)      # save_start=False drops the listed t0
    check_cora_dense(nd, ps, u, us, params, og, R, CORA_TIMES[1:])


def test_forced_rejections_still_match_the_replay():
    node, ps, st, u, params, og, R = cora_case(dt=1.0, reltol=1e-5, abstol=1e-5)
    nd = cora_node(node, saveat=CORA_TIMES)
    us, R = run_dense(nd, ps, st, u)
    assert nd.stats["nreject"] >= 1
    check_cora_dense(nd, ps, u, us, params, og, R, CORA_TIMES[1:])


def test_vmh_rhs_with_interpolated_scalar_saveat_against_the_float64_replay():
    N, T, saveat = 300, 0.4, 0.005
    g, og = spatial(N, 7)
    phi, gam = tutorial_mlps(width=24, msg=16, depth=3)
    node = ng.NeuralODE(ng.VMHConv(phi, gam, initialgraph=g), tspan=(0.0, T), adaptive=True, saveat=saveat, reltol=1e-9, abstol=1e-3,
                        interpolate_saveat=True)
    ps0, st = ng.setup(3, node)
    ps = prep(ps0, 3)
    rng = np.random.default_rng(13)
    u0 = rng.normal(size=(1, N)).astype(np.float32)
    u = torch.as_tensor(u0, device=DEV).requires_grad_(True)
    us, R = run_dense(node, ps, st, u, seed=14)
    times = node.save_times
    assert len(times) == 81 and tuple(us.shape) == (1, N, 81)
    stats = node.stats
    assert stats["naccept"] < len(times) - 1 and stats["ninterp"] > 0, stats["naccept"]     # saveat denser than the natural step

    ophi, ogam = omlp(phi, ps["ϕ"]), omlp(gam, ps["γ"])
    gphi = [dict(weight=np.zeros_like(L["weight"]), bias=np.zeros_like(L["bias"])) for L in ophi]
    ggam = [dict(weight=np.zeros_like(L["weight"]), bias=np.zeros_like(L["bias"])) for L in ogam]

    def vjp(cache, kbar):
        gr = O.vmh_conv_backward(cache, kbar)
        return gr["x"], gr

    def accumulate(gr):
        for dst, src in ((gphi, gr["phi"]), (ggam, gr["gamma"])):
            for d_, s_ in zip(dst, src):
                d_["weight"] += s_["weight"]
                d_["bias"] += np.asarray(s_["bias"]).reshape(d_["bias"].shape)
    rep, du0 = replay_dense(lambda x: O.vmh_conv(x, ophi, ogam, og), vjp, u0.astype(np.float64), stats["dts"], times, 0.0, T,
                            [R[:, :, j] for j in range(len(times))], accumulate)
    close(us, np.stack(rep, axis=2), 2e-4, 1e-5, "saved states")
    close(u.grad, du0, 5e-4, 1e-4, "du0")
    n1, o1 = mlp_grad_pairs(ps["ϕ"], gphi, phi)
    n2, o2 = mlp_grad_pairs(ps["γ"], ggam, gam)
    for (name, p), og_ in zip(n1 + n2, o1 + o2):
        close(p.grad, og_, 5e-4, 2e-4, f"d{name}")
    print(f"vmh interpolated saveat: naccept={stats['naccept']} nreject={stats['nreject']} nf={stats['nf']} saves={len(times)}")


# ---- edge cases and determinism ----------------------------------------------------------------------------------------------------

def test_a_save_on_a_step_end_is_the_step_state():
    d, N, W, b, u0, ps = linear_case()
    base = ng.NeuralODE(ng.Dense(d, d), tspan=(0.0, 2.0), adaptive=True)
    _, st = ng.setup(0, base)
    ut = torch.as_tensor(u0, device=DEV)
    base(ut, ps, st)
    dt = base.stats["dts"][0]
    t1 = 0.0 + dt
    node = ng.NeuralODE(ng.Dense(d, d), tspan=(0.0, 2.0), adaptive=True, saveat=[0.0, 0.5 * t1, t1])
    us, _ = node(ut, ps, st)
    assert node.stats["ninterp"] == 1
    assert torch.equal(us[:, :, 0], ut)                             # a listed t0 is u0
    # the first step restated with the solver's own launches: the same bits
    model, a, bb = node.model, NODE._TSIT5_A, NODE._TSIT5_B
    ur = NODE.rows_of(ut).contiguous()
    ks = []
    for i in range(6):
        terms = [ks[j] for j in range(i) if a[i][j] != 0.0]
        U = NODE._combine(ur, 1.0, terms, [dt * a[i][j] for j in range(i) if a[i][j] != 0.0]) if terms else ur
        ks.append(NODE.rows_of(model(U.T, ps, st)[0]).contiguous())
    u1 = NODE._combine(ur, 1.0, ks, [dt * bi for bi in bb])
    assert torch.equal(us[:, :, 2], u1.T)


def test_save_start_false_drops_t0():
    d, N, W, b, u0, ps = linear_case()
    ut = torch.as_tensor(u0, device=DEV)
    outs = []
    for ss in (True, False):
        node = ng.NeuralODE(ng.Dense(d, d), tspan=(0.0, 2.0), adaptive=True, saveat=0.3, interpolate_saveat=True, save_start=ss)
        _, st = ng.setup(0, node)
        outs.append(node(ut, ps, st)[0])
    assert tuple(outs[0].shape) == (d, N, 8) and tuple(outs[1].shape) == (d, N, 7)     # 0, 0.3 .. 1.8, 2.0
    assert torch.equal(outs[0][:, :, 0], ut) and torch.equal(outs[0][:, :, 1:], outs[1])


def test_two_solves_are_bitwise_identical():
    out = []
    for _ in range(2):
        node, ps, st, u, params, og, R = cora_case()
        nd = cora_node(node, saveat=CORA_TIMES + [1.0])
        us, _ = run_dense(nd, ps, st, u)
        out.append((nd.stats, [us.detach().clone(), u.grad.clone()] + [ps[l][p].grad.clone() for l in ps for p in ps[l]]))
    assert out[0][0] == out[1][0]
    for a_, b_ in zip(out[0][1], out[1][1]):
        assert torch.equal(a_, b_)
