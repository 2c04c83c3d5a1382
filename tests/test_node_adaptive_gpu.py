"""Adaptive Tsit5 on the generic solver path (NeuralODE(..., adaptive=True); docs/src/tutorials/graph_node.md:80-81 and VMH.md:87
solve with adaptive Tsit5): the scaled error norm kernel against numpy, a linear right-hand side against expm, and the tutorials'
right-hand sides against a float64 replay of the device's accepted steps -- a variable-dt restatement of the oracle's rk_solve /
rk_adjoint written here -- whose step sizes are checked against the restated controller (test_rk_adaptive_control.Restated) fed the
device's own EEst sequence."""
import ctypes as C
import time

import numpy as np
import pytest
import scipy.linalg
import torch

import ngpde_amd as ng
from ngpde_amd import _lib, synth as S
from ngpde_amd import node as NODE
from oracle import ngpde_oracle as O
from test_mp_gpu import close, mlp_grad_pairs, omlp, prep
from test_node_vmh_gpu import spatial, tutorial_mlps
from test_rk_adaptive_control import DONE, REJECT, Restated

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
A, B = O.TSIT5["a"], O.TSIT5["b"]
BTILDE = NODE._TSIT5_BTILDE


# ---- ngpde_rk_error_norm on its own ------------------------------------------------------------------------------------------

def device_norm(terms, coefs, up, un, abstol, reltol):
    lib = _lib.load()
    n = up.numel()
    ws = torch.empty(lib.ngpde_rk_error_norm_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    out = torch.full((1,), -1.0, dtype=torch.float64, device=DEV)
    arr = (C.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
    cf = (C.c_float * len(coefs))(*coefs)
    _lib.check(lib.ngpde_rk_error_norm(n, len(terms), arr, cf, up.data_ptr(), un.data_ptr(), abstol, reltol, ws.data_ptr(), out.data_ptr(),
                                       _lib.current_stream()))
    return float(out.item())


def numpy_norm(terms, coefs, up, un, abstol, reltol):
    e = sum(np.float64(np.float32(c)) * t.cpu().double().numpy() for c, t in zip(coefs, terms))
    sk = abstol + reltol * np.maximum(np.abs(up.cpu().double().numpy()), np.abs(un.cpu().double().numpy()))
    return float(np.sqrt(np.mean((e / sk) ** 2)))


def offset_tensor(n, off, gen):
    """n floats whose address is `off` floats past a 256-byte boundary (off = 0: the float4 path when n % 4 == 0)"""
    buf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
    t = buf[off:off + n]
    t.copy_(torch.randn(n, generator=gen).to(DEV))
    return t


@pytest.mark.parametrize("count", [1, 4096, 4099, 1 << 20, 777_777])
@pytest.mark.parametrize("n_terms", range(1, 9))
def test_error_norm_against_numpy(count, n_terms):
    gen = torch.Generator().manual_seed(count * 16 + n_terms)
    for off in ((0, 1) if count % 4 == 0 else (0,)):
        terms = [offset_tensor(count, off if j == n_terms - 1 else 0, gen) for j in range(n_terms)]
        up, un = offset_tensor(count, 0, gen), offset_tensor(count, 0, gen)
        coefs = [float(0.37 * (j + 1) * (-1) ** j * 1e-2) for j in range(n_terms)]
        for abstol, reltol in ((1e-6, 1e-3), (1e-3, 1e-9), (0.5, 0.0)):
            got = device_norm(terms, coefs, up, un, abstol, reltol)
            ref = numpy_norm(terms, coefs, up, un, abstol, reltol)
            assert abs(got - ref) <= 1e-6 * ref, (off, abstol, reltol, got, ref)
            assert device_norm(terms, coefs, up, un, abstol, reltol) == got       # bitwise reproducible


# ---- float64 replay of the accepted steps --------------------------------------------------------------------------------------

def restated_schedule(node, stats):
    """the restated controller fed the device's EEst sequence: (accepted dts, saved flags)"""
    t0, t1 = node.tspan
    ref = Restated(float(t0), float(t1), node.dt or 0.0, node.dtmax or 0.0, node.saveat or 0.0, node.maxiters)
    if node.dt is None:
        ref.initial_dt(*stats["init_norms"])
    dts, saved, act = [], [], None
    for e in stats["eests"]:
        dt = ref.dt
        act = ref.step(e)
        if act != REJECT:
            dts.append(dt)
            saved.append(bool(ref.saved))
    assert act == DONE
    return dts, saved


def replay(rhs, vjp, u0, dts, saved, save_start, dout, abstol, reltol, accumulate):
    """float64 solve over the given steps and its discrete adjoint.  dout: the cotangent of u(T), or with saveat the list of cotangents
    of the saved states.  Returns (u(T) or the saved states, du0, the float64 EEst of every step)"""
    u, tape, saves, eests = u0, [], ([u0] if save_start else []), []
    for n_step, dt in enumerate(dts):
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
        e = dt * sum(bt * k for bt, k in zip(BTILDE, ks + [rhs(un)[0]]))
        eests.append(float(np.sqrt(np.mean((e / (abstol + reltol * np.maximum(np.abs(u), np.abs(un)))) ** 2))))
        tape.append(caches)
        u = un
        if saved[n_step]:
            saves.append(u)
    saving = isinstance(dout, list)
    slot, start_slot, n_saved = (0 if save_start else None), [], (1 if save_start else 0)
    for n in range(len(dts)):
        start_slot.append(slot)
        if saved[n]:
            slot, n_saved = n_saved, n_saved + 1
        else:
            slot = None
    lam = dout[-1] if saving else dout
    for n in reversed(range(len(dts))):
        dt, ubars = dts[n], [None] * 6
        for i in reversed(range(6)):
            kbar = (dt * B[i]) * lam
            for j in range(i + 1, 6):
                if A[j][i] != 0.0:
                    kbar = kbar + (dt * A[j][i]) * ubars[j]
            ubars[i], pg = vjp(tape[n][i], kbar)
            accumulate(pg)
        for i in range(6):
            lam = lam + ubars[i]
        if saving and start_slot[n] is not None:
            lam = lam + dout[start_slot[n]]
    return (saves if saving else u), lam, eests


# ---- a linear right-hand side against expm -------------------------------------------------------------------------------------

def test_linear_rhs_against_expm():
    d, N, T = 8, 64, 2.0
    rng = np.random.default_rng(5)
    W = -0.3 * np.eye(d) + 0.8 * rng.normal(size=(d, d)) / np.sqrt(d)
    b = 0.1 * rng.normal(size=(d, 1))
    u0 = rng.normal(size=(d, N))
    M = np.zeros((d + 1, d + 1))
    M[:d, :d], M[:d, d:] = W.astype(np.float32), b.astype(np.float32)
    exact = (scipy.linalg.expm(T * M) @ np.vstack([u0.astype(np.float32), np.ones((1, N))]))[:d]
    ps = {"weight": torch.as_tensor(W.astype(np.float32), device=DEV), "bias": torch.as_tensor(b.astype(np.float32), device=DEV)}
    naccept = []
    for reltol, abstol in ((1e-3, 1e-6), (1e-5, 1e-7)):
        node = ng.NeuralODE(ng.Dense(d, d), tspan=(0.0, T), adaptive=True, reltol=reltol, abstol=abstol)
        _, st = ng.setup(0, node)
        uT, _ = node(torch.as_tensor(u0.astype(np.float32), device=DEV), ps, st)
        err = np.abs(uT.cpu().double().numpy() - exact).max()
        # Tsit5's local control keeps this problem's global error three orders below the tolerance (float64 rehearsal): 1x is the bound
        assert err <= 1.0 * (reltol * np.abs(exact).max() + abstol), (reltol, err)
        s = node.stats
        assert s["nf"] == 6 * (s["naccept"] + s["nreject"]) + 2
        assert s["t"] == T and abs(sum(s["dts"]) - T) < 1e-12 and len(s["dts"]) == s["naccept"]
        naccept.append(s["naccept"])
    assert naccept[1] > naccept[0]


# ---- the Cora tutorial's right-hand side -----------------------------------------------------------------------------------------

def cora_case(dt=None, reltol=1e-3, abstol=1e-3, maxiters=100_000, nan=False, act="relu"):
    N, PAIRS, D = 2708, 5278, 16
    rng = np.random.default_rng(11)
    s, t = S.preferential_pairs_graph(N, PAIRS, seed=1)
    params = [dict(weight=S.glorot_uniform(80 + k, D, D), bias=rng.normal(size=(D, 1)) * 0.1) for k in range(2)]
    if nan:
        params[1]["weight"][:] = np.nan
    u0 = rng.normal(size=(D, N))
    R = rng.normal(size=(D, N))
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0)
    rhs = ng.Chain(ng.GCNConv((D, D), act, initialgraph=g), ng.GCNConv((D, D), act, initialgraph=g))
    node = ng.NeuralODE(rhs, adaptive=True, reltol=reltol, abstol=abstol, save_start=False, dt=dt, maxiters=maxiters)
    _, st = ng.setup(0, node)
    ps = {f"layer_{k + 1}": {"weight": torch.as_tensor(params[k]["weight"].astype(np.float32), device=DEV).requires_grad_(True),
                             "bias": torch.as_tensor(params[k]["bias"].astype(np.float32), device=DEV).requires_grad_(True)}
          for k in range(2)}
    u = torch.as_tensor(u0.astype(np.float32), device=DEV).requires_grad_(True)
    return node, ps, st, u, params, O.Graph(s, t, num_nodes=N, index_base=0), R


def run_cora(node, ps, st, u, R):
    uT, _ = node(u, ps, st)
    (uT * torch.as_tensor(R.astype(np.float32), device=DEV)).sum().backward()
    return uT


def check_cora_against_replay(node, ps, u, uT, params, og, R):
    stats = node.stats
    dts, saved = restated_schedule(node, stats)
    assert dts == stats["dts"]                                   # the device's steps are the restated controller's, bit for bit
    rhs, vjp = O.gcn2_rhs([{k: v.astype(np.float32).astype(np.float64) for k, v in p.items()} for p in params], og, "relu")
    acc = [dict(weight=np.zeros_like(p["weight"]), bias=np.zeros_like(p["bias"])) for p in params]

    def accumulate(pg):
        for a_, g_ in zip(acc, pg):
            a_["weight"] += g_["weight"]
            a_["bias"] += g_["bias"].reshape(a_["bias"].shape)
    u0 = u.detach().cpu().double().numpy()
    uTo, du0, eests = replay(rhs, vjp, u0, dts, saved, False, R, node.abstol, node.reltol, accumulate)
    close(uT, uTo, 2e-4, 1e-5, "u(T)")
    close(u.grad, du0, 5e-4, 1e-4, "du0")
    for k in range(2):
        close(ps[f"layer_{k + 1}"]["weight"].grad, acc[k]["weight"], 5e-4, 1e-3, f"dW{k + 1}")
        close(ps[f"layer_{k + 1}"]["bias"].grad, acc[k]["bias"], 5e-4, 1e-3, f"db{k + 1}")
    assert max(eests) <= 1.0 + 1e-3, eests                      # every accepted step meets the tolerance in float64 too
    return stats


def test_cora_tutorial_rhs_against_the_float64_replay():
    node, ps, st, u, params, og, R = cora_case()
    t0 = time.perf_counter()
    uT = run_cora(node, ps, st, u, R)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    stats = check_cora_against_replay(node, ps, u, uT, params, og, R)
    assert stats["nf"] == 6 * (stats["naccept"] + stats["nreject"]) + 2 and stats["t"] == 1.0
    print(f"cora adaptive: naccept={stats['naccept']} nreject={stats['nreject']} nf={stats['nf']} wall(first call)={wall * 1e3:.1f} ms")


def test_forced_rejections_still_match_the_replay():
    node, ps, st, u, params, og, R = cora_case(dt=1.0, reltol=1e-5, abstol=1e-5)
    uT = run_cora(node, ps, st, u, R)
    stats = check_cora_against_replay(node, ps, u, uT, params, og, R)
    assert stats["nreject"] >= 1 and stats["nf"] == 6 * (stats["naccept"] + stats["nreject"]) + 1


def test_two_solves_are_bitwise_identical():
    out = []
    for _ in range(2):
        node, ps, st, u, params, og, R = cora_case()
        uT = run_cora(node, ps, st, u, R)
        out.append((node.stats, [uT.detach().clone(), u.grad.clone()] + [ps[l][p].grad.clone() for l in ps for p in ps[l]]))
    assert out[0][0] == out[1][0]
    for a_, b_ in zip(out[0][1], out[1][1]):
        assert torch.equal(a_, b_)


# ---- VMHConv with saveat (VMH.md:87) ---------------------------------------------------------------------------------------------

def test_vmh_rhs_with_saveat_against_the_float64_replay():
    N, T, saveat = 300, 0.4, 0.1
    g, og = spatial(N, 7)
    phi, gam = tutorial_mlps(width=24, msg=16, depth=3)
    node = ng.NeuralODE(ng.VMHConv(phi, gam, initialgraph=g), tspan=(0.0, T), adaptive=True, saveat=saveat, reltol=1e-9, abstol=1e-3)
    ps0, st = ng.setup(3, node)
    ps = prep(ps0, 3)
    rng = np.random.default_rng(13)
    u0 = rng.normal(size=(1, N)).astype(np.float32)
    u = torch.as_tensor(u0, device=DEV).requires_grad_(True)
    us, _ = node(u, ps, st)
    n_slots = int(round(T / saveat)) + 1
    assert tuple(us.shape) == (1, N, n_slots)
    R = rng.normal(size=(1, N, n_slots))
    (us * torch.as_tensor(R.astype(np.float32), device=DEV)).sum().backward()
    stats = node.stats
    dts, saved = restated_schedule(node, stats)
    assert dts == stats["dts"] and sum(saved) == n_slots - 1
    t, times = 0.0, []              # the saved states are those at exactly t0 + k saveat (steps land there, no interpolation)
    for dt, sv in zip(dts, saved):
        t += dt
        if sv:
            times.append(t)
    assert np.allclose(times, [saveat * k for k in range(1, n_slots)], rtol=0, atol=1e-12)

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
    saves, du0, eests = replay(lambda x: O.vmh_conv(x, ophi, ogam, og), vjp, u0.astype(np.float64), dts, saved, True,
                               [R[:, :, j] for j in range(n_slots)], node.abstol, node.reltol, accumulate)
    close(us, np.stack(saves, axis=2), 2e-4, 1e-5, "saved states")
    close(u.grad, du0, 5e-4, 1e-4, "du0")
    n1, o1 = mlp_grad_pairs(ps["ϕ"], gphi, phi)
    n2, o2 = mlp_grad_pairs(ps["γ"], ggam, gam)
    for (name, p), og_ in zip(n1 + n2, o1 + o2):
        close(p.grad, og_, 5e-4, 2e-4, f"d{name}")
    assert max(eests) <= 1.0 + 1e-3, eests
    print(f"vmh adaptive saveat: naccept={stats['naccept']} nreject={stats['nreject']} nf={stats['nf']}")


# ---- failure paths ---------------------------------------------------------------------------------------------------------------

def test_maxiters_and_nan_parameters_raise_promptly():
    node, ps, st, u, *_ = cora_case(maxiters=3)
    t0 = time.perf_counter()
    with pytest.raises(ng.NgpdeError) as e:
        node(u, ps, st)
    assert e.value.code == _lib.ERR_STATE and "maxiters" in str(e.value) and "t = " in str(e.value)
    for dt in (None, 0.1):          # the starting step sees f0 = NaN; a given step rejects until dtmin
        # (identity: relu -- max(x, 0) on the device -- would turn the NaN into 0 and the solve would be a finite one)
        node, ps, st, u, *_ = cora_case(dt=dt, nan=True, act="identity")
        with pytest.raises(ng.NgpdeError) as e:
            node(u, ps, st)
        assert e.value.code == _lib.ERR_STATE and ("dtmin" in str(e.value) or "not finite" in str(e.value)), str(e.value)
    assert time.perf_counter() - t0 < 60
