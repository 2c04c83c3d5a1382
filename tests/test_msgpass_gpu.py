"""GPU tests of the public message-passing API (propagate, apply_edges, aggregate_neighbors, softmax_edge_neighbors and the built-in
messages, /root/reference/src/NeuralGraphPDE.jl:5-11) against float64 numpy (oracle.propagate / gather / scatter / scatter_pullback),
a user layer written the way docs/src/devdoc.md:47-52 shows, inside and outside a NeuralODE.

Tolerances as test_mp_gpu.py: forward 1e-4 * max|ref| + 1e-5, gradients 5e-4 relative.
"""
import zlib

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from oracle import ngpde_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
AGGRS = ["+", "mean", "max", "min", "*"]


def close(a, ref, rtol=1e-4, atol=1e-5, what=""):
    a = a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    ref = np.asarray(ref, dtype=np.float64)
    assert a.shape == ref.shape, (what, a.shape, ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], ref[~fin]), f"{what}: non-finite entries differ"
    err = np.abs(a[fin] - ref[fin]).max() if fin.any() else 0.0
    bound = rtol * (np.abs(ref[fin]).max() if fin.any() else 0.0) + atol
    assert err <= bound, f"{what}: max err {err:.3e} > {bound:.3e}"


def gclose(a, ref, what=""):
    close(a, ref, rtol=5e-4, atol=1e-6, what=what)


def graphs():
    """(name, s, t, N) 0-based: the reference's test graph, a random one with isolated nodes, self loops and repeated edges, a hub of
    more than 300 in-edges, and an edgeless one"""
    rng = np.random.default_rng(7)
    out = [("reference", np.array([0, 0, 1, 2]), np.array([1, 2, 0, 0]), 3)]     # test/runtests.jl:11-13
    N = 40
    s, t = rng.integers(0, N - 6, 150), rng.integers(0, N - 6, 150)              # nodes 34..39 isolated
    s = np.concatenate([s, [3, 5, 5, 9, 9, 9]])                                  # self loops, repeated edges
    t = np.concatenate([t, [3, 5, 7, 2, 2, 2]])
    out.append(("random", s, t, N))
    N = 60
    hs, ht = rng.integers(0, N, 340), np.zeros(340, dtype=np.int64)              # node 0: 340 in-edges
    s2, t2 = rng.integers(0, N, 200), rng.integers(0, N, 200)
    out.append(("hub", np.concatenate([hs, s2]), np.concatenate([ht, t2]), N))
    out.append(("edgeless", np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64), 5))
    return out


GRAPHS = {name: (s, t, n) for name, s, t, n in graphs()}


def make(name, weighted=False):
    s, t, n = GRAPHS[name]
    w = np.random.default_rng(1).uniform(0.5, 1.5, s.size) if weighted else None
    g = ng.GNNGraph(s, t, num_nodes=n, index_base=0, edge_weight=None if w is None else w.astype(np.float32))
    og = O.Graph(s, t, num_nodes=n, index_base=0, edge_weight=w)
    return g, og


def draw(rng, shape, aggr):
    # products of up to 340 factors: keep them near 1
    return rng.uniform(0.9, 1.1, shape) if aggr == "*" else rng.normal(size=shape)


def dev(a, grad=True):
    return torch.as_tensor(np.asarray(a, dtype=np.float32), device=DEV).requires_grad_(grad)


def np_message(f, w):
    """float64 numpy forms of the built-in messages"""
    return {ng.copy_xj: lambda xi, xj, e: xj, ng.copy_xi: lambda xi, xj, e: xi,
            ng.xi_dot_xj: lambda xi, xj, e: (xi * xj).sum(axis=0, keepdims=True),
            ng.e_mul_xj: lambda xi, xj, e: e * xj, ng.w_mul_xj: lambda xi, xj, e: w.reshape(1, -1) * xj}[f]


def ref_grads(f, og, aggr, x, e, w, dout):
    """float64 pullback of propagate(f, g, aggr; xi=x, xj=x, e) for the built-ins: (dx, de)"""
    s, t, n = og.s, og.t, og.num_nodes
    xi, xj = O.gather(x, t), O.gather(x, s)
    m = np_message(f, w)(xi, xj, e)
    out = O.scatter(aggr, m, t, n)
    dm = O.scatter_pullback(aggr, m, t, n, out, dout)
    de = None
    if f is ng.copy_xj:
        dx = O.scatter("+", dm, s, n)
    elif f is ng.copy_xi:
        dx = O.scatter("+", dm, t, n)
    elif f is ng.xi_dot_xj:
        dx = O.scatter("+", dm * xj, t, n) + O.scatter("+", dm * xi, s, n)
    elif f is ng.w_mul_xj:
        dx = O.scatter("+", w.reshape(1, -1) * dm, s, n)
    else:
        dx = O.scatter("+", e * dm, s, n)
        de = (dm * xj).sum(axis=0, keepdims=True) if e.shape[0] == 1 else dm * xj
    return dx, de


def run_propagate(f, g, aggr, x, e, R):
    xt = dev(x)
    et = dev(e) if e is not None else None
    y = ng.propagate(f, g, aggr, xi=xt, xj=xt, e=et)
    y_ = torch.where(torch.isfinite(y), y, torch.zeros_like(y))
    (y_ * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
    return y, xt.grad, (et.grad if et is not None else None)


BUILTINS = [ng.copy_xj, ng.copy_xi, ng.xi_dot_xj, ng.e_mul_xj, ng.w_mul_xj]


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("aggr", AGGRS)
def test_builtin_messages_against_float64(name, aggr):
    g, og = make(name, weighted=(name == "random"))
    rng = np.random.default_rng(zlib.crc32(f"{name} {aggr}".encode()))
    E = og.num_edges
    w = og.edge_weight if og.edge_weight is not None else np.ones(E)
    for D in (1, 3, 64, 130):
        x = draw(rng, (D, og.num_nodes), aggr)
        for f in BUILTINS:
            xf = x / np.sqrt(D) if (aggr == "*" and f is ng.xi_dot_xj) else x      # (products of dot products near 1 as well)
            for ew in ((1, D) if f is ng.e_mul_xj else (None,)):
                e = draw(rng, (ew, E), aggr) if ew else None
                yo = O.propagate(np_message(f, w), og, aggr, xi=xf, xj=xf, e=e)
                R = rng.normal(size=yo.shape)
                y, dx, de = run_propagate(f, g, aggr, xf, e, R)
                what = f"{f.__name__} D={D} ew={ew}"
                close(y, yo, what=what)
                dxo, deo = ref_grads(f, og, aggr, xf, e, w, np.where(np.isfinite(yo), R, 0.0))
                gclose(dx, dxo, what="dx " + what)
                if e is not None:
                    gclose(de, deo, what="de " + what)


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("aggr", ["+", "mean"])
def test_fused_and_generic_paths_agree(name, aggr):
    g, _ = make(name, weighted=(name == "random"))
    rng = np.random.default_rng(5)
    E, N = g.num_edges, g.num_nodes
    w = np.asarray(g.edge_weight, dtype=np.float64).reshape(1, -1) if g.edge_weight is not None else np.ones((1, E))
    for D in (1, 3, 64, 130):
        x = rng.normal(size=(D, N))
        for f in (ng.copy_xj, ng.e_mul_xj, ng.w_mul_xj):
            for ew in ((1, D) if f is ng.e_mul_xj else (None,)):
                # the generic path runs the same message through the gather: w_mul_xj there is e_mul_xj with e = the weights
                e = rng.normal(size=(ew, E)) if ew else (w if f is ng.w_mul_xj else None)
                generic = ng.e_mul_xj if f is ng.w_mul_xj else f
                R = rng.normal(size=(D, N))
                y1, dx1, de1 = run_propagate(f, g, aggr, x, e, R)
                y2, dx2, de2 = run_propagate(lambda a, b, c, h=generic: h(a, b, c), g, aggr, x, e, R)   # not the built-in object
                what = f"{f.__name__} D={D} ew={ew}"
                close(y1, y2.detach().cpu().double().numpy(), rtol=1e-5, atol=1e-6, what=what)
                close(dx1, dx2.detach().cpu().double().numpy(), rtol=1e-5, atol=1e-6, what="dx " + what)
                if f is ng.e_mul_xj:
                    close(de1, de2.detach().cpu().double().numpy(), rtol=1e-5, atol=1e-6, what="de " + what)


def test_e_mul_xj_accepts_a_vector_of_edge_scalars():
    g, og = make("random")
    rng = np.random.default_rng(2)
    x, e = rng.normal(size=(64, og.num_nodes)), rng.normal(size=og.num_edges)
    y = ng.propagate(ng.e_mul_xj, g, "+", xj=dev(x, False), e=dev(e, False))
    close(y, O.propagate(lambda xi, xj, ee: ee.reshape(1, -1) * xj, og, "+", xj=x, e=e))


# ---- a user layer, as docs/src/devdoc.md:47-52 writes one ------------------------------------------------------------------------


class UserEdgeConv(ng.AbstractGNNContainerLayer):
    """ExplicitEdgeConv restated on ng.propagate: h'_i = aggr_j ϕ([h_i; h_j; x_j - x_i])"""

    layers = ("ϕ",)

    def __init__(self, ϕ, *, initialgraph=None, aggr="mean"):
        self.ϕ, self.aggr = ϕ, aggr
        self.initialgraph = ng.wrapgraph(initialgraph if initialgraph is not None else (lambda: ng.EMPTYGRAPH))

    def __call__(self, x, ps, st):
        g = st["graph"]
        xn = x if isinstance(x, dict) else {"preservedname": x}
        device = next(iter(xn.values())).device
        s = {k: torch.as_tensor(np.asarray(v), dtype=torch.float32, device=device) for k, v in g.ndata.items()}
        xs = {**xn, **s}

        def message(xi, xj, e):
            hi = [v for k, v in xi.items() if k != "x"]
            hj = [v for k, v in xj.items() if k != "x"]
            m, _ = self.ϕ(torch.cat(hi + hj + [xj["x"] - xi["x"]], dim=0), ps, st["ϕ"])
            return m

        return ng.propagate(message, g, self.aggr, xi=xs, xj=xs), st


def edgeconv_case(N=300, E=2500, h=6, seed=3):
    rng = np.random.default_rng(seed)
    pos = rng.random((2, N))
    s, t = rng.integers(0, N, E), rng.integers(0, N, E)
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0, ndata={"x": pos})
    og = O.Graph(s, t, num_nodes=N, index_base=0, ndata={"x": pos})
    return g, og, rng


def oracle_phi(phi, ps):
    return [dict(weight=ps[n]["weight"].detach().cpu().double().numpy(), bias=ps[n]["bias"].detach().cpu().double().numpy(),
                 act=l.activation) for n, l in zip(phi.names(), phi.chain)]


def device_params(ps, rng):
    ps = ng.to_device(ps, DEV)
    for lp in ps.values():
        lp["bias"] = torch.as_tensor(rng.normal(size=tuple(lp["bias"].shape)).astype(np.float32) * 0.3, device=DEV)
        for v in lp.values():
            v.requires_grad_(True)
    return ps


def flat_grads(ps):
    return [ps[n][k].grad for n in ps for k in ("weight", "bias")]


@pytest.mark.parametrize("aggr", ["mean", "+", "max"])
def test_user_layer_matches_explicit_edge_conv(aggr):
    h = 6
    g, og, rng = edgeconv_case(h=h)
    phi = ng.Chain(ng.Dense(2 * h + 2, 16, "tanh"), ng.Dense(16, 9, "tanh"))
    mine, ref = UserEdgeConv(phi, initialgraph=g, aggr=aggr), ng.ExplicitEdgeConv(phi, initialgraph=g, aggr=aggr)
    ps, st = ng.setup(3, mine)
    assert list(st) == ["ϕ", "graph"] and list(ps) == ["layer_1", "layer_2"]
    ps1 = device_params(ps, np.random.default_rng(4))
    ps2 = {n: {k: v.detach().clone().requires_grad_(True) for k, v in lp.items()} for n, lp in ps1.items()}
    x0 = rng.normal(size=(h, og.num_nodes)).astype(np.float32)
    x1, x2 = dev(x0), dev(x0)
    y1, _ = mine(x1, ps1, st)
    y2, _ = ref(x2, ps2, ng.setup(3, ref)[1])
    yo, c = O.explicit_edge_conv(x0.astype(np.float64), oracle_phi(phi, ps1), og, aggr)
    close(y1, y2.detach().cpu().double().numpy(), rtol=1e-5, atol=1e-6, what="y vs ExplicitEdgeConv")
    close(y1, yo, what="y vs float64")
    R = rng.normal(size=yo.shape) * np.isfinite(yo)
    Rt = torch.as_tensor(R, dtype=torch.float32, device=DEV)
    for y in (y1, y2):
        (torch.where(torch.isfinite(y), y, torch.zeros_like(y)) * Rt).sum().backward()
    close(x1.grad, x2.grad.cpu().double().numpy(), rtol=1e-5, atol=1e-6, what="dx vs ExplicitEdgeConv")
    for a, b in zip(flat_grads(ps1), flat_grads(ps2)):
        close(a, b.cpu().double().numpy(), rtol=1e-5, atol=1e-6, what="dparam vs ExplicitEdgeConv")
    gr = O.explicit_edge_conv_backward(c, R)
    gclose(x1.grad, gr["x"], what="dx vs float64")
    for a, gl in zip(flat_grads(ps1), [v for gp in gr["phi"] for v in (gp["weight"], gp["bias"])]):
        gclose(a, gl, what="dparam vs float64")


# ---- apply_edges ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("D", [1, 3, 64, 130])
def test_apply_edges_xi_dot_xj_in_coo_order(name, D):
    g, og = make(name)
    rng = np.random.default_rng(D)
    a, b = rng.normal(size=(D, og.num_nodes)), rng.normal(size=(D, og.num_nodes))
    at, bt = dev(a), dev(b)
    y = ng.apply_edges(ng.xi_dot_xj, g, xi=at, xj=bt)
    ref = (O.gather(a, og.t) * O.gather(b, og.s)).sum(axis=0, keepdims=True)
    close(y, ref)
    R = rng.normal(size=ref.shape)
    (y * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
    gclose(at.grad, O.scatter("+", R * O.gather(b, og.s), og.t, og.num_nodes), what="dxi")
    gclose(bt.grad, O.scatter("+", R * O.gather(a, og.t), og.s, og.num_nodes), what="dxj")


@pytest.mark.parametrize("name", list(GRAPHS))
def test_apply_edges_user_function(name):
    g, og = make(name)
    rng = np.random.default_rng(11)
    N, E = og.num_nodes, og.num_edges
    a, b, e = rng.normal(size=(5, N)), rng.normal(size=(5, N)), rng.normal(size=(5, E))
    at, bt, et = dev(a), dev(b), dev(e)
    y = ng.apply_edges(lambda xi, xj, ee: torch.tanh(xi["h"] * ee - xj["h"]), g, xi={"h": at}, xj={"h": bt}, e=et)
    ai, bj = O.gather(a, og.t), O.gather(b, og.s)
    z = ai * e - bj
    close(y, np.tanh(z))
    R = rng.normal(size=(5, E))
    (y * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
    dz = R * (1 - np.tanh(z) ** 2)
    gclose(at.grad, O.scatter("+", dz * e, og.t, N), what="dxi")
    gclose(bt.grad, O.scatter("+", -dz, og.s, N), what="dxj")
    gclose(et.grad, dz * ai, what="de")


def test_aggregate_neighbors_takes_coo_order():
    g, og = make("hub")
    rng = np.random.default_rng(9)
    for aggr in AGGRS:
        m = draw(rng, (7, og.num_edges), aggr)
        mt = dev(m)
        y = ng.aggregate_neighbors(g, aggr, mt)
        yo = O.scatter(aggr, m, og.t, og.num_nodes)
        close(y, yo, what=aggr)
        R = rng.normal(size=yo.shape) * np.isfinite(yo)
        (torch.where(torch.isfinite(y), y, torch.zeros_like(y)) * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
        gclose(mt.grad, O.scatter_pullback(aggr, m, og.t, og.num_nodes, yo, R), what="dm " + aggr)


# ---- softmax_edge_neighbors -------------------------------------------------------------------------------------------------------


def softmax_ref(e, t, n):
    mx = O.scatter("max", e, t, n)
    z = np.exp(e - O.gather(mx, t))
    return z / O.gather(O.scatter("+", z, t, n), t)


@pytest.mark.parametrize("name", list(GRAPHS))
@pytest.mark.parametrize("H", [1, 4])
def test_softmax_edge_neighbors(name, H):
    g, og = make(name)
    rng = np.random.default_rng(H)
    E, N = og.num_edges, og.num_nodes
    e = rng.normal(size=(H, E)) * 3
    et = dev(e)
    y = ng.softmax_edge_neighbors(g, et)
    yo = softmax_ref(e, og.t, N)
    close(y, yo)
    sums = O.scatter("+", y.detach().cpu().double().numpy(), og.t, N)
    has_in = np.bincount(og.t, minlength=N) > 0
    assert np.abs(sums[:, has_in] - 1).max(initial=0) < 1e-5
    R = rng.normal(size=(H, E))
    (y * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
    deo = yo * (R - O.gather(O.scatter("+", yo * R, og.t, N), og.t))
    gclose(et.grad, deo, what="de")


def test_softmax_edge_neighbors_large_logits_stay_finite():
    g, og = make("hub")
    rng = np.random.default_rng(0)
    e = rng.choice([-80.0, 80.0], size=(4, og.num_edges)) + rng.normal(size=(4, og.num_edges))
    y = ng.softmax_edge_neighbors(g, dev(e, False))
    assert torch.isfinite(y).all()
    close(y, softmax_ref(e, og.t, og.num_nodes))
    yv = ng.softmax_edge_neighbors(g, dev(e[0], False))      # a vector of logits: a vector back
    assert tuple(yv.shape) == (og.num_edges,) and torch.isfinite(yv).all()


# ---- reproducibility ---------------------------------------------------------------------------------------------------------------


def test_every_entry_is_bitwise_reproducible():
    g, og = make("hub")
    rng = np.random.default_rng(21)
    N, E = og.num_nodes, og.num_edges
    x, xb = rng.normal(size=(64, N)), rng.normal(size=(64, N))
    ed, e1, e4 = rng.normal(size=(64, E)), rng.normal(size=(1, E)), rng.normal(size=(4, E))

    def run():
        xt, xbt, edt, e1t, e4t = dev(x), dev(xb), dev(ed), dev(e1), dev(e4)
        outs = [ng.propagate(ng.e_mul_xj, g, "mean", xj=xt, e=edt), ng.propagate(ng.e_mul_xj, g, "+", xj=xt, e=e1t),
                ng.propagate(lambda a, b, c: a["h"] * b["h"], g, "+", xi={"h": xt}, xj={"h": xbt}),
                ng.apply_edges(ng.xi_dot_xj, g, xi=xt, xj=xbt), ng.softmax_edge_neighbors(g, e4t)]
        sum((o * (k + 1)).sum() for k, o in enumerate(outs)).backward()
        return [o.detach().cpu() for o in outs] + [v.grad.cpu() for v in (xt, xbt, edt, e1t, e4t)]

    a, b = run(), run()
    for u, v in zip(a, b):
        assert torch.equal(u, v)


# ---- inside a NeuralODE ------------------------------------------------------------------------------------------------------------


def test_user_layer_as_neural_ode_rhs():
    h, n_steps = 4, 10
    g, og, rng = edgeconv_case(N=120, E=600, h=h, seed=8)
    phi = ng.Chain(ng.Dense(2 * h + 2, 16, "tanh"), ng.Dense(16, h, "tanh"))
    layer = UserEdgeConv(phi, initialgraph=g, aggr="mean")
    node = ng.NeuralODE(layer, solver="tsit5", n_steps=n_steps)
    ps, st = ng.setup(5, node)
    ps = device_params(ps, np.random.default_rng(6))
    u0 = rng.normal(size=(h, og.num_nodes)).astype(np.float32)
    ut = dev(u0)
    uT, _ = node(ut, ps, st)
    opar = oracle_phi(phi, ps)
    pos = og.ndata["x"]

    def message(xi, xj, e):
        return O.mlp_forward(opar, np.concatenate([xi["h"], xj["h"], xj["x"] - xi["x"]]))[0]

    def rhs(u):
        return O.propagate(message, og, "mean", xi={"h": u, "x": pos}, xj={"h": u, "x": pos}), u

    uTo, tape = O.rk_solve(rhs, u0.astype(np.float64), O.TSIT5, 1.0 / n_steps, n_steps)
    close(uT, uTo, what="u(T)")

    def vjp(u, kbar):
        _, c = O.explicit_edge_conv(u, opar, og, "mean")
        return O.explicit_edge_conv_backward(c, kbar)["x"], None

    R = rng.normal(size=uTo.shape)
    (uT * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
    du0 = O.rk_adjoint(vjp, tape, R, O.TSIT5, 1.0 / n_steps, lambda pg: None)
    gclose(ut.grad, du0, what="du0")

    # adaptive Tsit5 at a tight tolerance lands on the fixed-step solution
    anode = ng.NeuralODE(layer, solver="tsit5", adaptive=True, reltol=1e-7, abstol=1e-9)
    with torch.no_grad():
        uA, _ = anode(dev(u0, False), ps, st)
    assert anode.stats["naccept"] >= 1
    close(uA, uT.detach().cpu().double().numpy(), rtol=1e-4, atol=1e-5, what="adaptive vs fixed")
