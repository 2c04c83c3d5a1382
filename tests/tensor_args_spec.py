"""The table behind tests/test_tensor_args_host.py and tests/test_tensor_args_gpu.py: one row per public callable that takes a
real-valued array, and the explicit set of the names that are not swept.

A row names the public callables it sweeps (`public`), builds its plain arguments as float32 numpy arrays in Julia's shapes
(`args`), calls the package on torch tensors of any dtype, strides and device (`call`) and states the same operation in float64
numpy on oracle/ngpde_oracle.py (`oracle`).  The tests apply the variants to the arguments; nothing here knows about them.

One graph serves all rows: 70 nodes (three 32-row tiles, the last one ragged) and about 300 edges between nodes at most six apart
(so that its tiles fit the LDS halo and GATConv 64 => 4 x 16 takes its one-launch form), with and without stored edge weights.
Only the smooth activations are used (identity, tanh, swish): no kink can flip between two evaluations.

Importing this module needs no GPU and builds nothing.
"""
import numpy as np
import torch

import ngpde_amd as ng
from oracle import ngpde_oracle as O

N = 70
SEED = 20240


def _graph_arrays():
    rng = np.random.default_rng(SEED)
    ss, tt = [], []
    for i in range(N):
        for off in rng.choice(np.array([o for o in range(-6, 7) if o != 0]), size=rng.integers(3, 7), replace=False):
            ss.append((i + off) % N)
            tt.append(i)
    s, t = np.array(ss, dtype=np.int64), np.array(tt, dtype=np.int64)
    E = s.size
    return dict(s=s, t=t, E=E, w=rng.uniform(0.5, 1.5, E).astype(np.float32), pos=rng.random((2, N)).astype(np.float32),
                ef=rng.random((1, E)).astype(np.float32), theta=rng.random(2).astype(np.float32),
                gi=np.repeat(np.arange(3), [23, 24, 23]).astype(np.int64))


_G = {}


def graphs():
    """the package's graphs and the oracle's, built once: plain / with node positions / with edge + graph features / with stored
    edge weights / as a batch of three graphs (per-graph readouts)"""
    if not _G:
        a = _graph_arrays()
        s, t = a["s"], a["t"]
        kw = dict(num_nodes=N, index_base=0)
        f64 = lambda v: np.asarray(v, dtype=np.float64)
        _G.update(a)
        _G["g"], _G["og"] = ng.GNNGraph(s, t, **kw), O.Graph(s, t, **kw)
        _G["g_pos"], _G["og_pos"] = ng.GNNGraph(s, t, ndata={"x": a["pos"]}, **kw), O.Graph(s, t, ndata={"x": f64(a["pos"])}, **kw)
        feats = dict(ndata={"x": a["pos"]}, edata={"e": a["ef"]}, gdata={"θ": a["theta"]})
        _G["g_mp"] = ng.GNNGraph(s, t, **feats, **kw)
        _G["og_mp"] = O.Graph(s, t, **{k: {n: f64(v) for n, v in d.items()} for k, d in feats.items()}, **kw)
        _G["g_w"], _G["og_w"] = ng.GNNGraph(s, t, edge_weight=a["w"], **kw), O.Graph(s, t, edge_weight=f64(a["w"]), **kw)
        _G["g_b"] = ng.GNNGraph(s, t, graph_indicator=a["gi"], **kw)
    return _G


# ---- parameter trees <-> flat argument dicts ---------------------------------------------------------------------------------------


def flatten(tree, prefix=""):
    out = {}
    for k, v in tree.items():
        if isinstance(v, dict):
            out.update(flatten(v, prefix + k + "."))
        else:
            out[prefix + k] = v
    return out


def unflatten(flat, like, prefix=""):
    return {k: (unflatten(flat, v, prefix + k + ".") if isinstance(v, dict) else flat[prefix + k]) for k, v in like.items()}


def _init_params(layer, seed):
    """the layer's initial parameters as float32 numpy arrays, biases drawn at random (the initialiser gives zeros)"""
    rng = np.random.default_rng(seed)
    ps, st = ng.setup(seed, layer)
    flat = {k: v.numpy().astype(np.float32) for k, v in flatten(ps).items()}
    for k, v in flat.items():
        if k.endswith("bias"):
            flat[k] = (rng.normal(size=v.shape) * 0.3).astype(np.float32)
    return ps, st, flat


def _mlp(layer, tree):
    """oracle form of a Dense / Chain of Dense with float64 parameters"""
    pairs = [(layer, tree)] if isinstance(layer, ng.Dense) else [(l, tree[n]) for n, l in zip(layer.names(), layer.chain)]
    return [dict(weight=p["weight"], bias=p.get("bias"), act=l.activation) for l, p in pairs]


def _mlp_grads(layer, grads, prefix):
    """{argument name: gradient} of a Dense / Chain of Dense from the oracle's per-layer list"""
    names = [""] if isinstance(layer, ng.Dense) else [n + "." for n in layer.names()]
    out = {}
    for n, g in zip(names, grads):
        for k, v in g.items():
            out[prefix + n + k] = v
    return out


# ---- rows ---------------------------------------------------------------------------------------------------------------------


class Row:
    """name: the row's id; public: the names of ng.__all__ it sweeps; grad: the arguments that get a gradient (None: all);
    fwd_tol / grad_tol: (rtol, atol) against float64 for tests/test_mp_gpu.close, grad_tol per argument with "*" as the default;
    reproducible: two plain calls give the same bits; refuses_cpu: a CPU array among GPU arrays raises ArgumentError (but for the
    arguments in cpu_accepted)"""
    name, public, grad = None, (), None
    fwd_tol = (1e-4, 1e-5)                     # test_mp_gpu.close at its defaults
    grad_tol = {"*": (5e-4, 2e-4)}
    reproducible, pullback, refuses_cpu = True, True, True
    cpu_accepted = ()                          # arguments that may stay on the CPU, with the reason in the row

    def args(self):
        raise NotImplementedError

    def call(self, t):
        raise NotImplementedError

    def oracle(self, a, R):
        raise NotImplementedError

    def tol(self, arg):
        return self.grad_tol.get(arg, self.grad_tol["*"])

    def grad_names(self):
        return tuple(self.args()) if self.grad is None else tuple(self.grad)


class LayerRow(Row):
    """one layer call y = layer(x, ps, st): the arguments are x and every parameter leaf (dotted names)"""

    def __init__(self, name, public, make, x_rows, seed, x_cols=N):
        self.name, self.public, self._make, self.x_shape, self.seed = name, public, make, (x_rows, x_cols), seed
        self._built = None

    def built(self):
        if self._built is None:
            layer, fwd, bwd = self._make()
            ps, st, flat = _init_params(layer, self.seed)
            self._built = dict(layer=layer, ps=ps, st=st, flat=flat, fwd=fwd, bwd=bwd)
        return self._built

    def args(self):
        b = self.built()
        x = np.random.default_rng(self.seed + 1).normal(size=self.x_shape).astype(np.float32)
        return {"x": x, **b["flat"]}

    def call(self, t):
        b = self.built()
        return b["layer"](t["x"], unflatten(t, b["ps"]), b["st"])[0]

    def rhs(self, a):
        """(x -> (y, cache), (cache, dy) -> {argument: gradient}) in float64 with the parameters of `a`"""
        b = self.built()
        tree = unflatten(a, b["ps"])
        return (lambda x: b["fwd"](tree, x)), (lambda c, dy: b["bwd"](tree, c, dy))

    def oracle(self, a, R):
        f, vjp = self.rhs(a)
        y, c = f(a["x"])
        return y, (None if R is None else vjp(c, R))


def _fix(grads, like):
    """the oracle's gradients in the arguments' shapes (a bias is (out x 1))"""
    return {k: np.asarray(v).reshape(like[k].shape) for k, v in grads.items() if k in like}


def _gcn(din, dout, act, gkey="g", **kw):
    def make():
        G = graphs()
        layer = ng.GCNConv((din, dout), act, initialgraph=G[gkey], **kw)
        og = G["o" + gkey]
        fwd = lambda p, x: O.gcn_conv(x, p["weight"], p["bias"], og, act, use_edge_weight=kw.get("use_edge_weight", False))
        bwd = lambda p, c, dy: O.gcn_conv_backward(c, dy)
        return layer, fwd, bwd
    return make


def _dense(din, dout, act):
    def make():
        layer = ng.Dense(din, dout, act)
        fwd = lambda p, x: O.mlp_forward(_mlp(layer, p), x)

        def bwd(p, c, dy):
            dx, gr = O.mlp_backward(_mlp(layer, p), c, dy)
            return {"x": dx, **_mlp_grads(layer, gr, "")}
        return layer, fwd, bwd
    return make


def _gat(din, c, heads, act, concat=True):
    def make():
        G = graphs()
        layer = ng.GATConv((din, c), act, heads=heads, concat=concat, initialgraph=G["g"])
        fwd = lambda p, x: O.gat_conv(x, p["weight"], p["a"], p["bias"], G["og"], heads, c, act, concat=concat)
        bwd = lambda p, cch, dy: O.gat_conv_backward(cch, dy)
        return layer, fwd, bwd
    return make


def _edgeconv(h):
    def make():
        G = graphs()
        phi = ng.Chain(ng.Dense(2 * h + 2, 16, "tanh"), ng.Dense(16, 9, "swish"))
        layer = ng.ExplicitEdgeConv(phi, initialgraph=G["g_pos"], aggr="mean")
        fwd = lambda p, x: O.explicit_edge_conv(x, _mlp(phi, p), G["og_pos"], "mean")

        def bwd(p, c, dy):
            gr = O.explicit_edge_conv_backward(c, dy)
            return {"x": gr["x"], **_mlp_grads(phi, gr["phi"], "")}
        return layer, fwd, bwd
    return make


def _vmh(h, phi_dims, gam_dims):
    def make():
        G = graphs()
        phi = ng.Chain(ng.Dense(2 * h + 2, phi_dims[0], "tanh"), ng.Dense(phi_dims[0], phi_dims[1]))
        gam = ng.Chain(ng.Dense(h + phi_dims[1], gam_dims[0], "tanh"), ng.Dense(gam_dims[0], gam_dims[1]))
        layer = ng.VMHConv(phi, gam, initialgraph=G["g_pos"], aggr="mean")
        fwd = lambda p, x: O.vmh_conv(x, _mlp(phi, p["ϕ"]), _mlp(gam, p["γ"]), G["og_pos"], "mean")

        def bwd(p, c, dy):
            gr = O.vmh_conv_backward(c, dy)
            return {"x": gr["x"], **_mlp_grads(phi, gr["phi"], "ϕ."), **_mlp_grads(gam, gr["gamma"], "γ.")}
        return layer, fwd, bwd
    return make


def _mppde(h):
    def make():
        G = graphs()
        phi = ng.Chain(ng.Dense(2 * h + 2 + 1 + 2, 16, "swish"), ng.Dense(16, 12, "swish"))
        psi = ng.Chain(ng.Dense(h + 12 + 2, 16, "swish"), ng.Dense(16, h))
        layer = ng.MPPDEConv(phi, psi, initialgraph=G["g_mp"], aggr="mean")
        fwd = lambda p, x: O.mppde_conv(x, _mlp(phi, p["ϕ"]), _mlp(psi, p["ψ"]), G["og_mp"], "mean")

        def bwd(p, c, dy):
            gr = O.mppde_conv_backward(c, dy)
            return {"x": gr["x"], **_mlp_grads(phi, gr["phi"], "ϕ."), **_mlp_grads(psi, gr["psi"], "ψ.")}
        return layer, fwd, bwd
    return make


def _gno(cin, cout):
    def make():
        G = graphs()
        phi = ng.Chain(ng.Dense(2 * 2 + 1, 16, "tanh"), ng.Dense(16, cin * cout))
        layer = ng.GNOConv((cin, cout), phi, "tanh", initialgraph=G["g_mp"])
        fwd = lambda p, x: O.gno_conv(x, _mlp(phi, p["ϕ"]), p["linear"]["weight"], p["linear"]["bias"], G["og_mp"], cin, cout, "tanh")

        def bwd(p, c, dy):
            gr = O.gno_conv_backward(c, dy)
            return {"x": gr["x"], "linear.weight": gr["weight"], "linear.bias": gr["bias"], **_mlp_grads(phi, gr["phi"], "ϕ.")}
        return layer, fwd, bwd
    return make


def _spectral(n):
    def make():
        layer = ng.SpectralConv(n)
        og = O.spectral_graph(n)
        fwd = lambda p, x: (O.spectral_conv(x, og, n), None)
        bwd = lambda p, c, dy: {"x": -O.spectral_conv(dy, og, n)}       # the operator is antisymmetric
        return layer, fwd, bwd
    return make


def _chain2(make_a, make_b):
    """Chain(layer_1, layer_2) of two layer factories"""
    def make():
        (la, fa, ba), (lb, fb, bb) = make_a(), make_b()
        layer = ng.Chain(la, lb)

        def fwd(p, x):
            y1, c1 = fa(p["layer_1"], x)
            y2, c2 = fb(p["layer_2"], y1)
            return y2, (c1, c2)

        def bwd(p, c, dy):
            g2 = bb(p["layer_2"], c[1], dy)
            g1 = ba(p["layer_1"], c[0], g2["x"])
            out = {"x": g1["x"]}
            out.update({"layer_1." + k: v for k, v in g1.items() if k != "x"})
            out.update({"layer_2." + k: v for k, v in g2.items() if k != "x"})
            return out
        return layer, fwd, bwd
    return make


class ApplyRow(LayerRow):
    """the same call through ng.apply(layer, x, ps, st)"""

    def call(self, t):
        b = self.built()
        return ng.apply(b["layer"], t["x"], unflatten(t, b["ps"]), b["st"])[0]


class GcnEdgeWeightRow(LayerRow):
    """GCNConv called with the `edge_weight` argument (src/layers.jl:200-233), which gets a gradient (ngpde_gcn_backward_ew).
    Weights that need no gradient are graph data: like the weights a GNNGraph stores they may be host arrays, and the graph handle
    uploads them with the normalisation it is built for (tests/test_gcn_gpu.py passes them so).  A weight leaf that requires a gradient
    must live on the GPU (ArgumentError)"""
    cpu_accepted = ("edge_weight",)

    def args(self):
        return {**super().args(), "edge_weight": graphs()["w"].copy()}

    def call(self, t):
        b = self.built()
        ps = unflatten(t, b["ps"])
        return b["layer"](t["x"], ps, b["st"], edge_weight=t["edge_weight"])[0]

    def oracle(self, a, R):
        b = self.built()
        p = unflatten(a, b["ps"])
        y, c = O.gcn_conv(a["x"], p["weight"], p["bias"], graphs()["og"], b["layer"].activation, edge_weight=a["edge_weight"].reshape(-1))
        return y, (None if R is None else O.gcn_conv_backward(c, R))


class NodeRow(Row):
    """NeuralODE(model): a fixed-step solve and its discrete adjoint, against oracle.rk_solve / rk_adjoint over the layer row's own
    float64 right-hand side.  resident: the solve must have taken a device-resident plan"""

    def __init__(self, name, layer_row, solver, n_steps, resident, grad_tol):
        self.name, self.public, self.layer_row, self.solver, self.n_steps, self.resident = name, ("NeuralODE",), layer_row, solver, n_steps, resident
        self.grad_tol = grad_tol
        self.node = None

    def built(self):
        if self.node is None:
            self.node = ng.NeuralODE(self.layer_row.built()["layer"], solver=self.solver, n_steps=self.n_steps, dt=0.25)
        return self.node

    def args(self):
        return self.layer_row.args()

    def call(self, t):
        b = self.layer_row.built()
        return self.built()(t["x"], unflatten(t, b["ps"]), b["st"])[0]

    def oracle(self, a, R):
        f, vjp = self.layer_row.rhs(a)
        tab = O.TABLEAUS[self.solver]
        uT, tape = O.rk_solve(f, a["x"], tab, 0.25, self.n_steps)
        if R is None:
            return uT, None
        acc = {}

        def accumulate(pg):
            for k, v in pg.items():
                acc[k] = acc.get(k, 0.0) + np.asarray(v).reshape(a[k].shape)

        def rhs_vjp(c, kbar):
            g = vjp(c, kbar)
            return g["x"], {k: v for k, v in g.items() if k != "x"}
        acc["x"] = O.rk_adjoint(rhs_vjp, tape, R, tab, 0.25, accumulate)
        return uT, acc


class FnRow(Row):
    """a public function of arrays: args / call / oracle given as callables"""

    def __init__(self, name, public, args, call, oracle, grad=None, **kw):
        self.name, self.public, self._args, self._call, self._oracle, self.grad = name, public, args, call, oracle, grad
        for k, v in kw.items():
            setattr(self, k, v)

    def args(self):
        return self._args()

    def call(self, t):
        return self._call(t)

    def oracle(self, a, R):
        return self._oracle(a, R)


def _rand(shape, seed):
    return lambda: np.random.default_rng(seed).normal(size=shape).astype(np.float32)


def _fn_rows():
    G = _graph_arrays()
    s, t, E = G["s"], G["t"], G["E"]
    indeg = np.bincount(t, minlength=N).astype(np.float64)
    cnt = np.where(indeg > 0, indeg, 1.0)
    MP = {"*": (5e-4, 1e-6)}               # tests/test_msgpass_gpu.py and tests/test_readout_gpu.py bound gradients by 5e-4, 1e-6
    rows = []

    def add(name, public, args, call, oracle, **kw):
        rows.append(FnRow(name, public, args, call, oracle, grad_tol=kw.pop("grad_tol", MP), **kw))

    # propagate with each built-in message
    add("propagate_copy_xj_sum", ("propagate", "copy_xj"), lambda: {"xj": _rand((8, N), 1)()},
        lambda a: ng.propagate(ng.copy_xj, graphs()["g"], "+", xj=a["xj"]),
        lambda a, R: (O.scatter("+", a["xj"][:, s], t, N), None if R is None else {"xj": O.scatter("+", R[:, t], s, N)}))

    def emul_oracle(a, R):
        m = a["e"] * a["xj"][:, s]
        y = O.scatter("mean", m, t, N)
        if R is None:
            return y, None
        dm = (R / cnt)[:, t]
        return y, {"xj": O.scatter("+", dm * a["e"], s, N), "e": (dm * a["xj"][:, s]).sum(axis=0, keepdims=True)}
    add("propagate_e_mul_xj_mean", ("propagate", "e_mul_xj"), lambda: {"xj": _rand((8, N), 2)(), "e": _rand((1, E), 3)()},
        lambda a: ng.propagate(ng.e_mul_xj, graphs()["g"], "mean", xj=a["xj"], e=a["e"]), emul_oracle)
    w64 = G["w"].astype(np.float64)
    add("propagate_w_mul_xj_sum", ("propagate", "w_mul_xj"), lambda: {"xj": _rand((5, N), 4)()},
        lambda a: ng.propagate(ng.w_mul_xj, graphs()["g_w"], "+", xj=a["xj"]),
        lambda a, R: (O.scatter("+", w64 * a["xj"][:, s], t, N), None if R is None else {"xj": O.scatter("+", w64 * R[:, t], s, N)}))
    add("propagate_copy_xi_sum", ("propagate", "copy_xi"), lambda: {"xi": _rand((5, N), 5)()},
        lambda a: ng.propagate(ng.copy_xi, graphs()["g"], "+", xi=a["xi"]),
        lambda a, R: (a["xi"] * indeg, None if R is None else {"xi": R * indeg}))

    def dot_edges(a):
        return (a["xi"][:, t] * a["xj"][:, s]).sum(axis=0, keepdims=True)

    def dot_grads(a, dm):
        return {"xi": O.scatter("+", dm * a["xj"][:, s], t, N), "xj": O.scatter("+", dm * a["xi"][:, t], s, N)}
    two = lambda seed: (lambda: {"xi": _rand((8, N), seed)(), "xj": _rand((8, N), seed + 1)()})
    add("propagate_xi_dot_xj_sum", ("propagate", "xi_dot_xj"), two(6),
        lambda a: ng.propagate(ng.xi_dot_xj, graphs()["g"], "+", xi=a["xi"], xj=a["xj"]),
        lambda a, R: (O.scatter("+", dot_edges(a), t, N), None if R is None else dot_grads(a, R[:, t])))
    add("apply_edges_xi_dot_xj", ("apply_edges",), two(8),
        lambda a: ng.apply_edges(ng.xi_dot_xj, graphs()["g"], xi=a["xi"], xj=a["xj"]),
        lambda a, R: (dot_edges(a), None if R is None else dot_grads(a, R)))
    add("apply_edges_e_mul_xj", ("apply_edges",), lambda: {"xj": _rand((5, N), 10)(), "e": _rand((5, E), 11)()},
        lambda a: ng.apply_edges(ng.e_mul_xj, graphs()["g"], xj=a["xj"], e=a["e"]),
        lambda a, R: (a["e"] * a["xj"][:, s], None if R is None else {"xj": O.scatter("+", R * a["e"], s, N), "e": R * a["xj"][:, s]}))
    add("aggregate_neighbors_mean", ("aggregate_neighbors",), lambda: {"m": _rand((6, E), 12)()},
        lambda a: ng.aggregate_neighbors(graphs()["g"], "mean", a["m"]),
        lambda a, R: (O.scatter("mean", a["m"], t, N), None if R is None else {"m": (R / cnt)[:, t]}))

    def seg_softmax(x, idx, n):
        mx = O.scatter("max", x, idx, n)
        ex = np.exp(x - mx[:, idx])
        return ex / O.scatter("+", ex, idx, n)[:, idx]

    def seg_softmax_oracle(key, idx, n):
        def oracle(a, R):
            y = seg_softmax(a[key], idx, n)
            if R is None:
                return y, None
            return y, {key: y * (R - O.scatter("+", y * R, idx, n)[:, idx])}
        return oracle
    add("softmax_edge_neighbors", ("softmax_edge_neighbors",), lambda: {"e": _rand((2, E), 13)()},
        lambda a: ng.softmax_edge_neighbors(graphs()["g"], a["e"]), seg_softmax_oracle("e", t, N))

    # per-graph readouts on the batch of three graphs (an edge belongs to its source's graph)
    gi = G["gi"]
    ge = gi[s]
    ncnt, ecnt = np.bincount(gi, minlength=3).astype(np.float64), np.bincount(ge, minlength=3).astype(np.float64)
    add("reduce_nodes_mean", ("reduce_nodes",), lambda: {"x": _rand((8, N), 14)()},
        lambda a: ng.reduce_nodes("mean", graphs()["g_b"], a["x"]),
        lambda a, R: (O.scatter("+", a["x"], gi, 3) / ncnt, None if R is None else {"x": (R / ncnt)[:, gi]}))
    add("reduce_edges_sum", ("reduce_edges",), lambda: {"e": _rand((5, E), 15)()},
        lambda a: ng.reduce_edges("+", graphs()["g_b"], a["e"]),
        lambda a, R: (O.scatter("+", a["e"], ge, 3), None if R is None else {"e": R[:, ge]}))
    add("softmax_nodes", ("softmax_nodes",), lambda: {"x": _rand((8, N), 16)()},
        lambda a: ng.softmax_nodes(graphs()["g_b"], a["x"]), seg_softmax_oracle("x", gi, 3))
    add("softmax_edges", ("softmax_edges",), lambda: {"e": _rand((5, E), 17)()},
        lambda a: ng.softmax_edges(graphs()["g_b"], a["e"]), seg_softmax_oracle("e", ge, 3))
    add("broadcast_nodes", ("broadcast_nodes",), lambda: {"u": _rand((8, 3), 18)()},
        lambda a: ng.broadcast_nodes(graphs()["g_b"], a["u"]),
        lambda a, R: (a["u"][:, gi], None if R is None else {"u": O.scatter("+", R, gi, 3)}))
    add("broadcast_edges", ("broadcast_edges",), lambda: {"u": _rand((5, 3), 19)()},
        lambda a: ng.broadcast_edges(graphs()["g_b"], a["u"]),
        lambda a, R: (a["u"][:, ge], None if R is None else {"u": O.scatter("+", R, ge, 3)}))

    # GraphMatrix.matmul: X @ A.T with A[s, t] = the summed weights of the edges s -> t
    A = np.zeros((N, N))
    np.add.at(A, (s, t), w64)
    matrix = {}

    def matmul(a):
        if "m" not in matrix:
            matrix["m"] = ng.adjacency_matrix(graphs()["g_w"])
        return matrix["m"].matmul(a["X"])
    add("graph_matrix_matmul", ("GraphMatrix", "adjacency_matrix"), lambda: {"X": _rand((6, N), 20)()}, matmul,
        lambda a, R: (a["X"] @ A.T, None if R is None else {"X": R @ A}))
    return rows


class OptimRow(Row):
    """flatten_parameters + one Adam step: the arguments are the parameter leaves, the result is the updated flat vector.
    flatten_parameters copies every leaf into one buffer on the device of the first (`ps |> device`): a CPU leaf among GPU leaves
    is copied like the others, not refused"""
    name, public, pullback, refuses_cpu = "optim_adam_step", (), False, False
    fwd_tol = (2e-6, 1e-7)                    # tests/test_optim_gpu.py

    def args(self):
        rng = np.random.default_rng(21)
        return {"weight": rng.normal(size=(5, 7)).astype(np.float32), "bias": rng.normal(size=(5, 1)).astype(np.float32)}

    @staticmethod
    def _grad(n):
        return np.linspace(-1.0, 1.0, n).astype(np.float32)

    def call(self, t):
        from ngpde_amd import optim
        flat, _ = optim.flatten_parameters({"weight": t["weight"], "bias": t["bias"]}, device="cuda")
        flat.grad.copy_(torch.as_tensor(self._grad(flat.numel())))
        st = optim.setup(optim.Adam(0.01), flat)
        optim.update(st, flat)
        return flat.data.reshape(1, -1)

    def oracle(self, a, R):
        x = np.concatenate([a["weight"].reshape(-1), a["bias"].reshape(-1)]).astype(np.float32)
        x1, _ = O.adam_step(x, self._grad(x.size), O.adam_init(x), 0.01)
        return np.asarray(x1, dtype=np.float64).reshape(1, -1), None


GCN_TOL = {"*": (2e-4, 1e-4), "x": (2e-4, 1e-5), "edge_weight": (2e-4, 1e-5)}     # tests/test_gcn_gpu.py
MP_TOL = {"*": (5e-4, 2e-4), "x": (5e-4, 1e-4)}                                   # tests/test_mp_gpu.py check_grads
GAT_TOL = {"*": (5e-4, 5e-4), "x": (5e-4, 1e-4)}                                  # tests/test_mp_gpu.py test_gat_parity_and_grads
SPECTRAL_TOL = {"*": (2e-4, 1e-3)}                                                # tests/test_mp_gpu.py, SpectralConv's gradient
NODE_GCN_TOL = {"*": (5e-4, 1e-3), "x": (5e-4, 1e-4)}      # tests/test_gcn_gpu.py, NeuralODE(GCNConv, GCNConv): du0, dW, db
NODE_GAT_TOL = {"*": (5e-4, 5e-4), "x": (5e-4, 1e-4)}      # tests/test_mp_gpu.py, NeuralODE(GATConv): parameters at atol 5e-4
NODE_VMH_TOL = {"*": (5e-4, 2e-4), "x": (5e-4, 1e-4)}      # tests/test_node_vmh_gpu.py through test_mp_gpu.check_grads


def _rows():
    L = LayerRow
    gcn64 = L("gcn_64x64_fused", ("GCNConv",), _gcn(64, 64, "tanh"), 64, 31)
    gcn75 = L("gcn_7x5_stored_weights", ("GCNConv",), _gcn(7, 5, "swish", "g_w", use_edge_weight=True), 7, 32)
    gcn57 = L("gcn_5x7", ("GCNConv",), _gcn(5, 7, "identity"), 5, 33)
    gcnew = GcnEdgeWeightRow("gcn_7x5_edge_weight_argument", ("GCNConv",), _gcn(7, 5, "tanh"), 7, 34)
    layers = [gcn64, gcn75, gcn57, gcnew]
    for r in layers:
        r.grad_tol = GCN_TOL
    mp = [L("dense_64x64", ("Dense",), _dense(64, 64, "tanh"), 64, 35), L("dense_5x3", ("Dense",), _dense(5, 3, "swish"), 5, 36),
          ApplyRow("chain_dense", ("Chain", "apply"), _chain2(_dense(5, 8, "tanh"), _dense(8, 3, "identity")), 5, 37),
          L("edgeconv", ("ExplicitEdgeConv",), _edgeconv(6), 6, 41), L("vmh", ("VMHConv",), _vmh(3, (16, 9), (16, 4)), 3, 42),
          L("mppde", ("MPPDEConv",), _mppde(5), 5, 43), L("gno", ("GNOConv",), _gno(6, 5), 6, 44)]
    for r in mp:
        r.grad_tol = MP_TOL
    gat = [L("gat_64_4x16_one_launch", ("GATConv",), _gat(64, 16, 4, "tanh"), 64, 38),
           L("gat_8_2x3_primitives", ("GATConv",), _gat(8, 3, 2, "swish"), 8, 39),
           L("gat_8_2x3_mean", ("GATConv",), _gat(8, 3, 2, "tanh", concat=False), 8, 40)]
    for r in gat:
        r.grad_tol = GAT_TOL
    spectral = L("spectral", ("SpectralConv",), _spectral(N), 3, 45)
    spectral.grad_tol = SPECTRAL_TOL
    # NeuralODE: two Euler steps and one Tsit5 step over each right-hand side
    rhs_gcn2 = L("rhs_gcn2_16", (), _chain2(_gcn(16, 16, "tanh"), _gcn(16, 16, "tanh")), 16, 46)
    rhs_gat = L("rhs_gat", (), _gat(64, 16, 4, "tanh"), 64, 47)
    rhs_vmh = L("rhs_vmh", (), _vmh(1, (60, 40), (60, 1)), 1, 48)
    rhs_generic = L("rhs_gcn_7x7", (), _gcn(7, 7, "tanh"), 7, 49)
    nodes = []
    for solver, steps in (("euler", 2), ("tsit5", 1)):
        for tag, rhs, resident, tol in (("gcn2", rhs_gcn2, True, NODE_GCN_TOL), ("gat", rhs_gat, True, NODE_GAT_TOL),
                                        ("vmh", rhs_vmh, True, NODE_VMH_TOL), ("generic", rhs_generic, False, NODE_GCN_TOL)):
            nodes.append(NodeRow(f"node_{solver}_{tag}", rhs, solver, steps, resident, tol))
    return layers + mp + gat + [spectral] + nodes + _fn_rows() + [OptimRow()]


ROWS = _rows()
ROWS_BY_NAME = {r.name: r for r in ROWS}
assert len(ROWS_BY_NAME) == len(ROWS)

# ---- graph data: real-valued arrays that a GNNGraph stores or a graph builder reads ----------------------------------------------------------
# Not arguments of a kernel call, but converted on the way to one by whoever consumes them (graphs._as_matrix_t / _device_points,
# graphops._f32_device, the handle's normalisation).  One row per consumer: the result on a graph whose data came in as a variant
# must equal, bit for bit, the result on the same values as a plain float32 contiguous device tensor.  Host arrays are accepted
# (graph data are uploaded); that the plain results are right is what each module's own GPU test checks against float64.


def _sym():
    G = _graph_arrays()
    return np.concatenate([G["s"], G["t"]]), np.concatenate([G["t"], G["s"]]), np.concatenate([G["w"], G["w"]])


def _wg(w):
    sb, tb, _ = _sym()
    return ng.GNNGraph(sb, tb, num_nodes=N, index_base=0, edge_weight=w)


def _set_get(w):
    sb, tb, _ = _sym()
    g = ng.set_edge_weight(ng.GNNGraph(sb, tb, num_nodes=N, index_base=0), w)
    assert ng.get_edge_weight(g) is w
    return ng.degree(g, "out")


def _plain_graph():
    sb, tb, _ = _sym()
    return ng.GNNGraph(sb, tb, num_nodes=N, index_base=0)


def _edges(g):
    return torch.as_tensor(np.stack(g.edge_index(0)))


def _feature_graph(kind):
    G = _graph_arrays()
    return lambda v: ng.GNNGraph(G["s"], G["t"], num_nodes=N, index_base=0, **{kind: {"x": v}}).packed(kind, "cuda")


class DataRow:
    def __init__(self, name, public, arg, call):
        self.name, self.public, self.arg, self.call = name, public, arg, call

    def value(self):
        G = _graph_arrays()
        return {"w": _sym()[2], "points": G["pos"], "ndata": G["pos"], "edata": np.concatenate([G["ef"], 2 * G["ef"]])}[self.arg]


DATA_ROWS = [
    DataRow("stored_weights_degree", ("GNNGraph", "degree"), "w", lambda w: ng.degree(_wg(w), "in")),
    DataRow("degree_argument", ("degree",), "w", lambda w: ng.degree(_plain_graph(), "both", edge_weight=w)),
    DataRow("set_get_edge_weight", ("set_edge_weight", "get_edge_weight"), "w", _set_get),
    DataRow("laplacian_matrix", ("laplacian_matrix",), "w", lambda w: ng.laplacian_matrix(_wg(w)).to_dense()),
    DataRow("normalized_laplacian", ("normalized_laplacian",), "w", lambda w: ng.normalized_laplacian(_wg(w)).to_dense()),
    DataRow("scaled_laplacian", ("scaled_laplacian",), "w", lambda w: ng.scaled_laplacian(_wg(w), lambda_max=2.0).to_dense()),
    DataRow("laplacian_lambda_max", ("laplacian_lambda_max",), "w", lambda w: torch.tensor([ng.laplacian_lambda_max(_wg(w))])),
    DataRow("random_walk_pe", ("random_walk_pe",), "w", lambda w: ng.random_walk_pe(_wg(w), 3)),
    DataRow("stored_weights_shortest_paths", ("GNNGraph",), "w", lambda w: ng.shortest_paths(_wg(w), [0]).dist),
    DataRow("stored_weights_w_mul_xj", ("GNNGraph",), "w", lambda w: ng.propagate(ng.w_mul_xj, _wg(w), "+", xj=torch.ones(2, N, device="cuda"))),
    DataRow("node_features", ("GNNGraph",), "ndata", _feature_graph("ndata")),
    DataRow("edge_features", ("GNNGraph",), "edata", _feature_graph("edata")),
    DataRow("radius_graph", ("radius_graph",), "points", lambda p: _edges(ng.radius_graph(p, 0.2))),
    DataRow("knn_graph", ("knn_graph",), "points", lambda p: _edges(ng.knn_graph(p, 4))),
]

# ---- the names of ng.__all__ that no row sweeps, each with the reason ---------------------------------------------------------------------
NO_ARRAY = "takes no real-valued array"
INDEX = "integer index arguments only, normalised by its module (graphops / editing / queries / sampling / traversal)"
STRICT = "refuses anything but float32 by name"
NOT_SWEPT = {
    **{n: NO_ARRAY for n in (
        "AbstractExplicitLayer", "AbstractGNNLayer", "AbstractGNNContainerLayer", "setup", "to_device", "updategraph", "wrapgraph", "drop", "EMPTYGRAPH",
        "rand_graph", "batch", "glorot_uniform", "glorot_normal", "zeros32", "NgpdeError", "DimensionMismatch", "ArgumentError",
        "graph_indicator", "CGInfo", "AdjacencyList", "Components", "ShortestPaths")},
    **{n: INDEX for n in (
        "has_self_loops", "has_multi_edges", "is_bidirected", "add_self_loops", "remove_self_loops", "remove_multi_edges", "to_bidirected",
        "induced_subgraph", "getgraph", "unbatch", "sample_neighbors", "rand_edge_split", "add_nodes", "add_edges", "remove_edges",
        "remove_nodes", "to_unidirected", "negative_sample", "has_isolated_nodes", "adjacency_list", "has_edge", "neighbors", "inneighbors",
        "outneighbors", "intersect", "connected_components", "is_connected", "split_components", "hop_distance", "neighborhood", "khop_adj")},
    "cg_solve": STRICT,
    "shortest_paths": STRICT,      # (its edge_weight argument; the graph's own stored weights are a DATA_ROWS row)
}
