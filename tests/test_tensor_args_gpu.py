"""Every Python entry against dtype, stride, offset and size variants of its real-valued arguments (the rule in the docstring of
layers.rows_of), on the device.  The rows -- one per public callable that takes a real-valued array, at one shape that takes the
entry's fused form and one that does not -- are in tests/tensor_args_spec.py; this file applies the variants.

For every row:
  baseline   (a) the plain call (fresh, float32, contiguous, allocator-aligned tensors) run twice gives the same bits, outputs and
                 gradients; (b) it matches the float64 oracle: the forward within test_mp_gpu.close at its defaults, each gradient
                 within the bound that entry's own GPU test uses (named next to the row's grad_tol in the spec).
  variants   applied to every real-valued argument, one at a time, then to all at once:
               float64      .double()                                       == plain, bit for bit; the leaf's gradient is float64 and
                                                                               equals the plain gradient cast
               bfloat16     .bfloat16()                                     == the call on .bfloat16().float(), bit for bit
               strided      every second element of a doubled buffer,       == plain, bit for bit
                            for a matrix also every second column
               order        the other storage order (row-major, where       == plain, bit for bit
                            column-major is native)
               stride0      expand of a scalar / a column to the shape      == the call on the materialised array, bit for bit
               offset       the same values one float into a longer         the float64 oracle within the bounds of (b): the form
                            storage, in the native order (no copy is made)  may change, so no bit claim; the pointer is asserted
                                                                            to be 4 bytes off a multiple of 16
               cpu          .cpu() of one argument                          ArgumentError
  cotangents a stride-0 cotangent (y.sum()), a cotangent in the other storage order and a float64 cotangent ((y.double() * M).sum())
             give the gradients of the plain contiguous float32 cotangent, bit for bit.
No public wrapper lets its caller supply an output buffer, so there is none to pre-fill with NaN.  No wrong-size array is passed to
anything here (tests/test_tensor_args_host.py refuses them on the CPU).

Misaligned pointers, per entry the layers call -- found by READING each launcher and kernel, before any of this ran:
  chooses its scalar form itself (tests every caller pointer for 16-byte alignment); the wrapper passes the view as it is
    ngpde_dense_forward / _backward          dense_forms.h aligned16() on every block, weight, y, save_z, dz, dx, partial
    ngpde_bias_act_forward                   gcn_generic.hip launch_bias_act: al16 of a, addend, bias, y, save_z
    ngpde_gather_forward / _backward         msgpass.hip: per array al16(x), al16(out_i), al16(out_j) / al16(g_i), al16(g_j), al16(dx)
    ngpde_propagate_emul_*                   msgpass.hip: al16 of X, out, x_own, de, e
    ngpde_apply_edges_dot_*                  msgpass.hip: al16(A), al16(B)
    ngpde_segment_reduce_*                   mp_kernels.hip launch_segment_reduce: al16(M), al16(out)
    ngpde_readout_*                          readout.hip: al16 of x / y / out / dout / dx / u and the workspace in all six entries
    ngpde_rk_stage_combine, _dense_output*,  optim.hip: the OR of all operand addresses & 15
    ngpde_rk_error_norm
  touches its caller pointers with 4-byte accesses only (one kernel, one float per access); the wrapper passes the view as it is
    ngpde_propagate_copy_xj                  gcn_generic.hip spmm_generic_kernel: x[idx], edge_weight[e], out[idx] as float
    ngpde_edge_permute                       mp_kernels.hip edge_permute_kernel: dst[..] = src[..] per float
    ngpde_softmax_edge_neighbors_*           msgpass.hip softmax_edge_fwd / bwd_kernel: e[..], y[..], dy[..], de[..] per float
    ngpde_bias_act_backward                  mp_kernels.hip dense_dz_kernel per float, gcn_generic.hip colsum kernels a[r * d + o]
    ngpde_spectral_weights                   mp_kernels.hip spectral_weight_kernel: e[i], w[i]
    ngpde_accumulate_many                    optim.hip accumulate_many_kernel: acc[i], g[i]
  neither holds, or not every launch behind the entry was traced: the WRAPPER copies a misaligned view into a fresh buffer
  (functional._f32a), so these entries never see such a pointer from Python
    ngpde_gcn_forward / _backward / _ew      gcn_fused.hip reads x, weight, bias, z, saved_agg, dy and writes y, save_z as float4, untested
                                             (the any-width path tests its block in api_gcn.hip one_seg; the fused one does not)
    ngpde_gat_layer_forward / _backward      gat_fused.hip: float4 tile loads, no pointer test
    ngpde_gat_forward / _backward            gat_scores_kernel reads wx and a per float and the backward tests wx | dout
                                             (mp_kernels.hip), but the fused forward (gat_fused.hip) has no test
    ngpde_edge_layer_*                       api_layers.hip runs Dense (tested), edge_combine (al16 tested, mp_kernels.hip) and the
                                             message-MLP launches of edge_mlp*.hip, which were not traced to every pointer
    ngpde_gno_layer_*                        gno_gform.hip tests its operands (& 15) for its own forms; gno_mfma.hip was not traced
    ngpde_node_gcn2_* / ngpde_ode_*          the persistent kernels stage weights with untested float4 loads (node_persistent.hip)
"""
import numpy as np
import pytest
import torch

import ngpde_amd as ng

import tensor_args_spec as T
from test_mp_gpu import close

pytestmark = pytest.mark.gpu
DEV = "cuda"

ROWS = T.ROWS
IDS = [r.name for r in ROWS]
PULLBACK_ROWS = [r for r in ROWS if r.pullback]


# ---- building arguments -------------------------------------------------------------------------------------------------------------


def native(t):
    """float32 copy of t's values in the package's native order (a matrix column-major, as Julia stores it) in a fresh allocation"""
    t = t.detach().to(torch.float32)
    return t.T.contiguous().T.clone(memory_format=torch.preserve_format) if t.dim() == 2 else t.contiguous().clone()


def v_float64(p):
    return p.double()


def v_bfloat16(p):
    return p.bfloat16()


def v_strided(p):
    if p.dim() == 2:
        buf = torch.full((2 * p.shape[1], 2 * p.shape[0]), float("nan"), device=p.device).T      # column-major, doubled both ways
        v = buf[::2, ::2]
    else:
        buf = torch.full((2 * p.numel(),), float("nan"), device=p.device)
        v = buf[::2]
    v.copy_(p)
    assert not v.is_contiguous() or v.numel() <= 1
    return v


def v_order(p):
    if p.dim() != 2 or min(p.shape) == 1:
        return None                                   # a vector has one storage order
    v = p.contiguous()                                # row-major
    assert not v.T.is_contiguous()
    return v


def v_stride0(p):
    if p.numel() == 1:
        return None                                   # one entry: nothing to expand
    if p.dim() == 2:
        v = (p[:1, :1] if p.shape[1] == 1 else p[:, :1]).expand(p.shape)       # a scalar for a column, else the first column
    else:
        v = p[:1].expand(p.shape)
    assert 0 in v.stride()
    return v


def v_offset(p):
    n = p.numel()
    buf = torch.full((n + 5,), float("nan"), device=p.device)
    assert buf.data_ptr() % 16 == 0
    flat = buf[1:1 + n]
    v = flat.view(p.shape[1], p.shape[0]).T if p.dim() == 2 else flat
    v.copy_(p)
    assert v.data_ptr() % 16 == 4                      # really 4 bytes off a multiple of 16
    assert (v.T if v.dim() == 2 else v).is_contiguous()                        # native order: no copy is made on the way in
    return v


def v_cpu(p):
    return p.cpu()


VARIANTS = {"float64": v_float64, "bfloat16": v_bfloat16, "strided": v_strided, "order": v_order, "stride0": v_stride0,
            "offset": v_offset, "cpu": v_cpu}
KEEPS_VALUES = {"float64", "strided", "order", "offset"}


# ---- running a row ------------------------------------------------------------------------------------------------------------------


class Plain:
    """a row's plain arguments on the device, its cotangent, its plain result and the float64 oracle: computed once, shared"""
    _cache = {}

    def __init__(self, row):
        self.row = row
        self.np_args = row.args()
        self.args = {k: native(torch.as_tensor(v, device=DEV)) for k, v in self.np_args.items()}
        if row.pullback:      # the cotangent has the result's shape, which the float64 statement of the row knows
            shape = row.oracle({k: np.asarray(v, dtype=np.float64) for k, v in self.np_args.items()}, None)[0].shape
            self.R = native(torch.as_tensor(np.random.default_rng(7).normal(size=shape), dtype=torch.float32, device=DEV))
            self.R_np = self.R.cpu().double().numpy()
        else:
            self.R = self.R_np = None
        self.y, self.grads = run(row, self.args, self.R)
        self.oracle = None

    @classmethod
    def of(cls, row):
        if row.name not in cls._cache:
            cls._cache[row.name] = cls(row)
        return cls._cache[row.name]

    def reference(self):
        if self.oracle is None:
            a64 = {k: v.cpu().double().numpy() for k, v in self.args.items()}
            yo, go = self.row.oracle(a64, self.R_np)
            self.oracle = (yo, None if go is None else T._fix(go, a64))
        return self.oracle


def run(row, args, R):
    """(y, {argument: gradient}) of one call; every argument that takes a gradient is a leaf with the given dtype and strides"""
    names = row.grad_names() if (row.pullback and R is not None) else ()
    leaves = {k: (v.detach().requires_grad_(True) if (k in names and v.is_floating_point()) else v.detach()) for k, v in args.items()}
    y = row.call(leaves)
    assert y.dtype == torch.float32, (row.name, y.dtype)                       # outputs stay float32
    if not names:
        return y.detach(), {}
    (y * R).sum().backward()
    return y.detach(), {k: leaves[k].grad for k in names}


def same_bits(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    assert torch.equal(a, b) or bool(((a == b) | (a.isnan() & b.isnan())).all()), \
        f"{what}: {int((a != b).sum())} of {a.numel()} entries differ, max |diff| {float((a.double() - b.double()).abs().max()):.3e}"


def against_oracle(row, plain, y, grads, what):
    yo, go = plain.reference()
    close(y, yo, *row.fwd_tol, what=f"{what}: forward")
    for k, g in grads.items():
        assert g is not None, (what, k)
        close(g, go[k], *row.tol(k), what=f"{what}: d{k}")


# ---- baseline -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_plain_call_is_reproducible_and_matches_float64(row):
    plain = Plain.of(row)
    y2, g2 = run(row, {k: native(v) for k, v in plain.args.items()}, plain.R)
    if row.reproducible:
        same_bits(y2, plain.y, f"{row.name}: second plain call")
        for k in g2:
            same_bits(g2[k], plain.grads[k], f"{row.name}: second plain call, d{k}")
    else:
        against_oracle(row, plain, y2, g2, f"{row.name}: second plain call")
    against_oracle(row, plain, plain.y, plain.grads, row.name)
    if isinstance(row, T.NodeRow) and row.resident:
        assert len(row.built()._plans) > 0, f"{row.name}: the solve did not take a device-resident plan"
    if isinstance(row, T.LayerRow) and row.name == "gat_64_4x16_one_launch":
        from ngpde_amd import functional as F
        layer, g = row.built()["layer"], T.graphs()["g"]
        assert F.gat_layer_supported(layer._graph(g).handle(), 64, 4, 16), "the graph's tiles do not fit the one-launch GAT layer"


# ---- variants -------------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("row", ROWS, ids=IDS)
def test_variant(row, variant):
    plain = Plain.of(row)
    make = VARIANTS[variant]
    names = list(plain.args)
    targets = [[k] for k in names] + ([names] if len(names) > 1 and variant != "cpu" else [])
    ran = 0
    for target in targets:
        vargs, skipped = dict(plain.args), False
        for k in target:
            v = make(plain.args[k])
            if v is None:
                skipped = len(target) == 1
                continue
            vargs[k] = v
        if skipped:
            continue
        what = f"{row.name} [{variant} of {'+'.join(target)}]"
        ran += 1
        if variant == "cpu":
            if row.refuses_cpu and target[0] not in row.cpu_accepted:
                with pytest.raises(ng.ArgumentError):
                    row.call(vargs)
            else:
                same_bits(run(row, vargs, None)[0], plain.y, what)
            continue
        y, grads = run(row, vargs, plain.R)
        if variant == "offset":
            against_oracle(row, plain, y, grads, what)
            continue
        if variant in KEEPS_VALUES:
            yref, gref = plain.y, plain.grads
        else:                                          # bfloat16 rounds, stride 0 repeats: the plain call on the materialised values
            yref, gref = run(row, {k: native(v) for k, v in vargs.items()}, plain.R)
        same_bits(y, yref, what)
        for k, g in grads.items():
            assert g is not None and g.dtype == vargs[k].dtype and tuple(g.shape) == tuple(vargs[k].shape), (what, k, g.dtype, tuple(g.shape))
            same_bits(g, gref[k].to(g.dtype), f"{what}: d{k}")
    assert ran > 0, (row.name, variant)


# ---- cotangents ---------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("row", PULLBACK_ROWS, ids=[r.name for r in PULLBACK_ROWS])
def test_cotangent_forms(row):
    plain = Plain.of(row)
    names = row.grad_names()

    def grads_of(back):
        leaves = {k: (v.detach().requires_grad_(True) if k in names else v) for k, v in plain.args.items()}
        back(row.call(leaves))
        return {k: leaves[k].grad for k in names}

    R = plain.R
    Rc = R.contiguous()                                                       # row-major (D x N)
    Rt = R.T.contiguous().T                                                   # column-major
    assert Rc.is_contiguous() and (Rt.T.is_contiguous() or min(R.shape) == 1)
    ref = grads_of(lambda y: y.backward(Rc))
    forms = {"other storage order": lambda y: y.backward(Rt), "float64": lambda y: (y.double() * R.double()).sum().backward()}
    for what, back in forms.items():
        got = grads_of(back)
        for k in names:
            same_bits(got[k], ref[k], f"{row.name}: {what} cotangent, d{k}")
    ones = grads_of(lambda y: y.backward(torch.ones(tuple(y.shape), device=DEV)))
    got = grads_of(lambda y: y.sum().backward())                              # a stride-0 cotangent
    for k in names:
        same_bits(got[k], ones[k], f"{row.name}: stride-0 cotangent, d{k}")


# ---- the GCNConv edge_weight gradient path ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize("form", ["float64", "1 x E", "1 x E float64", "strided"])
def test_gcn_edge_weight_leaf_forms(form):
    row = T.ROWS_BY_NAME["gcn_7x5_edge_weight_argument"]
    plain = Plain.of(row)
    w = plain.args["edge_weight"]
    leaf = {"float64": lambda: w.double(), "1 x E": lambda: w.reshape(1, -1).clone(), "1 x E float64": lambda: w.double().reshape(1, -1),
            "strided": lambda: v_strided(w)}[form]()
    y, grads = run(row, {**plain.args, "edge_weight": leaf}, plain.R)
    same_bits(y, plain.y, f"edge_weight {form}")
    g = grads["edge_weight"]
    assert g.dtype == leaf.dtype and tuple(g.shape) == tuple(leaf.shape), (g.dtype, tuple(g.shape))
    same_bits(g.reshape(-1), plain.grads["edge_weight"].to(g.dtype), f"d edge_weight, {form}")
    for k in ("x", "weight", "bias"):
        same_bits(grads[k], plain.grads[k], f"d{k} with edge_weight {form}")


def test_gcn_edge_weight_leaf_on_the_cpu_is_refused():
    row = T.ROWS_BY_NAME["gcn_7x5_edge_weight_argument"]
    plain = Plain.of(row)
    with pytest.raises(ng.ArgumentError):
        row.call({**plain.args, "edge_weight": plain.args["edge_weight"].cpu().requires_grad_(True)})


# ---- the autograd nodes under the layers, called directly ---------------------------------------------------------------------------------


def test_propagate_copy_xj_edge_weight_forms():
    # functional.propagate_copy_xj / propagate_sum with one weight per edge in every form, against the plain call bit for bit
    from ngpde_amd import functional as F
    G = T.graphs()
    h = G["g"].handle()
    w = torch.as_tensor(G["w"], device=DEV)
    x = torch.as_tensor(np.random.default_rng(3).normal(size=(T.N, 8)), dtype=torch.float32, device=DEV)
    s, t = G["s"], G["t"]
    for by_source in (False, True):
        plain = F.propagate_copy_xj(x, h, "+", w, by_source=by_source)
        ref = T.O.scatter("+", G["w"].astype(np.float64) * x.cpu().double().numpy().T[:, t if by_source else s], s if by_source else t, T.N)
        close(plain, ref.T, what=f"propagate_copy_xj by_source={by_source}")
        forms = {"float64": w.double(), "strided": v_strided(w), "1 x E": w.reshape(1, -1), "E x 1 strided": v_strided(w).reshape(-1, 1),
                 "offset": v_offset(w), "float64 1 x E": w.double().reshape(1, -1)}
        for name, v in forms.items():
            same_bits(F.propagate_copy_xj(x, h, "+", v, by_source=by_source), plain, f"propagate_copy_xj {name} by_source={by_source}")
        same_bits(F.propagate_copy_xj(v_strided(x.T).T, h, "+", w, by_source=by_source), plain, "propagate_copy_xj strided x")
        same_bits(F.propagate_copy_xj(x, h, "+", w[:1].expand(w.shape), by_source=by_source),
                  F.propagate_copy_xj(x, h, "+", w[:1].expand(w.shape).contiguous(), by_source=by_source), "propagate_copy_xj stride 0")
        same_bits(F.propagate_copy_xj(x, h, "+", w.bfloat16(), by_source=by_source),
                  F.propagate_copy_xj(x, h, "+", w.bfloat16().float(), by_source=by_source), "propagate_copy_xj bfloat16")
    xg = x.clone().requires_grad_(True)
    F.propagate_sum(xg, h, v_strided(w).double()).sum().backward()
    xp = x.clone().requires_grad_(True)
    F.propagate_sum(xp, h, w).sum().backward()
    same_bits(xg.grad, xp.grad, "propagate_sum pullback with float64 strided weights")
    with pytest.raises(ng.ArgumentError):
        F.propagate_copy_xj(x, h, "+", w.cpu())


@pytest.mark.parametrize("shape", ["out", "out x 1", "1 x out"])
def test_functional_bias_gradient_has_the_bias_shape(shape):
    # a direct caller of functional.dense / bias_act / gcn_conv with a 2-D (or float64) bias leaf gets its gradient in that shape and type
    from ngpde_amd import functional as F
    rng = np.random.default_rng(5)
    mk = lambda *s: torch.as_tensor(rng.normal(size=s), dtype=torch.float32, device=DEV)
    x, wt, b0 = mk(T.N, 7), mk(7, 5), mk(5)
    as_shape = {"out": lambda b: b.clone(), "out x 1": lambda b: b.reshape(-1, 1).double(), "1 x out": lambda b: b.reshape(1, -1).clone()}[shape]
    h = T.graphs()["g"].handle((True, None, False))
    calls = {"dense": lambda b: F.dense([x], wt, b, 2), "bias_act": lambda b: F.bias_act(x @ wt, None, b, 2),
             "gcn_conv": lambda b: F.gcn_conv(x, wt, b, h, 2)}
    for name, call in calls.items():
        ref = b0.clone().requires_grad_(True)
        yr = call(ref)
        yr.sum().backward()
        leaf = as_shape(b0).requires_grad_(True)
        y = call(leaf)
        y.sum().backward()
        same_bits(y.detach(), yr.detach(), f"{name} {shape}")
        assert leaf.grad.dtype == leaf.dtype and tuple(leaf.grad.shape) == tuple(leaf.shape), (name, leaf.grad.shape)
        same_bits(leaf.grad.reshape(-1), ref.grad.to(leaf.dtype), f"{name} {shape}: db")


# ---- graph data --------------------------------------------------------------------------------------------------------------------------

DATA_FORMS = {"float64": lambda v: v.double(), "bfloat16": lambda v: v.bfloat16(), "float16": lambda v: v.half(), "strided": v_strided,
              "order": v_order, "stride0": v_stride0, "cpu": lambda v: v.cpu(), "numpy float64": lambda v: v.cpu().double().numpy()}


@pytest.mark.parametrize("form", list(DATA_FORMS))
@pytest.mark.parametrize("row", T.DATA_ROWS, ids=[r.name for r in T.DATA_ROWS])
def test_graph_data_forms(row, form):
    """the result on graph data given in `form` == the result on the same values as a plain float32 contiguous device tensor, bit for
    bit (tests/tensor_args_spec.py DATA_ROWS); host arrays are uploaded, not refused"""
    plain = native(torch.as_tensor(row.value(), device=DEV))
    v = DATA_FORMS[form](plain)
    if v is None:
        return                                        # (a vector has one storage order)
    values = torch.as_tensor(v).to(DEV, torch.float32)
    ref = row.call(native(values))
    got = row.call(v)
    same_bits(torch.as_tensor(got).to(DEV), torch.as_tensor(ref).to(DEV), f"{row.name} [{form}]")
    if form in ("float64", "strided", "cpu", "numpy float64"):
        same_bits(torch.as_tensor(got).to(DEV), torch.as_tensor(row.call(plain)).to(DEV), f"{row.name} [{form}] vs plain")
