"""The Python layer between a caller's tensors and the C entries, without a GPU: the one rule for real-valued arrays (the docstring
of layers.rows_of) as far as it can be checked with CPU tensors.

  * the helpers (rows_of, vec_of, mat_of) give float32 contiguous arrays with equal values for every dtype, stride and offset, are
    differentiable, and copy nothing that already is in the kernels' order;
  * every layer, and NeuralODE over every right-hand side, refuses a parameter of the wrong size with DimensionMismatch BEFORE the graph
    handle is built or the library is entered: with CPU tensors a well-shaped call fails later, with another error (no device / no CPU
    fallback), so a DimensionMismatch can only have come from the size check.  No test hands a wrong-size array to a library entry;
  * every name in ng.__all__ is either swept by a row of tests/tensor_args_spec.py or listed there with the reason why not.

What these tests and their GPU companion would have shown before the rule, each from the code as it was:
  strided bias   the bias was `ps["bias"].reshape(-1)`, which keeps the stride of a view such as buf[::2]; the autograd nodes passed its
                 data_ptr() on without `.contiguous()`, so the kernel read the base buffer's neighbouring elements.
  float64 bias   nothing compared the dtype: the kernel read the first 4 n bytes of 8 n as float32 bit patterns.
  short bias     the layer path never compared the bias with `out` (only _check_plan_shapes did, for the resident plans): the kernel
                 read past the end of the array on the device.  Never run; refused here with CPU tensors only.
  GATConv        rows_of(ps["weight"]) and rows_of(ps["a"]) went to ngpde_gat_layer_forward / ngpde_gat_forward with no comparison against
                 (in, heads * c) and (2 c, heads): a wrong shape was not refused, the kernels walked the arrays by the layer's sizes.
"""
import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd.layers import mat_of, rows_of, vec_of

import tensor_args_spec as T


# ---- the helpers --------------------------------------------------------------------------------------------------------------------

BASE = torch.arange(12.0).reshape(3, 4) - 3.0          # small integers: exact in every dtype below


def _variants(x):
    """(name, tensor with x's values) for every dtype / stride / offset form"""
    big = torch.zeros(tuple(2 * d for d in x.shape))
    big[tuple(slice(None, None, 2) for _ in x.shape)] = x
    off = torch.zeros(x.numel() + 1)
    off[1:] = x.reshape(-1)
    return [("float64", x.double()), ("bfloat16", x.bfloat16()), ("int64", x.long()), ("float16", x.half()),
            ("stride 2", big[tuple(slice(None, None, 2) for _ in x.shape)]), ("offset", off[1:].reshape(x.shape)),
            ("numpy float64", x.double().numpy())]


@pytest.mark.parametrize("name,v", _variants(BASE), ids=[n for n, _ in _variants(BASE)])
def test_rows_of_gives_float32_contiguous_rows(name, v):
    r = rows_of(v)
    assert r.dtype == torch.float32 and r.is_contiguous() and tuple(r.shape) == (4, 3)
    assert torch.equal(r, BASE.T)


def test_rows_of_stride_zero():
    col = torch.tensor([[1.0], [2.0], [3.0]])
    r = rows_of(col.expand(3, 5))
    assert r.dtype == torch.float32 and r.is_contiguous() and torch.equal(r, col.expand(3, 5).T)
    assert r.stride() == (3, 1)                        # materialised: no stride 0 reaches a kernel


def test_rows_of_passes_a_column_major_float32_matrix_without_a_copy():
    rows = torch.randn(5, 3)
    x = rows.T                                         # (3 x 5) column-major: the package's native order
    assert rows_of(x).data_ptr() == rows.data_ptr()
    buf = torch.zeros(16)
    view = buf[1:16].reshape(5, 3).T                   # the same, one float into its storage
    assert rows_of(view).data_ptr() == buf.data_ptr() + 4
    assert rows_of(torch.randn(3, 5)).data_ptr() != 0 and rows_of(torch.randn(3, 5)).is_contiguous()      # row-major: one copy


def test_rows_of_refuses_what_is_no_real_matrix():
    with pytest.raises(ng.DimensionMismatch):
        rows_of(torch.zeros(3))
    with pytest.raises(ng.ArgumentError):
        rows_of(torch.zeros(3, 2, dtype=torch.complex64))


VEC = torch.tensor([-2.0, 0.0, 1.0, 5.0])


@pytest.mark.parametrize("shape", [(4,), (4, 1), (1, 4)])
@pytest.mark.parametrize("name,v", _variants(VEC), ids=[n for n, _ in _variants(VEC)])
def test_vec_of_gives_a_float32_contiguous_vector(name, v, shape):
    b = vec_of(v.reshape(shape), 4, "bias")
    assert b.dtype == torch.float32 and b.is_contiguous() and tuple(b.shape) == (4,) and torch.equal(b, VEC)


def test_vec_of_strided_column_does_not_read_its_neighbours():
    # the (out x 1) bias view of the issue: reshape(-1) alone keeps the stride, and a kernel would read 0 1 2 3 for 0 2 4 6
    view = torch.arange(8.0).reshape(8, 1)[::2]
    assert view.reshape(-1).stride() == (2,)
    b = vec_of(view, 4, "bias")
    assert b.is_contiguous() and b.tolist() == [0.0, 2.0, 4.0, 6.0]
    assert vec_of(torch.tensor(7.0).expand(4, 1), 4, "bias").stride() == (1,)
    assert vec_of(torch.tensor(7.0).expand(4, 1), 4, "bias").tolist() == [7.0] * 4


def test_vec_of_copies_nothing_that_is_a_float32_vector_already():
    b = torch.randn(6, 1)
    assert vec_of(b, 6, "bias").data_ptr() == b.data_ptr()
    assert vec_of(None, 6, "bias") is None


@pytest.mark.parametrize("n", [3, 5])
def test_vec_of_names_the_array_and_both_sizes(n):
    with pytest.raises(ng.DimensionMismatch) as e:
        vec_of(torch.zeros(4, 1), n, "layer_2: bias")
    assert "layer_2: bias" in str(e.value) and "4" in str(e.value) and str(n) in str(e.value)
    with pytest.raises(ng.DimensionMismatch):
        vec_of(torch.zeros(2, 2), 4, "bias")           # four entries, but no vector


def test_mat_of_checks_the_julia_shape():
    assert tuple(mat_of(torch.zeros(3, 5), (3, 5), "weight").shape) == (5, 3)
    with pytest.raises(ng.DimensionMismatch) as e:
        mat_of(torch.zeros(5, 3), (3, 5), "Dense: weight")
    assert "Dense: weight" in str(e.value) and "(5, 3)" in str(e.value) and "(3, 5)" in str(e.value)


@pytest.mark.parametrize("helper", ["rows_of", "vec_of"])
def test_a_float64_leaf_receives_a_float64_gradient(helper):
    leaf = torch.arange(6.0, dtype=torch.float64).reshape(3, 2).requires_grad_(True) if helper == "rows_of" else \
        torch.arange(6.0, dtype=torch.float64).reshape(6, 1).requires_grad_(True)
    out = rows_of(leaf) if helper == "rows_of" else vec_of(leaf, 6, "bias")
    assert out.dtype == torch.float32
    w = torch.arange(1.0, 7.0).reshape(out.shape)
    (out * w).sum().backward()
    assert leaf.grad.dtype == torch.float64 and tuple(leaf.grad.shape) == tuple(leaf.shape)
    want = w.T if helper == "rows_of" else w.reshape(6, 1)
    assert torch.equal(leaf.grad, want.double())       # the float32 gradient, cast


# ---- refusals before the handle and the library --------------------------------------------------------------------------------------

LAYER_ROWS = [r for r in T.ROWS if isinstance(r, (T.LayerRow, T.NodeRow))]


def _cpu_args(row):
    """plain float32 CPU tensors in the package's native order (matrices column-major)"""
    return {k: (torch.as_tensor(v).T.contiguous().T if v.ndim == 2 else torch.as_tensor(v)) for k, v in row.args().items()}


def _resized(t, dim, delta):
    shape = list(t.shape)
    shape[dim] += delta
    return torch.zeros(shape)


def _wrong_sizes(args):
    """(what, argument name, replacement): every bias one too short and one too long, every weight and attention matrix with one row
    or one column too many or too few"""
    for k, v in args.items():
        leaf = k.split(".")[-1]
        if leaf == "bias":
            yield "short bias", k, _resized(v, 0, -1)
            yield "long bias", k, _resized(v, 0, +1)
            yield "flat long bias", k, torch.zeros(v.numel() + 1)
        elif leaf in ("weight", "a"):
            for dim in (0, 1):
                for delta in (-1, +1):
                    if v.shape[dim] + delta > 0:
                        yield f"{leaf} dim {dim} {delta:+d}", k, _resized(v, dim, delta)
            yield f"{leaf} transposed", k, (torch.zeros(v.shape[1], v.shape[0]) if v.shape[0] != v.shape[1] else _resized(v, 0, 1))


@pytest.mark.parametrize("row", LAYER_ROWS, ids=[r.name for r in LAYER_ROWS])
def test_wrong_sizes_are_refused_before_the_handle_and_the_library(row):
    args = _cpu_args(row)
    # the well-shaped call gets past the size checks and fails where the device is needed: not a DimensionMismatch
    with pytest.raises(Exception) as ok:
        row.call(args)
    assert not isinstance(ok.value, ng.DimensionMismatch), ok.value
    assert isinstance(ok.value, ng.NgpdeError), ok.value
    cases = list(_wrong_sizes(args))
    assert cases or not [k for k in args if k != "x"]              # (SpectralConv has no parameters)
    for what, k, bad in cases:
        with pytest.raises(ng.DimensionMismatch) as e:
            row.call({**args, k: bad})
        assert k.split(".")[-1] in str(e.value), (what, k, e.value)        # the message names the array
    # the input, where the layer itself knows its width: a wrong feature count and, where it has a graph, a wrong node count
    layer = row.built()["layer"] if isinstance(row, T.LayerRow) else None
    if isinstance(layer, (ng.Dense, ng.GCNConv, ng.GATConv)):
        for dim in (0,) if isinstance(layer, ng.Dense) else (0, 1):
            with pytest.raises(ng.DimensionMismatch):
                row.call({**args, "x": _resized(args["x"], dim, +1)})


def test_every_layer_kind_has_a_refusal_row():
    kinds = {type(r.built()["layer"]).__name__ for r in LAYER_ROWS if isinstance(r, T.LayerRow)}
    assert kinds >= {"Dense", "GCNConv", "GATConv", "ExplicitEdgeConv", "VMHConv", "MPPDEConv", "GNOConv", "SpectralConv", "Chain"}
    gat = [r.built()["layer"] for r in LAYER_ROWS if isinstance(r, T.LayerRow) and isinstance(r.built()["layer"], ng.GATConv)]
    assert {l.concat for l in gat} == {True, False}
    rhs = {type(r.layer_row.built()["layer"]).__name__ for r in LAYER_ROWS if isinstance(r, T.NodeRow)}
    assert rhs >= {"Chain", "GATConv", "VMHConv", "GCNConv"}


def test_gcn_edge_weight_argument_sizes():
    row = T.ROWS_BY_NAME["gcn_7x5_edge_weight_argument"]
    args = _cpu_args(row)
    for delta in (-1, +1):
        with pytest.raises(ng.ArgumentError) as e:           # the reference's own error for this one (src/layers.jl:207)
            row.call({**args, "edge_weight": torch.zeros(args["edge_weight"].numel() + delta)})
        assert "Wrong number of edge weights" in str(e.value)


def test_propagate_copy_xj_checks_its_edge_weights_before_the_library():
    # functional.propagate_copy_xj / propagate_sum (SpectralConv's aggregation): one weight per edge of the handle's graph
    from ngpde_amd import functional as F

    class Handle:                                           # (what the wrapper reads of a graph handle before it enters the library)
        ptr, _n_edges = None, 12
    x = torch.zeros(5, 3)
    for n in (11, 13):
        for call in (F.propagate_copy_xj, F.propagate_sum):
            with pytest.raises(ng.DimensionMismatch) as e:
                call(x, Handle(), edge_weight=torch.zeros(n))
            assert "edge_weight" in str(e.value) and str(n) in str(e.value) and "12" in str(e.value)
    with pytest.raises(ng.DimensionMismatch):
        F.propagate_copy_xj(x, Handle(), edge_weight=torch.zeros(3, 4, 1))
    for ok in (torch.zeros(12), torch.zeros(1, 12), torch.zeros(12, dtype=torch.float64), torch.zeros(24)[::2]):
        with pytest.raises(ng.NgpdeError) as e:             # well-shaped: no CPU fallback
            F.propagate_copy_xj(x, Handle(), edge_weight=ok)
        assert not isinstance(e.value, ng.DimensionMismatch)


def test_functional_wrappers_refuse_a_bias_of_the_wrong_length_before_the_library():
    # the autograd nodes under the layers check what they pass on, too: a caller of functional.dense / bias_act / gat_layer with
    # CPU tensors gets the size error, not the device error
    from ngpde_amd import functional as F
    x, wt = torch.zeros(6, 5), torch.zeros(5, 3)
    for b in (torch.zeros(2), torch.zeros(4)):
        with pytest.raises(ng.DimensionMismatch):
            F.dense([x], wt, b, 0)
        with pytest.raises(ng.DimensionMismatch):
            F.bias_act(torch.zeros(6, 3), None, b, 0)
    with pytest.raises(ng.ArgumentError):                   # well-shaped: no CPU fallback
        F.dense([x], wt, torch.zeros(3), 0)


# ---- completeness ----------------------------------------------------------------------------------------------------------------------


def test_every_public_name_is_swept_or_listed():
    swept = {n for r in list(T.ROWS) + list(T.DATA_ROWS) for n in r.public}
    assert not (swept & set(T.NOT_SWEPT)), swept & set(T.NOT_SWEPT)
    missing = [n for n in ng.__all__ if n not in swept and n not in T.NOT_SWEPT]
    assert not missing, f"public names neither swept by a row of tensor_args_spec.ROWS nor listed in NOT_SWEPT: {missing}"
    stale = [n for n in list(swept) + list(T.NOT_SWEPT) if n not in ng.__all__]
    assert not stale, stale
    assert set(T.NOT_SWEPT.values()) <= {T.NO_ARRAY, T.INDEX, T.STRICT}
    # no reason may stand for a conversion nobody checks: besides the array-free names only the entries that refuse by name are exempt
    assert {n for n, why in T.NOT_SWEPT.items() if why == T.STRICT} == {"cg_solve", "shortest_paths"}


def test_strict_entries_refuse_by_name():
    from ngpde_amd import traversal
    g = T.graphs()["g"]
    for bad in (torch.ones(g.num_edges, dtype=torch.float64), np.ones(g.num_edges), torch.ones(g.num_edges, dtype=torch.bfloat16)):
        with pytest.raises(ng.ArgumentError) as e:
            traversal._path_weights(g, bad)
        assert "float32" in str(e.value)
    with pytest.raises(ng.DimensionMismatch):
        traversal._path_weights(g, torch.ones(g.num_edges + 1))
    assert traversal._path_weights(g, torch.ones(g.num_edges)) is not None


def test_the_rows_cover_what_the_sweep_lists():
    names = set(T.ROWS_BY_NAME)
    for solver in ("euler", "tsit5"):
        assert {f"node_{solver}_{k}" for k in ("gcn2", "gat", "vmh", "generic")} <= names
    assert len({r.name for r in T.ROWS if "propagate" in r.public}) >= 5     # each built-in message
    g = T.graphs()
    assert g["g"].num_nodes == 70 and 250 <= g["g"].num_edges <= 350 and g["g_w"].edge_weight is not None
    acts = {l.activation for r in T.ROWS if isinstance(r, T.LayerRow) for l in _dense_and_conv(r.built()["layer"])}
    assert acts <= {"identity", "tanh", "swish"}, acts


def _dense_and_conv(layer):
    if isinstance(layer, ng.Chain):
        return [x for l in layer.chain for x in _dense_and_conv(l)]
    out = [layer] if hasattr(layer, "activation") else []
    for name in getattr(layer, "layers", ()):
        out += _dense_and_conv(layer.sublayer(name))
    if hasattr(layer, "linear"):
        out.append(layer.linear)
    return out
