// api_gcn.hip -- C-ABI entry points of the GCNConv path (declared in include/ngpde.h).
// Replaces (l::GCNConv)(x, ps, st[, edge_weight]) of /root/reference/src/layers.jl:200-239 and the
// pullback Zygote derives for it.
#include <algorithm>

#include "common.h"

using namespace ngpde;

namespace {

// one block of the Dense kernels' segmented-input table
SegTable one_seg(const float *ptr, int width) {
  SegTable t;
  t.n = 1;
  t.ptr[0] = ptr;
  t.width[0] = width;
  t.vec[0] = (width % 4 == 0 && (reinterpret_cast<uintptr_t>(ptr) & 15) == 0) ? 1 : 0;
  for (int i = 1; i <= 4; ++i) t.offset[i] = width;
  return t;
}
SegGrad one_grad(float *ptr, int width) {
  SegGrad t;
  t.n = 1;
  t.ptr[0] = ptr;
  t.width[0] = width;
  for (int i = 1; i <= 4; ++i) t.offset[i] = width;
  return t;
}

int32_t check_common(const char *fn, const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act) {
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: graph is NULL", fn);
  NGPDE_REQUIRE(din > 0 && dout > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: din=%d dout=%d", fn, din, dout);
  NGPDE_REQUIRE(act >= NGPDE_ACT_IDENTITY && act <= NGPDE_ACT_SOFTPLUS, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: unknown activation code %d", fn, act);
  NGPDE_REQUIRE(g->has_norm, NGPDE_ERR_STATE, "%s: GCN normalisation not set (call ngpde_graph_set_gcn_norm)", fn);
  return NGPDE_OK;
}

}  // namespace

extern "C" {

size_t ngpde_gcn_workspace_bytes(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t backward) {
  return g ? gcn_workspace_bytes(gcn_layer_form(g->n_nodes, din, dout), backward != 0, false) : 0;
}

int32_t ngpde_gcn_forward(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act, const float *x,
                          const float *weight, const float *bias, float *y, float *save_agg, float *save_z,
                          void *workspace, size_t workspace_bytes, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  int32_t st = check_common("ngpde_gcn_forward", g, din, dout, act);
  if (st) return st;
  if (g->n_nodes == 0) return NGPDE_OK;  // EMPTYGRAPH (src/layers.jl:14): zero columns in, zero columns out
  NGPDE_REQUIRE(x && weight && y, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gcn_forward: x/weight/y is NULL");
  hipStream_t stream = (hipStream_t)stream_;
  const int64_t n = g->n_nodes;
  const GcnLayerForm f = gcn_layer_form(n, din, dout);   // (gcn_forms.h: the kind, the split, the workspace)
  if (f.fused()) {
    FusedFwdArgs a;
    a.g = g; a.d = din; a.act = act; a.x = x; a.wt = weight; a.bias = bias; a.y = y;
    a.save_agg = save_agg; a.save_z = save_z;
    return launch_fused_fwd(a, stream);
  }
  if ((st = check_workspace("ngpde_gcn_forward", workspace, workspace_bytes, gcn_workspace_bytes(f, false, false), 1))) return st;
  Workspace w(workspace);
  float *tmp = gcn_fwd_layout(w, f);
  if (f.aggregate_first()) {  // aggregate, then multiply (src/layers.jl:235-237)
    float *agg = save_agg ? save_agg : tmp;
    if ((st = launch_spmm_generic(g, false, true, din, NGPDE_AGGR_SUM, x, nullptr, agg, stream))) return st;
    return launch_dense_seg_fwd(n, one_seg(agg, din), din, dout, act, weight, bias, y, save_z, stream);
  }
  // multiply first (src/layers.jl:220-223) -- split over the input features when the row tiles alone cannot fill the chip,
  // the partial products summed in slab order --, then ONE launch: aggregation + bias + activation
  if ((st = launch_dense_seg_fwd_splitk(n, one_seg(x, din), din, dout, weight, tmp, f.nsplit, stream))) return st;
  if ((st = launch_sum_partials(n * dout, f.parts, (size_t)n * dout, tmp, stream))) return st;
  return launch_spmm_gcn_tail(g, dout, tmp, bias, act, y, save_z, stream);
}

}  // extern "C"

namespace {
// bias: only read when dedge_weight is asked for and Dout < Din (x3 = z - bias there)
int32_t gcn_backward_impl(const char *fn, const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act, const float *x, const float *weight,
                          const float *bias, const float *z, const float *saved_agg, const float *dy, float *dx, float *dweight, float *dbias,
                          float *dedge_weight, void *workspace, size_t workspace_bytes, ngpde_stream_t stream_) {
  int32_t st = check_common(fn, g, din, dout, act);
  if (st) return st;
  NGPDE_REQUIRE(dweight != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gcn_backward: dweight is NULL");
  if (dedge_weight && g->n_edges > 0 && g->n_nodes == 0) return fail(NGPDE_ERR_STATE, "edges without nodes");
  if (g->n_nodes == 0) {  // empty graph: zero gradients
    { const int32_t zs = launch_zero(dweight, (size_t)din * dout * 4, (hipStream_t)stream_); if (zs) return zs; }
    if (dbias) { const int32_t zs = launch_zero(dbias, (size_t)dout * 4, (hipStream_t)stream_); if (zs) return zs; }
    return NGPDE_OK;
  }
  NGPDE_REQUIRE(weight && z && dy, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gcn_backward: weight/z/dy is NULL");
  const int64_t n = g->n_nodes;
  const GcnLayerForm f = gcn_layer_form(n, din, dout);
  NGPDE_REQUIRE(!f.needs_saved_agg || saved_agg, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gcn_backward: saved_agg is NULL");
  NGPDE_REQUIRE(!f.needs_x || x, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gcn_backward: x is NULL");
  hipStream_t stream = (hipStream_t)stream_;
  if ((st = check_workspace(fn, workspace, workspace_bytes, gcn_workspace_bytes(f, true, dedge_weight != nullptr), 1))) return st;
  Workspace w(workspace);
  GcnBwdWs p;
  gcn_bwd_layout(w, f, dedge_weight != nullptr, p);
  float *const ew_xw = p.ew_xw, *const ew_nd = p.ew_nd;
  if (dedge_weight) {
    NGPDE_REQUIRE(x != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gcn_backward_ew: x is NULL");
    if (!dx) dx = p.ew_dx;      // the degree term needs the layer's input gradient
  }
  if (f.fused()) {
    float *const slab_dw = p.slab_dw, *const slab_db = p.slab_db, *const gbuf = p.gbuf;
    { const int32_t zs = launch_zero(slab_dw, (size_t)((char *)gbuf - (char *)slab_dw), stream); if (zs) return zs; }
    FusedBwdArgs a;
    a.g = g; a.d = din; a.act = act; a.aggregate = false; a.g_in = dy;
    a.do_dense = true; a.z = z; a.saved_agg = saved_agg; a.wt = weight; a.g_out = gbuf;
    a.slab_dw = slab_dw; a.slab_db = slab_db;
    if ((st = launch_fused_bwd(a, stream))) return st;
    if (dx) {
      FusedBwdArgs b;
      b.g = g; b.d = din; b.act = act; b.aggregate = true; b.g_in = gbuf; b.do_dense = false; b.store_t = dx;
      if ((st = launch_fused_bwd(b, stream))) return st;
    }
    const int ns = fused_num_slabs(n, din);
    if ((st = launch_reduce_slabs(slab_dw, ns, din * dout, din / 16, dweight, stream))) return st;
    if (dbias && (st = launch_reduce_slabs(slab_db, ns, dout, 0, dbias, stream))) return st;
    // gbuf = dz W^T = dL/dx3, saved_agg = x3, the propagated array is x itself
    if (dedge_weight) return launch_gcn_edge_weight_grad(g, din, gbuf, saved_agg, nullptr, dx, x, ew_nd, dedge_weight, stream);
    return NGPDE_OK;
  }
  float *const dz = p.dz, *const tmp = p.tmp, *const partial = p.partial;
  if ((st = launch_act_bwd(n * dout, act, dy, z, dz, stream))) return st;
  if (f.aggregate_first()) {   // y = act(agg W + b): dW = agg^T dz, db = column sums of dz (the weight pullback's bias row), dx = A^T (dz W^T)
    if ((st = launch_dense_seg_bwd_weight(n, one_seg(saved_agg, din), din, dout, dz, dweight, dbias, partial, stream))) return st;
    if (dx) {
      if ((st = launch_dense_seg_bwd_input(n, one_grad(tmp, din), din, dout, dz, weight, stream))) return st;
      if ((st = launch_spmm_generic(g, true, true, din, NGPDE_AGGR_SUM, tmp, nullptr, dx, stream))) return st;
      // tmp = dz W^T = dL/dx3, saved_agg = x3, the propagated array is x itself
      if (dedge_weight) return launch_gcn_edge_weight_grad(g, din, tmp, saved_agg, nullptr, dx, x, ew_nd, dedge_weight, stream);
    }
    return NGPDE_OK;
  }
  // y = act(A (x W) + b): db from dz; g = A^T dz; dW = x^T g; dx = g W^T
  if (dbias && (st = launch_colsum2(n, dout, dz, partial, dbias, stream))) return st;
  if ((st = launch_spmm_generic(g, true, true, dout, NGPDE_AGGR_SUM, dz, nullptr, tmp, stream))) return st;
  if ((st = launch_dense_seg_bwd_weight(n, one_seg(x, din), din, dout, tmp, dweight, nullptr, partial, stream))) return st;
  if (dx && (st = launch_dense_seg_bwd_input(n, one_grad(dx, din), din, dout, tmp, weight, stream))) return st;
  if (dedge_weight) {
    // the propagated array was x W (recomputed), its gradient is tmp = A^T dz, dL/dx3 = dz and x3 = z - bias
    if ((st = launch_dense_seg_fwd(n, one_seg(x, din), din, dout, NGPDE_ACT_IDENTITY, weight, nullptr, ew_xw, nullptr, stream))) return st;
    return launch_gcn_edge_weight_grad(g, dout, dz, z, bias, tmp, ew_xw, ew_nd, dedge_weight, stream);
  }
  return NGPDE_OK;
}
}  // namespace

extern "C" {

int32_t ngpde_gcn_backward(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act, const float *x,
                           const float *weight, const float *z, const float *saved_agg, const float *dy, float *dx,
                           float *dweight, float *dbias, void *workspace, size_t workspace_bytes,
                           ngpde_stream_t stream_) {
  NGPDE_RANGE();
  return gcn_backward_impl("ngpde_gcn_backward", g, din, dout, act, x, weight, nullptr, z, saved_agg, dy, dx, dweight, dbias, nullptr, workspace,
                           workspace_bytes, stream_);
}

size_t ngpde_gcn_backward_ew_workspace_bytes(const ngpde_graph_t *g, int32_t din, int32_t dout) {
  return g ? gcn_workspace_bytes(gcn_layer_form(g->n_nodes, din, dout), true, true) : 0;
}

int32_t ngpde_gcn_backward_ew(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act, const float *x, const float *weight,
                              const float *bias, const float *z, const float *saved_agg, const float *dy, float *dx, float *dweight,
                              float *dbias, float *dedge_weight, void *workspace, size_t workspace_bytes, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(dedge_weight != nullptr || (g && g->n_edges == 0), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gcn_backward_ew: dedge_weight is NULL");
  return gcn_backward_impl("ngpde_gcn_backward_ew", g, din, dout, act, x, weight, bias, z, saved_agg, dy, dx, dweight, dbias, dedge_weight, workspace,
                           workspace_bytes, stream_);
}

int32_t ngpde_propagate_copy_xj(const ngpde_graph_t *g, int32_t d, int32_t aggr, int32_t by_source, const float *x,
                                const float *edge_weight, float *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_propagate_copy_xj: graph is NULL");
  NGPDE_REQUIRE(d > 0 && x && out, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_propagate_copy_xj: bad arguments");
  return launch_spmm_generic(g, by_source != 0, false, d, aggr, x, edge_weight, out, (hipStream_t)stream);
}

}  // extern "C"
