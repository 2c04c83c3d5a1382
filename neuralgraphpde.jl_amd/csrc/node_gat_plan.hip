// node_gat_plan.hip -- GAT-style layer as right-hand side: the host plan of the device-resident solve + discrete adjoint
// (ngpde_node_gat_*; the plan struct is in plan_host.h, the kernels and their launchers in gat_fused.hip).  No kernels here.
#include "plan_host.h"

using namespace ngpde;

extern "C" {

int32_t ngpde_node_gat_supported(const ngpde_graph_t *g, int32_t din, int32_t heads, int32_t c) {
  return (g && din == 64 && gat_node_persistent_supported(g, heads, c)) ? 1 : 0;
}

int32_t ngpde_node_gat_create(const ngpde_graph_t *g, int32_t heads, int32_t c, float negative_slope, int32_t act, int32_t tableau,
                              int32_t n_steps, double dt, int32_t with_backward, ngpde_node_gat_t **out) {
  return ngpde_node_gat_create_batch(g, 1, heads, c, negative_slope, act, tableau, n_steps, dt, with_backward, out);
}

int32_t ngpde_node_gat_create_batch(const ngpde_graph_t *g, int32_t members, int32_t heads, int32_t c, float negative_slope, int32_t act,
                                    int32_t tableau, int32_t n_steps, double dt, int32_t with_backward, ngpde_node_gat_t **out) {
  NGPDE_RANGE();
  NGPDE_TRY(plan_check_create("ngpde_node_gat_create", g, out, tableau, n_steps, act, members));
  NGPDE_REQUIRE(gat_node_persistent_supported(g, heads, c), NGPDE_ERR_UNSUPPORTED,
                "ngpde_node_gat_create: needs 64 => heads x c = 64 with heads in {1, 2, 4}, tiles that fit the LDS halo in both directions "
                "and at most as many tiles as the device keeps resident (use the generic solver otherwise)");
  std::unique_ptr<ngpde_node_gat> p(new (std::nothrow) ngpde_node_gat());
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gat_create: out of host memory");
  p->g = g; p->heads = heads; p->c = c; p->act = act; p->slope = negative_slope; p->n_steps = n_steps; p->with_bwd = with_backward != 0;
  p->members = members;
  const Tableau tb = make_tableau(tableau);
  const int S = p->S = tb.S;
  // the coefficients exactly as the generic solver passes them to ngpde_rk_stage_combine: float(dt * a_ij) formed in double
  std::vector<float> cf((size_t)(S + 1) * 8, 0.f), cb((size_t)S * 8);
  for (int i = 0; i < S; ++i) {
    for (int j = 0; j < i; ++j) cf[(size_t)i * 8 + j] = (float)(dt * tb.a[i][j]);
    cf[(size_t)S * 8 + i] = (float)(dt * tb.b[i]);
  }
  rk_adjoint8(tb, dt, cb.data());
  p->row_elems = (size_t)g->n_nodes * 64;
  p->alpha_elems = (size_t)std::max<int64_t>(g->n_edges, 1) * heads;
  const size_t phases = (size_t)n_steps * S, nt = (size_t)g->n_sched / kTileRows, M = (size_t)members, slots = members > 1 ? 2 : 1;
  const size_t edges = (size_t)std::max<int64_t>(g->n_edges, 1);
  DeviceBlocks &m = p->mem;
  const float coef_unused[90] = {0.f};
  NGPDE_TRY(node_persistent_setup(g, coef_unused, &p->persist, false));
  NGPDE_TRY(m.take(&p->cf, cf.size()));
  NGPDE_TRY(m.take(&p->cb, std::max<size_t>(cb.size(), 64)));
  NGPDE_TRY(m.take(&p->kbuf, slots * 7 * p->row_elems));   // per slot: k_0..k_5 and (batches) u
  NGPDE_TRY(m.take(&p->xs, M * (p->with_bwd ? phases : 2) * p->row_elems));
  p->tape_bytes = M * (p->with_bwd ? phases : 2) * p->row_elems * 4;
  if (p->with_bwd) {
    if (act != NGPDE_ACT_IDENTITY) {
      NGPDE_TRY(m.take(&p->yz, M * phases * p->row_elems));
      p->tape_bytes += M * phases * p->row_elems * 4;
    }
    NGPDE_TRY(m.take(&p->alpha, M * phases * p->alpha_elems));
    p->tape_bytes += M * phases * p->alpha_elems * 4;
    NGPDE_TRY(m.take(&p->ubar, slots * 6 * p->row_elems));
    NGPDE_TRY(m.take(&p->dzbuf, slots * 2 * p->row_elems));
    NGPDE_TRY(m.take(&p->dscore, slots * 2 * gat_node_dscore_elems(g)));
    NGPDE_TRY(m.take(&p->dal, slots * (size_t)g->n_nodes * heads));
    NGPDE_TRY(m.take(&p->slabs, nt * (64 * 64 + 64 + 128)));
    NGPDE_TRY(m.take(&p->xpad, edges));
    DeviceBlocks tmp;   // (freed when the create returns, whichever way)
    int *scratch = nullptr;
    NGPDE_TRY(tmp.take(&scratch, edges));
    NGPDE_TRY(launch_gat_node_xpad(g, scratch, p->xpad, nullptr));
    NGPDE_HIP_CHECK(hipStreamSynchronize(nullptr));
  }
  NGPDE_HIP_CHECK(hipMemcpy(p->cf, cf.data(), cf.size() * 4, hipMemcpyHostToDevice));
  NGPDE_HIP_CHECK(hipMemcpy(p->cb, cb.data(), cb.size() * 4, hipMemcpyHostToDevice));
  NGPDE_HIP_CHECK(hipStreamSynchronize(nullptr));   // (node_persistent_setup's memsets: include/ngpde.h, "Creates")
  *out = p.release();
  return NGPDE_OK;
}

int32_t ngpde_node_gat_destroy(ngpde_node_gat_t *p) {
  NGPDE_RANGE();
  delete p;
  return NGPDE_OK;
}

size_t ngpde_node_gat_tape_bytes(const ngpde_node_gat_t *p) { return p ? p->tape_bytes : 0; }

int32_t ngpde_node_gat_fault(ngpde_node_gat_t *p, ngpde_stream_t stream, int32_t *fault) {
  NGPDE_RANGE();
  return plan_fault("ngpde_node_gat_fault", p, stream, fault);
}

int32_t ngpde_node_gat_forward(ngpde_node_gat_t *p, const float *u0, const float *weight, const float *a, const float *bias, float *uT,
                               ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gat_forward: plan is NULL");
  if (p->g->n_nodes == 0) return NGPDE_OK;
  NGPDE_REQUIRE(u0 && weight && a && uT, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gat_forward: NULL argument");
  NGPDE_REQUIRE_LIVE("ngpde_node_gat_forward", p);
  hipStream_t stream = (hipStream_t)stream_;
  const size_t phases = (size_t)p->n_steps * p->S, xs_stride = (p->with_bwd ? phases : 2) * p->row_elems;
  for (int mb = 0; mb < p->members; ++mb)   // slot 0 of every member's stage-input array = the input of its phase 1
    NGPDE_HIP_CHECK(hipMemcpyAsync(p->xs + (size_t)mb * xs_stride, u0 + (size_t)mb * p->row_elems, p->row_elems * 4, hipMemcpyDeviceToDevice, stream));
  GatNodeFwd f;
  f.g = p->g; f.ps = &p->persist; f.heads = p->heads; f.act = p->act; f.n_steps = p->n_steps; f.S = p->S; f.slope = p->slope;
  f.taped = p->with_bwd; f.u_in = u0; f.wt = weight; f.a = a; f.bias = bias; f.u_out = uT; f.xs = p->xs; f.yz = p->yz; f.alpha = p->alpha;
  f.kbuf = p->kbuf; f.cf = p->cf;
  f.n_members = p->members; f.xs_stride = xs_stride; f.yz_stride = phases * p->row_elems; f.alpha_stride = phases * p->alpha_elems;
  const int32_t st = launch_gat_node_fwd(f, stream);
  if (st == NGPDE_OK) p->solved = true;
  return st;
}

int32_t ngpde_node_gat_backward(ngpde_node_gat_t *p, const float *weight, const float *a, const float *duT, float *du0, float *dweight,
                                float *da, float *dbias, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gat_backward: plan is NULL");
  NGPDE_REQUIRE(p->with_bwd, NGPDE_ERR_STATE, "ngpde_node_gat_backward: the plan was created without a backward pass");
  NGPDE_REQUIRE(p->solved, NGPDE_ERR_STATE, "ngpde_node_gat_backward: no forward solve has filled the tape");
  NGPDE_REQUIRE(weight && a && duT && du0 && dweight && da, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gat_backward: NULL argument");
  NGPDE_REQUIRE_LIVE("ngpde_node_gat_backward", p);
  const size_t nt = (size_t)p->g->n_sched / kTileRows;
  GatNodeBwd b;
  b.g = p->g; b.ps = &p->persist; b.heads = p->heads; b.act = p->act; b.n_steps = p->n_steps; b.S = p->S; b.slope = p->slope;
  b.wt = weight; b.a = a; b.xs = p->xs; b.yz = p->yz; b.alpha = p->alpha; b.duT = duT; b.lam = du0; b.ubar = p->ubar; b.dzbuf = p->dzbuf;
  b.dscore = p->dscore; b.dal = p->dal; b.slab_dw = p->slabs; b.slab_db = p->slabs + nt * 64 * 64; b.slab_u = b.slab_db + nt * 64;
  b.xpad = p->xpad; b.cb = p->cb; b.dwt = dweight; b.da = da; b.db = dbias;
  {
    const size_t phases = (size_t)p->n_steps * p->S;
    b.n_members = p->members; b.xs_stride = phases * p->row_elems; b.yz_stride = phases * p->row_elems; b.alpha_stride = phases * p->alpha_elems;
  }
  return launch_gat_node_bwd(b, (hipStream_t)stream_);
}

}  // extern "C"
