// node_vmh_plan.hip -- VMHConv as right-hand side: the host plan of the device-resident solve + discrete adjoint (ngpde_node_vmh_*;
// the plan struct is in plan_host.h, the kernels and their launchers in node_vmh.hip) and the pool its tapes are parked in.  No
// kernels here.
#include "plan_host.h"

using namespace ngpde;

// The tapes of a VMH plan are tens of GB at the tutorial's minibatch size, and a training loop that batches its point clouds in a new
// order every epoch (VMH.md:120, DataLoader(shuffle = true)) builds a new plan per step: allocating and freeing such blocks each time
// costs 0.02 - 6 s per step (measured: hipFree of 124 GB 0.8 s, the hipMalloc after it up to 6 s).  Freed tapes are therefore parked
// (at most kTapePoolMax blocks) and handed to the next plan whose need they fit.  A parked block is not zeroed again: it was zeroed
// when allocated, what it holds since is finite, and the 16-float blocks of a row a solve does not write feed only the rows /
// columns of the padded 64 x 64 weight-pullback result that launch_vmh_copy_block never copies out.
namespace {
constexpr size_t kTapePoolMax = 8;
struct TapeBlock {
  float *ptr;
  size_t floats;
  int device;
};
int tape_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}
std::mutex g_tape_mu;
std::vector<TapeBlock> g_tape_pool;

// (the block's CAPACITY and the device it was allocated on travel with it: a block that came from the pool larger than the plan's
// need goes back with its full size, on its own device)
float *tape_pool_take(size_t floats, size_t *capacity) {   // the smallest parked block that fits without wasting more than half of itself
  const int dev = tape_device();
  std::lock_guard<std::mutex> lock(g_tape_mu);
  int best = -1;
  for (int i = 0; i < (int)g_tape_pool.size(); ++i)
    if (g_tape_pool[i].device == dev && g_tape_pool[i].floats >= floats && g_tape_pool[i].floats <= 2 * floats + 1024 &&
        (best < 0 || g_tape_pool[i].floats < g_tape_pool[best].floats))
      best = i;
  if (best < 0) return nullptr;
  float *ptr = g_tape_pool[best].ptr;
  *capacity = g_tape_pool[best].floats;
  g_tape_pool.erase(g_tape_pool.begin() + best);
  return ptr;
}
size_t tape_pool_release_all() {   // (before a fresh allocation that would not fit beside the parked blocks)
  std::lock_guard<std::mutex> lock(g_tape_mu);
  size_t n = g_tape_pool.size();
  for (auto &b : g_tape_pool) (void)hipFree(b.ptr);
  g_tape_pool.clear();
  return n;
}
void tape_pool_give(float *ptr, size_t floats, int device) {
  if (!ptr) return;
  std::lock_guard<std::mutex> lock(g_tape_mu);
  if (floats < (64u << 20) / 4 || g_tape_pool.size() >= kTapePoolMax) {   // small blocks and an overfull pool: back to the device
    (void)hipFree(ptr);
    return;
  }
  g_tape_pool.push_back({ptr, floats, device});
}
}  // namespace

ngpde_node_vmh::~ngpde_node_vmh() {
  float *const tapes[4] = {tape_phi, tape_gam, dz_phi, dz_gam};
  for (int k = 0; k < 4; ++k) {
    mem.give_up(tapes[k]);   // (a fresh block was taken from `mem`, a parked one was not)
    tape_pool_give(tapes[k], tape_cap[k], tape_dev);
  }
}

static int32_t vmh_shape(int32_t hd, int32_t pd, int32_t n_phi, const int32_t *phi_dims, const int32_t *phi_acts, int32_t n_gamma,
                         const int32_t *gamma_dims, const int32_t *gamma_acts, int32_t aggr, VmhShape *s) {
  NGPDE_REQUIRE(phi_dims && phi_acts && gamma_dims && gamma_acts, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh: NULL layer table");
  NGPDE_REQUIRE(n_phi >= 1 && n_phi <= kVmhMaxL && n_gamma >= 1 && n_gamma <= kVmhMaxL, NGPDE_ERR_UNSUPPORTED,
                "ngpde_node_vmh: 1 to %d Dense layers per MLP", kVmhMaxL);
  s->hd = hd; s->pd = pd; s->aggr = aggr; s->n_phi = n_phi; s->n_gam = n_gamma;
  for (int l = 0; l <= n_phi; ++l) s->phi_dims[l] = phi_dims[l];
  for (int l = 0; l <= n_gamma; ++l) s->gam_dims[l] = gamma_dims[l];
  for (int l = 0; l < n_phi; ++l) s->phi_act[l] = phi_acts[l];
  for (int l = 0; l < n_gamma; ++l) s->gam_act[l] = gamma_acts[l];
  return NGPDE_OK;
}

// a tape: a parked block that fits, else a fresh zeroed one (held by the plan's memory until the destructor parks it)
static int32_t vmh_tape(ngpde_node_vmh *p, float **ptr, size_t floats, size_t *cap) {
  floats = std::max<size_t>(floats, 64);
  *cap = floats;
  if ((*ptr = tape_pool_take(floats, cap)) != nullptr) return NGPDE_OK;
  if (p->mem.take(ptr, floats) != NGPDE_OK) {
    (void)hipGetLastError();
    if (tape_pool_release_all() == 0 || p->mem.take(ptr, floats) != NGPDE_OK) {
      (void)hipGetLastError();
      return fail(NGPDE_ERR_HIP, "ngpde_node_vmh_create: %.1f GB of tape do not fit the device", floats * 4 / 1e9);
    }
  }
  NGPDE_HIP_CHECK(hipMemset(*ptr, 0, floats * 4));
  return NGPDE_OK;
}

// the device side of a plan whose g, shape, n_steps and with_bwd are set
static int32_t vmh_build(ngpde_node_vmh *p, const float *pos, int tableau, double dt) {
  const ngpde_graph *g = p->g;
  const Tableau tb = make_tableau(tableau);
  const int S = p->S = tb.S, pd = p->shape.pd;
  float cf[48] = {0}, cb[64] = {0};   // forward: node_persistent.hip's table
  rk_forward6(tb, dt, cf);
  rk_adjoint8(tb, dt, cb);
  const size_t N = (size_t)g->n_nodes, E = (size_t)std::max<int64_t>(g->n_edges, 1), evals = (size_t)p->n_steps * S;
  DeviceBlocks &m = p->mem;
  const float coef_unused[90] = {0.f};
  NGPDE_TRY(node_persistent_setup(g, coef_unused, &p->persist, false));
  NGPDE_TRY(m.take(&p->pos, N * pd));
  NGPDE_HIP_CHECK(hipMemcpy(p->pos, pos, N * pd * 4, hipMemcpyDeviceToDevice));
  NGPDE_TRY(m.take(&p->cf, 48));
  NGPDE_TRY(m.take(&p->cb, 64));
  NGPDE_TRY(m.take(&p->x, 2 * N, true));
  NGPDE_TRY(m.take(&p->state, 16 * N, true));
  if (p->with_bwd) {
    NGPDE_TRY(m.take(&p->srcpos, (size_t)g->n_sched * kSlotWidth));
    NGPDE_TRY(m.take(&p->srcdeg, (size_t)g->n_sched));
    NGPDE_TRY(launch_vmh_srcpos(g, p->srcpos, p->srcdeg, nullptr));
    NGPDE_HIP_CHECK(hipStreamSynchronize(nullptr));
    // (zeroed once: the padded columns of a layer's rows are never written, and the weight-pullback GEMMs read whole 64-wide rows)
    const size_t tp = (size_t)p->shape.n_phi * evals * E * 64, tg = (size_t)p->shape.n_gam * evals * N * 64;
    p->tape_dev = tape_device();
    NGPDE_TRY(vmh_tape(p, &p->tape_phi, tp, &p->tape_cap[0]));
    NGPDE_TRY(vmh_tape(p, &p->tape_gam, tg, &p->tape_cap[1]));
    NGPDE_TRY(vmh_tape(p, &p->dz_phi, tp, &p->tape_cap[2]));
    NGPDE_TRY(vmh_tape(p, &p->dz_gam, tg, &p->tape_cap[3]));
    NGPDE_TRY(m.take(&p->dsrc, 2 * E, true));
    p->tape_bytes = 2 * (tp + tg) * 4;
    p->partial_floats = (size_t)dense_weight_chunks((int64_t)(evals * E), 64, 64) * 65 * 64 + 64;
    p->partial_floats = std::max(p->partial_floats, (size_t)dense_weight_chunks((int64_t)(evals * N), 64, 64) * 65 * 64 + 64);
    NGPDE_TRY(m.take(&p->partial, p->partial_floats));
    NGPDE_TRY(m.take(&p->dwpad, 64 * 64 + 64));
  }
  NGPDE_HIP_CHECK(hipMemcpy(p->cf, cf, sizeof cf, hipMemcpyHostToDevice));
  NGPDE_HIP_CHECK(hipMemcpy(p->cb, cb, sizeof cb, hipMemcpyHostToDevice));
  // the copy of pos and the zeroing above are NULL-stream work a device-to-device hipMemcpy / hipMemset may return ahead of: the solves run
  // on the caller's streams, which the NULL stream does not order (include/ngpde.h, "Creates")
  NGPDE_HIP_CHECK(hipStreamSynchronize(nullptr));
  return NGPDE_OK;
}

extern "C" {

int32_t ngpde_node_vmh_supported(const ngpde_graph_t *g, int32_t hd, int32_t pd, int32_t n_phi, const int32_t *phi_dims, const int32_t *phi_acts,
                                 int32_t n_gamma, const int32_t *gamma_dims, const int32_t *gamma_acts, int32_t aggr) {
  VmhShape s;
  if (!g || vmh_shape(hd, pd, n_phi, phi_dims, phi_acts, n_gamma, gamma_dims, gamma_acts, aggr, &s) != NGPDE_OK) return 0;
  return node_vmh_supported(g, s) ? 1 : 0;
}

int32_t ngpde_node_vmh_create(const ngpde_graph_t *g, int32_t hd, int32_t pd, const float *pos, int32_t n_phi, const int32_t *phi_dims,
                              const int32_t *phi_acts, int32_t n_gamma, const int32_t *gamma_dims, const int32_t *gamma_acts, int32_t aggr,
                              int32_t tableau, int32_t n_steps, double dt, int32_t with_backward, ngpde_node_vmh_t **out) {
  NGPDE_RANGE();
  NGPDE_TRY(plan_check_create("ngpde_node_vmh_create", g, out, tableau, n_steps, NGPDE_ACT_IDENTITY, 1));
  NGPDE_REQUIRE(pos != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_create: pos is NULL");
  VmhShape shape;
  NGPDE_TRY(vmh_shape(hd, pd, n_phi, phi_dims, phi_acts, n_gamma, gamma_dims, gamma_acts, aggr, &shape));
  NGPDE_REQUIRE(node_vmh_supported(g, shape), NGPDE_ERR_UNSUPPORTED,
                "ngpde_node_vmh_create: needs a scalar state, 1-3 position coordinates, MLPs of 2-4 Dense layers up to 64 wide with identity / relu / "
                "tanh / sigmoid hidden and identity output layers, + or mean aggregation, tiles that fit the LDS halo in both directions and "
                "neighbour at most 63 other tiles each, and at most 64 tiles per resident workgroup (use the generic solver otherwise)");
  std::unique_ptr<ngpde_node_vmh> p(new (std::nothrow) ngpde_node_vmh());
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_create: out of host memory");
  p->g = g; p->shape = shape; p->n_steps = n_steps; p->with_bwd = with_backward != 0;
  const int32_t st = vmh_build(p.get(), pos, tableau, dt);
  if (st != NGPDE_OK) {   // a plan that did not fit: nothing of it stays parked
    p.reset();
    (void)tape_pool_release_all();
    return st;
  }
  *out = p.release();
  return NGPDE_OK;
}

int32_t ngpde_node_vmh_destroy(ngpde_node_vmh_t *p) {
  NGPDE_RANGE();
  delete p;
  return NGPDE_OK;
}

size_t ngpde_node_vmh_tape_bytes(const ngpde_node_vmh_t *p) { return p ? p->tape_bytes : 0; }

size_t ngpde_release_cached_memory(void) {
  size_t bytes = 0;
  {
    std::lock_guard<std::mutex> lock(g_tape_mu);
    for (const auto &b : g_tape_pool) bytes += b.floats * 4;
  }
  (void)tape_pool_release_all();
  return bytes;
}

int32_t ngpde_node_vmh_fault(ngpde_node_vmh_t *p, ngpde_stream_t stream, int32_t *fault) {
  NGPDE_RANGE();
  return plan_fault("ngpde_node_vmh_fault", p, stream, fault);
}

static void vmh_fill(const ngpde_node_vmh *p, VmhLaunch &a, const float *const *phi_w, const float *const *phi_b, const float *const *gam_w,
                     const float *const *gam_b) {
  a.g = p->g; a.ps = &p->persist; a.shape = p->shape; a.n_steps = p->n_steps; a.S = p->S; a.pos = p->pos;
  for (int l = 0; l < p->shape.n_phi; ++l) { a.phi_w[l] = phi_w[l]; a.phi_b[l] = phi_b ? phi_b[l] : nullptr; }
  for (int l = 0; l < p->shape.n_gam; ++l) { a.gam_w[l] = gam_w[l]; a.gam_b[l] = gam_b ? gam_b[l] : nullptr; }
  a.x0 = p->x; a.x1 = p->x + p->g->n_nodes; a.state = p->state; a.srcpos = p->srcpos; a.srcdeg = p->srcdeg; a.tape_phi = p->tape_phi; a.tape_gam = p->tape_gam; a.dz_phi = p->dz_phi; a.dz_gam = p->dz_gam;
  a.dsrc = p->dsrc; a.cf = p->cf; a.cb = p->cb;
}

// the number of saved states of a plan under saveat, or -1 (save_every must divide the plan's steps)
static int vmh_saved_states(const ngpde_node_vmh *p, int32_t save_every, int32_t save_start) {
  if (save_every < 1 || p->n_steps % save_every) return -1;
  return p->n_steps / save_every + (save_start ? 1 : 0);
}

int32_t ngpde_node_vmh_forward(ngpde_node_vmh_t *p, const float *u0, const float *const *phi_weight, const float *const *phi_bias,
                               const float *const *gamma_weight, const float *const *gamma_bias, float *uT, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_forward: plan is NULL");
  // u(T) alone = the one state saved after the last step
  return ngpde_node_vmh_forward_saveat(p, u0, phi_weight, phi_bias, gamma_weight, gamma_bias, p->n_steps, 0, uT, stream_);
}

int32_t ngpde_node_vmh_forward_saveat(ngpde_node_vmh_t *p, const float *u0, const float *const *phi_weight, const float *const *phi_bias,
                                      const float *const *gamma_weight, const float *const *gamma_bias, int32_t save_every,
                                      int32_t save_start, float *uT, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_forward: plan is NULL");
  const int T = vmh_saved_states(p, save_every, save_start);
  NGPDE_REQUIRE(T >= 1, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_forward_saveat: save_every = %d must be >= 1 and divide the plan's %d steps",
                (int)save_every, p->n_steps);
  if (p->g->n_nodes == 0) return NGPDE_OK;
  NGPDE_REQUIRE(u0 && uT && phi_weight && gamma_weight && u0 != uT, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_forward: NULL argument (or uT aliasing u0)");
  for (int l = 0; l < p->shape.n_phi; ++l) NGPDE_REQUIRE(phi_weight[l], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_forward: phi weight %d is NULL", l);
  for (int l = 0; l < p->shape.n_gam; ++l) NGPDE_REQUIRE(gamma_weight[l], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_forward: gamma weight %d is NULL", l);
  NGPDE_REQUIRE_LIVE("ngpde_node_vmh_forward", p);
  VmhLaunch a;
  vmh_fill(p, a, phi_weight, phi_bias, gamma_weight, gamma_bias);
  a.u_in = u0;
  if (T == 1 && !save_start) {
    a.u_out = uT;
  } else {
    a.save = uT; a.save_every = save_every; a.save_off = save_start ? 1 : 0;
  }
  const int32_t st = launch_node_vmh_fwd(a, (hipStream_t)stream_);
  if (st == NGPDE_OK) p->solved = true;
  return st;
}

int32_t ngpde_node_vmh_backward(ngpde_node_vmh_t *p, const float *const *phi_weight, const float *const *gamma_weight, const float *duT,
                                float *du0, float *const *dphi_weight, float *const *dphi_bias, float *const *dgamma_weight,
                                float *const *dgamma_bias, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_backward: plan is NULL");
  return ngpde_node_vmh_backward_saveat(p, phi_weight, gamma_weight, p->n_steps, 0, duT, du0, dphi_weight, dphi_bias, dgamma_weight, dgamma_bias,
                                        stream_);
}

int32_t ngpde_node_vmh_backward_saveat(ngpde_node_vmh_t *p, const float *const *phi_weight, const float *const *gamma_weight, int32_t save_every,
                                       int32_t save_start, const float *duT, float *du0, float *const *dphi_weight,
                                       float *const *dphi_bias, float *const *dgamma_weight, float *const *dgamma_bias, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_backward: plan is NULL");
  const int T = vmh_saved_states(p, save_every, save_start);
  NGPDE_REQUIRE(T >= 1, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_backward_saveat: save_every = %d must be >= 1 and divide the plan's %d steps",
                (int)save_every, p->n_steps);
  NGPDE_REQUIRE(p->with_bwd, NGPDE_ERR_STATE, "ngpde_node_vmh_backward: the plan was created without a backward pass");
  NGPDE_REQUIRE(p->solved, NGPDE_ERR_STATE, "ngpde_node_vmh_backward: no forward solve has filled the tape");
  NGPDE_REQUIRE(phi_weight && gamma_weight && duT && du0 && dphi_weight && dgamma_weight, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_backward: NULL argument");
  NGPDE_REQUIRE_LIVE("ngpde_node_vmh_backward", p);
  hipStream_t stream = (hipStream_t)stream_;
  const size_t N = (size_t)p->g->n_nodes, E = (size_t)p->g->n_edges, evals = (size_t)p->n_steps * p->S;
  // lambda starts as the cotangent of the last saved state (= u(T)); the kernel adds the earlier ones at their times
  const float *last = duT + (size_t)(T - 1) * N;
  if (du0 != last) NGPDE_HIP_CHECK(hipMemcpyAsync(du0, last, N * 4, hipMemcpyDeviceToDevice, stream));
  VmhLaunch a;
  vmh_fill(p, a, phi_weight, nullptr, gamma_weight, nullptr);
  a.lam = du0;
  if (T > 1) {
    NGPDE_REQUIRE(du0 < duT || du0 >= duT + (size_t)T * N, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_vmh_backward_saveat: du0 lies inside the cotangent array");
    a.dsave = duT; a.save_every = save_every; a.save_off = save_start ? 1 : 0;
  }
  int32_t st;
  if ((st = launch_node_vmh_bwd(a, stream))) return st;
  // dW_l = A_l^T dZ_l, db_l = column sums of dZ_l over the rows of ALL evaluations: one weight-pullback GEMM per layer on the tapes
  auto layer_grad = [&](const float *tape, const float *dz, size_t rows, int din, int dout, float *dw, float *db) -> int32_t {
    SegTable segs;
    segs.n = 1; segs.ptr[0] = tape; segs.width[0] = 64; segs.row_div[0] = 1; segs.vec[0] = 1;
    for (int k = 1; k <= 4; ++k) segs.offset[k] = 64;
    int32_t s2;
    if ((s2 = launch_dense_seg_bwd_weight((int64_t)rows, segs, 64, 64, dz, p->dwpad, p->dwpad + 64 * 64, p->partial, stream))) return s2;
    if (dw && (s2 = launch_vmh_copy_block(p->dwpad, 64, dw, dout, din, dout, stream))) return s2;
    if (db && (s2 = launch_vmh_copy_block(p->dwpad + 64 * 64, 64, db, dout, 1, dout, stream))) return s2;
    return NGPDE_OK;
  };
  for (int l = 0; l < p->shape.n_phi; ++l)
    if ((st = layer_grad(p->tape_phi + (size_t)l * evals * E * 64, p->dz_phi + (size_t)l * evals * E * 64, evals * E, p->shape.phi_dims[l],
                         p->shape.phi_dims[l + 1], dphi_weight[l], dphi_bias ? dphi_bias[l] : nullptr)))
      return st;
  for (int l = 0; l < p->shape.n_gam; ++l)
    if ((st = layer_grad(p->tape_gam + (size_t)l * evals * N * 64, p->dz_gam + (size_t)l * evals * N * 64, evals * N, p->shape.gam_dims[l],
                         p->shape.gam_dims[l + 1], dgamma_weight[l], dgamma_bias ? dgamma_bias[l] : nullptr)))
      return st;
  return NGPDE_OK;
}

}  // extern "C"
