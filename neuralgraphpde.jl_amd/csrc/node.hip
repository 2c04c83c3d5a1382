// node.hip -- device-resident fixed-step neural graph ODE over Chain(GCNConv(d=>d), GCNConv(d=>d)),
// forward solve + discrete adjoint, each replayed from one HIP graph.
//
// Caller of the hot path in the reference: the tutorial's NeuralODE wrapper evaluates
//   dudt(u, p, t) = Chain(GCNConv(nhidden => nhidden, relu), GCNConv(nhidden => nhidden, relu))(u, p, st)
// once per Runge-Kutta stage (/root/reference/docs/src/tutorials/graph_node.md:59-66, :78) and its
// pullback once per stage of the reverse pass (:54, :127).  Here every stage is two fused launches:
//   forward  : [aggregate + MFMA + act] for layer 1, [aggregate + MFMA + act + next-stage input
//              u_n + dt*sum_j a_ij k_j (or the step update with b_j)] for layer 2;
//   backward : [A^T-aggregate + mask + MFMA(dZ W, X^T dZ)] for layer 1, and one launch that finishes
//              stage i (A^T-aggregate -> U-bar_i), forms the next stage's K-bar = dt*b*lambda +
//              dt*sum_j a_ji U-bar_j (or the lambda update at the step boundary) and runs layer 2's
//              dense backward for that next stage.
#include <vector>

#include "plan_host.h"
#include "switches.h"

using namespace ngpde;

namespace {

// dst[i][:] = src[i][:] * c[i]   (invert: / c[i]) -- entry to / exit from the pre-scaled form of the pipeline
// What rides along with an entry / exit kernel of a plan (one launch instead of three): a raw copy of the source rows (the plan keeps u0
// for ngpde_node_profile) and the fault latch of the persistent launch that ran just before (abort word of that launch -> the plan's
// sticky fault word; node_persistent.hip launched a kernel of its own for it until round 5)
struct RowsExtra {
  float4 *keep = nullptr;
  const unsigned *abort_word = nullptr;
  unsigned *fault = nullptr;
};
__global__ void scale_rows_kernel(size_t n4, int lpr, int invert, const float4 *__restrict__ src, const float *__restrict__ c,
                                  size_t n_nodes, float4 *__restrict__ dst, RowsExtra x) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0 && x.abort_word && *x.abort_word != 0) *x.fault = 1u;
  if (i >= n4) return;
  const float ci = c[(i / lpr) % n_nodes];   // (a batch of identical graphs repeats the member's coefficients)
  const float f = invert ? 1.0f / ci : ci;
  const float4 v = src[i];
  if (x.keep) x.keep[i] = v;
  dst[i] = make_float4(v.x * f, v.y * f, v.z * f, v.w * f);
}

int32_t launch_scale_rows(const float *src, const float *c, float *dst, int64_t n, int d, bool invert, hipStream_t stream,
                          int members = 1, RowsExtra x = RowsExtra()) {
  const size_t n4 = (size_t)n * members * d / 4;
  if (n4 == 0) return NGPDE_OK;
  hipLaunchKernelGGL(scale_rows_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, n4, d / 4, invert ? 1 : 0,
                     reinterpret_cast<const float4 *>(src), c, (size_t)n, reinterpret_cast<float4 *>(dst), x);
  NGPDE_LAUNCH_CHECK("scale_rows_kernel");
  return NGPDE_OK;
}

// The same with a change of row width: dst rows are `d_out` wide, src rows `d_in` (columns beyond the narrower of the two are
// written as zeros / dropped) -- entry to / exit from a plan that runs a narrow state on the 64-wide persistent kernels.
__global__ void scale_rows_width_kernel(size_t n4, int lpr_in, int lpr_out, int invert, const float4 *__restrict__ src,
                                        const float *__restrict__ c, size_t n_nodes, float4 *__restrict__ dst, RowsExtra x) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // one float4 of dst
  if (i == 0 && x.abort_word && *x.abort_word != 0) *x.fault = 1u;
  if (i >= n4) return;
  const size_t row = i / lpr_out;
  const int q = (int)(i - row * lpr_out);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (q < lpr_in) {
    const float ci = c[row % n_nodes];
    const float f = invert ? 1.0f / ci : ci;
    const float4 s = src[row * lpr_in + q];
    if (x.keep) x.keep[row * lpr_in + q] = s;   // (keep has the SOURCE's row width: asked for on the way in, lpr_in <= lpr_out)
    v = make_float4(s.x * f, s.y * f, s.z * f, s.w * f);
  }
  dst[i] = v;
}

int32_t launch_scale_rows_width(const float *src, int d_in, const float *c, float *dst, int d_out, int64_t n, bool invert,
                                hipStream_t stream, int members = 1, RowsExtra x = RowsExtra()) {
  if (d_in == d_out) return launch_scale_rows(src, c, dst, n, d_in, invert, stream, members, x);
  const size_t n4 = (size_t)n * members * d_out / 4;
  if (n4 == 0) return NGPDE_OK;
  hipLaunchKernelGGL(scale_rows_width_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream, n4, d_in / 4, d_out / 4,
                     invert ? 1 : 0, reinterpret_cast<const float4 *>(src), c, (size_t)n, reinterpret_cast<float4 *>(dst), x);
  NGPDE_LAUNCH_CHECK("scale_rows_width_kernel");
  return NGPDE_OK;
}

// The caller's parameters -> the plan's [d][d] / [d] copies in ONE launch (they were four copies, or two 2-D copies and two copies for a
// widened plan: the du x du block of the zero-padded d x d matrix, whose padding is written once at creation); a NULL bias is zeros
__global__ void pack_params_kernel(const float *__restrict__ w1u, const float *__restrict__ b1u, const float *__restrict__ w2u,
                                   const float *__restrict__ b2u, int du, int d, float *__restrict__ w1, float *__restrict__ b1,
                                   float *__restrict__ w2, float *__restrict__ b2) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, mm = du * du;
  if (i < mm) w1[(i / du) * d + i % du] = w1u[i];
  else if (i < 2 * mm) w2[((i - mm) / du) * d + (i - mm) % du] = w2u[i - mm];
  else if (i < 2 * mm + du) b1[i - 2 * mm] = b1u ? b1u[i - 2 * mm] : 0.f;
  else if (i < 2 * mm + 2 * du) b2[i - 2 * mm - du] = b2u ? b2u[i - 2 * mm - du] : 0.f;
}
int32_t launch_pack_params(const float *w1u, const float *b1u, const float *w2u, const float *b2u, int du, int d, float *w1, float *b1,
                           float *w2, float *b2, hipStream_t stream) {
  const int total = 2 * du * du + 2 * du;
  hipLaunchKernelGGL(pack_params_kernel, dim3((total + 255) / 256), dim3(256), 0, stream, w1u, b1u, w2u, b2u, du, d, w1, b1, w2, b2);
  NGPDE_LAUNCH_CHECK("pack_params_kernel");
  return NGPDE_OK;
}

// The four slab reductions of an adjoint (dW1, db1, dW2, db2) in ONE launch, written where the caller wants them -- its own du x du /
// du arrays (the leading block of the plan's d x d accumulation when the plan is widened) -- with reduce_slabs_kernel's sums in its
// order (gcn_fused.hip: bitwise the same numbers); block (0, 0) latches the fault word of the adjoint launch in front of it
struct Reduce4 {
  const float *slab[4];
  float *out[4];        // NULL: not asked for
  int len[4], ct[4];    // ct > 0: a [D][D] matrix in MFMA tile order (D = 16 ct), ct == 0: a vector
  int n_slabs, du;
  const unsigned *abort_word;
  unsigned *fault;
};
__global__ __launch_bounds__(1024) void reduce4_slabs_kernel(const Reduce4 r) {
  __shared__ float part[16][64];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && r.abort_word && *r.abort_word != 0) *r.fault = 1u;
  const int job = blockIdx.y;
  const float *__restrict__ slab = r.slab[job];
  float *__restrict__ out = r.out[job];
  const int len = r.len[job], ct = r.ct[job], n_slabs = r.n_slabs;
  if (out == nullptr || (int)blockIdx.x * 64 >= len) return;   // (block-uniform)
  const int el = threadIdx.x & 63, part_id = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + el;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (e < len) {
    int b = part_id;
    for (; b + 48 < n_slabs; b += 64) {
      s0 += slab[(size_t)b * len + e];
      s1 += slab[(size_t)(b + 16) * len + e];
      s2 += slab[(size_t)(b + 32) * len + e];
      s3 += slab[(size_t)(b + 48) * len + e];
    }
    for (; b < n_slabs; b += 16) s0 += slab[(size_t)b * len + e];
  }
  part[part_id][el] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (part_id == 0 && e < len) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += part[k][el];
    if (ct > 0) {  // e = (tt * 64 + lane) * 4 + reg  ->  dWt[(mt*16 + 4*kq + reg)][nt*16 + i]
      const int reg = e & 3, ln = (e >> 2) & 63, tt = e >> 8;
      const int mt = tt / ct, nt = tt % ct;
      const int row = mt * 16 + 4 * (ln >> 4) + reg, col = nt * 16 + (ln & 15);
      if (row < r.du && col < r.du) out[row * r.du + col] = v;
    } else if (e < r.du) {
      out[e] = v;
    }
  }
}

// [h][w] block between matrices of row pitch spitch / dpitch (elements): the parameters of a widened plan
int32_t copy_block(float *dst, int dpitch, const float *src, int spitch, int w, int h, hipStream_t stream) {
  NGPDE_HIP_CHECK(hipMemcpy2DAsync(dst, (size_t)dpitch * sizeof(float), src, (size_t)spitch * sizeof(float), (size_t)w * sizeof(float),
                                   (size_t)h, hipMemcpyDeviceToDevice, stream));
  return NGPDE_OK;
}

bool act_needs_z(int act) {
  return !(act == NGPDE_ACT_IDENTITY || act == NGPDE_ACT_RELU || act == NGPDE_ACT_LEAKYRELU);
}

// profiling pass: start/stop events on every stride-th launch, tagged by kernel role
struct Prof {
  int stride = 1, counter = 0;
  std::vector<hipEvent_t> ev0, ev1;
  std::vector<int> role;
  bool want(int r, hipEvent_t *a, hipEvent_t *b) {
    if ((counter++ % stride) != 0) return false;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return false;
    ev0.push_back(e0); ev1.push_back(e1); role.push_back(r);
    *a = e0; *b = e1;
    return true;
  }
  ~Prof() {
    for (hipEvent_t e : ev0) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev1) (void)hipEventDestroy(e);
  }
};

int32_t enqueue_forward(ngpde_node *p, hipStream_t stream, int *launches, Prof *prof = nullptr) {
  const Tableau &tb = p->tb;
  int32_t st;
  int count = 0;
  for (int n = 0; n < p->n_steps; ++n) {
    for (int i = 0; i < tb.S; ++i) {
      FusedFwdArgs f1;
      f1.g = p->g; f1.d = p->d; f1.act = p->act;
      f1.x = (i == 0) ? p->u : p->ustage;
      f1.wt = p->w1; f1.bias = p->b1;
      f1.y = p->slot(n, i, 1);
      f1.save_agg = p->with_bwd ? p->slot(n, i, 0) : nullptr;
      f1.save_z = (p->with_bwd && p->needs_z) ? p->slot(n, i, 4) : nullptr;
      f1.save_mask = p->mask_mode ? p->mask_slot(n, i, 1) : nullptr;
      f1.pre = p->pre;
      f1.of = p->has_of ? &p->of : nullptr;
      if (prof) prof->want(0, &f1.ev_start, &f1.ev_stop);
      if ((st = launch_fused_fwd(f1, stream))) return st;
      FusedFwdArgs f2;
      f2.g = p->g; f2.d = p->d; f2.act = p->act;
      f2.x = p->slot(n, i, 1);
      f2.wt = p->w2; f2.bias = p->b2;
      f2.y = p->slot(n, i, 3);
      f2.save_agg = p->with_bwd ? p->slot(n, i, 2) : nullptr;
      f2.save_z = (p->with_bwd && p->needs_z) ? p->slot(n, i, 5) : nullptr;
      f2.save_mask = p->mask_mode ? p->mask_slot(n, i, 2) : nullptr;
      f2.pre = p->pre;
      f2.of = p->has_of ? &p->of : nullptr;
      // epilogue: next stage input, or the step update after the last stage
      const bool last = (i == tb.S - 1);
      const std::vector<double> &row = last ? tb.b : tb.a[i + 1];
      f2.has_comb = true;
      f2.comb_out = last ? p->u : p->ustage;
      f2.comb.n = 0;
      f2.comb.ptr[f2.comb.n] = p->u;
      f2.comb.coef[f2.comb.n++] = 1.0f;
      for (int j = 0; j < i; ++j) {
        if (row[j] == 0.0) continue;
        f2.comb.ptr[f2.comb.n] = p->slot(n, j, 3);
        f2.comb.coef[f2.comb.n++] = (float)(p->dt * row[j]);
      }
      f2.comb.coef_self = (float)(p->dt * row[i]);
      if (prof) prof->want(1, &f2.ev_start, &f2.ev_stop);
      if ((st = launch_fused_fwd(f2, stream))) return st;
      count += 2;
    }
  }
  if (launches) *launches = count;
  return NGPDE_OK;
}

void fill_dense(const ngpde_node *p, FusedBwdArgs &a, int layer, int step, int stage) {
  a.do_dense = true;
  a.pre = p->pre;
  if (p->mask_mode) a.mask = p->mask_slot(step, stage, layer);
  if (layer == 2) {
    a.z = p->needs_z ? p->slot(step, stage, 5) : p->slot(step, stage, 3);
    a.saved_agg = p->slot(step, stage, 2);
    a.wt = p->w2; a.g_out = p->g2; a.slab_dw = p->slab_dw2; a.slab_db = p->slab_db2;
  } else {
    a.z = p->needs_z ? p->slot(step, stage, 4) : p->slot(step, stage, 1);
    a.saved_agg = p->slot(step, stage, 0);
    a.wt = p->w1; a.g_out = p->g1; a.slab_dw = p->slab_dw1; a.slab_db = p->slab_db1;
  }
}

int32_t enqueue_backward(ngpde_node *p, hipStream_t stream, int *launches, Prof *prof = nullptr) {
  const Tableau &tb = p->tb;
  const int S = tb.S;
  int32_t st;
  int count = 0;
  // zero the slabs with a kernel, not hipMemsetAsync: a memset node captured into the graph is not reliably ordered before
  // the first kernel node on replays after the first (observed: dW drifting in the 7th digit from the second replay on,
  // garbage with unpaired workgroups; eager launches were always right)
  if ((st = launch_zero(p->slabs, p->slab_bytes, stream))) return st;
  {  // K-bar of the last stage of the last step, then layer 2's dense backward
    FusedBwdArgs a;
    a.g = p->g; a.d = p->d; a.act = p->act;
    a.aggregate = false; a.g_in = p->lam;
    a.has_comb = true; a.comb.n = 0; a.comb.coef_self = (float)(p->dt * tb.b[S - 1]);
    fill_dense(p, a, 2, p->n_steps - 1, S - 1);
    if ((st = launch_fused_bwd(a, stream))) return st;
    ++count;
  }
  for (int n = p->n_steps - 1; n >= 0; --n) {
    for (int i = S - 1; i >= 0; --i) {
      FusedBwdArgs m;  // layer 1 of stage i: dY1 = A^T g2
      m.g = p->g; m.d = p->d; m.act = p->act;
      m.aggregate = true; m.g_in = p->g2;
      fill_dense(p, m, 1, n, i);
      if (prof) prof->want(2, &m.ev_start, &m.ev_stop);
      if ((st = launch_fused_bwd(m, stream))) return st;
      FusedBwdArgs e;  // U-bar_i = A^T g1, then the next stage's K-bar and layer-2 dense backward
      e.g = p->g; e.d = p->d; e.act = p->act;
      e.aggregate = true; e.g_in = p->g1;
      e.has_comb = true; e.comb.n = 0;
      if (i >= 1) {
        e.store_t = p->ubar[i];
        e.comb.ptr[e.comb.n] = p->lam;
        e.comb.coef[e.comb.n++] = (float)(p->dt * tb.b[i - 1]);
        for (int j = i + 1; j < S; ++j) {
          if (tb.a[j][i - 1] == 0.0) continue;
          e.comb.ptr[e.comb.n] = p->ubar[j];
          e.comb.coef[e.comb.n++] = (float)(p->dt * tb.a[j][i - 1]);
        }
        e.comb.coef_self = (float)(p->dt * tb.a[i][i - 1]);
        fill_dense(p, e, 2, n, i - 1);
      } else {
        // lambda_n = lambda_{n+1} + sum_j U-bar_j
        e.comb.ptr[e.comb.n] = p->lam;
        e.comb.coef[e.comb.n++] = 1.0f;
        for (int j = 1; j < S; ++j) {
          e.comb.ptr[e.comb.n] = p->ubar[j];
          e.comb.coef[e.comb.n++] = 1.0f;
        }
        e.comb.coef_self = 1.0f;
        e.store_v = p->lam;
        if (n > 0) {
          e.v_scale = (float)(p->dt * tb.b[S - 1]);
          fill_dense(p, e, 2, n - 1, S - 1);
        } else {
          e.do_dense = false;
          e.pre = p->pre;
        }
      }
      if (prof && e.do_dense) prof->want(3, &e.ev_start, &e.ev_stop);
      if ((st = launch_fused_bwd(e, stream))) return st;
      count += 2;
    }
  }
  const int dd = p->d * p->d;
  const int ns = fused_num_slabs(p->n, p->d);   // the slabs beyond it stay zero
  if ((st = launch_reduce_slabs(p->slab_dw1, ns, dd, p->d / 16, p->dw1, stream))) return st;
  if ((st = launch_reduce_slabs(p->slab_db1, ns, p->d, 0, p->db1, stream))) return st;
  if ((st = launch_reduce_slabs(p->slab_dw2, ns, dd, p->d / 16, p->dw2, stream))) return st;
  if ((st = launch_reduce_slabs(p->slab_db2, ns, p->d, 0, p->db2, stream))) return st;
  count += 4;
  if (launches) *launches = count;
  return NGPDE_OK;
}

// the persistent forms: ONE launch for the whole solve / the whole adjoint (node_persistent.hip)
// fold_latch: the caller's next kernel on the stream latches the fault word (ngpde_node_gcn2_forward: the exit scaling)
int32_t enqueue_forward_persistent(ngpde_node *p, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr, bool fold_latch = false) {
  NodePersistFwd a;
  a.no_latch = fold_latch;
  a.g = p->g; a.ps = &p->persist; a.n_steps = p->n_steps; a.S = p->tb.S; a.act = p->act; a.n_members = p->members;
  a.u_in = p->u; a.u_out = p->u;     // a tile writes its rows of u(T) only after all its readers are past phase 1
  a.bufA = p->ustage; a.bufB = p->pbuf;
  a.w1 = p->w1; a.b1 = p->b1; a.w2 = p->w2; a.b2 = p->b2;
  a.row_elems = p->row_elems;
  if (p->with_bwd) {
    a.tape = p->tape; a.masks = p->masks; a.mask_bytes = p->mask_bytes; a.ztape = p->ztape;
  }
  a.interleave = p->interleave; a.pair = p->pair; a.k_tiles = p->ktiles; a.state = p->kstate;
  a.of = p->has_of ? &p->of : nullptr;
  a.ev_start = ev0; a.ev_stop = ev1;
  return launch_node_fwd_persistent(a, stream);
}

// out[4] = where dW1, db1, dW2, db2 go (du x du / du arrays; NULL entries are skipped); nullptr: the plan's own d x d / d buffers
int32_t enqueue_backward_persistent(ngpde_node *p, hipStream_t stream, hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr,
                                    float *const *out = nullptr) {
  NodePersistBwd a;
  a.no_latch = true;   // (the reduction below latches)
  a.g = p->g; a.ps = &p->persist; a.n_steps = p->n_steps; a.S = p->tb.S; a.n_members = p->members; a.act = p->act;
  a.lam = p->lam; a.g1 = p->g1; a.g2 = p->g2; a.w1 = p->w1; a.w2 = p->w2;
  a.tape = p->tape; a.masks = p->masks; a.row_elems = p->row_elems; a.mask_bytes = p->mask_bytes; a.ztape = p->ztape;
  a.slab_dw1 = p->slab_dw1; a.slab_db1 = p->slab_db1; a.slab_dw2 = p->slab_dw2; a.slab_db2 = p->slab_db2;
  a.interleave = p->interleave; a.pair = p->pair; a.ubar = p->pubar; a.k_tiles = p->ktiles;
  a.ev_start = ev0; a.ev_stop = ev1;
  int32_t st;
  if ((st = launch_node_bwd_persistent(a, stream))) return st;
  const int dd = p->d * p->d;
  Reduce4 r;
  r.n_slabs = (p->pair || p->ktiles) ? p->persist.pair_wgs : p->persist.n_tiles;   // one slab per workgroup, each written once at the end of the launch
  r.slab[0] = p->slab_dw1; r.slab[1] = p->slab_db1; r.slab[2] = p->slab_dw2; r.slab[3] = p->slab_db2;
  r.len[0] = r.len[2] = dd; r.len[1] = r.len[3] = p->d;
  r.ct[0] = r.ct[2] = p->d / 16; r.ct[1] = r.ct[3] = 0;
  if (out) {
    for (int j = 0; j < 4; ++j) r.out[j] = out[j];
    r.du = p->du;
  } else {
    r.out[0] = p->dw1; r.out[1] = p->db1; r.out[2] = p->dw2; r.out[3] = p->db2;
    r.du = p->d;
  }
  r.abort_word = node_persistent_abort_word(&p->persist); r.fault = p->persist.fault;
  hipLaunchKernelGGL(reduce4_slabs_kernel, dim3((dd + 63) / 64, 4), dim3(1024), 0, stream, r);
  NGPDE_LAUNCH_CHECK("reduce4_slabs_kernel");
  return NGPDE_OK;
}

int32_t capture(ngpde_node *p, bool backward) {
  hipGraph_t graph = nullptr;
  NGPDE_HIP_CHECK(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeRelaxed));
  int count = 0;
  int32_t st = backward ? enqueue_backward(p, p->cap_stream, &count) : enqueue_forward(p, p->cap_stream, &count);
  hipError_t e = hipStreamEndCapture(p->cap_stream, &graph);
  if (st) {
    if (graph) (void)hipGraphDestroy(graph);
    return st;
  }
  if (e != hipSuccess) {
    if (graph) (void)hipGraphDestroy(graph);
    return fail(NGPDE_ERR_HIP, "hipStreamEndCapture failed: %s", hipGetErrorString(e));
  }
  hipGraphExec_t exec = nullptr;
  e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    (void)hipGraphDestroy(graph);
    return fail(NGPDE_ERR_HIP, "hipGraphInstantiate failed: %s", hipGetErrorString(e));
  }
  if (backward) {
    p->bwd_graph = graph; p->bwd_exec = exec; p->bwd_launches = count;
  } else {
    p->fwd_graph = graph; p->fwd_exec = exec; p->fwd_launches = count;
  }
  return NGPDE_OK;
}

}  // namespace

ngpde_node::~ngpde_node() {
  if (fwd_exec) (void)hipGraphExecDestroy(fwd_exec);
  if (bwd_exec) (void)hipGraphExecDestroy(bwd_exec);
  if (fwd_graph) (void)hipGraphDestroy(fwd_graph);
  if (bwd_graph) (void)hipGraphDestroy(bwd_graph);
  if (cap_stream) (void)hipStreamDestroy(cap_stream);
  own_first_tables_free(&of);
}

extern "C" {

int32_t ngpde_node_destroy(ngpde_node_t *p) {
  NGPDE_RANGE();
  delete p;
  return NGPDE_OK;
}

int32_t ngpde_node_gcn2_create(const ngpde_graph_t *g, int32_t d, int32_t act, int32_t tableau, int32_t n_steps,
                               float dt, int32_t with_backward, ngpde_node_t **out) {
  NGPDE_RANGE();
  return ngpde_node_gcn2_create_batch(g, 1, d, act, tableau, n_steps, dt, with_backward, out);
}

// d: the width the kernels run at; du <= d: the caller's width (see ngpde_node::du)
static int32_t node_create(const ngpde_graph_t *g, int32_t members, int32_t d, int32_t du, int32_t act, int32_t tableau,
                           int32_t n_steps, float dt, int32_t with_backward, ngpde_node_t **out) {
  if (g && out && members >= 1) {   // a handle without normalisation (ERR_STATE) and a width without kernels (ERR_UNSUPPORTED) are
    *out = nullptr;                 // reported before an invalid activation, tableau or step count, as they always were
    NGPDE_REQUIRE(g->has_norm, NGPDE_ERR_STATE, "ngpde_node_gcn2_create: GCN normalisation not set");
    NGPDE_REQUIRE(fused_supported(d, d), NGPDE_ERR_UNSUPPORTED,
                  "ngpde_node_gcn2_create: d must be one of 16, 32, 64, 128 (got %d)", d);
  }
  NGPDE_TRY(plan_check_create("ngpde_node_gcn2_create", g, out, tableau, n_steps, act, members));
  NGPDE_REQUIRE(g->n_nodes >= 1, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gcn2_create: empty graph");
  std::unique_ptr<ngpde_node> p(new (std::nothrow) ngpde_node());
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "out of host memory");
  p->g = g; p->d = d; p->du = du; p->act = act; p->n_steps = n_steps; p->dt = dt;
  p->with_bwd = with_backward != 0;
  p->needs_z = p->with_bwd && act_needs_z(act);
  p->tb = make_tableau(tableau);
  p->S = p->tb.S;
  p->n = g->n_nodes;
  p->members = members;
  p->row_elems = (size_t)p->n * d;
  p->all_elems = (size_t)members * p->row_elems;
  p->nb = fused_num_blocks(p->n);
  p->mask_mode = p->with_bwd && act == NGPDE_ACT_RELU && !switch_on(Switch::NoMask);
  p->pre = fused_prescaled_supported(g, d) && !switch_on(Switch::NoPrescale);
  // The persistent form (node_persistent.hip) is decided here, before the tape is sized: with an activation other than relu its
  // adjoint reads the pre-activations from a tape of its own layout.  (Interleaved batches: relu only.)
  int pmode = p->pre ? node_persistent_mode(g, d, act, p->with_bwd) : 0;
  // Graphs with hubs (a tile beyond the handle's 96-row halo lists, BASELINE config 1): the hub geometry of the persistent kernels, on
  // pre-scaled arrays like every persistent plan -- both directions or not at all (there is no pre-scaled replayed plan for them)
  bool hub = !p->pre && pmode == 0 && !switch_on(Switch::NoPrescale) && node_persistent_hub_possible(g, d) &&
             (!p->with_bwd || p->mask_mode || act != NGPDE_ACT_RELU);
  if (hub) {
    pmode = 4;
    p->pre = true;
  }
  p->pair = pmode == 2 && members == 1 && (!p->with_bwd || p->mask_mode);
  p->ktiles = (pmode == 3 && members == 1) ? node_persistent_rounds(g) : 0;
  bool want_persist = (pmode == 1 && (!p->with_bwd || p->mask_mode || (act != NGPDE_ACT_RELU && members == 1))) || p->pair || p->ktiles > 0 || hub;
  const int S = p->S;
  if (want_persist) {
    p->persistent = true;
    // stage-indexed coefficient tables (device memory): forward cf[i][j], adjoint dtb[j], cu[i][j]
    float coef[90] = {0};   // forward: rk_forward6 at 0 .. 41; adjoint: dt b at 42 + j, cu[i][j] (j > i >= 1) at 48 + i * 6 + j,
                            // self weights at 84 + i  (node_persistent.hip)
    const Tableau &tb = p->tb;
    rk_forward6(tb, dt, coef);
    for (int i = 0; i < S; ++i) coef[42 + i] = (float)(dt * tb.b[i]);
    for (int i = 1; i < S; ++i) {
      for (int j = i + 1; j < S; ++j) coef[48 + i * 6 + j] = (float)(dt * tb.a[j][i - 1]);
      coef[84 + i] = (float)(dt * tb.a[i][i - 1]);
    }
    const int32_t st = node_persistent_setup(g, coef, &p->persist, p->pair, hub);
    if (st == NGPDE_ERR_UNSUPPORTED) p->persistent = false;   // a wait list too long for one polling wave (or neighbouring tile pairs): the replayed plan
    else if (st != NGPDE_OK) return st;
    if (p->persistent && p->ktiles > 0) p->persist.pair_wgs = (p->persist.n_tiles + p->ktiles - 1) / p->ktiles;   // tile rounds: the grid is ceil(tiles / K)
  }
  if (!p->persistent) {
    p->pair = false;
    p->ktiles = 0;
  }
  if (hub && !p->persistent) {   // hub geometry refused (a cap): the unscaled replayed plan
    p->pre = false;
    hub = false;
    node_persistent_free(&p->persist);
  }
  p->hub = hub;
  // own-first slot tables (common.h: OwnFirst): for every pre-scaled plan on the handle's own tile lists -- persistent in any form or
  // replayed, one member or a batch, weighted or not -- so that all of them sum a row's neighbours in ONE order and stay bitwise
  // comparable; NGPDE_NO_OWN_FIRST=1 keeps the handle's order (A/B runs)
  // Only for graphs of one wave of workgroups (<= two 32-row tiles per CU): the forms for larger graphs -- tile pairs, tile rounds -- have
  // no exposed wait to fill and would only pay the padding rounds (32 768 nodes - 1.2 %, 65 536 - 0.7 %); the rule looks at the graph
  // and the device alone, never at a plan-selecting switch, so a graph's persistent and replayed plans always agree on it.
  int dev_ = 0, cus_ = 0;
  const bool one_wave = hipGetDevice(&dev_) == hipSuccess && hipDeviceGetAttribute(&cus_, hipDeviceAttributeMultiprocessorCount, dev_) == hipSuccess &&
                        p->nb <= 2 * cus_;
  if (p->pre && !hub && one_wave && !switch_on(Switch::NoOwnFirst)) {
    NGPDE_TRY(own_first_tables_build(g, &p->of, nullptr));
    p->has_of = true;
  }
  // activations other than relu: the persistent adjoint reads the pre-activations from a tape of its own layout
  p->ztape_mode = p->with_bwd && !p->mask_mode && p->persistent;
  p->slots = p->mask_mode ? 2 : (p->ztape_mode ? 4 : (p->with_bwd ? (p->needs_z ? 6 : 4) : 4));
  p->mask_bytes = p->mask_mode ? fused_mask_bytes(p->n, d) : 0;
  // two members at a time; one after the other in the hub geometry and under NGPDE_NO_INTERLEAVE=1 (the form the interleaved kernels are
  // compared with bit for bit)
  p->interleave = members > 1 && !hub && !switch_on(Switch::NoInterleave);
  const size_t xslots = p->interleave ? 2 : 1;   // [N][d] arrays per exchanged buffer
  DeviceBlocks &m = p->mem;
  NGPDE_TRY(m.take(&p->u, p->all_elems));
  NGPDE_TRY(m.take(&p->ustage, xslots * p->row_elems));
  NGPDE_TRY(m.take(&p->u0keep, (size_t)members * p->n * du));
  const bool padded = du != d;   // the padding of a widened plan's parameters is written once, here
  for (float **w : {&p->w1, &p->w2}) NGPDE_TRY(m.take(w, (size_t)d * d, padded));
  for (float **b : {&p->b1, &p->b2}) NGPDE_TRY(m.take(b, d, padded));
  const size_t tape_elems = (size_t)(p->with_bwd ? n_steps : 1) * S * p->slots * p->all_elems;
  p->tape_bytes = tape_elems * sizeof(float);
  NGPDE_TRY(m.take(&p->tape, tape_elems));
  if (p->mask_mode) {
    const size_t mb = (size_t)members * n_steps * S * 2 * p->mask_bytes;
    NGPDE_TRY(m.take(&p->ybuf, (size_t)S * 2 * p->row_elems));
    NGPDE_TRY(m.take(&p->masks, mb));
    p->tape_bytes += mb + (size_t)S * 2 * p->row_elems * sizeof(float);
  }
  if (p->with_bwd) {
    NGPDE_TRY(m.take(&p->lam, p->all_elems));
    for (float **x : {&p->g1, &p->g2}) NGPDE_TRY(m.take(x, xslots * p->row_elems));
    if (p->interleave || p->pair || p->ktiles) NGPDE_TRY(m.take(&p->pubar, 2 * 5 * p->row_elems));
    p->ubar.assign(S, nullptr);
    for (int j = 1; j < S; ++j) NGPDE_TRY(m.take(&p->ubar[j], p->row_elems));
    const size_t dd = (size_t)d * d;
    const size_t per = (size_t)p->nb * (dd + d);
    p->slab_bytes = 2 * per * sizeof(float);
    NGPDE_TRY(m.take(&p->slabs, 2 * per));
    p->slab_dw1 = p->slabs;
    p->slab_db1 = p->slab_dw1 + (size_t)p->nb * dd;
    p->slab_dw2 = p->slab_db1 + (size_t)p->nb * d;
    p->slab_db2 = p->slab_dw2 + (size_t)p->nb * dd;
    for (float **w : {&p->dw1, &p->dw2}) NGPDE_TRY(m.take(w, dd));
    for (float **b : {&p->db1, &p->db2}) NGPDE_TRY(m.take(b, d));
  }
  if (p->persistent) NGPDE_TRY(m.take(&p->pbuf, xslots * p->row_elems));
  if (p->ktiles) NGPDE_TRY(m.take(&p->kstate, 7 * p->row_elems));
  if (p->ztape_mode) p->ztape = p->tape + (size_t)n_steps * S * 2 * p->all_elems;
  NGPDE_REQUIRE(members == 1 || p->persistent, NGPDE_ERR_UNSUPPORTED,
                "ngpde_node_gcn2_create_batch: the member-by-member solve exists for the persistent plan only "
                "(d = 64, relu, unweighted, at most two 32-row tiles per CU); batch the graphs into one handle instead");
  if (p->persistent) {
    p->fwd_launches = 2;                          // flag reset, the solve (the fault latch rides on the exit scaling)
    p->bwd_launches = p->with_bwd ? 3 : 0;        // flag reset, the adjoint, ONE reduction of the four slab sets (it latches too)
  } else {
    hipError_t e = hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking);
    NGPDE_REQUIRE(e == hipSuccess, NGPDE_ERR_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    NGPDE_TRY(capture(p.get(), false));
    if (p->with_bwd) NGPDE_TRY(capture(p.get(), true));
  }
  // the zeroed parameter padding of a widened plan and node_persistent_setup's memsets are NULL-stream work that may return ahead of its
  // completion; the solves run on the caller's streams, which the NULL stream does not order (include/ngpde.h, "Creates")
  NGPDE_HIP_CHECK(hipStreamSynchronize(nullptr));
  *out = p.release();
  return NGPDE_OK;
}

int32_t ngpde_node_gcn2_create_batch(const ngpde_graph_t *g, int32_t members, int32_t d, int32_t act, int32_t tableau,
                                     int32_t n_steps, float dt, int32_t with_backward, ngpde_node_t **out) {
  NGPDE_RANGE();
  // d = 16 / 32 where the 64-wide persistent solver can take the graph: run widened (NGPDE_NO_WIDEN=1: the native-width replayed plan)
  if (out && g && (d == 16 || d == 32) && !switch_on(Switch::NoWiden) && g->has_norm && g->n_nodes >= 1 &&
      (node_persistent_mode(g, 64, act, with_backward != 0) != 0 || node_persistent_hub_possible(g, 64))) {
    ngpde_node_t *w = nullptr;
    if (node_create(g, members, 64, d, act, tableau, n_steps, dt, with_backward, &w) == NGPDE_OK) {
      if (w->persistent) {
        *out = w;
        return NGPDE_OK;
      }
      delete w;
    }
  }
  return node_create(g, members, d, d, act, tableau, n_steps, dt, with_backward, out);
}

size_t ngpde_node_tape_bytes(const ngpde_node_t *p) { return p ? p->tape_bytes : 0; }

int32_t ngpde_node_launch_count(const ngpde_node_t *p, int32_t *forward, int32_t *backward) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_launch_count: plan is NULL");
  if (forward) *forward = p->fwd_launches;
  if (backward) *backward = p->bwd_launches;
  return NGPDE_OK;
}

int32_t ngpde_node_flags(const ngpde_node_t *p, int32_t *flags) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr && flags != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_flags: NULL argument");
  *flags = (p->pre ? NGPDE_NODE_PRESCALED : 0) | (p->mask_mode ? NGPDE_NODE_SIGN_MASKS : 0) |
           (p->persistent ? NGPDE_NODE_PERSISTENT_FWD : 0) | (p->persistent && p->with_bwd ? NGPDE_NODE_PERSISTENT_BWD : 0) |
           (p->pair ? NGPDE_NODE_TILE_PAIRS : 0) | (p->ktiles ? NGPDE_NODE_TILE_ROUNDS : 0) | (p->du != p->d ? NGPDE_NODE_WIDENED : 0) |
           (p->hub ? NGPDE_NODE_HUB_GEOMETRY : 0) | (p->has_of ? NGPDE_NODE_OWN_FIRST : 0);
  return NGPDE_OK;
}

int32_t ngpde_node_fault(ngpde_node_t *p, ngpde_stream_t stream, int32_t *fault) {
  NGPDE_RANGE();
  return plan_fault("ngpde_node_fault", p, stream, fault);
}

int32_t ngpde_node_pipeline_stats(ngpde_node_t *p, ngpde_stream_t stream_, int64_t *ahead_forward, int64_t *ahead_backward,
                                  int64_t *slot_phases) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_pipeline_stats: plan is NULL");
  if (ahead_forward) *ahead_forward = 0;
  if (ahead_backward) *ahead_backward = 0;
  if (slot_phases) *slot_phases = 0;
  if (!p->persist.stats) return NGPDE_OK;
  const int nt = p->persist.n_tiles;
  std::vector<int> h((size_t)nt * 2);
  NGPDE_HIP_CHECK(hipMemcpyAsync(h.data(), p->persist.stats, h.size() * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream_));
  NGPDE_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream_));
  int64_t f = 0, b = 0;
  for (int t = 0; t < nt; ++t) f += h[2 * t], b += h[2 * t + 1];
  if (ahead_forward) *ahead_forward = f;
  if (ahead_backward) *ahead_backward = b;
  if (slot_phases) *slot_phases = (int64_t)nt * p->members * p->n_steps * p->tb.S * 2;
  return NGPDE_OK;
}

int32_t ngpde_node_gcn2_forward(ngpde_node_t *p, const float *u0, const float *w1, const float *b1, const float *w2,
                                const float *b2, float *uT, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gcn2_forward: plan is NULL");
  NGPDE_REQUIRE(u0 && w1 && w2 && uT, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gcn2_forward: NULL argument");
  NGPDE_REQUIRE_LIVE("ngpde_node_gcn2_forward", p);
  hipStream_t stream = (hipStream_t)stream_;
  const size_t user_bytes = (size_t)p->members * p->n * p->du * sizeof(float);
  // entry: three launches where there were up to nine stream operations (round 5) -- u0 scaled into the plan and kept raw by one kernel,
  // the four parameter arrays by one
  if (p->pre) {
    RowsExtra x;
    x.keep = reinterpret_cast<float4 *>(p->u0keep);
    int32_t st = launch_scale_rows_width(u0, p->du, p->g->c, p->u, p->d, p->n, false, stream, p->members, x);
    if (st) return st;
  } else {
    NGPDE_HIP_CHECK(hipMemcpyAsync(p->u, u0, p->all_elems * sizeof(float), hipMemcpyDeviceToDevice, stream));
    NGPDE_HIP_CHECK(hipMemcpyAsync(p->u0keep, u0, user_bytes, hipMemcpyDeviceToDevice, stream));
  }
  {
    int32_t st = launch_pack_params(w1, b1, w2, b2, p->du, p->d, p->w1, p->b1, p->w2, p->b2, stream);
    if (st) return st;
  }
  const bool fold_latch = p->persistent && p->pre;   // (the exit scaling latches the launch's fault word)
  if (p->persistent) {
    int32_t st = enqueue_forward_persistent(p, stream, nullptr, nullptr, fold_latch);
    if (st) return st;
  } else {
    NGPDE_HIP_CHECK(hipGraphLaunch(p->fwd_exec, stream));
  }
  if (p->pre) {
    RowsExtra x;
    if (fold_latch) { x.abort_word = node_persistent_abort_word(&p->persist); x.fault = p->persist.fault; }
    int32_t st = launch_scale_rows_width(p->u, p->d, p->g->c, uT, p->du, p->n, true, stream, p->members, x);
    if (st) return st;
  } else {
    NGPDE_HIP_CHECK(hipMemcpyAsync(uT, p->u, p->all_elems * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  p->solved = true;
  ++p->generation;
  p->backward_pending = p->with_bwd;
  return NGPDE_OK;
}

int32_t ngpde_node_generation(const ngpde_node_t *p, uint64_t *generation, int32_t *backward_pending) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_generation: plan is NULL");
  if (generation) *generation = p->generation;
  if (backward_pending) *backward_pending = p->backward_pending ? 1 : 0;
  return NGPDE_OK;
}

int32_t ngpde_node_expect_generation(const ngpde_node_t *p, uint64_t generation) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_expect_generation: plan is NULL");
  NGPDE_REQUIRE(p->generation == generation, NGPDE_ERR_STATE,
                "the plan's tape belongs to solve %llu, not %llu: another forward ran on this plan before this backward "
                "(one solve in flight per plan; use one plan per outstanding solve)",
                (unsigned long long)p->generation, (unsigned long long)generation);
  return NGPDE_OK;
}

int32_t ngpde_node_gcn2_backward(ngpde_node_t *p, const float *duT, float *du0, float *dw1, float *db1, float *dw2,
                                 float *db2, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gcn2_backward: plan is NULL");
  NGPDE_REQUIRE(p->with_bwd, NGPDE_ERR_STATE, "ngpde_node_gcn2_backward: plan was created without backward");
  NGPDE_REQUIRE(p->solved, NGPDE_ERR_STATE, "ngpde_node_gcn2_backward: forward has not been run");
  NGPDE_REQUIRE(duT != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_gcn2_backward: duT is NULL");
  NGPDE_REQUIRE_LIVE("ngpde_node_gcn2_backward", p);
  hipStream_t stream = (hipStream_t)stream_;
  const size_t dd = (size_t)p->d * p->d * sizeof(float), db = (size_t)p->du * sizeof(float);
  if (p->pre) {   // u(T) = u~(T) ./ c  =>  dL/du~(T) = duT ./ c
    int32_t st = launch_scale_rows_width(duT, p->du, p->g->c, p->lam, p->d, p->n, true, stream, p->members);
    if (st) return st;
  } else {
    NGPDE_HIP_CHECK(hipMemcpyAsync(p->lam, duT, p->all_elems * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  if (p->persistent) {   // (its one reduction launch writes the four gradients where the caller wants them)
    float *const outs[4] = {dw1, db1, dw2, db2};
    int32_t st = enqueue_backward_persistent(p, stream, nullptr, nullptr, outs);
    if (st) return st;
  } else {
    NGPDE_HIP_CHECK(hipGraphLaunch(p->bwd_exec, stream));
  }
  if (du0 && p->pre) {   // u~0 = c .* u0  =>  du0 = c .* dL/du~0
    int32_t st = launch_scale_rows_width(p->lam, p->d, p->g->c, du0, p->du, p->n, false, stream, p->members);
    if (st) return st;
  } else if (du0) {
    NGPDE_HIP_CHECK(hipMemcpyAsync(du0, p->lam, p->all_elems * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  p->backward_pending = false;
  if (p->persistent) return NGPDE_OK;
  if (p->du != p->d) {
    int32_t st;
    if (dw1 && (st = copy_block(dw1, p->du, p->dw1, p->d, p->du, p->du, stream))) return st;
    if (dw2 && (st = copy_block(dw2, p->du, p->dw2, p->d, p->du, p->du, stream))) return st;
  } else {
    if (dw1) NGPDE_HIP_CHECK(hipMemcpyAsync(dw1, p->dw1, dd, hipMemcpyDeviceToDevice, stream));
    if (dw2) NGPDE_HIP_CHECK(hipMemcpyAsync(dw2, p->dw2, dd, hipMemcpyDeviceToDevice, stream));
  }
  if (db1) NGPDE_HIP_CHECK(hipMemcpyAsync(db1, p->db1, db, hipMemcpyDeviceToDevice, stream));
  if (db2) NGPDE_HIP_CHECK(hipMemcpyAsync(db2, p->db2, db, hipMemcpyDeviceToDevice, stream));
  return NGPDE_OK;
}

int32_t ngpde_node_profile(ngpde_node_t *p, int32_t stride, float *out_us, int32_t *out_count,
                           ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(p != nullptr && out_us != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_profile: NULL argument");
  NGPDE_REQUIRE(p->solved, NGPDE_ERR_STATE, "ngpde_node_profile: run a forward solve first");
  NGPDE_REQUIRE(stride >= 1, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_node_profile: stride must be >= 1");
  hipStream_t stream = (hipStream_t)stream_;
  Prof prof;
  prof.stride = stride;
  int32_t st;
  if (p->pre) {
    if ((st = launch_scale_rows_width(p->u0keep, p->du, p->g->c, p->u, p->d, p->n, false, stream, p->members))) return st;
  } else {
    NGPDE_HIP_CHECK(hipMemcpyAsync(p->u, p->u0keep, p->all_elems * sizeof(float), hipMemcpyDeviceToDevice, stream));
  }
  hipEvent_t pe[4] = {nullptr, nullptr, nullptr, nullptr};
  if (p->persistent) {
    prof.want(0, &pe[0], &pe[1]);
    if ((st = enqueue_forward_persistent(p, stream, pe[0], pe[1]))) return st;
  } else if ((st = enqueue_forward(p, stream, nullptr, &prof))) return st;
  if (p->with_bwd) {
    // adjoint seed of loss = sum(u(T)): ones
    std::vector<float> ones(p->all_elems, 1.0f);
    NGPDE_HIP_CHECK(hipMemcpyAsync(p->lam, ones.data(), p->all_elems * sizeof(float), hipMemcpyHostToDevice, stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    if (p->persistent) {
      prof.counter = 0;
      prof.want(2, &pe[2], &pe[3]);
      if ((st = enqueue_backward_persistent(p, stream, pe[2], pe[3]))) return st;
    } else if ((st = enqueue_backward(p, stream, nullptr, &prof))) return st;
  }
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  double sum[4] = {0, 0, 0, 0};
  int cnt[4] = {0, 0, 0, 0};
  for (size_t k = 0; k < prof.role.size(); ++k) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, prof.ev0[k], prof.ev1[k]) != hipSuccess) continue;
    sum[prof.role[k]] += ms * 1000.0;
    cnt[prof.role[k]]++;
  }
  for (int r = 0; r < 4; ++r) {
    out_us[r] = cnt[r] ? (float)(sum[r] / cnt[r]) : 0.f;
    if (out_count) out_count[r] = cnt[r];
  }
  return NGPDE_OK;
}

}  // extern "C"
