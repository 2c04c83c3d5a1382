// msgpass.hip -- the public message-passing API the reference re-exports from GraphNeuralNetworks.jl (src/NeuralGraphPDE.jl:5-11:
// propagate, apply_edges, aggregate_neighbors, softmax_edge_neighbors and the built-in messages) and tells users to build their own
// layers on (docs/src/devdoc.md:47-52).  The reduction half is segment_reduce_* / edge_permute (mp_kernels.hip); this file holds
//   K1  the node -> edge gather of up to 4 arrays (xi = X[t_p], xj = X[s_p], p order) and its pullback,
//   K2  propagate(e_mul_xj | w_mul_xj | copy_xj, g, + | mean) without an [E][D] message array, and its pullback,
//   K3  apply_edges(xi_dot_xj) straight into COO order, and its pullback,
//   K4  softmax_edge_neighbors (per target over its incoming edges), and its pullback.
// Every kernel is one wave per node row (by target, or by source for the pullbacks towards sources), atomic-free; the lanes are
// (entry slot, column): `dpl` lanes cover one chunk of a row's columns, 64 / dpl entries are processed at once, and the slots'
// partial sums are combined by a fixed xor butterfly, so every result is bitwise reproducible from run to run.  Columns are float4
// where the width is a multiple of 4 and the arrays are 16-byte aligned, floats otherwise.
#include <algorithm>

#include "common.h"
#include "device_utils.h"
#include "row_lanes.h"

namespace ngpde {

namespace {

constexpr int kMaxGather = 4;

// (the float / float4 forms of the operations the row loops need, and lanes_per_entry: row_lanes.h)

// sum over the entries q = rs + slot, rs + slot + slots, ... < re of term(q): four independent terms in flight, then the slots'
// partials combined across the wave (every lane of a column ends with the same bits)
template <typename T, typename F>
__device__ __forceinline__ T row_sum(int rs, int re, int slot, int slots, int dpl, F term) {
  T acc[4] = {vzero(T()), vzero(T()), vzero(T()), vzero(T())};
  for (int q0 = rs + slot; q0 < re; q0 += 4 * slots) {
    T v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + u * slots;
      v[u] = q < re ? term(q) : vzero(T());
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = vadd(acc[u], v[u]);
  }
  T a = vadd(vadd(acc[0], acc[1]), vadd(acc[2], acc[3]));
  for (int o = dpl; o < 64; o <<= 1) a = vadd(a, vxor(a, o));
  return a;
}

struct GatherArgs {
  int n;
  const float *x[kMaxGather];
  float *xi[kMaxGather];  // [E][w] p order, or NULL
  float *xj[kMaxGather];
  int w[kMaxGather];      // row width in floats
  int vec[kMaxGather];    // float4 rows
};

struct ScatterArgs {
  int n;
  const float *dxi[kMaxGather];  // [E][w] p order, or NULL
  const float *dxj[kMaxGather];
  float *dx[kMaxGather];         // [N][w]
  int w[kMaxGather];
  int vec[kMaxGather];
};

// ---- K1: xi_p = X[i], xj_p = X[col_p] for the entries p of target row i; the row's entries are contiguous in p order, so the
// wave walks (entry, column) pairs of the whole row flat and every store is coalesced
template <typename T>
__device__ __forceinline__ void gather_row(int i, int rs, int re, const int *__restrict__ col, const T *__restrict__ X, T *xi, T *xj,
                                           int w, int lane) {
  const int total = (re - rs) * w;
  const T *xrow = X + (size_t)i * w;
  T *xi_r = xi ? xi + (size_t)rs * w : nullptr;
  T *xj_r = xj ? xj + (size_t)rs * w : nullptr;
  for (int k0 = 0; k0 < total; k0 += 256) {   // four (entry, column) pairs per lane in flight
    T v[4] = {vzero(T()), vzero(T()), vzero(T()), vzero(T())};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * 64 + lane;
      if (k < total && xj_r) {
        const int q = k / w;
        v[u] = X[(size_t)col[rs + q] * w + (k - q * w)];
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int k = k0 + u * 64 + lane;
      if (k < total) {
        if (xi_r) xi_r[k] = xrow[k % w];
        if (xj_r) xj_r[k] = v[u];
      }
    }
  }
}

__global__ __launch_bounds__(256) void gather_fwd_kernel(int n_nodes, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                         GatherArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_nodes) return;
  const int rs = rowptr[row], re = rowptr[row + 1];
  for (int k = 0; k < a.n; ++k) {
    if (a.vec[k])
      gather_row<float4>(row, rs, re, col, reinterpret_cast<const float4 *>(a.x[k]), reinterpret_cast<float4 *>(a.xi[k]),
                         reinterpret_cast<float4 *>(a.xj[k]), a.w[k] / 4, lane);
    else
      gather_row<float>(row, rs, re, col, a.x[k], a.xi[k], a.xj[k], a.w[k], lane);
  }
}

// dX[i] = sum_{p in in(i)} dxi_p + sum_{q in out(i)} dxj_{xpos_q}  (the by-source list read through xpos, as edge_sum_by_source_kernel)
template <typename T>
__device__ __forceinline__ void scatter_row(int i, int rs_t, int re_t, int rs_s, int re_s, const int *__restrict__ xpos,
                                            const T *__restrict__ dxi, const T *__restrict__ dxj, T *__restrict__ dx, int w, int lane) {
  const int dpl = lanes_per_entry(w), slots = 64 / dpl, slot = lane / dpl, cl = lane % dpl;
  for (int c0 = 0; c0 < w; c0 += dpl) {
    const int c = min(c0 + cl, w - 1);
    T s = vzero(T());
    if (dxi) s = row_sum<T>(rs_t, re_t, slot, slots, dpl, [&](int p) { return dxi[(size_t)p * w + c]; });
    if (dxj) s = vadd(s, row_sum<T>(rs_s, re_s, slot, slots, dpl, [&](int q) { return dxj[(size_t)xpos[q] * w + c]; }));
    if (slot == 0 && c0 + cl < w) dx[(size_t)i * w + c] = s;
  }
}

__global__ __launch_bounds__(256) void gather_bwd_kernel(int n_nodes, const int *__restrict__ rowptr_t, const int *__restrict__ rowptr_s,
                                                         const int *__restrict__ xpos_s, ScatterArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_nodes) return;
  const int rs_t = rowptr_t[row], re_t = rowptr_t[row + 1], rs_s = rowptr_s[row], re_s = rowptr_s[row + 1];
  for (int k = 0; k < a.n; ++k) {
    if (a.vec[k])
      scatter_row<float4>(row, rs_t, re_t, rs_s, re_s, xpos_s, reinterpret_cast<const float4 *>(a.dxi[k]),
                          reinterpret_cast<const float4 *>(a.dxj[k]), reinterpret_cast<float4 *>(a.dx[k]), a.w[k] / 4, lane);
    else
      scatter_row<float>(row, rs_t, re_t, rs_s, re_s, xpos_s, a.dxi[k], a.dxj[k], a.dx[k], a.w[k], lane);
  }
}

// ---- K2: out_i = aggr_{p in in(i)} e_{eid_p} * X[col_p]   (EW: 0 = no e (copy_xj), 1 = a scalar per edge, 2 = a row per edge).
// Rows are walked by target (forward: rowptr/col/eid of by_t) -- the same kernel, by source, is the pullback's transposed sum when
// `deg_rowptr` names the OTHER direction's row pointers for the mean's 1/deg of each entry's far end.
template <typename T, int EW>
__global__ __launch_bounds__(256) void emul_sum_kernel(int n_nodes, int w, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                       const int *__restrict__ eid, const T *__restrict__ X, const float *__restrict__ e,
                                                       int mean_own, const int *__restrict__ deg_rowptr, T *__restrict__ out,
                                                       const T *__restrict__ x_own, T *__restrict__ de) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_nodes) return;
  const int rs = rowptr[row], re = rowptr[row + 1];
  const int dpl = lanes_per_entry(w), slots = 64 / dpl, slot = lane / dpl, cl = lane % dpl;
  const T *E = reinterpret_cast<const T *>(e);
  for (int c0 = 0; c0 < w; c0 += dpl) {
    const int c = min(c0 + cl, w - 1);
    const bool ok = c0 + cl < w;
    const T xo = (de && EW == 2) ? x_own[(size_t)row * w + c] : vzero(T());
    T s = row_sum<T>(rs, re, slot, slots, dpl, [&](int p) {
      const int other = col[p];
      T v = X[(size_t)other * w + c];
      if (deg_rowptr) v = vscale(1.0f / (float)(deg_rowptr[other + 1] - deg_rowptr[other]), v);   // (other has >= 1 entry: p)
      if constexpr (EW == 1) return vscale(e[eid[p]], v);
      if constexpr (EW == 2) {
        const size_t ep = (size_t)eid[p] * w + c;
        if (de && ok) de[ep] = vmul(v, xo);      // the pullback's de_e = dout_t / deg_t * x_s
        return vmul(E[ep], v);
      }
      return v;
    });
    if (mean_own) s = re > rs ? vscale(1.0f / (float)(re - rs), s) : vzero(T());
    if (out && slot == 0 && ok) out[(size_t)row * w + c] = s;
  }
}

// ---- K3: out_{eid_p} = scale_i <A[i], B[col_p]> for the entries p of target row i (scale = 1 / deg_i when `mean`).  Entries of a
// slot loop in step, so the lanes of one entry reduce the dot product among themselves (xor offsets < dpl stay inside the entry).
template <typename T>
__global__ __launch_bounds__(256) void edge_dot_kernel(int n_nodes, int w, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                       const int *__restrict__ eid, const T *__restrict__ A, const T *__restrict__ B,
                                                       int mean, float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_nodes) return;
  const int rs = rowptr[row], re = rowptr[row + 1];
  const int dpl = lanes_per_entry(w), slots = 64 / dpl, slot = lane / dpl, cl = lane % dpl;
  const float scale = (mean && re > rs) ? 1.0f / (float)(re - rs) : 1.0f;
  const T *arow = A + (size_t)row * w;
  for (int p0 = rs; p0 < re; p0 += slots) {   // wave-uniform trip count: every lane reaches the shuffles
    const int p = p0 + slot;
    const bool valid = p < re;
    const T *brow = B + (size_t)col[valid ? p : rs] * w;
    float acc = 0.f;
    for (int c = cl; c < w; c += dpl) acc += vhsum(vmul(arow[c], brow[c]));
    for (int o = 1; o < dpl; o <<= 1) acc += __shfl_xor(acc, o);
    if (valid && cl == 0) out[eid[p]] = scale * acc;
  }
}

// ---- K4: y = softmax over the incoming edges of each target, per head; e, y [E][H] in COO order, read / written through eid.
// Lanes (slot, head); three passes over the row's entries: max, sum of exp(e - max), y = exp(e - max) / sum.
__global__ __launch_bounds__(256) void softmax_edge_fwd_kernel(int n_nodes, int h, const int *__restrict__ rowptr, const int *__restrict__ eid,
                                                               const float *__restrict__ e, float *__restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_nodes) return;
  const int rs = rowptr[row], re = rowptr[row + 1];
  const int dpl = lanes_per_entry(h), slots = 64 / dpl, slot = lane / dpl, cl = lane % dpl;
  for (int c0 = 0; c0 < h; c0 += dpl) {
    const int c = min(c0 + cl, h - 1);
    float m = -INFINITY;
    for (int p = rs + slot; p < re; p += slots) m = fmaxf(m, e[(size_t)eid[p] * h + c]);
    for (int o = dpl; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
    const float s = row_sum<float>(rs, re, slot, slots, dpl, [&](int p) { return expf(e[(size_t)eid[p] * h + c] - m); });
    if (c0 + cl < h)
      for (int p = rs + slot; p < re; p += slots) {
        const size_t ep = (size_t)eid[p] * h + c;
        y[ep] = expf(e[ep] - m) / s;
      }
  }
}

// de = y (dy - sum_row y dy)
__global__ __launch_bounds__(256) void softmax_edge_bwd_kernel(int n_nodes, int h, const int *__restrict__ rowptr, const int *__restrict__ eid,
                                                               const float *__restrict__ y, const float *__restrict__ dy,
                                                               float *__restrict__ de) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_nodes) return;
  const int rs = rowptr[row], re = rowptr[row + 1];
  const int dpl = lanes_per_entry(h), slots = 64 / dpl, slot = lane / dpl, cl = lane % dpl;
  for (int c0 = 0; c0 < h; c0 += dpl) {
    const int c = min(c0 + cl, h - 1);
    const float s = row_sum<float>(rs, re, slot, slots, dpl, [&](int p) {
      const size_t ep = (size_t)eid[p] * h + c;
      return y[ep] * dy[ep];
    });
    if (c0 + cl < h)
      for (int p = rs + slot; p < re; p += slots) {
        const size_t ep = (size_t)eid[p] * h + c;
        de[ep] = y[ep] * (dy[ep] - s);
      }
  }
}

inline unsigned rows4(int64_t rows) { return (unsigned)((rows + 3) / 4); }

// the flat (entry, column) index of the gather walks one row in int: a hub's in-degree times the width must fit
int32_t check_row_span(const char *fn, const ngpde_graph *g, int64_t w) {
  NGPDE_REQUIRE((int64_t)std::max(g->max_in_degree, g->max_out_degree) * w < ((int64_t)1 << 31), NGPDE_ERR_UNSUPPORTED,
                "%s: a row of %d entries x %lld floats exceeds 2^31", fn, (int)std::max(g->max_in_degree, g->max_out_degree), (long long)w);
  return NGPDE_OK;
}

template <typename T, int EW>
void emul_launch(const ngpde_graph *g, const Csr &rows, int w, const T *X, const float *e, int mean_own, const int *deg_rowptr, T *out,
                 const T *x_own, T *de, hipStream_t stream) {
  hipLaunchKernelGGL((emul_sum_kernel<T, EW>), dim3(rows4(g->n_nodes)), dim3(256), 0, stream, (int)g->n_nodes, w, rows.rowptr, rows.col,
                     rows.eid, X, e, mean_own, deg_rowptr, out, x_own, de);
}

// EW from the runtime e width, T from the alignment of every row array the launch touches
int32_t launch_emul(const ngpde_graph *g, const Csr &rows, int d, int ew, const float *X, const float *e, int mean_own,
                    const int *deg_rowptr, float *out, const float *x_own, float *de, hipStream_t stream) {
  const bool v4 = d % 4 == 0 && al16(X) && al16(out) && al16(x_own) && al16(de) && (ew != 2 || al16(e));
  const int mode = ew == 0 ? 0 : (ew == 1 ? 1 : 2);
#define NGPDE_EMUL_(T, EW) emul_launch<T, EW>(g, rows, v4 ? d / 4 : d, reinterpret_cast<const T *>(X), e, mean_own, deg_rowptr, \
                                              reinterpret_cast<T *>(out), reinterpret_cast<const T *>(x_own), reinterpret_cast<T *>(de), stream)
  if (v4) {
    if (mode == 0) NGPDE_EMUL_(float4, 0); else if (mode == 1) NGPDE_EMUL_(float4, 1); else NGPDE_EMUL_(float4, 2);
  } else {
    if (mode == 0) NGPDE_EMUL_(float, 0); else if (mode == 1) NGPDE_EMUL_(float, 1); else NGPDE_EMUL_(float, 2);
  }
#undef NGPDE_EMUL_
  NGPDE_LAUNCH_CHECK("emul_sum_kernel");
  return NGPDE_OK;
}

int32_t launch_edge_dot(const ngpde_graph *g, int d, const float *A, const float *B, int mean, float *out, hipStream_t stream) {
  if (d % 4 == 0 && al16(A) && al16(B))
    hipLaunchKernelGGL(edge_dot_kernel<float4>, dim3(rows4(g->n_nodes)), dim3(256), 0, stream, (int)g->n_nodes, d / 4, g->by_t.rowptr,
                       g->by_t.col, g->by_t.eid, reinterpret_cast<const float4 *>(A), reinterpret_cast<const float4 *>(B), mean, out);
  else
    hipLaunchKernelGGL(edge_dot_kernel<float>, dim3(rows4(g->n_nodes)), dim3(256), 0, stream, (int)g->n_nodes, d, g->by_t.rowptr,
                       g->by_t.col, g->by_t.eid, A, B, mean, out);
  NGPDE_LAUNCH_CHECK("edge_dot_kernel");
  return NGPDE_OK;
}

int32_t check_aggr_sum_mean(const char *fn, int32_t aggr) {
  NGPDE_REQUIRE(aggr == NGPDE_AGGR_SUM || aggr == NGPDE_AGGR_MEAN, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: aggregation %d not fused (+ and mean only; the others go through the gather and ngpde_segment_reduce_*)", fn, aggr);
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_gather_forward(const ngpde_graph_t *g, int32_t n, const float *const *x, const int32_t *width, float *const *xi,
                             float *const *xj, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(n >= 0 && n <= kMaxGather, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gather_forward: 0..%d arrays, got %d", kMaxGather, n);
  NGPDE_REQUIRE(n == 0 || (x && width), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gather_forward: NULL array table");
  for (int k = 0; k < n; ++k)
    NGPDE_REQUIRE(width[k] >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_gather_forward: negative width %d (array %d)", width[k], k);
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gather_forward: graph is NULL");
  GatherArgs a{};
  for (int k = 0; k < n; ++k) {
    float *oi = xi ? xi[k] : nullptr, *oj = xj ? xj[k] : nullptr;
    if (width[k] == 0 || g->n_edges == 0 || !(oi || oj)) continue;
    NGPDE_REQUIRE(x[k], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gather_forward: array %d is NULL", k);
    if (int32_t st = check_row_span("ngpde_gather_forward", g, width[k])) return st;
    const int m = a.n++;
    a.x[m] = x[k], a.xi[m] = oi, a.xj[m] = oj, a.w[m] = width[k];
    a.vec[m] = width[k] % 4 == 0 && al16(x[k]) && al16(oi) && al16(oj);
  }
  if (a.n == 0 || g->n_nodes == 0) return NGPDE_OK;
  hipLaunchKernelGGL(gather_fwd_kernel, dim3(rows4(g->n_nodes)), dim3(256), 0, (hipStream_t)stream, (int)g->n_nodes, g->by_t.rowptr,
                     g->by_t.col, a);
  NGPDE_LAUNCH_CHECK("gather_fwd_kernel");
  return NGPDE_OK;
}

int32_t ngpde_gather_backward(const ngpde_graph_t *g, int32_t n, const int32_t *width, const float *const *dxi, const float *const *dxj,
                              float *const *dx, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(n >= 0 && n <= kMaxGather, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gather_backward: 0..%d arrays, got %d", kMaxGather, n);
  NGPDE_REQUIRE(n == 0 || (width && dx), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gather_backward: NULL array table");
  for (int k = 0; k < n; ++k)
    NGPDE_REQUIRE(width[k] >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_gather_backward: negative width %d (array %d)", width[k], k);
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_gather_backward: graph is NULL");
  ScatterArgs a{};
  for (int k = 0; k < n; ++k) {
    if (width[k] == 0 || !dx[k]) continue;
    const float *gi = (dxi && g->n_edges) ? dxi[k] : nullptr, *gj = (dxj && g->n_edges) ? dxj[k] : nullptr;
    const int m = a.n++;   // (no edge-side gradient: the row sums are zeros, written like any other)
    a.dxi[m] = gi, a.dxj[m] = gj, a.dx[m] = dx[k], a.w[m] = width[k];
    a.vec[m] = width[k] % 4 == 0 && al16(gi) && al16(gj) && al16(dx[k]);
  }
  if (a.n == 0 || g->n_nodes == 0) return NGPDE_OK;
  hipLaunchKernelGGL(gather_bwd_kernel, dim3(rows4(g->n_nodes)), dim3(256), 0, (hipStream_t)stream, (int)g->n_nodes, g->by_t.rowptr,
                     g->by_s.rowptr, g->by_s.xpos, a);
  NGPDE_LAUNCH_CHECK("gather_bwd_kernel");
  return NGPDE_OK;
}

int32_t ngpde_propagate_emul_forward(const ngpde_graph_t *g, int32_t d, int32_t e_width, int32_t aggr, const float *x, const float *e,
                                     float *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(d >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_propagate_emul_forward: negative width %d", d);
  if (int32_t st = check_aggr_sum_mean("ngpde_propagate_emul_forward", aggr)) return st;
  NGPDE_REQUIRE(e_width == 0 || e_width == 1 || e_width == d, NGPDE_ERR_DIMENSION_MISMATCH,
                "ngpde_propagate_emul_forward: e has %d rows, expected 1 or %d", e_width, d);
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_propagate_emul_forward: graph is NULL");
  if (g->n_nodes == 0 || d == 0) return NGPDE_OK;
  NGPDE_REQUIRE(out && (g->n_edges == 0 || (x && (e_width == 0 || e))), NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_propagate_emul_forward: NULL argument");
  const int ew = e_width == 0 ? 0 : (e_width == 1 && d != 1 ? 1 : 2);
  return launch_emul(g, g->by_t, d, ew, x, e, aggr == NGPDE_AGGR_MEAN, nullptr, out, nullptr, nullptr, (hipStream_t)stream);
}

int32_t ngpde_propagate_emul_backward(const ngpde_graph_t *g, int32_t d, int32_t e_width, int32_t aggr, const float *x, const float *e,
                                      const float *dout, float *dx, float *de, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(d >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_propagate_emul_backward: negative width %d", d);
  if (int32_t st = check_aggr_sum_mean("ngpde_propagate_emul_backward", aggr)) return st;
  NGPDE_REQUIRE(e_width == 0 || e_width == 1 || e_width == d, NGPDE_ERR_DIMENSION_MISMATCH,
                "ngpde_propagate_emul_backward: e has %d rows, expected 1 or %d", e_width, d);
  NGPDE_REQUIRE(!(de && e_width == 0), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_propagate_emul_backward: de without e");
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_propagate_emul_backward: graph is NULL");
  if (g->n_nodes == 0 || d == 0 || !(dx || de)) return NGPDE_OK;
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(dout && (g->n_edges == 0 || ((e_width == 0 || e) && (x || !de))), NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_propagate_emul_backward: NULL argument");
  const int ew = e_width == 0 ? 0 : (e_width == 1 && d != 1 ? 1 : 2);
  const int *deg = aggr == NGPDE_AGGR_MEAN ? g->by_t.rowptr : nullptr;
  // dx_j = sum over the edges leaving j of e_e * dout_{t_e} (/ deg t_e); the width-D de_e = dout_t (/ deg t) * x_s in the same walk
  if (dx || (de && ew == 2)) {
    if (int32_t st = launch_emul(g, g->by_s, d, ew, dout, e, 0, deg, dx, ew == 2 ? x : nullptr, ew == 2 ? de : nullptr, stream)) return st;
  }
  // the width-1 de_e = <dout_t, x_s> (/ deg t): apply_edges(xi_dot_xj) of (dout, x)
  if (de && ew == 1 && g->n_edges) return launch_edge_dot(g, d, dout, x, aggr == NGPDE_AGGR_MEAN, de, stream);
  return NGPDE_OK;
}

int32_t ngpde_apply_edges_dot_forward(const ngpde_graph_t *g, int32_t d, const float *xi, const float *xj, float *out,
                                      ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(d >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_apply_edges_dot_forward: negative width %d", d);
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_apply_edges_dot_forward: graph is NULL");
  if (g->n_edges == 0) return NGPDE_OK;
  NGPDE_REQUIRE(out, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_apply_edges_dot_forward: out is NULL");
  if (d == 0) return launch_zero(out, (size_t)g->n_edges * 4, (hipStream_t)stream);
  NGPDE_REQUIRE(xi && xj, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_apply_edges_dot_forward: NULL argument");
  return launch_edge_dot(g, d, xi, xj, 0, out, (hipStream_t)stream);
}

int32_t ngpde_apply_edges_dot_backward(const ngpde_graph_t *g, int32_t d, const float *xi, const float *xj, const float *dout, float *dxi,
                                       float *dxj, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(d >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_apply_edges_dot_backward: negative width %d", d);
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_apply_edges_dot_backward: graph is NULL");
  if (g->n_nodes == 0 || d == 0) return NGPDE_OK;
  NGPDE_REQUIRE(g->n_edges == 0 || (dout && (!dxi || xj) && (!dxj || xi)), NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_apply_edges_dot_backward: NULL argument");
  hipStream_t stream = (hipStream_t)stream_;
  int32_t st;
  // dxi_i = sum_{p in in(i)} dout_e xj_{s}: propagate(e_mul_xj, +) with the scalar dout; dxj_j = the transposed walk with xi
  if (dxi && (st = launch_emul(g, g->by_t, d, d == 1 ? 2 : 1, xj, dout, 0, nullptr, dxi, nullptr, nullptr, stream))) return st;
  if (dxj && (st = launch_emul(g, g->by_s, d, d == 1 ? 2 : 1, xi, dout, 0, nullptr, dxj, nullptr, nullptr, stream))) return st;
  return NGPDE_OK;
}

int32_t ngpde_softmax_edge_neighbors_forward(const ngpde_graph_t *g, int32_t h, const float *e, float *y, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(h >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_softmax_edge_neighbors_forward: negative width %d", h);
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_softmax_edge_neighbors_forward: graph is NULL");
  if (g->n_edges == 0 || h == 0) return NGPDE_OK;
  NGPDE_REQUIRE(e && y, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_softmax_edge_neighbors_forward: NULL argument");
  hipLaunchKernelGGL(softmax_edge_fwd_kernel, dim3(rows4(g->n_nodes)), dim3(256), 0, (hipStream_t)stream, (int)g->n_nodes, h,
                     g->by_t.rowptr, g->by_t.eid, e, y);
  NGPDE_LAUNCH_CHECK("softmax_edge_fwd_kernel");
  return NGPDE_OK;
}

int32_t ngpde_softmax_edge_neighbors_backward(const ngpde_graph_t *g, int32_t h, const float *y, const float *dy, float *de,
                                              ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(h >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_softmax_edge_neighbors_backward: negative width %d", h);
  NGPDE_REQUIRE(g != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_softmax_edge_neighbors_backward: graph is NULL");
  if (g->n_edges == 0 || h == 0) return NGPDE_OK;
  NGPDE_REQUIRE(y && dy && de, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_softmax_edge_neighbors_backward: NULL argument");
  hipLaunchKernelGGL(softmax_edge_bwd_kernel, dim3(rows4(g->n_nodes)), dim3(256), 0, (hipStream_t)stream, (int)g->n_nodes, h,
                     g->by_t.rowptr, g->by_t.eid, y, dy, de);
  NGPDE_LAUNCH_CHECK("softmax_edge_bwd_kernel");
  return NGPDE_OK;
}

}  // extern "C"
