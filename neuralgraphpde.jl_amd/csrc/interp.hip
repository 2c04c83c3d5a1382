// interp.hip -- k-nearest-neighbour interpolation between two point sets (include/ngpde_interp.h): the normalised Shepard weights
// of a k-NN query result, the weighted gather y_q = sum_j w_qj x[idx_qj], the by-point transpose of idx, and the pullback
// xbar_i = sum over the slots of point i of w[slot] * ybar[slot / k].  [UPSTREAM torch_geometric's knn_interpolate; the search is
// NearestNeighbors.knn, which ngpde_knn_query (neighbors.hip) stands for.]
// Both hot kernels are gathers of rows of d floats with a handful of flops each: what matters is how rows are spread over lanes.
//   forward   a group of dpl = lanes_per_entry(d) lanes per query, 64 / dpl queries per wave; a lane owns one feature column per
//             chunk of dpl columns, so a neighbour's row is one coalesced read; the k (idx, w) pairs of a query are loaded once by
//             the lanes of its group (dpl at a time) and handed round with __shfl; the sum runs in ascending j from 0.f.
//   backward  one wave per point, lanes laid out (slot, column) as in row_lanes.h: 64 / dpl slot lanes walk the point's slots side
//             by side, each in ascending order, and a fixed xor butterfly combines them -- no atomics, bitwise reproducible, and a
//             point named by hundreds of queries is not one lane's walk when d is small.
// The library is compiled with -ffp-contract=off: no product below is fused into its sum.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/ngpde_interp.h"
#include "common.h"
#include "device_scratch.h"
#include "row_lanes.h"
#include "workspace.h"

namespace ngpde {
namespace {

// w_j / W with c_j = max(d2_j, FLT_MIN), w_j = c_0 / c_j (all 1 where c_0 is inf), W = the sum in ascending j from 0.f
__global__ void interp_weights_kernel(int64_t m, int k, const float *__restrict__ d2, float *__restrict__ w) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m) return;
  const float *row = d2 + q * k;
  const float c0 = fmaxf(row[0], FLT_MIN);
  const bool flat = c0 == INFINITY;
  float W = 0.f;
  for (int j = 0; j < k; ++j) W = W + (flat ? 1.f : c0 / fmaxf(row[j], FLT_MIN));
  for (int j = 0; j < k; ++j) w[q * k + j] = (flat ? 1.f : c0 / fmaxf(row[j], FLT_MIN)) / W;
}

__global__ __launch_bounds__(256) void interp_forward_kernel(int n, int64_t m, int k, int d, const int32_t *__restrict__ idx,
                                                             const float *__restrict__ w, const float *__restrict__ x,
                                                             float *__restrict__ y) {
  const int lane = threadIdx.x & 63;
  const int dpl = lanes_per_entry(d), per_wave = 64 / dpl, grp = lane / dpl, cl = lane % dpl;
  const int64_t first = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * per_wave;   // the wave's first query
  if (first >= m) return;
  const int64_t q = first + grp;
  const bool live = q < m;
  const int64_t qr = live ? q : m - 1;   // a group past the end stays in the shuffles and stores nothing
  for (int c0 = 0; c0 < d; c0 += dpl) {
    const int c = c0 + cl;
    const bool ok = live && c < d;
    float acc = 0.f;
    for (int j0 = 0; j0 < k; j0 += dpl) {
      int my_i = -1;
      float my_w = 0.f;
      if (j0 + cl < k) {
        my_i = idx[qr * k + j0 + cl];
        my_w = w[qr * k + j0 + cl];
      }
      const int cnt = min(dpl, k - j0);
      for (int u0 = 0; u0 < cnt; u0 += 4) {   // four row reads in flight, summed in ascending j
        float t[4];
        bool use[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int src = grp * dpl + min(u0 + u, dpl - 1);
          const int i = __shfl(my_i, src);
          const float wi = __shfl(my_w, src);
          use[u] = ok && u0 + u < cnt && (unsigned)i < (unsigned)n;
          t[u] = use[u] ? wi * x[(size_t)i * d + c] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
          if (use[u]) acc = acc + t[u];
      }
    }
    if (ok) y[q * d + c] = acc;
  }
}

__global__ void interp_ptr_kernel(int64_t n, int64_t mk, const unsigned *__restrict__ key_sorted, int32_t *__restrict__ ptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  ptr[i] = (int32_t)lower_bound_dev<unsigned>(key_sorted, mk, (unsigned)i);
}

__global__ __launch_bounds__(256) void interp_backward_kernel(int n, int64_t mk, int k, int d, const int32_t *__restrict__ ptr,
                                                              const int32_t *__restrict__ slot, const float *__restrict__ w,
                                                              const float *__restrict__ ybar, float *__restrict__ xbar) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;
  const int rs = max(ptr[row], 0), re = (int)min((int64_t)ptr[row + 1], mk);
  const int dpl = lanes_per_entry(d), slots = 64 / dpl, sl = lane / dpl, cl = lane % dpl;
  for (int c0 = 0; c0 < d; c0 += dpl) {
    const int c = min(c0 + cl, d - 1);
    float a = 0.f;
    for (int p0 = rs + sl; p0 < re; p0 += 4 * slots) {   // four gathers in flight, summed in ascending order
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * slots;
        const int pos = p < re ? slot[p] : -1;
        const bool use = (unsigned)pos < (unsigned)mk;
        v[u] = use ? w[pos] * ybar[(size_t)(pos / k) * d + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (p0 + u * slots < re) a = a + v[u];
    }
    for (int o = dpl; o < 64; o <<= 1) a = a + __shfl_xor(a, o);
    if (sl == 0 && c0 + cl < d) xbar[(size_t)row * d + c] = a;
  }
}

// the caller workspace of the transpose: the sorted point keys of the m * k positions (the sort's own temporary is the call's)
struct TransposeWs {
  unsigned *key_sorted;
};
void transpose_layout(Workspace &ws, int64_t mk, TransposeWs *out) { out->key_sorted = ws.take<unsigned>((size_t)mk); }

int32_t check_sizes(const char *fn, int64_t n, int64_t m, int32_t k) {
  NGPDE_REQUIRE(n >= 0 && n <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: number of points %lld outside 0:2^31-1", fn, (long long)n);
  NGPDE_REQUIRE(m >= 0 && m <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: number of queries %lld outside 0:2^31-1", fn, (long long)m);
  NGPDE_REQUIRE(k >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: k must be >= 0 (got %d)", fn, k);
  NGPDE_REQUIRE(m * (int64_t)k <= 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "%s: m * k = %lld, more than int32 positions", fn,
                (long long)(m * (int64_t)k));
  return NGPDE_OK;
}

}  // namespace
}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_knn_interp_weights(int64_t m, int32_t k, const float *d2, float *w, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_sizes("knn_interp_weights", 0, m, k);
  if (st) return st;
  if (m == 0 || k == 0) return NGPDE_OK;
  NGPDE_REQUIRE(d2 != nullptr && w != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_weights: d2 or w is NULL");
  hipLaunchKernelGGL(interp_weights_kernel, dim3(blocks_for(m)), dim3(kB), 0, (hipStream_t)stream, m, k, d2, w);
  NGPDE_LAUNCH_CHECK("interp_weights_kernel");
  return NGPDE_OK;
}

int32_t ngpde_knn_interp_forward(int64_t n, int64_t m, int32_t k, int32_t d, const int32_t *idx, const float *w, const float *x,
                                 float *y, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_sizes("knn_interp_forward", n, m, k);
  if (st) return st;
  NGPDE_REQUIRE(d >= 1, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_forward: the feature width must be >= 1 (got %d)", d);
  if (m == 0) return NGPDE_OK;
  NGPDE_REQUIRE(y != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_forward: y is NULL");
  hipStream_t hs = (hipStream_t)stream;
  if (n == 0 || k == 0) {   // an empty sum
    NGPDE_HIP_CHECK(hipMemsetAsync(y, 0, (size_t)m * d * sizeof(float), hs));
    return NGPDE_OK;
  }
  NGPDE_REQUIRE(idx != nullptr && w != nullptr && x != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_forward: idx, w or x is NULL");
  const int per_wave = 64 / lanes_per_entry(d);
  const int64_t waves = (m + per_wave - 1) / per_wave;
  hipLaunchKernelGGL(interp_forward_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, hs, (int)n, m, k, d, idx, w, x, y);
  NGPDE_LAUNCH_CHECK("interp_forward_kernel");
  return NGPDE_OK;
}

size_t ngpde_knn_interp_transpose_workspace_bytes(int64_t n, int64_t m, int32_t k) {
  if (n < 0 || n > 0x7fffffffLL || m < 0 || k < 0 || m > 0x7fffffffLL || m * (int64_t)k > 0x7fffffffLL) return 0;
  TransposeWs t;
  return measure(transpose_layout, m * (int64_t)k, &t);
}

int32_t ngpde_knn_interp_transpose(int64_t n, int64_t m, int32_t k, const int32_t *idx, int32_t *ptr, int32_t *slot, void *workspace,
                                   size_t workspace_bytes, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_sizes("knn_interp_transpose", n, m, k);
  if (st) return st;
  NGPDE_REQUIRE(ptr != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_transpose: ptr is NULL");
  const int64_t mk = m * (int64_t)k;
  hipStream_t hs = (hipStream_t)stream;
  if (mk == 0) {
    NGPDE_HIP_CHECK(hipMemsetAsync(ptr, 0, ((size_t)n + 1) * sizeof(int32_t), hs));
    NGPDE_HIP_CHECK(hipStreamSynchronize(hs));
    return NGPDE_OK;
  }
  NGPDE_REQUIRE(idx != nullptr && slot != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_transpose: idx or slot is NULL");
  TransposeWs t;
  const size_t needed = measure(transpose_layout, mk, &t);
  if ((st = check_workspace("knn_interp_transpose", workspace, workspace_bytes, needed, 4))) return st;
  Workspace ws(workspace);
  transpose_layout(ws, mk, &t);
  Scratch sc;
  // one stable sort of the positions 0 .. m*k-1 by the point they name: equal keys keep their order, so a point's slots ascend.
  // Keys are compared as unsigned over all 32 bits: an index outside 0:n-1 sorts behind ptr[n] and belongs to no row.
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, reinterpret_cast<const unsigned *>(idx), t.key_sorted,
                                     rocprim::counting_iterator<int32_t>(0), slot, (size_t)mk, 0u, 32u, hs);
  };
  if ((st = with_temp(sc, sort))) return st;
  hipLaunchKernelGGL(interp_ptr_kernel, dim3(blocks_for(n + 1)), dim3(kB), 0, hs, n, mk, t.key_sorted, ptr);
  NGPDE_LAUNCH_CHECK("interp_ptr_kernel");
  NGPDE_HIP_CHECK(hipStreamSynchronize(hs));
  return NGPDE_OK;
}

int32_t ngpde_knn_interp_backward(int64_t n, int64_t m, int32_t k, int32_t d, const int32_t *ptr, const int32_t *slot, const float *w,
                                  const float *ybar, float *xbar, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_sizes("knn_interp_backward", n, m, k);
  if (st) return st;
  NGPDE_REQUIRE(d >= 1, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_backward: the feature width must be >= 1 (got %d)", d);
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(xbar != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "knn_interp_backward: xbar is NULL");
  hipStream_t hs = (hipStream_t)stream;
  const int64_t mk = m * (int64_t)k;
  if (mk == 0) {   // no query names a point
    NGPDE_HIP_CHECK(hipMemsetAsync(xbar, 0, (size_t)n * d * sizeof(float), hs));
    return NGPDE_OK;
  }
  NGPDE_REQUIRE(ptr != nullptr && slot != nullptr && w != nullptr && ybar != nullptr, NGPDE_ERR_INVALID_ARGUMENT,
                "knn_interp_backward: ptr, slot, w or ybar is NULL");
  hipLaunchKernelGGL(interp_backward_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, hs, (int)n, mk, k, d, ptr, slot, w, ybar, xbar);
  NGPDE_LAUNCH_CHECK("interp_backward_kernel");
  return NGPDE_OK;
}

}  // extern "C"
