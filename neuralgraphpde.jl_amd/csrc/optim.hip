// optim.hip -- optimiser step on the FLAT parameter vector: the reference's tutorials keep
// the parameters as one ComponentArray and call Optimisers.update on it (/root/reference/docs/src/tutorials/
// graph_node.md:90,122-129 Adam; VMH.md:97 Rprop).  One launch right behind the gradient all-reduce on the same stream;
// the 1/world averaging of the reduced gradient is folded into the kernel (grad_scale).
#include <algorithm>

#include "common.h"
#include "device_utils.h"

namespace ngpde {
namespace {

// [UPSTREAM Optimisers.jl Adam]: m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
//                               x -= eta * (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
__global__ void adam_kernel(int64_t n, float *__restrict__ x, const float *__restrict__ g, float *__restrict__ m,
                            float *__restrict__ v, float eta, float b1, float b2, float eps, float c1, float c2, float gs) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = gs * g[i];
    const float mi = b1 * m[i] + (1.0f - b1) * gi;
    const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    x[i] -= mi / c1 / (sqrtf(vi / c2) + eps) * eta;
  }
}

// [UPSTREAM Optimisers.jl Rprop]: per-element step size grows by l2 while the gradient keeps its sign, shrinks by l1 when it
// flips (and that step is skipped: the remembered gradient becomes 0); x -= step * sign(remembered gradient)
__global__ void rprop_kernel(int64_t n, float *__restrict__ x, const float *__restrict__ g, float *__restrict__ gprev,
                             float *__restrict__ step, float l1, float l2, float smin, float smax, float gs) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float gi = gs * g[i], p = gprev[i] * gi;
    float s = step[i];
    s = p > 0.f ? fminf(s * l2, smax) : (p < 0.f ? fmaxf(s * l1, smin) : s);
    const float keep = p < 0.f ? 0.f : gi;
    step[i] = s;
    gprev[i] = keep;
    x[i] -= s * (keep > 0.f ? 1.f : (keep < 0.f ? -1.f : 0.f));
  }
}

// out = c_self * base + sum_k coef[k] * term[k]: the Runge-Kutta stage input u + dt sum_j a_ij k_j, the step update, and the
// combinations of the discrete adjoint, for a right-hand side whose stages are evaluated by arbitrary layers.  float4 path when
// everything is 16-byte aligned.
struct CombK {
  const float *term[8];
  float coef[8];
};
// `out` may alias `base` or a term (in-place accumulation of parameter cotangents: element i is read, then written, by one thread):
// no __restrict__ on them
template <int N, class T>
__global__ void rk_combine_kernel(int64_t count, float c_self, const T *base, const CombK k, T *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    T t[N > 0 ? N : 1];
#pragma unroll
    for (int j = 0; j < N; ++j) t[j] = reinterpret_cast<const T *>(k.term[j])[i];   // all loads first
    T v;
    if constexpr (sizeof(T) == 16) {
      v = base ? f4_scale(c_self, base[i]) : f4_zero();
#pragma unroll
      for (int j = 0; j < N; ++j) v = f4_fma(k.coef[j], t[j], v);
    } else {
      v = base ? c_self * base[i] : 0.f;
#pragma unroll
      for (int j = 0; j < N; ++j) v = fmaf(k.coef[j], t[j], v);
    }
    out[i] = v;
  }
}

// acc[k][i] += g[k][i] for up to kManyMax small arrays in one launch (blockIdx.y = array): the parameter cotangents of one
// right-hand-side pullback added to their accumulators (out aliases base: a thread reads and writes element i only)
constexpr int kManyMax = 24;
struct ManyK {
  float *acc[kManyMax];
  const float *g[kManyMax];
  int64_t count[kManyMax];
};
__global__ void accumulate_many_kernel(const ManyK k) {
  const int a = blockIdx.y;
  float *acc = k.acc[a];
  const float *g = k.g[a];
  const int64_t n = k.count[a];
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) acc[i] = fmaf(1.0f, g[i], 1.0f * acc[i]);
}

template <class T>
void launch_rk_combine(int n_terms, int64_t count, float c_self, const float *base, const CombK &k, float *out, hipStream_t stream) {
  const dim3 grid((unsigned)std::min<int64_t>((count + 255) / 256, 4096)), block(256);
  const T *b = reinterpret_cast<const T *>(base);
  T *o = reinterpret_cast<T *>(out);
  switch (n_terms) {
    case 0: hipLaunchKernelGGL((rk_combine_kernel<0, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    case 1: hipLaunchKernelGGL((rk_combine_kernel<1, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    case 2: hipLaunchKernelGGL((rk_combine_kernel<2, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    case 3: hipLaunchKernelGGL((rk_combine_kernel<3, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    case 4: hipLaunchKernelGGL((rk_combine_kernel<4, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    case 5: hipLaunchKernelGGL((rk_combine_kernel<5, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    case 6: hipLaunchKernelGGL((rk_combine_kernel<6, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    case 7: hipLaunchKernelGGL((rk_combine_kernel<7, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
    default: hipLaunchKernelGGL((rk_combine_kernel<8, T>), grid, block, 0, stream, count, c_self, b, k, o); break;
  }
}

// Dense output of one accepted step at up to kDenseMax save times: out[j] = 1 * u_prev + sum_i coef[j][i] k[i] (Tsit5's free
// interpolant with coef[j][i] = dt b_i(theta_j)).  u_prev and the stages are read once for all outputs; every output is the fmaf chain
// rk_combine_kernel forms with c_self = 1 (all loads first, then the chain in stage order), so it is bitwise one stage-combine call.
// The j loop is unrolled against the constant bound with a uniform early exit: the kernel-argument arrays are only ever indexed by
// constants.
constexpr int kDenseMax = 16;
struct DenseK {
  const float *k[8];
  float *out[kDenseMax];
  float coef[kDenseMax][8];
  int n_out;
};
template <int N, class T>
__global__ void rk_dense_output_kernel(int64_t count, const T *u_prev, const DenseK d) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    T t[N];
#pragma unroll
    for (int s = 0; s < N; ++s) t[s] = reinterpret_cast<const T *>(d.k[s])[i];     // all loads first
    const T u = u_prev[i];
#pragma unroll
    for (int j = 0; j < kDenseMax; ++j) {
      if (j >= d.n_out) break;
      T v;
      if constexpr (sizeof(T) == 16) {
        v = f4_scale(1.0f, u);
#pragma unroll
        for (int s = 0; s < N; ++s) v = f4_fma(d.coef[j][s], t[s], v);
      } else {
        v = 1.0f * u;
#pragma unroll
        for (int s = 0; s < N; ++s) v = fmaf(d.coef[j][s], t[s], v);
      }
      reinterpret_cast<T *>(d.out[j])[i] = v;
    }
  }
}

// Its adjoint over up to kDenseMax cotangents: kbar[s] = (first ? 0 : 1 * kbar[s]) + sum_j coef[j][s] dout[j] (the fmaf chain in j
// order) and, when ubar is given, ubar = 1 * ubar + sum_j 1 * dout[j].  Each cotangent is read once; a later launch of a longer list
// continues the chains from the partial sums (first = 0), as chained stage-combine calls would.
struct DensePullK {
  const float *dout[kDenseMax];
  float *kbar[8];
  float coef[kDenseMax][8];
  int n_out;
  int first;
};
template <int N, class T>
__global__ void __launch_bounds__(256) rk_dense_output_pullback_kernel(int64_t count, T *ubar, const DensePullK d) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    // every load before the first store: a load behind a store to an array that may alias it would wait for that store
    T g[kDenseMax], v[N], w;
#pragma unroll
    for (int j = 0; j < kDenseMax; ++j)
      if (j < d.n_out) g[j] = reinterpret_cast<const T *>(d.dout[j])[i];
    if constexpr (sizeof(T) == 16) {
#pragma unroll
      for (int s = 0; s < N; ++s) v[s] = d.first ? f4_zero() : f4_scale(1.0f, reinterpret_cast<const T *>(d.kbar[s])[i]);
      w = ubar ? f4_scale(1.0f, ubar[i]) : f4_zero();
#pragma unroll
      for (int s = 0; s < N; ++s) {
#pragma unroll
        for (int j = 0; j < kDenseMax; ++j)
          if (j < d.n_out) v[s] = f4_fma(d.coef[j][s], g[j], v[s]);
      }
#pragma unroll
      for (int j = 0; j < kDenseMax; ++j)
        if (j < d.n_out) w = f4_fma(1.0f, g[j], w);
    } else {
#pragma unroll
      for (int s = 0; s < N; ++s) v[s] = d.first ? 0.f : 1.0f * reinterpret_cast<const T *>(d.kbar[s])[i];
      w = ubar ? 1.0f * ubar[i] : 0.f;
#pragma unroll
      for (int s = 0; s < N; ++s) {
#pragma unroll
        for (int j = 0; j < kDenseMax; ++j)
          if (j < d.n_out) v[s] = fmaf(d.coef[j][s], g[j], v[s]);
      }
#pragma unroll
      for (int j = 0; j < kDenseMax; ++j)
        if (j < d.n_out) w = fmaf(1.0f, g[j], w);
    }
#pragma unroll
    for (int s = 0; s < N; ++s) reinterpret_cast<T *>(d.kbar[s])[i] = v[s];
    if (ubar) ubar[i] = w;
  }
}

#define NGPDE_STAGE_SWITCH(n, KERNEL, ...)                                                      \
  switch (n) {                                                                                  \
    case 1: hipLaunchKernelGGL((KERNEL<1, T>), __VA_ARGS__); break;                             \
    case 2: hipLaunchKernelGGL((KERNEL<2, T>), __VA_ARGS__); break;                             \
    case 3: hipLaunchKernelGGL((KERNEL<3, T>), __VA_ARGS__); break;                             \
    case 4: hipLaunchKernelGGL((KERNEL<4, T>), __VA_ARGS__); break;                             \
    case 5: hipLaunchKernelGGL((KERNEL<5, T>), __VA_ARGS__); break;                             \
    case 6: hipLaunchKernelGGL((KERNEL<6, T>), __VA_ARGS__); break;                             \
    case 7: hipLaunchKernelGGL((KERNEL<7, T>), __VA_ARGS__); break;                             \
    default: hipLaunchKernelGGL((KERNEL<8, T>), __VA_ARGS__); break;                            \
  }

template <class T>
void launch_rk_dense_output(int n_stages, int64_t count, const float *u_prev, const DenseK &d, hipStream_t stream) {
  const dim3 grid((unsigned)std::min<int64_t>((count + 255) / 256, 4096)), block(256);
  const T *u = reinterpret_cast<const T *>(u_prev);
  NGPDE_STAGE_SWITCH(n_stages, rk_dense_output_kernel, grid, block, 0, stream, count, u, d)
}

template <class T>
void launch_rk_dense_output_pullback(int n_stages, int64_t count, float *ubar, const DensePullK &d, hipStream_t stream) {
  const dim3 grid((unsigned)std::min<int64_t>((count + 255) / 256, 4096)), block(256);
  T *ub = reinterpret_cast<T *>(ubar);
  NGPDE_STAGE_SWITCH(n_stages, rk_dense_output_pullback_kernel, grid, block, 0, stream, count, ub, d)
}
#undef NGPDE_STAGE_SWITCH

// Scaled RMS norm of an embedded error estimate (OrdinaryDiffEq calculate_residuals + the default internalnorm):
//   out = sqrt( (1/count) sum_i ( e_i / (abstol + reltol max(|u_prev_i|, |u_new_i|)) )^2 ),  e_i = sum_j coef[j] term[j][i]
// e_i is formed exactly as rk_combine_kernel forms it with base = NULL (all loads first, then the fmaf chain in term order); the
// residual and its square are taken in double.  Two passes, no atomics: pass 1 writes one partial per block (thread sums in
// grid-stride order, a 64-lane shuffle tree per wave, the four waves' sums added in wave order), pass 2 is one block that adds the
// partials in the same fixed order.  Same inputs, same launch geometry (it depends on count only): the same bits.
constexpr int kNormThreads = 256;
constexpr int kNormMaxBlocks = 2048;

__device__ __forceinline__ double block_sum_256(double v) {
  __shared__ double wave_sum[kNormThreads / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];     // (read by thread 0 only)
}

__device__ __forceinline__ double scaled_sq(float e, float up, float un, double abstol, double reltol) {
  const double r = (double)e / (abstol + reltol * (double)fmaxf(fabsf(up), fabsf(un)));
  return r * r;
}

template <int N, class T>
__global__ void __launch_bounds__(kNormThreads) rk_error_norm_partial_kernel(int64_t count, const CombK k, const T *u_prev,
                                                                             const T *u_new, double abstol, double reltol,
                                                                             double *__restrict__ partial) {
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x) {
    T t[N];
#pragma unroll
    for (int j = 0; j < N; ++j) t[j] = reinterpret_cast<const T *>(k.term[j])[i];   // all loads first
    const T up = u_prev[i], un = u_new[i];
    if constexpr (sizeof(T) == 16) {
      float4 e = f4_zero();
#pragma unroll
      for (int j = 0; j < N; ++j) e = f4_fma(k.coef[j], t[j], e);
      acc += scaled_sq(e.x, up.x, un.x, abstol, reltol);
      acc += scaled_sq(e.y, up.y, un.y, abstol, reltol);
      acc += scaled_sq(e.z, up.z, un.z, abstol, reltol);
      acc += scaled_sq(e.w, up.w, un.w, abstol, reltol);
    } else {
      float e = 0.f;
#pragma unroll
      for (int j = 0; j < N; ++j) e = fmaf(k.coef[j], t[j], e);
      acc += scaled_sq(e, up, un, abstol, reltol);
    }
  }
  const double s = block_sum_256(acc);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void __launch_bounds__(kNormThreads) rk_error_norm_final_kernel(int n_partial, int64_t count, const double *__restrict__ partial,
                                                                           double *__restrict__ out) {
  double acc = 0.0;
  for (int b = threadIdx.x; b < n_partial; b += kNormThreads) acc += partial[b];
  const double s = block_sum_256(acc);
  if (threadIdx.x == 0) *out = sqrt(s / (double)count);
}

int norm_blocks(int64_t count) { return (int)std::min<int64_t>((count + kNormThreads - 1) / kNormThreads, kNormMaxBlocks); }

template <class T>
void launch_rk_error_norm(int n_terms, int64_t count, const CombK &k, const float *u_prev, const float *u_new, double abstol, double reltol,
                          int blocks, double *partial, hipStream_t stream) {
  const T *up = reinterpret_cast<const T *>(u_prev), *un = reinterpret_cast<const T *>(u_new);
  const dim3 grid((unsigned)blocks), block(kNormThreads);
  switch (n_terms) {
    case 1: hipLaunchKernelGGL((rk_error_norm_partial_kernel<1, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
    case 2: hipLaunchKernelGGL((rk_error_norm_partial_kernel<2, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
    case 3: hipLaunchKernelGGL((rk_error_norm_partial_kernel<3, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
    case 4: hipLaunchKernelGGL((rk_error_norm_partial_kernel<4, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
    case 5: hipLaunchKernelGGL((rk_error_norm_partial_kernel<5, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
    case 6: hipLaunchKernelGGL((rk_error_norm_partial_kernel<6, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
    case 7: hipLaunchKernelGGL((rk_error_norm_partial_kernel<7, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
    default: hipLaunchKernelGGL((rk_error_norm_partial_kernel<8, T>), grid, block, 0, stream, count, k, up, un, abstol, reltol, partial); break;
  }
}

}  // namespace
}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_rk_stage_combine(int64_t count, float c_self, const float *base, int32_t n_terms, const float *const *terms,
                               const float *coefs, float *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(count >= 0 && n_terms >= 0 && n_terms <= 8, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_stage_combine: count >= 0 and 0 <= n_terms <= 8 required (got %lld, %d)", (long long)count, n_terms);
  if (count == 0) return NGPDE_OK;
  NGPDE_REQUIRE(out && (n_terms == 0 || (terms && coefs)), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_stage_combine: NULL argument");
  CombK k;
  uintptr_t bits = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(base);
  for (int j = 0; j < 8; ++j) {
    k.term[j] = j < n_terms ? terms[j] : nullptr;
    k.coef[j] = j < n_terms ? coefs[j] : 0.f;
    NGPDE_REQUIRE(j >= n_terms || terms[j], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_stage_combine: term %d is NULL", j);
    bits |= reinterpret_cast<uintptr_t>(k.term[j]);
  }
  if (count % 4 == 0 && (bits & 15) == 0) launch_rk_combine<float4>(n_terms, count / 4, c_self, base, k, out, (hipStream_t)stream);
  else launch_rk_combine<float>(n_terms, count, c_self, base, k, out, (hipStream_t)stream);
  NGPDE_LAUNCH_CHECK("rk_combine_kernel");
  return NGPDE_OK;
}

int32_t ngpde_rk_dense_output(int64_t count, const float *u_prev, int32_t n_stages, const float *const *k, int32_t n_out,
                              const float *coefs, float *const *outs, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(count >= 0 && n_stages >= 1 && n_stages <= 8 && n_out >= 0, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_dense_output: count >= 0, 1 <= n_stages <= 8 and n_out >= 0 required (got %lld, %d, %d)", (long long)count,
                n_stages, n_out);
  if (count == 0 || n_out == 0) return NGPDE_OK;
  NGPDE_REQUIRE(u_prev && k && coefs && outs, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_dense_output: NULL argument");
  uintptr_t kbits = reinterpret_cast<uintptr_t>(u_prev);
  for (int s = 0; s < n_stages; ++s) {
    NGPDE_REQUIRE(k[s], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_dense_output: stage %d is NULL", s);
    kbits |= reinterpret_cast<uintptr_t>(k[s]);
  }
  for (int j = 0; j < n_out; ++j) NGPDE_REQUIRE(outs[j], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_dense_output: output %d is NULL", j);
  for (int j0 = 0; j0 < n_out; j0 += kDenseMax) {
    DenseK d{};
    d.n_out = std::min(kDenseMax, n_out - j0);
    uintptr_t bits = kbits;
    for (int s = 0; s < n_stages; ++s) d.k[s] = k[s];
    for (int j = 0; j < d.n_out; ++j) {
      d.out[j] = outs[j0 + j];
      bits |= reinterpret_cast<uintptr_t>(d.out[j]);
      for (int s = 0; s < n_stages; ++s) d.coef[j][s] = coefs[(size_t)(j0 + j) * n_stages + s];
    }
    if (count % 4 == 0 && (bits & 15) == 0) launch_rk_dense_output<float4>(n_stages, count / 4, u_prev, d, (hipStream_t)stream);
    else launch_rk_dense_output<float>(n_stages, count, u_prev, d, (hipStream_t)stream);
    NGPDE_LAUNCH_CHECK("rk_dense_output_kernel");
  }
  return NGPDE_OK;
}

int32_t ngpde_rk_dense_output_pullback(int64_t count, int32_t n_out, const float *const *douts, int32_t n_stages, const float *coefs,
                                       float *ubar, float *const *kbar, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(count >= 0 && n_stages >= 1 && n_stages <= 8 && n_out >= 1, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_dense_output_pullback: count >= 0, 1 <= n_stages <= 8 and n_out >= 1 required (got %lld, %d, %d)",
                (long long)count, n_stages, n_out);
  if (count == 0) return NGPDE_OK;
  NGPDE_REQUIRE(douts && coefs && kbar, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_dense_output_pullback: NULL argument");
  uintptr_t kbits = reinterpret_cast<uintptr_t>(ubar);
  for (int s = 0; s < n_stages; ++s) {
    NGPDE_REQUIRE(kbar[s], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_dense_output_pullback: stage cotangent %d is NULL", s);
    kbits |= reinterpret_cast<uintptr_t>(kbar[s]);
  }
  for (int j = 0; j < n_out; ++j)
    NGPDE_REQUIRE(douts[j], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_dense_output_pullback: cotangent %d is NULL", j);
  for (int j0 = 0; j0 < n_out; j0 += kDenseMax) {
    DensePullK d{};
    d.n_out = std::min(kDenseMax, n_out - j0);
    d.first = j0 == 0;
    uintptr_t bits = kbits;
    for (int s = 0; s < n_stages; ++s) d.kbar[s] = kbar[s];
    for (int j = 0; j < d.n_out; ++j) {
      d.dout[j] = douts[j0 + j];
      bits |= reinterpret_cast<uintptr_t>(d.dout[j]);
      for (int s = 0; s < n_stages; ++s) d.coef[j][s] = coefs[(size_t)(j0 + j) * n_stages + s];
    }
    if (count % 4 == 0 && (bits & 15) == 0) launch_rk_dense_output_pullback<float4>(n_stages, count / 4, ubar, d, (hipStream_t)stream);
    else launch_rk_dense_output_pullback<float>(n_stages, count, ubar, d, (hipStream_t)stream);
    NGPDE_LAUNCH_CHECK("rk_dense_output_pullback_kernel");
  }
  return NGPDE_OK;
}

size_t ngpde_rk_error_norm_workspace_bytes(int64_t count) {
  return count > 0 ? (size_t)norm_blocks(count) * sizeof(double) : 0;
}

int32_t ngpde_rk_error_norm(int64_t count, int32_t n_terms, const float *const *terms, const float *coefs, const float *u_prev,
                            const float *u_new, double abstol, double reltol, void *workspace, double *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(count > 0 && n_terms >= 1 && n_terms <= 8, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_error_norm: count >= 1 and 1 <= n_terms <= 8 required (got %lld, %d)", (long long)count, n_terms);
  NGPDE_REQUIRE(terms && coefs && u_prev && u_new && workspace && out, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_error_norm: NULL argument");
  NGPDE_REQUIRE(abstol >= 0.0 && reltol >= 0.0 && abstol + reltol > 0.0, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_rk_error_norm: abstol, reltol >= 0, not both 0, required (got %g, %g)", abstol, reltol);
  CombK k;
  uintptr_t bits = reinterpret_cast<uintptr_t>(u_prev) | reinterpret_cast<uintptr_t>(u_new);
  for (int j = 0; j < 8; ++j) {
    k.term[j] = j < n_terms ? terms[j] : nullptr;
    k.coef[j] = j < n_terms ? coefs[j] : 0.f;
    NGPDE_REQUIRE(j >= n_terms || terms[j], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rk_error_norm: term %d is NULL", j);
    bits |= reinterpret_cast<uintptr_t>(k.term[j]);
  }
  const int blocks = norm_blocks(count);
  double *partial = static_cast<double *>(workspace);
  if (count % 4 == 0 && (bits & 15) == 0)
    launch_rk_error_norm<float4>(n_terms, count / 4, k, u_prev, u_new, abstol, reltol, blocks, partial, (hipStream_t)stream);
  else
    launch_rk_error_norm<float>(n_terms, count, k, u_prev, u_new, abstol, reltol, blocks, partial, (hipStream_t)stream);
  NGPDE_LAUNCH_CHECK("rk_error_norm_partial_kernel");
  hipLaunchKernelGGL(rk_error_norm_final_kernel, dim3(1), dim3(kNormThreads), 0, (hipStream_t)stream, blocks, count, partial, out);
  NGPDE_LAUNCH_CHECK("rk_error_norm_final_kernel");
  return NGPDE_OK;
}

int32_t ngpde_accumulate_many(int32_t n_arrays, float *const *acc, const float *const *g, const int64_t *counts, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(n_arrays >= 0, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_accumulate_many: n_arrays < 0");
  if (n_arrays == 0) return NGPDE_OK;
  NGPDE_REQUIRE(acc && g && counts, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_accumulate_many: NULL argument");
  for (int a = 0; a < n_arrays; ++a)      // every array before the first launch: a refused call has written nothing
    NGPDE_REQUIRE(counts[a] >= 0 && (counts[a] == 0 || (acc[a] && g[a])), NGPDE_ERR_INVALID_ARGUMENT,
                  "ngpde_accumulate_many: array %d is NULL or has a negative count", a);
  for (int a0 = 0; a0 < n_arrays; a0 += kManyMax) {
    ManyK k{};
    const int m = std::min(kManyMax, n_arrays - a0);
    int64_t longest = 0;
    for (int a = 0; a < m; ++a) {
      k.acc[a] = acc[a0 + a]; k.g[a] = g[a0 + a]; k.count[a] = counts[a0 + a];
      longest = std::max(longest, counts[a0 + a]);
    }
    if (longest == 0) continue;
    const dim3 grid((unsigned)std::min<int64_t>((longest + 255) / 256, 1024), (unsigned)m);
    hipLaunchKernelGGL(accumulate_many_kernel, grid, dim3(256), 0, (hipStream_t)stream, k);
    NGPDE_LAUNCH_CHECK("accumulate_many_kernel");
  }
  return NGPDE_OK;
}

int32_t ngpde_adam_step(int64_t n, float *x, const float *grad, float *m, float *v, float eta, float beta1, float beta2,
                        float eps, int64_t step, float grad_scale, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(n >= 0 && step >= 1, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_adam_step: n >= 0 and step >= 1 required");
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(x && grad && m && v, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_adam_step: NULL argument");
  const float c1 = 1.0f - powf(beta1, (float)step), c2 = 1.0f - powf(beta2, (float)step);
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, x, grad, m, v, eta, beta1, beta2, eps, c1, c2,
                     grad_scale);
  NGPDE_LAUNCH_CHECK("adam_kernel");
  return NGPDE_OK;
}

int32_t ngpde_rprop_step(int64_t n, float *x, const float *grad, float *grad_prev, float *step_size, float shrink, float grow,
                         float step_min, float step_max, float grad_scale, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(n >= 0, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rprop_step: n < 0");
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(x && grad && grad_prev && step_size, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_rprop_step: NULL argument");
  const int blocks = (int)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(rprop_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n, x, grad, grad_prev, step_size, shrink, grow,
                     step_min, step_max, grad_scale);
  NGPDE_LAUNCH_CHECK("rprop_kernel");
  return NGPDE_OK;
}

}  // extern "C"
