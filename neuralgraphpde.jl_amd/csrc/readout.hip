// readout.hip -- the per-graph readouts the reference re-exports from GraphNeuralNetworks.jl (src/NeuralGraphPDE.jl:5-7: reduce_nodes,
// reduce_edges, softmax_nodes, softmax_edges, broadcast_nodes, broadcast_edges) over a block-diagonal batch.
//
// A readout has the opposite shape of a neighbourhood reduction: 1 to a few hundred segments (graphs) of 10^3 to 10^5 rows each, so
// one wave per segment (mp_kernels.hip, msgpass.hip) would leave the chip empty.  A plan (ngpde_readout) therefore cuts every segment
// into chunks of at most kChunkRows rows, and
//   chunk reduce  one 256-thread workgroup per chunk: lanes (row slot, column) as in msgpass.hip, four loads in flight per lane, the
//                 slots combined by the fixed xor butterfly, the four waves through LDS in wave order; writes partial[chunk][d], or
//                 the finished row when the segment is that one chunk;
//   finish        one wave per (segment, column chunk) folds the segment's partials in chunk order (slots + butterfly again), applies
//                 the mean's 1 / count and writes the identity for empty segments; skipped when every segment is exactly one chunk;
//   item-wise     grid-stride kernels for the pullbacks, the softmax's normalisation and the broadcast.
// The term is a functor: one chunk-reduce body serves sum / mean, max, min, the softmax's (running max, sum of exp) pair and the
// softmax pullback's sum of y dy.  No atomics; the chunking is the plan's alone, so every result is bitwise equal from run to run and
// independent of the grid.  float4 columns where d % 4 == 0 and every array is 16-byte aligned.  No allocation outside create.
#include <algorithm>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "device_scratch.h"
#include "device_utils.h"
#include "row_lanes.h"

struct ngpde_readout {
  int64_t n_items = 0;
  int32_t n_segments = 1;
  int32_t contiguous = 1;         // ids non-decreasing: sorted position = item
  int64_t n_chunks = 0;
  bool need_finish = false;       // some segment has no chunk or more than one
  int32_t *seg_of_item = nullptr;   // [n]
  int32_t *segptr = nullptr;        // [S + 1] sorted positions of each segment
  int32_t *perm = nullptr;          // [n] item at each sorted position (stable by item), or NULL when contiguous
  int32_t *chunk_seg = nullptr, *chunk_begin = nullptr, *chunk_end = nullptr;   // [n_chunks] sorted positions [begin, end)
  int32_t *seg_chunkptr = nullptr;  // [S + 1]
};

namespace ngpde {

namespace {

constexpr int kChunkRows = 256;   // rows per chunk: the starting value, no alternative measured yet ("Per-graph readouts")
constexpr unsigned kMaxGrid = 2048;   // memory-bound grid-stride launches: 256 CUs x 8 workgroups

struct View {
  const int32_t *seg_of_item, *segptr, *perm, *chunk_seg, *chunk_begin, *chunk_end, *seg_chunkptr;
};
inline View view_of(const ngpde_readout *r) {
  return View{r->seg_of_item, r->segptr, r->perm, r->chunk_seg, r->chunk_begin, r->chunk_end, r->seg_chunkptr};
}

// ---- building the plan -----------------------------------------------------------------------------------------------------------

// flags: [0] an id outside its range, [1] ids not non-decreasing, [2] a segment with no chunk or more than one
__global__ void seg_ids_kernel(int64_t n, const int32_t *__restrict__ id, const int32_t *__restrict__ index, int id_base, int n_segments,
                               int32_t *__restrict__ seg, int32_t *__restrict__ iota, int *__restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int v = 0, prev = 0;
    if (id) {
      v = id[index ? index[i] : i] - id_base;
      prev = i > 0 ? id[index ? index[i - 1] : i - 1] - id_base : v;
    }
    if (v < 0 || v >= n_segments) {
      flags[0] = 1;
      v = 0;
    }
    if (prev > v) flags[1] = 1;
    seg[i] = v;
    iota[i] = (int32_t)i;
  }
}

// key: the segment ids in sorted order.  Position i in 0..n starts every segment in (key[i - 1], key[i]]
__global__ void segptr_kernel(int64_t n, int n_segments, const int32_t *__restrict__ key, int32_t *__restrict__ segptr) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
    const int a = i == 0 ? -1 : key[i - 1], b = i == n ? n_segments : key[i];
    for (int s = a + 1; s <= b; ++s) segptr[s] = (int32_t)i;
  }
}

__global__ void seg_chunk_count_kernel(int n_segments, const int32_t *__restrict__ segptr, int32_t *__restrict__ count,
                                       int *__restrict__ flags) {
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s <= n_segments; s += gridDim.x * blockDim.x) {
    const int c = s < n_segments ? (segptr[s + 1] - segptr[s] + kChunkRows - 1) / kChunkRows : 0;
    if (s < n_segments && c != 1) flags[2] = 1;
    count[s] = c;
  }
}

__global__ void chunk_fill_kernel(int64_t n_chunks, int n_segments, const int32_t *__restrict__ segptr,
                                  const int32_t *__restrict__ seg_chunkptr, int32_t *__restrict__ chunk_seg,
                                  int32_t *__restrict__ chunk_begin, int32_t *__restrict__ chunk_end) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_chunks; k += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = n_segments;   // the segment s with seg_chunkptr[s] <= k < seg_chunkptr[s + 1]
    while (hi - lo > 1) {
      const int mid = lo + (hi - lo) / 2;
      if (seg_chunkptr[mid] <= k) lo = mid; else hi = mid;
    }
    const int64_t begin = (int64_t)segptr[lo] + (k - seg_chunkptr[lo]) * kChunkRows;
    chunk_seg[k] = lo;
    chunk_begin[k] = (int32_t)begin;
    const int64_t seg_end = segptr[lo + 1];
    chunk_end[k] = (int32_t)(begin + kChunkRows < seg_end ? begin + kChunkRows : seg_end);
  }
}

int32_t build_plan(ngpde_readout *r, const int32_t *id, const int32_t *index, int id_base, hipStream_t stream) {
  const int64_t n = r->n_items;
  const int S = r->n_segments;
  Scratch sc;
  int32_t st;
  int32_t *iota = nullptr, *key = nullptr, *count = nullptr;
  int *flags = nullptr;
  if ((st = dev_alloc(&r->seg_of_item, (size_t)n)) || (st = dev_alloc(&r->segptr, (size_t)S + 1)) ||
      (st = dev_alloc(&r->seg_chunkptr, (size_t)S + 1)) || (st = sc.get(&iota, (size_t)n)) || (st = sc.get(&count, (size_t)S + 1)) ||
      (st = sc.get(&flags, 3)))
    return st;
  NGPDE_HIP_CHECK(hipMemsetAsync(flags, 0, 3 * sizeof(int), stream));
  hipLaunchKernelGGL(seg_ids_kernel, dim3(std::min(blocks_for(n), kMaxGrid)), dim3(kB), 0, stream, n, id, index, id_base, S,
                     r->seg_of_item, iota, flags);
  NGPDE_LAUNCH_CHECK("seg_ids_kernel");
  int h_flags[3] = {0, 0, 0};
  NGPDE_HIP_CHECK(hipMemcpyAsync(h_flags, flags, 2 * sizeof(int), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  NGPDE_REQUIRE(!h_flags[0], NGPDE_ERR_INVALID_ARGUMENT, "graph_indicator holds an id outside %d:%d", id_base, id_base + S - 1);
  r->contiguous = h_flags[1] ? 0 : 1;
  const int32_t *sorted_key = r->seg_of_item;
  if (!r->contiguous) {   // stable sort of the items by segment: ties keep the item order, so the plan is deterministic
    if ((st = dev_alloc(&r->perm, (size_t)n)) || (st = sc.get(&key, (size_t)n))) return st;
    const unsigned end_bit = bits_for(S);
    const unsigned *key_in = reinterpret_cast<const unsigned *>(r->seg_of_item);   // (ids are checked: non-negative)
    unsigned *key_out = reinterpret_cast<unsigned *>(key);
    auto sort = [&](void *tmp, size_t &bytes) {
      return rocprim::radix_sort_pairs(tmp, bytes, key_in, key_out, iota, r->perm, (size_t)n, 0u, end_bit, stream);
    };
    if ((st = with_temp(sc, sort))) return st;
    sorted_key = key;
  }
  hipLaunchKernelGGL(segptr_kernel, dim3(std::min(blocks_for(n + 1), kMaxGrid)), dim3(kB), 0, stream, n, S, sorted_key, r->segptr);
  NGPDE_LAUNCH_CHECK("segptr_kernel");
  hipLaunchKernelGGL(seg_chunk_count_kernel, dim3(std::min(blocks_for((int64_t)S + 1), kMaxGrid)), dim3(kB), 0, stream, S, r->segptr,
                     count, flags);
  NGPDE_LAUNCH_CHECK("seg_chunk_count_kernel");
  auto scan = [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, count, r->seg_chunkptr, (int32_t)0, (size_t)S + 1, rocprim::plus<int32_t>(), stream);
  };
  if ((st = with_temp(sc, scan))) return st;
  int32_t h_chunks = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_chunks, r->seg_chunkptr + S, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipMemcpyAsync(h_flags + 2, flags + 2, sizeof(int), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  r->n_chunks = h_chunks;
  r->need_finish = h_flags[2] != 0;
  if ((st = dev_alloc(&r->chunk_seg, (size_t)h_chunks)) || (st = dev_alloc(&r->chunk_begin, (size_t)h_chunks)) ||
      (st = dev_alloc(&r->chunk_end, (size_t)h_chunks)))
    return st;
  if (h_chunks) {
    hipLaunchKernelGGL(chunk_fill_kernel, dim3(std::min(blocks_for(h_chunks), kMaxGrid)), dim3(kB), 0, stream, (int64_t)h_chunks, S,
                       r->segptr, r->seg_chunkptr, r->chunk_seg, r->chunk_begin, r->chunk_end);
    NGPDE_LAUNCH_CHECK("chunk_fill_kernel");
  }
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));   // the scratch arrays are freed on return
  return NGPDE_OK;
}

// ---- the terms of the chunk reduce -----------------------------------------------------------------------------------------------
// A term names its accumulator type A and: identity(), term(flat index of (item, column)), combine(a, b), finalize(a, rows of the
// segment), and exchange(a, xor offset) for the butterfly.

__device__ __forceinline__ float vfill(float, float v) { return v; }
__device__ __forceinline__ float4 vfill(float4, float v) { return make_float4(v, v, v, v); }

template <typename T>
struct SumTerm {   // sum; mean when `mean`
  using A = T;
  const T *x;
  int mean;
  __device__ __forceinline__ A identity() const { return vzero(T()); }
  __device__ __forceinline__ A term(size_t k) const { return x[k]; }
  __device__ __forceinline__ A combine(A a, A b) const { return vadd(a, b); }
  __device__ __forceinline__ A exchange(A a, int o) const { return vxor(a, o); }
  __device__ __forceinline__ A finalize(A a, int count) const { return (mean && count > 0) ? vscale(1.0f / (float)count, a) : a; }
};

template <typename T, bool MAX>
struct ExtremumTerm {
  using A = T;
  const T *x;
  __device__ __forceinline__ A identity() const { return vfill(T(), MAX ? -INFINITY : INFINITY); }
  __device__ __forceinline__ A term(size_t k) const { return x[k]; }
  __device__ __forceinline__ A combine(A a, A b) const { return MAX ? vmax(a, b) : vmin(a, b); }
  __device__ __forceinline__ A exchange(A a, int o) const { return vxor(a, o); }
  __device__ __forceinline__ A finalize(A a, int) const { return a; }
};

template <typename T>
struct DotTerm {   // sum of y .* dy (the softmax pullback's per-segment constant)
  using A = T;
  const T *y, *dy;
  __device__ __forceinline__ A identity() const { return vzero(T()); }
  __device__ __forceinline__ A term(size_t k) const { return vmul(y[k], dy[k]); }
  __device__ __forceinline__ A combine(A a, A b) const { return vadd(a, b); }
  __device__ __forceinline__ A exchange(A a, int o) const { return vxor(a, o); }
  __device__ __forceinline__ A finalize(A a, int) const { return a; }
};

// the softmax's statistics in one pass: m = the maximum so far, s = the sum of exp(x - m)
template <typename T>
struct MaxSum {
  T m, s;
};
__device__ __forceinline__ void maxsum_combine(float am, float as, float bm, float bs, float &m, float &s) {
  m = fmaxf(am, bm);
  const float sa = am == m ? as : as * fast_exp(am - m);   // (the side that holds the maximum is not rescaled: -inf - -inf never forms)
  const float sb = bm == m ? bs : bs * fast_exp(bm - m);
  s = sa + sb;
}
__device__ __forceinline__ MaxSum<float> maxsum_combine(MaxSum<float> a, MaxSum<float> b) {
  MaxSum<float> r;
  maxsum_combine(a.m, a.s, b.m, b.s, r.m, r.s);
  return r;
}
__device__ __forceinline__ MaxSum<float4> maxsum_combine(MaxSum<float4> a, MaxSum<float4> b) {
  MaxSum<float4> r;
  maxsum_combine(a.m.x, a.s.x, b.m.x, b.s.x, r.m.x, r.s.x);
  maxsum_combine(a.m.y, a.s.y, b.m.y, b.s.y, r.m.y, r.s.y);
  maxsum_combine(a.m.z, a.s.z, b.m.z, b.s.z, r.m.z, r.s.z);
  maxsum_combine(a.m.w, a.s.w, b.m.w, b.s.w, r.m.w, r.s.w);
  return r;
}

template <typename T>
struct SoftmaxTerm {
  using A = MaxSum<T>;
  const T *x;
  __device__ __forceinline__ A identity() const { return A{vfill(T(), -INFINITY), vzero(T())}; }
  __device__ __forceinline__ A term(size_t k) const { return A{x[k], vfill(T(), 1.0f)}; }
  __device__ __forceinline__ A combine(A a, A b) const { return maxsum_combine(a, b); }
  __device__ __forceinline__ A exchange(A a, int o) const { return A{vxor(a.m, o), vxor(a.s, o)}; }
  __device__ __forceinline__ A finalize(A a, int) const { return a; }
};

// combine over q = start, start + step, ... < end of load(q): four independent terms in flight per lane, folded in a fixed order
template <typename Op, typename L>
__device__ __forceinline__ typename Op::A fold_strided(const Op &op, int64_t start, int64_t end, int step, L load) {
  using A = typename Op::A;
  A acc[4] = {op.identity(), op.identity(), op.identity(), op.identity()};
  for (int64_t q0 = start; q0 < end; q0 += 4 * (int64_t)step) {
    A v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = q0 + (int64_t)u * step;
      v[u] = q < end ? load(q) : op.identity();
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = op.combine(acc[u], v[u]);
  }
  return op.combine(op.combine(acc[0], acc[1]), op.combine(acc[2], acc[3]));
}

// ---- chunk reduce: one workgroup per chunk; w = row width in columns of T -------------------------------------------------------
template <typename Op>
__global__ __launch_bounds__(256) void chunk_reduce_kernel(View p, int w, Op op, typename Op::A *__restrict__ partial,
                                                           typename Op::A *__restrict__ fin) {
  using A = typename Op::A;
  __shared__ A lds[4][64];
  const int k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int seg = p.chunk_seg[k], begin = p.chunk_begin[k], end = p.chunk_end[k];
  const bool whole = p.seg_chunkptr[seg + 1] - p.seg_chunkptr[seg] == 1;   // the segment is this chunk: finished in this launch
  const int dpl = lanes_per_entry(w), slots = 64 / dpl, slot = lane / dpl, cl = lane % dpl;
  for (int c0 = 0; c0 < w; c0 += dpl) {   // (workgroup-uniform trip count: every thread reaches the barriers)
    const int c = min(c0 + cl, w - 1);
    A a = fold_strided(op, (int64_t)begin + wave * slots + slot, end, 4 * slots, [&](int64_t q) {
      const size_t item = p.perm ? (size_t)p.perm[q] : (size_t)q;
      return op.term(item * w + c);
    });
    for (int o = dpl; o < 64; o <<= 1) a = op.combine(a, op.exchange(a, o));
    if (slot == 0) lds[wave][cl] = a;
    __syncthreads();
    if (wave == 0 && slot == 0 && c0 + cl < w) {
      a = op.combine(op.combine(op.combine(lds[0][cl], lds[1][cl]), lds[2][cl]), lds[3][cl]);
      if (whole) fin[(size_t)seg * w + c] = op.finalize(a, end - begin);
      else partial[(size_t)k * w + c] = a;
    }
    __syncthreads();
  }
}

// ---- finish: one wave per (segment, column chunk) folds the segment's partials in chunk order ------------------------------------
template <typename Op>
__global__ __launch_bounds__(256) void finish_kernel(View p, int n_segments, int w, Op op, const typename Op::A *__restrict__ partial,
                                                     typename Op::A *__restrict__ fin) {
  using A = typename Op::A;
  const int lane = threadIdx.x & 63;
  const int dpl = lanes_per_entry(w), slots = 64 / dpl, slot = lane / dpl, cl = lane % dpl;
  const int col_chunks = (w + dpl - 1) / dpl;
  const int64_t job = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (job >= (int64_t)n_segments * col_chunks) return;
  const int seg = (int)(job / col_chunks), c0 = (int)(job % col_chunks) * dpl;
  const int kb = p.seg_chunkptr[seg], ke = p.seg_chunkptr[seg + 1];
  if (ke - kb == 1) return;   // written by the chunk reduce
  const int c = min(c0 + cl, w - 1);
  A a = fold_strided(op, kb + slot, ke, slots, [&](int64_t k) { return partial[(size_t)k * w + c]; });
  for (int o = dpl; o < 64; o <<= 1) a = op.combine(a, op.exchange(a, o));
  if (slot == 0 && c0 + cl < w) fin[(size_t)seg * w + c] = op.finalize(a, p.segptr[seg + 1] - p.segptr[seg]);
}

template <typename Op>
int32_t launch_reduce(const ngpde_readout *r, int w, const Op &op, typename Op::A *partial, typename Op::A *fin, hipStream_t stream) {
  const View p = view_of(r);
  if (r->n_chunks) {
    hipLaunchKernelGGL(chunk_reduce_kernel<Op>, dim3((unsigned)r->n_chunks), dim3(256), 0, stream, p, w, op, partial, fin);
    NGPDE_LAUNCH_CHECK("chunk_reduce_kernel");
  }
  if (r->need_finish) {
    const int dpl = lanes_per_entry(w);
    const int64_t jobs = (int64_t)r->n_segments * ((w + dpl - 1) / dpl);
    hipLaunchKernelGGL(finish_kernel<Op>, dim3((unsigned)((jobs + 3) / 4)), dim3(256), 0, stream, p, r->n_segments, w, op, partial, fin);
    NGPDE_LAUNCH_CHECK("finish_kernel");
  }
  return NGPDE_OK;
}

// ---- item-wise kernels: f(flat index of (item, column), flat index of (segment, column), segment) --------------------------------
template <typename F>
__global__ __launch_bounds__(256) void item_kernel(int64_t n, int w, const int32_t *__restrict__ seg_of_item, F f) {
  const int dpl = lanes_per_entry(w), rows = 256 / dpl, r = threadIdx.x / dpl, cl = threadIdx.x % dpl;
  for (int64_t i = (int64_t)blockIdx.x * rows + r; i < n; i += (int64_t)gridDim.x * rows) {
    const int seg = seg_of_item[i];
    for (int c = cl; c < w; c += dpl) f((size_t)i * w + c, (size_t)seg * w + c, seg);
  }
}

template <typename F>
int32_t launch_items(const ngpde_readout *r, int w, const F &f, hipStream_t stream) {
  if (r->n_items == 0) return NGPDE_OK;
  const int dpl = lanes_per_entry(w);
  const int64_t wgs = (r->n_items + 256 / dpl - 1) / (256 / dpl);
  hipLaunchKernelGGL(item_kernel<F>, dim3((unsigned)std::min<int64_t>(wgs, kMaxGrid)), dim3(256), 0, stream, r->n_items, w,
                     r->seg_of_item, f);
  NGPDE_LAUNCH_CHECK("item_kernel");
  return NGPDE_OK;
}

__device__ __forceinline__ float soft_y(float x, float m, float s) { return fast_exp(x - m) / s; }
__device__ __forceinline__ float4 soft_y(float4 x, float4 m, float4 s) {
  return make_float4(soft_y(x.x, m.x, s.x), soft_y(x.y, m.y, s.y), soft_y(x.z, m.z, s.z), soft_y(x.w, m.w, s.w));
}
__device__ __forceinline__ float vsub(float a, float b) { return a - b; }
__device__ __forceinline__ float4 vsub(float4 a, float4 b) { return make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

template <typename T>
struct ReducePullback {   // dx_i = dout_seg (/ count for mean; where x_i == out_seg for max / min: every tied entry)
  const T *x, *out, *dout;
  T *dx;
  const int32_t *segptr;
  int aggr;
  __device__ __forceinline__ void operator()(size_t k, size_t ks, int seg) const {
    T g = dout[ks];
    if (aggr == NGPDE_AGGR_MEAN) g = vscale(1.0f / (float)(segptr[seg + 1] - segptr[seg]), g);   // (the segment holds this item)
    if (aggr == NGPDE_AGGR_MAX || aggr == NGPDE_AGGR_MIN) g = vsel_eq(x[k], out[ks], g);
    dx[k] = g;
  }
};
template <typename T>
struct SoftmaxApply {
  const T *x;
  const MaxSum<T> *stat;
  T *y;
  __device__ __forceinline__ void operator()(size_t k, size_t ks, int) const {
    const MaxSum<T> st = stat[ks];
    y[k] = soft_y(x[k], st.m, st.s);
  }
};
template <typename T>
struct SoftmaxPullback {
  const T *y, *dy, *cs;
  T *dx;
  __device__ __forceinline__ void operator()(size_t k, size_t ks, int) const { dx[k] = vmul(y[k], vsub(dy[k], cs[ks])); }
};
template <typename T>
struct Broadcast {
  const T *u;
  T *out;
  __device__ __forceinline__ void operator()(size_t k, size_t ks, int) const { out[k] = u[ks]; }
};

// floats of the largest workspace an entry lays out: softmax forward's [S][d] statistics and [n_chunks][d] partials, both pairs
size_t workspace_floats(const ngpde_readout *r, int64_t d) { return (size_t)(2 * ((int64_t)r->n_segments + r->n_chunks) * d); }

// the common head of every entry; aggr NULL: the entry takes none
int32_t check_entry(const char *fn, const ngpde_readout *r, int32_t d, const int32_t *aggr, bool takes_workspace, const void *workspace,
                    size_t bytes) {
  NGPDE_REQUIRE(d >= 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: negative width %d", fn, d);
  NGPDE_REQUIRE(!aggr || *aggr == NGPDE_AGGR_SUM || *aggr == NGPDE_AGGR_MEAN || *aggr == NGPDE_AGGR_MAX || *aggr == NGPDE_AGGR_MIN,
                NGPDE_ERR_INVALID_ARGUMENT, "%s: aggregation %d not supported (the readouts take +, mean, max and min)", fn, *aggr);
  NGPDE_REQUIRE(r != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: readout is NULL", fn);
  if (takes_workspace && d > 0) {
    const size_t need = workspace_floats(r, d) * sizeof(float);
    if (need > 0)   // (a width the plan needs nothing for may come with no workspace)
      if (int32_t st = check_workspace(fn, workspace, bytes, need, 1)) return st;
  }
  return NGPDE_OK;
}

template <typename T>
int32_t reduce_fwd(const ngpde_readout *r, int w, int aggr, const float *x, float *out, void *ws, hipStream_t stream) {
  const T *X = reinterpret_cast<const T *>(x);
  T *O = reinterpret_cast<T *>(out), *P = reinterpret_cast<T *>(ws);
  switch (aggr) {
    case NGPDE_AGGR_MAX: return launch_reduce(r, w, ExtremumTerm<T, true>{X}, P, O, stream);
    case NGPDE_AGGR_MIN: return launch_reduce(r, w, ExtremumTerm<T, false>{X}, P, O, stream);
    default: return launch_reduce(r, w, SumTerm<T>{X, aggr == NGPDE_AGGR_MEAN}, P, O, stream);
  }
}

template <typename T>
int32_t softmax_fwd(const ngpde_readout *r, int w, const float *x, float *y, void *ws, hipStream_t stream) {
  MaxSum<T> *stat = reinterpret_cast<MaxSum<T> *>(ws), *partial = stat + (size_t)r->n_segments * w;
  if (int32_t st = launch_reduce(r, w, SoftmaxTerm<T>{reinterpret_cast<const T *>(x)}, partial, stat, stream)) return st;
  return launch_items(r, w, SoftmaxApply<T>{reinterpret_cast<const T *>(x), stat, reinterpret_cast<T *>(y)}, stream);
}

template <typename T>
int32_t softmax_bwd(const ngpde_readout *r, int w, const float *y, const float *dy, float *dx, void *ws, hipStream_t stream) {
  const T *Y = reinterpret_cast<const T *>(y), *DY = reinterpret_cast<const T *>(dy);
  T *cs = reinterpret_cast<T *>(ws), *partial = cs + (size_t)r->n_segments * w;
  if (int32_t st = launch_reduce(r, w, DotTerm<T>{Y, DY}, partial, cs, stream)) return st;
  return launch_items(r, w, SoftmaxPullback<T>{Y, DY, cs, reinterpret_cast<T *>(dx)}, stream);
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_readout_create(int64_t n_items, const int32_t *id, const int32_t *index, int32_t id_base, int32_t n_segments,
                             ngpde_stream_t stream, ngpde_readout_t **out) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_create: out is NULL");
  *out = nullptr;
  NGPDE_REQUIRE(n_items >= 0 && n_items <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "number of items %lld outside 0:2^31-1",
                (long long)n_items);
  NGPDE_REQUIRE(n_segments >= 1, NGPDE_ERR_INVALID_ARGUMENT, "n_segments must be >= 1");
  NGPDE_REQUIRE(id != nullptr || n_segments == 1, NGPDE_ERR_INVALID_ARGUMENT, "n_segments > 1 needs a graph_indicator");
  ngpde_readout *r = new ngpde_readout();
  r->n_items = n_items;
  r->n_segments = n_segments;
  if (int32_t st = build_plan(r, id, id ? index : nullptr, id_base, (hipStream_t)stream)) {
    ngpde_readout_destroy(r);
    return st;
  }
  *out = r;
  return NGPDE_OK;
}

int32_t ngpde_readout_destroy(ngpde_readout_t *r) {
  NGPDE_RANGE();
  if (!r) return NGPDE_OK;
  for (int32_t *p : {r->seg_of_item, r->segptr, r->perm, r->chunk_seg, r->chunk_begin, r->chunk_end, r->seg_chunkptr})
    if (p) (void)hipFree(p);
  delete r;
  return NGPDE_OK;
}

int32_t ngpde_readout_info(const ngpde_readout_t *r, int64_t *n_items, int32_t *n_segments, int32_t *contiguous, int64_t *n_chunks,
                           int32_t *chunk_rows) {
  NGPDE_REQUIRE(r != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_info: readout is NULL");
  if (n_items) *n_items = r->n_items;
  if (n_segments) *n_segments = r->n_segments;
  if (contiguous) *contiguous = r->contiguous;
  if (n_chunks) *n_chunks = r->n_chunks;
  if (chunk_rows) *chunk_rows = kChunkRows;
  return NGPDE_OK;
}

size_t ngpde_readout_workspace_bytes(const ngpde_readout_t *r, int32_t d) {
  if (!r || d <= 0) return 0;
  return workspace_floats(r, d) * sizeof(float);
}

int32_t ngpde_readout_reduce_forward(const ngpde_readout_t *r, int32_t d, int32_t aggr, const float *x, float *out, void *workspace,
                                     size_t workspace_bytes, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_entry("ngpde_readout_reduce_forward", r, d, &aggr, true, workspace, workspace_bytes)) return st;
  if (d == 0) return NGPDE_OK;
  NGPDE_REQUIRE(out && (x || r->n_items == 0), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_reduce_forward: NULL argument");
  if (d % 4 == 0 && al16(x) && al16(out) && al16(workspace)) return reduce_fwd<float4>(r, d / 4, aggr, x, out, workspace, (hipStream_t)stream);
  return reduce_fwd<float>(r, d, aggr, x, out, workspace, (hipStream_t)stream);
}

int32_t ngpde_readout_reduce_backward(const ngpde_readout_t *r, int32_t d, int32_t aggr, const float *x, const float *out,
                                      const float *dout, float *dx, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_entry("ngpde_readout_reduce_backward", r, d, &aggr, false, nullptr, 0)) return st;
  if (d == 0 || r->n_items == 0) return NGPDE_OK;
  const bool ext = aggr == NGPDE_AGGR_MAX || aggr == NGPDE_AGGR_MIN;
  NGPDE_REQUIRE(dout && dx && (!ext || (x && out)), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_reduce_backward: NULL argument");
  if (d % 4 == 0 && al16(x) && al16(out) && al16(dout) && al16(dx))
    return launch_items(r, d / 4, ReducePullback<float4>{reinterpret_cast<const float4 *>(x), reinterpret_cast<const float4 *>(out),
                                                         reinterpret_cast<const float4 *>(dout), reinterpret_cast<float4 *>(dx), r->segptr, aggr},
                        (hipStream_t)stream);
  return launch_items(r, d, ReducePullback<float>{x, out, dout, dx, r->segptr, aggr}, (hipStream_t)stream);
}

int32_t ngpde_readout_softmax_forward(const ngpde_readout_t *r, int32_t d, const float *x, float *y, void *workspace,
                                      size_t workspace_bytes, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_entry("ngpde_readout_softmax_forward", r, d, nullptr, true, workspace, workspace_bytes)) return st;
  if (d == 0 || r->n_items == 0) return NGPDE_OK;
  NGPDE_REQUIRE(x && y, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_softmax_forward: NULL argument");
  if (d % 4 == 0 && al16(x) && al16(y) && al16(workspace)) return softmax_fwd<float4>(r, d / 4, x, y, workspace, (hipStream_t)stream);
  return softmax_fwd<float>(r, d, x, y, workspace, (hipStream_t)stream);
}

int32_t ngpde_readout_softmax_backward(const ngpde_readout_t *r, int32_t d, const float *y, const float *dy, float *dx, void *workspace,
                                       size_t workspace_bytes, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_entry("ngpde_readout_softmax_backward", r, d, nullptr, true, workspace, workspace_bytes)) return st;
  if (d == 0 || r->n_items == 0) return NGPDE_OK;
  NGPDE_REQUIRE(y && dy && dx, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_softmax_backward: NULL argument");
  if (d % 4 == 0 && al16(y) && al16(dy) && al16(dx) && al16(workspace))
    return softmax_bwd<float4>(r, d / 4, y, dy, dx, workspace, (hipStream_t)stream);
  return softmax_bwd<float>(r, d, y, dy, dx, workspace, (hipStream_t)stream);
}

int32_t ngpde_readout_broadcast_forward(const ngpde_readout_t *r, int32_t d, const float *u, float *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_entry("ngpde_readout_broadcast_forward", r, d, nullptr, false, nullptr, 0)) return st;
  if (d == 0 || r->n_items == 0) return NGPDE_OK;
  NGPDE_REQUIRE(u && out, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_broadcast_forward: NULL argument");
  if (d % 4 == 0 && al16(u) && al16(out))
    return launch_items(r, d / 4, Broadcast<float4>{reinterpret_cast<const float4 *>(u), reinterpret_cast<float4 *>(out)}, (hipStream_t)stream);
  return launch_items(r, d, Broadcast<float>{u, out}, (hipStream_t)stream);
}

int32_t ngpde_readout_broadcast_backward(const ngpde_readout_t *r, int32_t d, const float *dout, float *du, void *workspace,
                                         size_t workspace_bytes, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_entry("ngpde_readout_broadcast_backward", r, d, nullptr, true, workspace, workspace_bytes)) return st;
  if (d == 0) return NGPDE_OK;
  NGPDE_REQUIRE(du && (dout || r->n_items == 0), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_readout_broadcast_backward: NULL argument");
  if (d % 4 == 0 && al16(dout) && al16(du) && al16(workspace)) return reduce_fwd<float4>(r, d / 4, NGPDE_AGGR_SUM, dout, du, workspace, (hipStream_t)stream);
  return reduce_fwd<float>(r, d, NGPDE_AGGR_SUM, dout, du, workspace, (hipStream_t)stream);
}

}  // extern "C"
