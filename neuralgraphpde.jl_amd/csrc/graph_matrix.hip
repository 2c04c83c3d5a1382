// graph_matrix.hip -- the graph as a sparse matrix (include/ngpde.h, "graph matrices"): the assembly of the adjacency matrix, the
// Laplacian and the normalised (optionally scaled) Laplacian from a COO list that lives in HBM, a symmetry check, the largest
// eigenvalue of such a matrix by a device-resident Lanczos iteration over all graphs of a batch at once, and the sparse x sparse
// product behind khop_adj.  A matrix here is coalesced COO sorted by (row, column) with a row pointer: rows / cols / vals / row_ptr.
//
// Order guarantees, all by construction (no float atomics anywhere; the flag words use integer atomics, which commute):
//   assembly     the copies (E edges, then the N diagonal positions where the kind stores them) are sorted stably by the 64-bit key
//                row * n + col (rocPRIM radix sort): entries ascend by (row, col), the members of an entry ascend by copy number, i.e.
//                by COO position with the diagonal copy last; one lane adds an entry's weights in that order, one lane adds a row's
//                entries front to back
//   product      the expanded list is written row by row in ascending middle index and sorted stably by row * n + col: one lane adds
//                an entry's terms in ascending middle index
//   Lanczos      every inner product is per graph: a 256-thread workgroup per chunk of kDotChunk nodes of ONE graph (lane-strided sums,
//                the fixed xor butterfly, the four waves in wave order), then one lane per (graph, vector) folds the graph's partials in
//                chunk order.  The chunking depends on the graphs' sizes alone, never on the grid.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "coo_compact.h"
#include "philox.h"

namespace ngpde {

namespace {

// device flag words of one call
enum { fBad = 0, fCount = 1, fZeroRow = 2, fOrder = 3, fCsr = 4 };

constexpr int kDotChunk = 1024;     // nodes per inner-product chunk: four per lane of the 256-thread workgroup
constexpr int kSpmvLanes = 8;       // lanes per matrix row in the sparse product with a vector
constexpr int kCheckEvery = 8;      // Lanczos steps between two read-backs of the tridiagonal matrix
constexpr int kMaxIter = 4096;      // grid.y of the multi-vector inner product

// the stable sort of m 64-bit keys below 2^end_bit with their positions as the payload
int32_t sort_positions(int64_t m, unsigned end_bit, unsigned long long *key, unsigned long long *key_sorted, int32_t *iota, int32_t *perm,
                       Scratch &sc, hipStream_t stream) {
  return with_temp(sc, [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, key, key_sorted, iota, perm, (size_t)m, 0u, end_bit, stream);
  });
}

// ---- assembly -----------------------------------------------------------------------------------------------------------------
// copy c < E is edge c (its ends swapped for dir = in), copy c >= E the diagonal position of node c - E.  An end outside the node
// range raises fBad and the copy takes key 0.
__global__ void matrix_keys_kernel(int64_t m, int64_t n_edges, int64_t n, int base, int dir_in, const int32_t *__restrict__ s,
                                   const int32_t *__restrict__ t, unsigned long long *__restrict__ key, int32_t *__restrict__ iota,
                                   int32_t *__restrict__ flags) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= m) return;
  int64_t a, b;
  if (c < n_edges) {
    a = (int64_t)(dir_in ? t[c] : s[c]) - base;
    b = (int64_t)(dir_in ? s[c] : t[c]) - base;
    if (a < 0 || a >= n || b < 0 || b >= n) {
      atomicOr(&flags[fBad], 1);
      a = b = 0;
    }
  } else {
    a = b = c - n_edges;
  }
  key[c] = (unsigned long long)a * (unsigned long long)n + (unsigned long long)b;
  iota[c] = (int32_t)c;
}

__global__ void heads_kernel(int64_t m, const unsigned long long *__restrict__ key, int32_t *__restrict__ head) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < m) head[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}

// incl = the inclusive scan of the heads: the sorted copy p lies in entry incl[p] - 1.  member / group_of are nullable.
__global__ void entries_kernel(int64_t m, int64_t n, const unsigned long long *__restrict__ key, const int32_t *__restrict__ copy,
                               const int32_t *__restrict__ head, const int32_t *__restrict__ incl, int32_t *__restrict__ rows,
                               int32_t *__restrict__ cols, int32_t *__restrict__ group_ptr, int32_t *__restrict__ member,
                               int32_t *__restrict__ group_of, int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int32_t g = incl[p] - 1;
  const int32_t c = copy[p];
  if (member) member[p] = c;
  if (group_of) group_of[c] = g;
  if (head[p]) {
    const unsigned long long k = key[p];
    rows[g] = (int32_t)(k / (unsigned long long)n);
    cols[g] = (int32_t)(k % (unsigned long long)n);
    group_ptr[g] = (int32_t)p;
  }
  if (p == m - 1) {
    group_ptr[g + 1] = (int32_t)m;
    flags[fCount] = g + 1;
  }
}

// a lane per entry: the weights of its edge copies in copy order, then the added self loop's 1
__global__ void entry_values_kernel(int64_t m, int64_t n_edges, int add_loops, const int32_t *__restrict__ group_ptr,
                                    const int32_t *__restrict__ member, const float *__restrict__ w, const int32_t *__restrict__ flags,
                                    float *__restrict__ a, float *__restrict__ sym_tol) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m || g >= flags[fCount]) return;
  float acc = 0.f, asum = 0.f;
  int cnt = 0;
  for (int32_t p = group_ptr[g]; p < group_ptr[g + 1]; ++p) {
    const int32_t c = member[p];
    if (c < n_edges) {
      const float v = w ? w[c] : 1.0f;
      acc += v;
      asum += fabsf(v);
      ++cnt;
    } else if (add_loops) {
      acc += 1.0f;
    }
  }
  a[g] = acc;
  if (sym_tol) sym_tol[g] = cnt > 1 ? (float)(cnt - 1) * 1.1920929e-07f * asum : 0.f;
}

__global__ void row_ptr_kernel(int64_t n, const int32_t *__restrict__ rows, const int32_t *__restrict__ flags, int32_t *__restrict__ row_ptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  row_ptr[i] = (int32_t)lower_bound_dev(rows, (int64_t)flags[fCount], (int32_t)i);
}

// a lane per row: its entries front to back.  kind NORM: a row sum that is not positive raises fZeroRow (the smallest such node)
__global__ void row_sums_kernel(int64_t n, int kind, const int32_t *__restrict__ row_ptr, const float *__restrict__ a,
                                float *__restrict__ deg, int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float d = 0.f;
  for (int32_t p = row_ptr[i]; p < row_ptr[i + 1]; ++p) d += a[p];
  deg[i] = d;
  if (kind == NGPDE_MATRIX_NORM_LAPLACIAN && !(d > 0.f)) atomicMax(&flags[fZeroRow], (int32_t)(n - i));
}

__global__ void matrix_values_kernel(int64_t m, int kind, int32_t n_graphs, const int32_t *__restrict__ graph_of,
                                     const float *__restrict__ scale, const int32_t *__restrict__ rows, const int32_t *__restrict__ cols,
                                     const float *__restrict__ a, const float *__restrict__ deg, float *__restrict__ vals,
                                     int32_t *__restrict__ flags) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m || g >= flags[fCount]) return;
  const int32_t i = rows[g], j = cols[g];
  const float av = a[g], eye = i == j ? 1.0f : 0.f;
  if (kind == NGPDE_MATRIX_ADJ) {
    vals[g] = av;
  } else if (kind == NGPDE_MATRIX_LAPLACIAN) {
    vals[g] = i == j ? deg[i] - av : -av;
  } else {
    const float di = deg[i], dj = deg[j];
    if (!(di > 0.f) || !(dj > 0.f)) return;   // (fZeroRow is up: nothing is written through such a row sum)
    const float ci = 1.0f / sqrtf(di), cj = 1.0f / sqrtf(dj);
    float l = eye - (ci * av) * cj;
    if (scale) {
      const int32_t gr = graph_of ? graph_of[i] : 0;
      if (gr < 0 || gr >= n_graphs) {
        atomicOr(&flags[fOrder], 1);
        return;
      }
      l = (2.0f / scale[gr]) * l - eye;
    }
    vals[g] = l;
  }
}

// ---- symmetry -----------------------------------------------------------------------------------------------------------------
// a lane per off-diagonal entry (i, j): (j, i) is looked up in row j by bisection.  first = the smallest i * n + j that fails.
__global__ void symmetry_kernel(int64_t n, int64_t nnz, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ rows,
                                const int32_t *__restrict__ cols, const float *__restrict__ vals, const float *__restrict__ tol,
                                unsigned long long *__restrict__ first, int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= nnz) return;
  const int64_t i = rows[p], j = cols[p];
  if (i < 0 || i >= n || j < 0 || j >= n) {
    atomicOr(&flags[fCsr], 1);
    return;
  }
  if (i == j) return;
  const int64_t b = row_ptr[j], e = row_ptr[j + 1];
  if (b < 0 || e > nnz || b > e) {
    atomicOr(&flags[fCsr], 1);
    return;
  }
  const int64_t q = b + lower_bound_dev(cols + b, e - b, (int32_t)i);
  bool ok = q < e && cols[q] == (int32_t)i;
  if (ok) {
    const float bound = tol ? tol[p] + tol[q] : 0.f;
    ok = fabsf(vals[p] - vals[q]) <= bound;
  }
  if (!ok) atomicMin(first, (unsigned long long)i * (unsigned long long)n + (unsigned long long)j);
}

// ---- sparse x sparse ----------------------------------------------------------------------------------------------------------
// cnt[q] = the length of row p_cols[q] of A: what entry q of P expands to
__global__ void expand_count_kernel(int64_t nnz_p, int64_t n, int64_t nnz_a, const int32_t *__restrict__ p_cols,
                                    const int32_t *__restrict__ a_row_ptr, long long *__restrict__ cnt, int32_t *__restrict__ flags) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= nnz_p) return;
  const int64_t j = p_cols[q];
  long long c = 0;
  if (j < 0 || j >= n) {
    atomicOr(&flags[fBad], 1);
  } else {
    const int64_t b = a_row_ptr[j], e = a_row_ptr[j + 1];
    if (b < 0 || e > nnz_a || b > e) atomicOr(&flags[fCsr], 1);
    else c = e - b;
  }
  cnt[q] = c;
}

// off = the exclusive scan of cnt, off[nnz_p] = the total.  A lane per expanded term x: its entry q of P by bisection, so a hub row
// is spread over as many lanes as it has terms.  The offsets are the caller's (ngpde_csr_spgemm_count wrote them): a term whose place
// in its row of A does not exist raises fCsr and is not read.
__global__ void expand_kernel(int64_t total, int64_t nnz_p, int64_t n, int64_t nnz_a, const long long *__restrict__ off, const int32_t *__restrict__ p_rows,
                              const int32_t *__restrict__ p_cols, const float *__restrict__ p_vals, const int32_t *__restrict__ a_row_ptr,
                              const int32_t *__restrict__ a_cols, const float *__restrict__ a_vals, unsigned long long *__restrict__ key,
                              int32_t *__restrict__ iota, float *__restrict__ prod, int32_t *__restrict__ flags) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= total) return;
  if (x == 0 && off[nnz_p] != total) atomicOr(&flags[fCsr], 1);
  int64_t lo = 0, hi = nnz_p;   // the last q with off[q] <= x
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  const int64_t q = lo, r = x - off[q], j = p_cols[q];
  int64_t row = p_rows[q], c = 0, pa = -1;
  if (j >= 0 && j < n) {
    const int64_t b = a_row_ptr[j], e = a_row_ptr[j + 1];
    if (b >= 0 && e <= nnz_a && r >= 0 && b + r < e) pa = b + r;
  }
  if (pa < 0) {
    atomicOr(&flags[fCsr], 1);
    row = 0;
  } else {
    c = a_cols[pa];
    if (c < 0 || c >= n || row < 0 || row >= n) {
      atomicOr(&flags[fBad], 1);
      c = row = 0;
    }
  }
  key[x] = (unsigned long long)row * (unsigned long long)n + (unsigned long long)c;
  iota[x] = (int32_t)x;
  prod[x] = pa < 0 ? 0.f : p_vals[q] * a_vals[pa];
}

// a lane per entry of the product: its terms in sorted order, i.e. ascending middle index
__global__ void product_values_kernel(int64_t m, const int32_t *__restrict__ group_ptr, const int32_t *__restrict__ perm,
                                      const float *__restrict__ prod, const int32_t *__restrict__ flags, float *__restrict__ vals) {
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= m || g >= flags[fCount]) return;
  const int32_t begin = group_ptr[g], end = group_ptr[g + 1];
  float acc = prod[perm[begin]];
  for (int32_t p = begin + 1; p < end; ++p) acc += prod[perm[p]];
  vals[g] = acc;
}

int32_t expand_offsets(int64_t n, int64_t nnz_p, const int32_t *p_cols, const int32_t *a_row_ptr, int64_t nnz_a, long long **off,
                       int32_t *flags, Scratch &sc, hipStream_t stream) {   // *off: the caller's buffer, or NULL: a temporary
  long long *cnt = nullptr;
  int32_t st;
  if ((st = sc.get(&cnt, (size_t)nnz_p + 1)) || (!*off && (st = sc.get(off, (size_t)nnz_p + 1)))) return st;
  NGPDE_HIP_CHECK(hipMemsetAsync(cnt + nnz_p, 0, sizeof(long long), stream));
  hipLaunchKernelGGL(expand_count_kernel, dim3(blocks_for(nnz_p)), dim3(kB), 0, stream, nnz_p, n, nnz_a, p_cols, a_row_ptr, cnt, flags);
  NGPDE_LAUNCH_CHECK("expand_count_kernel");
  return with_temp(sc, [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, cnt, *off, 0ll, (size_t)nnz_p + 1, rocprim::plus<long long>(), stream);
  });
}

int32_t check_product(const char *fn, int64_t n, int64_t nnz_p, int64_t nnz_a, const int32_t *p_cols, const int32_t *a_row_ptr) {
  NGPDE_REQUIRE(n >= 0 && nnz_p >= 0 && nnz_a >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n %lld, nnz_p %lld, nnz_a %lld)", fn,
                (long long)n, (long long)nnz_p, (long long)nnz_a);
  NGPDE_REQUIRE(n <= 0x7fffffffLL && nnz_p <= 0x7fffffffLL && nnz_a <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: a size above 2^31 - 1 (n %lld, nnz_p %lld, nnz_a %lld)", fn, (long long)n, (long long)nnz_p, (long long)nnz_a);
  NGPDE_REQUIRE(nnz_p == 0 || (p_cols && a_row_ptr), NGPDE_ERR_INVALID_ARGUMENT, "%s: p_cols / a_row_ptr is NULL", fn);
  NGPDE_REQUIRE(nnz_p == 0 || n > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %lld entries in a matrix without rows", fn,
                (long long)nnz_p);
  return NGPDE_OK;
}

// ---- Lanczos ------------------------------------------------------------------------------------------------------------------
// stop: int32[2][n_graphs] -- row 0 is set on the device (step limit, exhausted Krylov space), row 1 by the host (converged)
__device__ __forceinline__ bool stopped(const int32_t *__restrict__ stop, int n_graphs, int g) { return (stop[g] | stop[n_graphs + g]) != 0; }

__global__ void csr_check_kernel(int64_t n, int64_t nnz, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ cols,
                                 int32_t n_graphs, const int32_t *__restrict__ graph_of, int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < nnz && (cols[p] < 0 || cols[p] >= n)) atomicOr(&flags[fCsr], 1);
  if (p < n) {
    if (row_ptr[p] > row_ptr[p + 1] || row_ptr[p] < 0 || row_ptr[p + 1] > nnz) atomicOr(&flags[fCsr], 1);
    if (graph_of) {
      if (graph_of[p] < 0 || graph_of[p] >= n_graphs) atomicOr(&flags[fBad], 1);
      if (p > 0 && graph_of[p] < graph_of[p - 1]) atomicOr(&flags[fOrder], 1);
    }
  }
  if (p == 0 && (row_ptr[0] != 0 || row_ptr[n] != nnz)) atomicOr(&flags[fCsr], 1);
}

__global__ void graph_ptr_kernel(int64_t n, int32_t n_graphs, const int32_t *__restrict__ graph_of, int32_t *__restrict__ gptr) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n_graphs) return;
  gptr[g] = graph_of ? (int32_t)lower_bound_dev(graph_of, n, (int32_t)g) : (g == 0 ? 0 : (int32_t)n);
}

struct LanczosView {
  int64_t n;
  int32_t n_graphs, ld, n_chunks;
  const int32_t *graph_of, *gptr, *cptr, *chunk_graph, *chunk_begin, *chunk_end;
  int32_t *stop, *steps;
  float *V, *w, *y, *partial, *h, *alpha, *beta, *coef, *anorm, *theta;
};

// the start vector: uniform in [0.5, 1.5) from the node's position inside its graph
__global__ void start_kernel(LanczosView L, unsigned long long seed) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  const int g = L.graph_of ? L.graph_of[i] : 0;
  const unsigned long long pos = (unsigned long long)(i - L.gptr[g]);
  const unsigned long long r = philox_draw(seed, kStreamLanczos, (uint32_t)pos, (uint32_t)(pos >> 32));
  L.w[i] = 0.5f + (float)(r >> 41) * 1.1920929e-07f;   // (23 bits: every value is a float of [0.5, 1.5) exactly)
}

// y = M x over the rows of the graphs still running: kSpmvLanes lanes per row, entries lane-strided, a fixed xor butterfly
__global__ __launch_bounds__(256) void csr_spmv_kernel(LanczosView L, int all, const int32_t *__restrict__ row_ptr,
                                                       const int32_t *__restrict__ cols, const float *__restrict__ vals,
                                                       const float *__restrict__ x, float *__restrict__ y) {
  const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = gid / kSpmvLanes;
  const int lane = (int)(gid % kSpmvLanes);
  bool live = row < L.n;
  if (live && !all) live = !stopped(L.stop, L.n_graphs, L.graph_of ? L.graph_of[row] : 0);
  float acc = 0.f;
  if (live)
    for (int32_t p = row_ptr[row] + lane; p < row_ptr[row + 1]; p += kSpmvLanes) acc += vals[p] * x[cols[p]];
#pragma unroll
  for (int o = kSpmvLanes / 2; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (live && lane == 0) y[row] = acc;
}

// partial[k][c] = sum over chunk c of a_k[i] * b[i]; grid (n_chunks, vectors)
__global__ __launch_bounds__(256) void chunk_dot_kernel(LanczosView L, int all, const float *__restrict__ a, const float *__restrict__ b) {
  __shared__ float sh[4];
  const int c = blockIdx.x, k = blockIdx.y;
  if (!all && stopped(L.stop, L.n_graphs, L.chunk_graph[c])) return;   // (uniform over the workgroup)
  const float *__restrict__ ak = a + (size_t)k * (size_t)L.n;
  float acc = 0.f;
  for (int32_t i = L.chunk_begin[c] + (int32_t)threadIdx.x; i < L.chunk_end[c]; i += 256) acc += ak[i] * b[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) L.partial[(size_t)k * L.n_chunks + c] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ float fold_partials(const LanczosView &L, int g, int k) {
  float s = 0.f;
  for (int32_t c = L.cptr[g]; c < L.cptr[g + 1]; ++c) s += L.partial[(size_t)k * L.n_chunks + c];
  return s;
}

// h[g][k] = the graph's partials in chunk order; alpha[g][j] takes (pass 0) or adds (pass 1) h[g][j]
__global__ void fold_dots_kernel(LanczosView L, int all, int n_vec, int j, int pass) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= L.n_graphs * n_vec) return;
  const int g = idx / n_vec, k = idx - g * n_vec;
  if (!all && stopped(L.stop, L.n_graphs, g)) return;
  const float s = fold_partials(L, g, k);
  L.h[(size_t)g * L.ld + k] = s;
  if (j >= 0 && k == j) L.alpha[(size_t)g * L.ld + j] = pass ? L.alpha[(size_t)g * L.ld + j] + s : s;
}

// w -= sum_k h[g][k] v_k, k ascending (one classical Gram-Schmidt pass)
__global__ void orthogonalise_kernel(LanczosView L, int n_vec) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  const int g = L.graph_of ? L.graph_of[i] : 0;
  if (stopped(L.stop, L.n_graphs, g)) return;
  float x = L.w[i];
  for (int k = 0; k < n_vec; ++k) x -= L.h[(size_t)g * L.ld + k] * L.V[(size_t)k * L.n + i];
  L.w[i] = x;
}

// per graph after step j: beta_j = |w|, the step count, and the two stops the device can decide
__global__ void step_kernel(LanczosView L, int j, int max_iter) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= L.n_graphs || stopped(L.stop, L.n_graphs, g)) return;
  const int size = L.gptr[g + 1] - L.gptr[g];
  if (size == 0) {   // a graph without nodes takes no step: 0 steps, lambda 0
    L.stop[g] = 1;
    return;
  }
  const float beta = sqrtf(fold_partials(L, g, 0));
  const size_t at = (size_t)g * L.ld + j;
  L.beta[at] = beta;
  L.steps[g] = j + 1;
  const float an = fmaxf(L.anorm[g], fabsf(L.alpha[at]) + beta + (j > 0 ? L.beta[at - 1] : 0.f));
  L.anorm[g] = an;
  if (j + 1 >= (size < max_iter ? size : max_iter) || !(beta > 8.0f * FLT_EPSILON * an)) L.stop[g] = 1;
}

// out[i] = in[i] / den[g] (root: / sqrt(den[g])) over the graphs still running (all: every graph)
__global__ void scale_kernel(LanczosView L, int all, const float *__restrict__ in, const float *__restrict__ den, int den_at, int root,
                             float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  const int g = L.graph_of ? L.graph_of[i] : 0;
  if (!all && stopped(L.stop, L.n_graphs, g)) return;
  const float d = den[(size_t)g * L.ld + den_at];
  out[i] = in[i] / (root ? sqrtf(d) : d);
}

// y = sum_k coef[g][k] v_k over the steps the graph took
__global__ void ritz_kernel(LanczosView L) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  const int g = L.graph_of ? L.graph_of[i] : 0;
  float x = 0.f;
  for (int k = 0; k < L.steps[g]; ++k) x += L.coef[(size_t)g * L.ld + k] * L.V[(size_t)k * L.n + i];
  L.w[i] = x;
}

// w = w - theta[g] y  (w holds M y)
__global__ void residual_kernel(LanczosView L) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= L.n) return;
  L.w[i] = L.w[i] - L.theta[L.graph_of ? L.graph_of[i] : 0] * L.y[i];
}

__global__ void results_kernel(LanczosView L, float *__restrict__ lambda, float *__restrict__ residual, int32_t *__restrict__ iterations) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= L.n_graphs) return;
  lambda[g] = L.theta[g];
  if (residual) residual[g] = sqrtf(fold_partials(L, g, 0));
  if (iterations) iterations[g] = L.steps[g];
}

// The eigenvalues and vectors of the symmetric tridiagonal matrix (d: diagonal, e[i]: the entry between i and i + 1) by the implicit
// QL iteration (EISPACK tql2); z [m][m] row-major, starts as the identity, ends with the vectors in its columns.
bool tridiagonal_ql(std::vector<double> &d, std::vector<double> &e, int m, std::vector<double> &z) {
  e[m - 1] = 0.0;
  for (int l = 0; l < m; ++l) {
    int iter = 0, mm;
    do {
      for (mm = l; mm < m - 1; ++mm) {
        const double dd = std::fabs(d[mm]) + std::fabs(d[mm + 1]);
        if (std::fabs(e[mm]) <= DBL_EPSILON * dd) break;
      }
      if (mm != l) {
        if (iter++ == 120) return false;
        double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
        double r = std::hypot(g, 1.0);
        g = d[mm] - d[l] + e[l] / (g + std::copysign(r, g));
        double s = 1.0, c = 1.0, p = 0.0;
        int i;
        for (i = mm - 1; i >= l; --i) {
          double f = s * e[i];
          const double b = c * e[i];
          e[i + 1] = (r = std::hypot(f, g));
          if (r == 0.0) {
            d[i + 1] -= p;
            e[mm] = 0.0;
            break;
          }
          s = f / r;
          c = g / r;
          g = d[i + 1] - p;
          r = (d[i] - g) * s + 2.0 * c * b;
          d[i + 1] = g + (p = s * r);
          g = c * r - b;
          for (int k = 0; k < m; ++k) {
            f = z[(size_t)k * m + i + 1];
            z[(size_t)k * m + i + 1] = s * z[(size_t)k * m + i] + c * f;
            z[(size_t)k * m + i] = c * z[(size_t)k * m + i] - s * f;
          }
        }
        if (r == 0.0 && i >= l) continue;
        d[l] -= p;
        e[l] = g;
        e[mm] = 0.0;
      }
    } while (mm != l);
  }
  return true;
}

// the largest Ritz value of the first m steps and its unit coefficient vector
bool largest_ritz(const float *alpha, const float *beta, int m, double *theta, std::vector<double> &coef) {
  std::vector<double> d(m), e(m, 0.0), z((size_t)m * m, 0.0);
  for (int k = 0; k < m; ++k) {
    d[k] = alpha[k];
    if (k + 1 < m) e[k] = beta[k];
    z[(size_t)k * m + k] = 1.0;
  }
  if (!tridiagonal_ql(d, e, m, z)) return false;
  int best = 0;
  for (int k = 1; k < m; ++k)
    if (d[k] > d[best]) best = k;
  *theta = d[best];
  coef.resize(m);
  for (int k = 0; k < m; ++k) coef[k] = z[(size_t)k * m + best];
  return true;
}

// the view's pieces, in workspace order.  The entry clears alpha .. coef and anorm .. stop as one span each and reads alpha and beta
// back as one block, so these stay neighbours
void lanczos_layout(Workspace &w, int64_t n, int32_t n_graphs, int32_t max_iter, LanczosView &L) {
  const size_t max_chunks = (size_t)((n + kDotChunk - 1) / kDotChunk + n_graphs);
  const size_t gl = (size_t)n_graphs * (size_t)max_iter;
  L.V = w.take<float>((size_t)max_iter * (size_t)n);
  L.w = w.take<float>((size_t)n);
  L.y = w.take<float>((size_t)n);
  L.partial = w.take<float>((size_t)max_iter * max_chunks);
  L.h = w.take<float>(gl);
  L.alpha = w.take<float>(gl);
  L.beta = w.take<float>(gl);
  L.coef = w.take<float>(gl);
  L.anorm = w.take<float>((size_t)n_graphs);
  L.theta = w.take<float>((size_t)n_graphs);
  L.steps = w.take<int32_t>((size_t)n_graphs);
  L.stop = w.take<int32_t>(2 * (size_t)n_graphs);
  L.gptr = w.take<int32_t>((size_t)n_graphs + 1);
  L.cptr = w.take<int32_t>((size_t)n_graphs + 1);
  L.chunk_graph = w.take<int32_t>(max_chunks);
  L.chunk_begin = w.take<int32_t>(max_chunks);
  L.chunk_end = w.take<int32_t>(max_chunks);
}

size_t lanczos_bytes(int64_t n, int32_t n_graphs, int32_t max_iter) {
  LanczosView L;
  return measure(lanczos_layout, n, n_graphs, max_iter, L);
}

int32_t check_lanczos_sizes(const char *fn, int64_t n, int64_t nnz, int32_t n_graphs, int32_t max_iter) {
  NGPDE_REQUIRE(n >= 0 && nnz >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n %lld, nnz %lld)", fn, (long long)n, (long long)nnz);
  NGPDE_REQUIRE(n <= 0x7fffffffLL && nnz <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: a size above 2^31 - 1 (n %lld, nnz %lld)", fn,
                (long long)n, (long long)nnz);
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_graphs %d, at least 1", fn, n_graphs);
  NGPDE_REQUIRE(max_iter >= 1 && max_iter <= kMaxIter, NGPDE_ERR_INVALID_ARGUMENT, "%s: max_iter %d outside 1 : %d", fn, max_iter, kMaxIter);
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_coo_matrix(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t kind, int32_t dir,
                         int32_t add_self_loops, const float *w, int32_t n_graphs, const int32_t *graph_of, const float *scale, int32_t *rows,
                         int32_t *cols, float *vals, int32_t *row_ptr, int32_t *group_ptr, int32_t *member, int32_t *group_of, float *adj,
                         float *deg, float *sym_tol, int64_t *nnz_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_matrix";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(n_nodes >= 0 && n_edges >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n_nodes %lld, n_edges %lld)", fn,
                (long long)n_nodes, (long long)n_edges);
  NGPDE_REQUIRE(nnz_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: nnz_out is NULL", fn);
  *nnz_out = 0;
  NGPDE_REQUIRE(kind == NGPDE_MATRIX_ADJ || kind == NGPDE_MATRIX_LAPLACIAN || kind == NGPDE_MATRIX_NORM_LAPLACIAN, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: kind %d is none of NGPDE_MATRIX_ADJ / LAPLACIAN / NORM_LAPLACIAN", fn, kind);
  NGPDE_REQUIRE(dir == NGPDE_DIR_OUT || dir == NGPDE_DIR_IN, NGPDE_ERR_INVALID_ARGUMENT, "%s: dir %d is neither NGPDE_DIR_OUT nor NGPDE_DIR_IN", fn,
                dir);
  NGPDE_REQUIRE(!add_self_loops || kind == NGPDE_MATRIX_NORM_LAPLACIAN, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: add_self_loops belongs to NGPDE_MATRIX_NORM_LAPLACIAN", fn);
  NGPDE_REQUIRE(!scale || (kind == NGPDE_MATRIX_NORM_LAPLACIAN && n_graphs >= 1 && (n_graphs == 1 || graph_of)), NGPDE_ERR_INVALID_ARGUMENT,
                "%s: scale needs NGPDE_MATRIX_NORM_LAPLACIAN, n_graphs >= 1 and, for more than one graph, graph_of", fn);
  const int64_t m = n_edges + (kind == NGPDE_MATRIX_ADJ ? 0 : n_nodes);
  NGPDE_REQUIRE(n_nodes <= 0x7fffffffLL && n_edges <= 0x7fffffffLL && m <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: %lld nodes and %lld edges: the nodes, the edges and the copies to sort are at most 2^31 - 1 each", fn, (long long)n_nodes,
                (long long)n_edges);
  NGPDE_REQUIRE(n_edges == 0 || (s && t), NGPDE_ERR_INVALID_ARGUMENT, "%s: s / t is NULL", fn);
  NGPDE_REQUIRE(n_edges == 0 || n_nodes > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %lld edges on a graph without nodes", fn,
                (long long)n_edges);
  NGPDE_REQUIRE(row_ptr != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: row_ptr is NULL", fn);
  NGPDE_REQUIRE(m == 0 || (rows && cols && vals && group_ptr && member && group_of), NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  if (m == 0) {
    NGPDE_HIP_CHECK(hipMemsetAsync(row_ptr, 0, ((size_t)n_nodes + 1) * sizeof(int32_t), stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    return NGPDE_OK;
  }
  Scratch sc;
  int32_t *flags = nullptr, *iota = nullptr, *copy = nullptr, *head = nullptr, *incl = nullptr;
  unsigned long long *key = nullptr, *key_sorted = nullptr;
  float *a = adj, *d = deg;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&key, (size_t)m)) || (st = sc.get(&key_sorted, (size_t)m)) ||
      (st = sc.get(&iota, (size_t)m)) || (st = sc.get(&copy, (size_t)m)) || (st = sc.get(&head, (size_t)m)) || (st = sc.get(&incl, (size_t)m)))
    return st;
  if (!a && (st = sc.get(&a, (size_t)m))) return st;
  if (!d && kind != NGPDE_MATRIX_ADJ && (st = sc.get(&d, (size_t)n_nodes))) return st;
  hipLaunchKernelGGL(matrix_keys_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, n_edges, n_nodes, index_base, dir == NGPDE_DIR_IN ? 1 : 0, s,
                     t, key, iota, flags);
  NGPDE_LAUNCH_CHECK("matrix_keys_kernel");
  if ((st = sort_positions(m, bits_for((unsigned long long)n_nodes * (unsigned long long)n_nodes), key, key_sorted, iota, copy, sc, stream)))
    return st;
  hipLaunchKernelGGL(heads_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, key_sorted, head);
  NGPDE_LAUNCH_CHECK("heads_kernel");
  if ((st = scan_i32(true, head, incl, (size_t)m, sc, stream))) return st;
  hipLaunchKernelGGL(entries_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, n_nodes, key_sorted, copy, head, incl, rows, cols, group_ptr,
                     member, group_of, flags);
  NGPDE_LAUNCH_CHECK("entries_kernel");
  hipLaunchKernelGGL(entry_values_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, n_edges, add_self_loops ? 1 : 0, group_ptr, member, w, flags,
                     a, sym_tol);
  NGPDE_LAUNCH_CHECK("entry_values_kernel");
  hipLaunchKernelGGL(row_ptr_kernel, dim3(blocks_for(n_nodes + 1)), dim3(kB), 0, stream, n_nodes, rows, flags, row_ptr);
  NGPDE_LAUNCH_CHECK("row_ptr_kernel");
  if (d) {
    hipLaunchKernelGGL(row_sums_kernel, dim3(blocks_for(n_nodes)), dim3(kB), 0, stream, n_nodes, kind, row_ptr, a, d, flags);
    NGPDE_LAUNCH_CHECK("row_sums_kernel");
  }
  hipLaunchKernelGGL(matrix_values_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, kind, n_graphs, graph_of, scale, rows, cols, a, d, vals,
                     flags);
  NGPDE_LAUNCH_CHECK("matrix_values_kernel");
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[fBad], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references a node outside the %lld nodes", fn,
                (long long)n_nodes);
  NGPDE_REQUIRE(!h[fOrder], NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of holds an id outside 0:%d", fn, n_graphs - 1);
  NGPDE_REQUIRE(!h[fZeroRow], NGPDE_ERR_INVALID_ARGUMENT,
                "%s: the row sum of node %lld is not positive: the normalised Laplacian divides by its square root (an isolated node?)", fn,
                (long long)(n_nodes - h[fZeroRow]));
  *nnz_out = h[fCount];
  return NGPDE_OK;
}

int32_t ngpde_csr_check_symmetric(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *rows, const int32_t *cols, const float *vals,
                                  const float *tol, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_check_symmetric";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(n >= 0 && nnz >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n %lld, nnz %lld)", fn, (long long)n, (long long)nnz);
  NGPDE_REQUIRE(n <= 0x7fffffffLL && nnz <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: a size above 2^31 - 1 (n %lld, nnz %lld)", fn,
                (long long)n, (long long)nnz);
  if (nnz == 0) return NGPDE_OK;
  NGPDE_REQUIRE(row_ptr && rows && cols && vals, NGPDE_ERR_INVALID_ARGUMENT, "%s: row_ptr / rows / cols / vals is NULL", fn);
  Scratch sc;
  int32_t *flags = nullptr;
  unsigned long long *first = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&first, 1))) return st;
  NGPDE_HIP_CHECK(hipMemsetAsync(first, 0xff, sizeof(unsigned long long), stream));
  hipLaunchKernelGGL(symmetry_kernel, dim3(blocks_for(nnz)), dim3(kB), 0, stream, n, nnz, row_ptr, rows, cols, vals, tol, first, flags);
  NGPDE_LAUNCH_CHECK("symmetry_kernel");
  unsigned long long h_first = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_first, first, sizeof(h_first), hipMemcpyDeviceToHost, stream));
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[fCsr], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an entry or a row pointer lies outside the %lld x %lld matrix", fn,
                (long long)n, (long long)n);
  NGPDE_REQUIRE(h_first == ~0ull, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: the matrix is not symmetric: entry (%llu, %llu) has no equal partner at (%llu, %llu) (a directed edge, or weights that "
                "differ by more than the rounding of their sums)",
                fn, h_first / (unsigned long long)n, h_first % (unsigned long long)n, h_first % (unsigned long long)n,
                h_first / (unsigned long long)n);
  return NGPDE_OK;
}

size_t ngpde_csr_lambda_max_workspace_bytes(int64_t n, int32_t n_graphs, int32_t max_iter) {
  if (n < 0 || n > 0x7fffffffLL || n_graphs < 1 || max_iter < 1 || max_iter > kMaxIter) return 0;
  return lanczos_bytes(n, n_graphs, max_iter);
}

int32_t ngpde_csr_lambda_max(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *cols, const float *vals, int32_t n_graphs,
                             const int32_t *graph_of, int32_t max_iter, float tol, uint64_t seed, float *lambda_out, float *residual_out,
                             int32_t *iterations_out, float *vector_out, void *workspace, size_t workspace_bytes, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_lambda_max";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_lanczos_sizes(fn, n, nnz, n_graphs, max_iter)) return st;
  NGPDE_REQUIRE(tol >= 0.f && std::isfinite(tol), NGPDE_ERR_INVALID_ARGUMENT, "%s: tol %g is not a finite number >= 0", fn, (double)tol);
  NGPDE_REQUIRE(n_graphs == 1 || graph_of, NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of is NULL with %d graphs", fn, n_graphs);
  NGPDE_REQUIRE(lambda_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: lambda_out is NULL", fn);
  NGPDE_REQUIRE(row_ptr && (nnz == 0 || (cols && vals)), NGPDE_ERR_INVALID_ARGUMENT, "%s: row_ptr / cols / vals is NULL", fn);
  if (int32_t st = check_workspace(fn, workspace, workspace_bytes, lanczos_bytes(n, n_graphs, max_iter), 1)) return st;
  Workspace w(workspace);
  LanczosView L;
  lanczos_layout(w, n, n_graphs, max_iter, L);
  L.n = n;
  L.n_graphs = n_graphs;
  L.ld = max_iter;
  L.graph_of = graph_of;
  if (vector_out) L.y = vector_out;
  // the kernels only read the view's tables; the setup below fills them
  auto writable = [](const int32_t *p) { return const_cast<int32_t *>(p); };
  int32_t *gptr = writable(L.gptr), *cptr = writable(L.cptr), *chunk_graph = writable(L.chunk_graph), *chunk_begin = writable(L.chunk_begin),
          *chunk_end = writable(L.chunk_end);
  auto span = [](const void *from, const void *to) { return (size_t)((const char *)to - (const char *)from); };

  // ---- setup: the CSR lists and the graph ids checked, the graphs' node ranges read back once, the chunk table uploaded
  Scratch sc;
  int32_t *flags = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream))) return st;
  hipLaunchKernelGGL(csr_check_kernel, dim3(blocks_for(std::max(n, nnz))), dim3(kB), 0, stream, n, nnz, row_ptr, cols, n_graphs, graph_of, flags);
  NGPDE_LAUNCH_CHECK("csr_check_kernel");
  hipLaunchKernelGGL(graph_ptr_kernel, dim3(blocks_for((int64_t)n_graphs + 1)), dim3(kB), 0, stream, n, n_graphs, graph_of, gptr);
  NGPDE_LAUNCH_CHECK("graph_ptr_kernel");
  std::vector<int32_t> h_gptr((size_t)n_graphs + 1);
  NGPDE_HIP_CHECK(hipMemcpyAsync(h_gptr.data(), gptr, h_gptr.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  int32_t hf[kFlagWords];
  if ((st = read_flags(flags, hf, stream))) return st;
  NGPDE_REQUIRE(!hf[fCsr], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: a column or a row pointer lies outside the %lld x %lld matrix", fn,
                (long long)n, (long long)n);
  NGPDE_REQUIRE(!hf[fBad], NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of holds an id outside 0:%d", fn, n_graphs - 1);
  NGPDE_REQUIRE(!hf[fOrder], NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of is not non-decreasing: the nodes of a graph must be contiguous", fn);
  std::vector<int32_t> h_cptr((size_t)n_graphs + 1, 0), h_cg, h_cb, h_ce;
  for (int g = 0; g < n_graphs; ++g) {
    for (int32_t b = h_gptr[g]; b < h_gptr[g + 1]; b += kDotChunk) {
      h_cg.push_back(g);
      h_cb.push_back(b);
      h_ce.push_back(std::min<int32_t>(b + kDotChunk, h_gptr[g + 1]));
    }
    h_cptr[g + 1] = (int32_t)h_cg.size();
  }
  L.n_chunks = (int32_t)h_cg.size();
  NGPDE_HIP_CHECK(hipMemcpyAsync(cptr, h_cptr.data(), h_cptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  if (L.n_chunks) {
    const size_t cb = (size_t)L.n_chunks * sizeof(int32_t);
    NGPDE_HIP_CHECK(hipMemcpyAsync(chunk_graph, h_cg.data(), cb, hipMemcpyHostToDevice, stream));
    NGPDE_HIP_CHECK(hipMemcpyAsync(chunk_begin, h_cb.data(), cb, hipMemcpyHostToDevice, stream));
    NGPDE_HIP_CHECK(hipMemcpyAsync(chunk_end, h_ce.data(), cb, hipMemcpyHostToDevice, stream));
  }
  NGPDE_HIP_CHECK(hipMemsetAsync(L.anorm, 0, span(L.anorm, gptr), stream));   // anorm, theta, steps, stop
  NGPDE_HIP_CHECK(hipMemsetAsync(L.alpha, 0, span(L.alpha, L.anorm), stream));   // alpha, beta, coef

  const size_t gl = (size_t)n_graphs * (size_t)max_iter;
  const size_t beta_at = (size_t)(L.beta - L.alpha);
  std::vector<float> h_ab(beta_at + gl, 0.f);   // alpha, the layout's padding, beta
  std::vector<int32_t> h_steps((size_t)n_graphs, 0), h_stop((size_t)n_graphs, 0), h_done((size_t)n_graphs, 0);
  std::vector<double> coef;
  auto read_state = [&]() -> int32_t {
    NGPDE_HIP_CHECK(hipMemcpyAsync(h_ab.data(), L.alpha, h_ab.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
    NGPDE_HIP_CHECK(hipMemcpyAsync(h_steps.data(), L.steps, h_steps.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    NGPDE_HIP_CHECK(hipMemcpyAsync(h_stop.data(), L.stop, h_stop.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    return NGPDE_OK;
  };
  const dim3 node_grid(blocks_for(n)), spmv_grid(blocks_for(n * kSpmvLanes)), graph_grid(blocks_for(n_graphs));

  if (n > 0 && L.n_chunks > 0) {
    // ---- v_0 = the start vector, normalised per graph
    hipLaunchKernelGGL(start_kernel, node_grid, dim3(kB), 0, stream, L, (unsigned long long)seed);
    NGPDE_LAUNCH_CHECK("start_kernel");
    hipLaunchKernelGGL(chunk_dot_kernel, dim3(L.n_chunks, 1), dim3(256), 0, stream, L, 1, L.w, L.w);
    NGPDE_LAUNCH_CHECK("chunk_dot_kernel");
    hipLaunchKernelGGL(fold_dots_kernel, graph_grid, dim3(kB), 0, stream, L, 1, 1, -1, 0);
    NGPDE_LAUNCH_CHECK("fold_dots_kernel");
    hipLaunchKernelGGL(scale_kernel, node_grid, dim3(kB), 0, stream, L, 1, L.w, L.h, 0, 1, L.V);
    NGPDE_LAUNCH_CHECK("scale_kernel");
    // ---- the steps
    for (int j = 0; j < max_iter; ++j) {
      const float *vj = L.V + (size_t)j * (size_t)n;
      hipLaunchKernelGGL(csr_spmv_kernel, spmv_grid, dim3(256), 0, stream, L, 0, row_ptr, cols, vals, vj, L.w);
      NGPDE_LAUNCH_CHECK("csr_spmv_kernel");
      for (int pass = 0; pass < 2; ++pass) {   // full reorthogonalisation: two classical Gram-Schmidt passes against v_0 .. v_j
        hipLaunchKernelGGL(chunk_dot_kernel, dim3(L.n_chunks, j + 1), dim3(256), 0, stream, L, 0, L.V, L.w);
        NGPDE_LAUNCH_CHECK("chunk_dot_kernel");
        hipLaunchKernelGGL(fold_dots_kernel, dim3(blocks_for((int64_t)n_graphs * (j + 1))), dim3(kB), 0, stream, L, 0, j + 1, j, pass);
        NGPDE_LAUNCH_CHECK("fold_dots_kernel");
        hipLaunchKernelGGL(orthogonalise_kernel, node_grid, dim3(kB), 0, stream, L, j + 1);
        NGPDE_LAUNCH_CHECK("orthogonalise_kernel");
      }
      hipLaunchKernelGGL(chunk_dot_kernel, dim3(L.n_chunks, 1), dim3(256), 0, stream, L, 0, L.w, L.w);
      NGPDE_LAUNCH_CHECK("chunk_dot_kernel");
      hipLaunchKernelGGL(step_kernel, graph_grid, dim3(kB), 0, stream, L, j, max_iter);
      NGPDE_LAUNCH_CHECK("step_kernel");
      if (j + 1 == max_iter) break;
      hipLaunchKernelGGL(scale_kernel, node_grid, dim3(kB), 0, stream, L, 0, L.w, L.beta, j, 0, L.V + (size_t)(j + 1) * (size_t)n);
      NGPDE_LAUNCH_CHECK("scale_kernel");
      if ((j + 1) % kCheckEvery != 0) continue;
      // ---- every kCheckEvery steps: the small eigenproblems on the host; a converged graph is frozen
      if ((st = read_state())) return st;
      bool all_done = true;
      for (int g = 0; g < n_graphs; ++g) {
        if (!h_stop[g] && !h_done[g] && h_steps[g] > 0) {
          const int m = h_steps[g];
          double theta = 0.0;
          NGPDE_REQUIRE(largest_ritz(&h_ab[(size_t)g * max_iter], &h_ab[beta_at + (size_t)g * max_iter], m, &theta, coef), NGPDE_ERR_STATE,
                        "%s: the tridiagonal eigenproblem of graph %d did not converge (a NaN in the matrix?)", fn, g);
          const double bound = std::fabs((double)h_ab[beta_at + (size_t)g * max_iter + m - 1] * coef[m - 1]);
          if (bound <= (double)tol * std::fabs(theta)) h_done[g] = 1;
        }
        all_done = all_done && (h_stop[g] || h_done[g]);
      }
      NGPDE_HIP_CHECK(hipMemcpyAsync(L.stop + n_graphs, h_done.data(), h_done.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
      if (all_done) break;
    }
  }
  // ---- the Ritz pair of every graph, and its residual by one more product
  if ((st = read_state())) return st;
  std::vector<float> h_coef(gl, 0.f), h_theta((size_t)n_graphs, 0.f);
  for (int g = 0; g < n_graphs; ++g) {
    const int m = h_steps[g];
    if (m == 0) continue;
    double theta = 0.0;
    NGPDE_REQUIRE(largest_ritz(&h_ab[(size_t)g * max_iter], &h_ab[beta_at + (size_t)g * max_iter], m, &theta, coef), NGPDE_ERR_STATE,
                  "%s: the tridiagonal eigenproblem of graph %d did not converge (a NaN in the matrix?)", fn, g);
    h_theta[g] = (float)theta;
    for (int k = 0; k < m; ++k) h_coef[(size_t)g * max_iter + k] = (float)coef[k];
  }
  NGPDE_HIP_CHECK(hipMemcpyAsync(L.coef, h_coef.data(), gl * sizeof(float), hipMemcpyHostToDevice, stream));
  NGPDE_HIP_CHECK(hipMemcpyAsync(L.theta, h_theta.data(), (size_t)n_graphs * sizeof(float), hipMemcpyHostToDevice, stream));
  if (n > 0 && L.n_chunks > 0) {
    hipLaunchKernelGGL(ritz_kernel, node_grid, dim3(kB), 0, stream, L);
    NGPDE_LAUNCH_CHECK("ritz_kernel");
    hipLaunchKernelGGL(chunk_dot_kernel, dim3(L.n_chunks, 1), dim3(256), 0, stream, L, 1, L.w, L.w);
    NGPDE_LAUNCH_CHECK("chunk_dot_kernel");
    hipLaunchKernelGGL(fold_dots_kernel, graph_grid, dim3(kB), 0, stream, L, 1, 1, -1, 0);
    NGPDE_LAUNCH_CHECK("fold_dots_kernel");
    hipLaunchKernelGGL(scale_kernel, node_grid, dim3(kB), 0, stream, L, 1, L.w, L.h, 0, 1, L.y);
    NGPDE_LAUNCH_CHECK("scale_kernel");
    hipLaunchKernelGGL(csr_spmv_kernel, spmv_grid, dim3(256), 0, stream, L, 1, row_ptr, cols, vals, L.y, L.w);
    NGPDE_LAUNCH_CHECK("csr_spmv_kernel");
    hipLaunchKernelGGL(residual_kernel, node_grid, dim3(kB), 0, stream, L);
    NGPDE_LAUNCH_CHECK("residual_kernel");
    hipLaunchKernelGGL(chunk_dot_kernel, dim3(L.n_chunks, 1), dim3(256), 0, stream, L, 1, L.w, L.w);
    NGPDE_LAUNCH_CHECK("chunk_dot_kernel");
  }
  hipLaunchKernelGGL(results_kernel, graph_grid, dim3(kB), 0, stream, L, lambda_out, residual_out, iterations_out);
  NGPDE_LAUNCH_CHECK("results_kernel");
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));   // (the host arrays uploaded above leave scope)
  return NGPDE_OK;
}

int32_t ngpde_csr_spgemm_count(int64_t n, int64_t nnz_p, const int32_t *p_cols, int64_t nnz_a, const int32_t *a_row_ptr, int64_t limit,
                               int64_t *offsets_out, int64_t *total_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_spgemm_count";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_product(fn, n, nnz_p, nnz_a, p_cols, a_row_ptr)) return st;
  NGPDE_REQUIRE(total_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: total_out is NULL", fn);
  *total_out = 0;
  NGPDE_REQUIRE(limit >= 0 && limit <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: limit %lld outside 0 : 2^31 - 1", fn, (long long)limit);
  if (nnz_p == 0) return NGPDE_OK;
  Scratch sc;
  int32_t *flags = nullptr;
  long long *off = reinterpret_cast<long long *>(offsets_out);
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = expand_offsets(n, nnz_p, p_cols, a_row_ptr, nnz_a, &off, flags, sc, stream))) return st;
  long long total = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&total, off + nnz_p, sizeof(total), hipMemcpyDeviceToHost, stream));
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[fBad] && !h[fCsr], NGPDE_ERR_DIMENSION_MISMATCH,
                "%s: DimensionMismatch: a column of P or a row pointer of A lies outside the %lld x %lld matrices", fn, (long long)n, (long long)n);
  NGPDE_REQUIRE(total <= limit, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: the product is too dense: %lld terms to expand, at most %lld (expand, sort, combine holds every term once)", fn, total,
                (long long)limit);
  *total_out = total;
  return NGPDE_OK;
}

int32_t ngpde_csr_spgemm(int64_t n, int64_t nnz_p, const int32_t *p_rows, const int32_t *p_cols, const float *p_vals, int64_t nnz_a,
                         const int32_t *a_row_ptr, const int32_t *a_cols, const float *a_vals, const int64_t *offsets, int64_t total,
                         int32_t *rows_out, int32_t *cols_out, float *vals_out, int32_t *row_ptr_out, int64_t *nnz_out,
                         ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_spgemm";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_product(fn, n, nnz_p, nnz_a, p_cols, a_row_ptr)) return st;
  NGPDE_REQUIRE(nnz_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: nnz_out is NULL", fn);
  *nnz_out = 0;
  NGPDE_REQUIRE(total >= 0 && total <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: total %lld outside 0 : 2^31 - 1", fn, (long long)total);
  NGPDE_REQUIRE(row_ptr_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: row_ptr_out is NULL", fn);
  NGPDE_REQUIRE(total == 0 || (p_rows && p_vals && a_cols && a_vals && offsets && rows_out && cols_out && vals_out), NGPDE_ERR_INVALID_ARGUMENT,
                "%s: an input list, offsets or an output is NULL", fn);
  NGPDE_REQUIRE(total == 0 || nnz_p > 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: total is %lld for a matrix P without entries", fn, (long long)total);
  Scratch sc;
  int32_t *flags = nullptr, *iota = nullptr, *perm = nullptr, *head = nullptr, *incl = nullptr, *group_ptr = nullptr;
  const long long *off = reinterpret_cast<const long long *>(offsets);
  unsigned long long *key = nullptr, *key_sorted = nullptr;
  float *prod = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream))) return st;
  if (total == 0) {
    NGPDE_HIP_CHECK(hipMemsetAsync(row_ptr_out, 0, ((size_t)n + 1) * sizeof(int32_t), stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    return NGPDE_OK;
  }
  if ((st = sc.get(&key, (size_t)total)) || (st = sc.get(&key_sorted, (size_t)total)) || (st = sc.get(&iota, (size_t)total)) ||
      (st = sc.get(&perm, (size_t)total)) || (st = sc.get(&head, (size_t)total)) || (st = sc.get(&incl, (size_t)total)) ||
      (st = sc.get(&group_ptr, (size_t)total + 1)) || (st = sc.get(&prod, (size_t)total)))
    return st;
  hipLaunchKernelGGL(expand_kernel, dim3(blocks_for(total)), dim3(kB), 0, stream, total, nnz_p, n, nnz_a, off, p_rows, p_cols, p_vals, a_row_ptr, a_cols,
                     a_vals, key, iota, prod, flags);
  NGPDE_LAUNCH_CHECK("expand_kernel");
  if ((st = sort_positions(total, bits_for((unsigned long long)n * (unsigned long long)n), key, key_sorted, iota, perm, sc, stream))) return st;
  hipLaunchKernelGGL(heads_kernel, dim3(blocks_for(total)), dim3(kB), 0, stream, total, key_sorted, head);
  NGPDE_LAUNCH_CHECK("heads_kernel");
  if ((st = scan_i32(true, head, incl, (size_t)total, sc, stream))) return st;
  hipLaunchKernelGGL(entries_kernel, dim3(blocks_for(total)), dim3(kB), 0, stream, total, n, key_sorted, perm, head, incl, rows_out, cols_out,
                     group_ptr, (int32_t *)nullptr, (int32_t *)nullptr, flags);
  NGPDE_LAUNCH_CHECK("entries_kernel");
  hipLaunchKernelGGL(product_values_kernel, dim3(blocks_for(total)), dim3(kB), 0, stream, total, group_ptr, perm, prod, flags, vals_out);
  NGPDE_LAUNCH_CHECK("product_values_kernel");
  hipLaunchKernelGGL(row_ptr_kernel, dim3(blocks_for(n + 1)), dim3(kB), 0, stream, n, rows_out, flags, row_ptr_out);
  NGPDE_LAUNCH_CHECK("row_ptr_kernel");
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[fCsr], NGPDE_ERR_INVALID_ARGUMENT, "%s: offsets / total are not what ngpde_csr_spgemm_count gives for these matrices", fn);
  NGPDE_REQUIRE(!h[fBad], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: a row of P or a column of A lies outside the %lld x %lld matrices",
                fn, (long long)n, (long long)n);
  *nnz_out = h[fCount];
  return NGPDE_OK;
}

}  // extern "C"
