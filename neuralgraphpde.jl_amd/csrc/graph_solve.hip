// graph_solve.hip -- the inverse side of a graph matrix (include/ngpde.h, "graph solves"): (shift I + scale M) x_d = b_d for every
// feature row d of B by a (Jacobi-preconditioned) conjugate-gradient iteration over all graphs of a batch and all columns at once.
// Every (graph, column) PAIR is its own CG -- its own scalars, its own stop, its own iteration count -- and the whole iteration lives
// on the device: the host enqueues three launches per step and, with check_every > 0, reads one word every check_every steps.
//
// Layout.  The iteration state x, r, p, q is node-major, [n][dp] with dp = 64 * (slabs - 1) + w_last (the last slab's width rounded up
// to a power of two): the gather of an entry is one contiguous read across the lanes of its columns.  B, x0 and X are (D x N) as
// GraphMatrix.matmul takes them; the transpose happens where B is loaded and where a pair that stops writes its X.  A 1024-thread
// workgroup owns one 256-row CHUNK of one graph (a graph's chunks start at its first node) and one slab of at most 64 columns.  In a
// slab of width W a wave holds 64 / W row slots x W columns and every lane owns max(1, W / 4) consecutive rows, so a wave covers 16
// rows (W >= 4), 32 rows (W = 2) or 64 rows (W = 1) and 16, 8 or 4 waves of the workgroup work; narrow slabs put several rows on a
// wave instead of idling its lanes.
//
// Order guarantees (no float atomics; the flag words and the count of running pairs use integer atomics, which commute):
//   product        one lane per (row, column): the row's entries in ascending column from 0.0f, one multiply and one add each; then
//                  q = shift * p + scale * that
//   inner product  per chunk the balanced binary tree over its 256 rows (row 2 j with row 2 j + 1, then pairs of pairs, ...; rows past
//                  the graph's end are 0.0f).  A lane adds its own rows through a carry stack, the lanes of a wave continue the tree
//                  with xor shuffles, the waves through LDS: the three stages are levels of the SAME tree whatever W is, so a column's
//                  sums depend on neither D, the slab nor the lane mapping
//   fold           a pair's scalar is its graph's chunk sums added in chunk order from 0.0f, by (a lane of) every workgroup that
//                  needs it: all of them get the same bits
// The launches of step `it` freeze a pair whose stop_it is below `it`: they neither read nor write its columns.  A launch that stops a
// pair writes stop_it = it, which the workgroups of the same launch read as "running" whether they see the old or the new value.
#include <climits>
#include <cmath>
#include <cstdint>

#include "common.h"
#include "device_scratch.h"

namespace ngpde {

namespace {

// device words of one call (the head of the workspace)
enum { fAny = 0, fCsr = 1, fBad = 2, fOrder = 3, fDiag = 4, fRunning = 5, kCgWords = 8 };
// slots of the chunk sums
enum { sPQ = 0, sRZ = 1, sRR = 2, sBB = 3, kSlots = 4 };
// modes of the update launch
enum { mStep = 0, mResidual = 1, mStart = 2 };

constexpr int kChunk = 256;      // rows per chunk of an inner product
constexpr int kBlock = 1024;     // threads per workgroup: 16 waves
constexpr int kSlab = 64;        // columns per slab
constexpr int kMaxWaves = 16;

struct CgView {
  int64_t n, max_chunks;
  int32_t n_graphs, d, dp, n_slabs, w_last, max_iter;
  const int32_t *row_ptr, *cols, *graph_of;
  const float *vals;
  float shift, scale, rtol, atol;
  int32_t *words, *gptr, *cptr, *stop_it, *brk;
  float *dinv, *x, *r, *p, *q, *partial, *rho, *tol;
  float *X, *residual;
  int32_t *status, *iterations;
};

// ---- setup --------------------------------------------------------------------------------------------------------------------
__global__ void cg_check_kernel(int64_t n, int64_t nnz, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ cols, int32_t n_graphs,
                                const int32_t *__restrict__ graph_of, int32_t *__restrict__ words) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int bad = -1;
  if (p < nnz && (cols[p] < 0 || cols[p] >= n)) bad = fCsr;
  if (p < n) {
    if (row_ptr[p] > row_ptr[p + 1] || row_ptr[p] < 0 || row_ptr[p + 1] > nnz) bad = fCsr;
    if (graph_of) {
      if (graph_of[p] < 0 || graph_of[p] >= n_graphs) bad = fBad;
      else if (p > 0 && graph_of[p] < graph_of[p - 1]) bad = fOrder;
    }
  }
  if (p == 0 && (row_ptr[0] != 0 || row_ptr[n] != nnz)) bad = fCsr;
  if (bad >= 0) {
    atomicOr(&words[bad], 1);
    atomicOr(&words[fAny], 1);
  }
}

// gptr[g] = the first node of graph g; dinv[i] = 1 / (shift + scale * M_ii) (jacobi) or 1.  A diagonal that is not > 0 raises fDiag
// (n - i: the largest is the smallest node).  Nothing is read through lists that the check refused.
__global__ void cg_setup_kernel(CgView V, int jacobi) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (V.words[fCsr] | V.words[fBad] | V.words[fOrder]) return;
  if (i <= V.n_graphs) V.gptr[i] = V.graph_of ? (int32_t)lower_bound_dev(V.graph_of, V.n, (int32_t)i) : (i == 0 ? 0 : (int32_t)V.n);
  if (i >= V.n) return;
  float dv = 1.0f;
  if (jacobi) {
    const int64_t b = V.row_ptr[i], e = V.row_ptr[i + 1];
    const int64_t at = b + lower_bound_dev(V.cols + b, e - b, (int32_t)i);
    const float m = (at < e && V.cols[at] == (int32_t)i) ? V.vals[at] : 0.f;
    const float dg = V.shift + V.scale * m;
    if (!(dg > 0.f)) {
      atomicMax(&V.words[fDiag], (int32_t)(V.n - i));
      atomicOr(&V.words[fAny], 1);
    }
    dv = 1.0f / dg;
  }
  V.dinv[i] = dv;
}

// one workgroup: cptr = the scan of the graphs' chunk counts, the pairs' state, the defaults of the three info arrays (a graph
// without nodes: converged, 0 iterations, residual 0; refused input: every pair is a breakdown) and the count of running pairs
__global__ __launch_bounds__(kBlock) void cg_pairs_kernel(CgView V) {
  const int bad = V.words[fAny];
  if (threadIdx.x == 0) {
    int32_t c = 0, live = 0;
    for (int g = 0; g < V.n_graphs; ++g) {
      V.cptr[g] = c;
      const int32_t size = bad ? 0 : V.gptr[g + 1] - V.gptr[g];
      c += (size + kChunk - 1) / kChunk;
      live += size > 0;
    }
    V.cptr[V.n_graphs] = c;
    V.words[fRunning] = live * V.d;
  }
  for (int64_t k = threadIdx.x; k < (int64_t)V.n_graphs * V.dp; k += kBlock) {
    V.stop_it[k] = INT_MAX;
    V.brk[k] = 0;
    const int64_t g = k / V.dp, c = k - g * V.dp;
    if (c < V.d) {
      V.status[g * V.d + c] = bad ? 2 : 0;
      V.iterations[g * V.d + c] = 0;
      V.residual[g * V.d + c] = 0.f;
    }
  }
}

// ---- the iteration ------------------------------------------------------------------------------------------------------------
struct Geo {
  int g, chunk, begin, end, col0, W, lgW, rpt, lgR, nw, wave, col, row0;
  bool on;          // the lane holds a column of the matrix B in a wave that works
  bool first;       // the workgroup of its graph's first chunk: the one writer of the pairs' scalars
};

// false (for the whole workgroup): no chunk here, or refused input
__device__ __forceinline__ bool geometry(const CgView &V, Geo &G) {
  if (V.words[fAny]) return false;
  const int c = blockIdx.x;
  if (c >= V.cptr[V.n_graphs]) return false;
  int lo = 0, hi = V.n_graphs;   // cptr[lo] <= c < cptr[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (V.cptr[mid] <= c) lo = mid;
    else hi = mid;
  }
  G.g = lo;
  G.chunk = c;
  G.first = c == V.cptr[lo];
  G.begin = V.gptr[lo] + (c - V.cptr[lo]) * kChunk;
  G.end = min(G.begin + kChunk, V.gptr[lo + 1]);
  const int slab = blockIdx.y;
  G.col0 = slab * kSlab;
  G.W = slab == V.n_slabs - 1 ? V.w_last : kSlab;
  G.lgW = __ffs(G.W) - 1;
  G.rpt = G.W >= 4 ? G.W >> 2 : 1;
  G.lgR = __ffs(G.rpt) - 1;
  const int rows_per_wave = (64 >> G.lgW) * G.rpt;
  G.nw = kChunk / rows_per_wave;
  G.wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  G.col = G.col0 + (lane & (G.W - 1));
  G.row0 = G.begin + G.wave * rows_per_wave + (lane >> G.lgW) * G.rpt;
  G.on = G.wave < G.nw && G.col < V.d;
  return true;
}

// the lowest levels of the tree: leaf k of a lane's 2^lg consecutive rows, k ascending
struct TreeAcc {
  float s0, s1, s2, s3, s4;
  __device__ __forceinline__ void push(float v, int k) {
    if (!(k & 1)) { s0 = v; return; }
    v = s0 + v;
    if (!(k & 2)) { s1 = v; return; }
    v = s1 + v;
    if (!(k & 4)) { s2 = v; return; }
    v = s2 + v;
    if (!(k & 8)) { s3 = v; return; }
    s4 = s3 + v;
  }
  __device__ __forceinline__ float total(int lg) const { return lg == 0 ? s0 : lg == 1 ? s1 : lg == 2 ? s2 : lg == 3 ? s3 : s4; }
};

// the rest of the tree: across the row slots of a wave, then across the waves; lane t < W of the workgroup ends with column
// col0 + t's chunk sum and stores it unless that pair is frozen.  Every thread of the workgroup calls this.
__device__ __forceinline__ void chunk_sum_store(const CgView &V, const Geo &G, float v, float (*sh)[kSlab], int slot, int it,
                                                const int *go = nullptr) {   // go[t]: the caller's own word on "this pair takes the step"
  for (int o = G.W; o < 64; o <<= 1) v += __shfl_xor(v, o);
  const int lane = threadIdx.x & 63;
  if (G.wave < G.nw && lane < G.W) sh[G.wave][lane] = v;
  __syncthreads();
  const int t = threadIdx.x;
  if (t < G.W) {
    for (int s = 1; s < G.nw; s <<= 1)
      for (int j = 0; j < G.nw; j += 2 * s) sh[j][t] += sh[j + s][t];
    const int col = G.col0 + t;
    if (go ? go[t] != 0 : (col < V.d && V.stop_it[(size_t)G.g * V.dp + col] >= it))
      V.partial[((size_t)slot * V.max_chunks + G.chunk) * V.dp + col] = sh[0][t];
  }
  __syncthreads();
}

__device__ __forceinline__ float fold(const CgView &V, int slot, int g, int col) {
  float s = 0.f;
  const float *__restrict__ part = V.partial + (size_t)slot * V.max_chunks * V.dp + col;
  for (int32_t c = V.cptr[g]; c < V.cptr[g + 1]; ++c) s += part[(size_t)c * V.dp];
  return s;
}

// r = B, x = x0 (or 0), both transposed into the node-major state; the chunk sums of b . b
__global__ __launch_bounds__(kBlock) void cg_load_kernel(CgView V, const float *__restrict__ B, const float *__restrict__ x0) {
  __shared__ float sh[kMaxWaves][kSlab];
  Geo G;
  if (!geometry(V, G)) return;
  TreeAcc t;
  for (int k = 0; k < G.rpt; ++k) {
    const int row = G.row0 + k;
    float leaf = 0.f;
    if (G.on && row < G.end) {
      const size_t at = (size_t)row * V.dp + G.col, from = (size_t)G.col * (size_t)V.n + row;
      const float b = B[from];
      V.r[at] = b;
      V.x[at] = x0 ? x0[from] : 0.f;
      leaf = b * b;
    }
    t.push(leaf, k);
  }
  chunk_sum_store(V, G, t.total(G.lgR), sh, sBB, 0);
}

// launch 1 of a step: q = (shift I + scale M) v and the chunk sums of v . q
__global__ __launch_bounds__(kBlock) void cg_product_kernel(CgView V, int it, const float *__restrict__ v) {
  __shared__ float sh[kMaxWaves][kSlab];
  Geo G;
  if (!geometry(V, G)) return;
  const bool live = G.on && V.stop_it[(size_t)G.g * V.dp + G.col] >= it;
  const size_t dp = V.dp;
  const float *__restrict__ vc = v + G.col;
  TreeAcc t;
  for (int k = 0; k < G.rpt; ++k) {
    const int row = G.row0 + k;
    float leaf = 0.f;
    if (live && row < G.end) {
      int32_t e = V.row_ptr[row];
      const int32_t e1 = V.row_ptr[row + 1];
      float acc = 0.f;
      for (; e + 4 <= e1; e += 4) {   // (four gathers in flight; the adds stay in entry order)
        const int32_t c0 = V.cols[e], c1 = V.cols[e + 1], c2 = V.cols[e + 2], c3 = V.cols[e + 3];
        const float a0 = V.vals[e], a1 = V.vals[e + 1], a2 = V.vals[e + 2], a3 = V.vals[e + 3];
        const float v0 = vc[c0 * dp], v1 = vc[c1 * dp], v2 = vc[c2 * dp], v3 = vc[c3 * dp];
        acc += a0 * v0;
        acc += a1 * v1;
        acc += a2 * v2;
        acc += a3 * v3;
      }
      for (; e < e1; ++e) acc += V.vals[e] * vc[V.cols[e] * dp];
      const float pv = vc[row * dp];
      const float qv = V.shift * pv + V.scale * acc;
      V.q[row * dp + G.col] = qv;
      leaf = pv * qv;
    }
    t.push(leaf, k);
  }
  chunk_sum_store(V, G, t.total(G.lgR), sh, sPQ, it);
}

// launch 2 of a step: alpha = rho / (p . q); x += alpha p; r -= alpha q; the chunk sums of r . z (z = dinv r) and r . r.
// mode mResidual: r -= q (q = A x0); mode mStart: r as loaded.  A step with p . q <= 0 or a non-finite alpha changes nothing: the
// first workgroup marks the pair (brk = it) and launch 3 stops it.
__global__ __launch_bounds__(kBlock) void cg_update_kernel(CgView V, int it, int mode) {
  __shared__ float sh[kMaxWaves][kSlab], sh2[kMaxWaves][kSlab];
  __shared__ float s_alpha[kSlab];
  __shared__ int s_go[kSlab];
  Geo G;
  if (!geometry(V, G)) return;
  const size_t dp = V.dp;
  if (threadIdx.x < G.W) {
    const int col = G.col0 + threadIdx.x;
    const size_t pair = (size_t)G.g * dp + col;
    float alpha = 1.0f;
    int go = col < V.d && V.stop_it[pair] >= it;
    if (go && mode == mStep) {
      const float pq = fold(V, sPQ, G.g, col);
      alpha = V.rho[(size_t)((it - 1) & 1) * V.n_graphs * dp + pair] / pq;
      const bool broke = !(pq > 0.f) || !isfinite(alpha);
      if (G.first) V.brk[pair] = broke ? it : 0;
      if (broke) go = 0;
    }
    s_alpha[threadIdx.x] = alpha;
    s_go[threadIdx.x] = go;
  }
  __syncthreads();
  const int lc = G.col - G.col0;
  const bool go = G.on && s_go[lc];
  const float alpha = s_alpha[lc];
  TreeAcc trz, trr;
  for (int k = 0; k < G.rpt; ++k) {
    const int row = G.row0 + k;
    float lrz = 0.f, lrr = 0.f;
    if (go && row < G.end) {
      const size_t at = row * dp + G.col;
      float r = V.r[at];
      if (mode == mStep) {
        const float pv = V.p[at];
        V.x[at] = V.x[at] + alpha * pv;
      }
      if (mode != mStart) {
        r = r - alpha * V.q[at];
        V.r[at] = r;
      }
      const float z = r * V.dinv[row];
      lrz = r * z;
      lrr = r * r;
    }
    trz.push(lrz, k);
    trr.push(lrr, k);
  }
  chunk_sum_store(V, G, trz.total(G.lgR), sh, sRZ, it, s_go);
  chunk_sum_store(V, G, trr.total(G.lgR), sh2, sRR, it, s_go);
}

// launch 3 of a step: rho' = r . z, beta = rho' / rho, the stops, p = z + beta p.  A pair that stops here writes its X (transposed
// back) and, through its graph's first workgroup, its info, stop_it = it and one decrement of the running count.
__global__ __launch_bounds__(kBlock) void cg_direction_kernel(CgView V, int it) {
  __shared__ float s_beta[kSlab];
  __shared__ int s_state[kSlab];   // -2 frozen, -1 goes on, 0 / 1 / 2 stops with that status
  Geo G;
  if (!geometry(V, G)) return;
  const size_t dp = V.dp;
  if (threadIdx.x < G.W) {
    const int col = G.col0 + threadIdx.x;
    const size_t pair = (size_t)G.g * dp + col;
    float beta = 0.f;
    int state = -2;
    if (col < V.d && V.stop_it[pair] >= it) {
      const bool broke = it > 0 && V.brk[pair] == it;
      const float rr = fold(V, sRR, G.g, col);   // (after a breakdown: of the r that the step left unchanged)
      const float res = sqrtf(rr);
      float tol, rho = 0.f;
      if (it == 0) {
        tol = fmaxf(V.rtol * sqrtf(fold(V, sBB, G.g, col)), V.atol);
      } else {
        tol = V.tol[pair];
      }
      if (!broke) {
        rho = fold(V, sRZ, G.g, col);
        if (it > 0) beta = rho / V.rho[(size_t)((it - 1) & 1) * V.n_graphs * dp + pair];
      }
      if (broke || !isfinite(rr) || !isfinite(rho) || !isfinite(beta)) state = 2;
      else if (res <= tol) state = 0;
      else if (it >= V.max_iter) state = 1;
      else state = -1;
      if (G.first) {
        V.rho[(size_t)(it & 1) * V.n_graphs * dp + pair] = rho;
        if (it == 0) V.tol[pair] = tol;
        if (state >= 0) {
          const size_t out = (size_t)G.g * V.d + col;
          V.status[out] = state;
          V.iterations[out] = broke ? it - 1 : it;
          V.residual[out] = res;
          V.stop_it[pair] = it;
          atomicSub(&V.words[fRunning], 1);
        }
      }
    }
    s_beta[threadIdx.x] = beta;
    s_state[threadIdx.x] = state;
  }
  __syncthreads();
  if (!G.on) return;
  const int lc = G.col - G.col0;
  const int state = s_state[lc];
  const float beta = s_beta[lc];
  if (state == -2) return;
  for (int k = 0; k < G.rpt; ++k) {
    const int row = G.row0 + k;
    if (row >= G.end) break;
    const size_t at = row * dp + G.col;
    if (state >= 0) {
      V.X[(size_t)G.col * (size_t)V.n + row] = V.x[at];
    } else {
      const float z = V.r[at] * V.dinv[row];
      V.p[at] = it == 0 ? z : z + beta * V.p[at];
    }
  }
}

int32_t pow2_ceil(int32_t v) {
  int32_t p = 1;
  while (p < v) p <<= 1;
  return p;
}

// the view's geometry (n, n_graphs, d, dp, n_slabs, w_last, max_chunks) and its pieces, in workspace order
void cg_layout(Workspace &w, int64_t n, int32_t n_graphs, int32_t n_rhs, CgView &V) {
  V.n = n, V.n_graphs = n_graphs, V.d = n_rhs;
  V.n_slabs = (n_rhs + kSlab - 1) / kSlab;
  V.w_last = pow2_ceil(n_rhs - (V.n_slabs - 1) * kSlab);
  V.dp = (V.n_slabs - 1) * kSlab + V.w_last;
  V.max_chunks = (n + kChunk - 1) / kChunk + n_graphs;
  const size_t pairs = (size_t)n_graphs * (size_t)V.dp, state = (size_t)n * (size_t)V.dp;
  V.words = w.take<int32_t>(kCgWords);
  V.gptr = w.take<int32_t>((size_t)n_graphs + 1);
  V.cptr = w.take<int32_t>((size_t)n_graphs + 1);
  V.stop_it = w.take<int32_t>(pairs);
  V.brk = w.take<int32_t>(pairs);
  V.dinv = w.take<float>((size_t)n);
  V.x = w.take<float>(state);
  V.r = w.take<float>(state);
  V.p = w.take<float>(state);
  V.q = w.take<float>(state);
  V.partial = w.take<float>((size_t)kSlots * (size_t)V.max_chunks * (size_t)V.dp);
  V.rho = w.take<float>(2 * pairs);
  V.tol = w.take<float>(pairs);
}

size_t cg_bytes(int64_t n, int32_t n_graphs, int32_t n_rhs) {
  CgView V;
  return measure(cg_layout, n, n_graphs, n_rhs, V);
}

bool cg_sizes_ok(int64_t n, int32_t n_graphs, int32_t n_rhs) {
  if (n < 0 || n > 0x7fffffffLL || n_graphs < 1 || n_rhs < 1) return false;
  const int64_t dp = (int64_t)((n_rhs + kSlab - 1) / kSlab) * kSlab;
  // the state's positions and the grid: row * dp + col below 2^63 anyway; the pairs and the chunk count must fit int32 / grid.x
  return (int64_t)n_graphs * dp <= 0x7fffffffLL && (n + kChunk - 1) / kChunk + n_graphs <= 0x7fffffffLL && n_rhs <= 65535 * kSlab;
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

size_t ngpde_csr_cg_workspace_bytes(int64_t n, int32_t n_graphs, int32_t n_rhs) {
  if (!cg_sizes_ok(n, n_graphs, n_rhs)) return 0;
  return cg_bytes(n, n_graphs, n_rhs);
}

int32_t ngpde_csr_cg(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *cols, const float *vals, int32_t n_graphs,
                     const int32_t *graph_of, float shift, float scale, int32_t n_rhs, const float *B, const float *x0, float *X,
                     int32_t precondition, float rtol, float atol, int32_t max_iter, int32_t check_every, int32_t *status_out,
                     int32_t *iterations_out, float *residual_out, void *workspace, size_t workspace_bytes, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_cg";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(n >= 0 && nnz >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n %lld, nnz %lld)", fn, (long long)n, (long long)nnz);
  NGPDE_REQUIRE(n <= 0x7fffffffLL && nnz <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: a size above 2^31 - 1 (n %lld, nnz %lld)", fn,
                (long long)n, (long long)nnz);
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_graphs %d, at least 1", fn, n_graphs);
  NGPDE_REQUIRE(n_rhs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_rhs %d, at least 1", fn, n_rhs);
  NGPDE_REQUIRE(cg_sizes_ok(n, n_graphs, n_rhs), NGPDE_ERR_INVALID_ARGUMENT, "%s: %d graphs x %d columns are more pairs than the iteration holds",
                fn, n_graphs, n_rhs);
  NGPDE_REQUIRE(n_graphs == 1 || graph_of, NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of is NULL with %d graphs", fn, n_graphs);
  NGPDE_REQUIRE(std::isfinite(shift) && std::isfinite(scale), NGPDE_ERR_INVALID_ARGUMENT, "%s: shift %g / scale %g is not finite", fn,
                (double)shift, (double)scale);
  NGPDE_REQUIRE(precondition == NGPDE_CG_NONE || precondition == NGPDE_CG_JACOBI, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: precondition %d is neither NGPDE_CG_NONE nor NGPDE_CG_JACOBI", fn, precondition);
  NGPDE_REQUIRE(rtol >= 0.f && std::isfinite(rtol), NGPDE_ERR_INVALID_ARGUMENT, "%s: rtol %g is not a finite number >= 0", fn, (double)rtol);
  NGPDE_REQUIRE(atol >= 0.f && std::isfinite(atol), NGPDE_ERR_INVALID_ARGUMENT, "%s: atol %g is not a finite number >= 0", fn, (double)atol);
  NGPDE_REQUIRE(max_iter >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: max_iter %d is negative", fn, max_iter);
  NGPDE_REQUIRE(check_every >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: check_every %d is negative", fn, check_every);
  NGPDE_REQUIRE(row_ptr && (nnz == 0 || (cols && vals)), NGPDE_ERR_INVALID_ARGUMENT, "%s: row_ptr / cols / vals is NULL", fn);
  NGPDE_REQUIRE(n == 0 || (B && X), NGPDE_ERR_INVALID_ARGUMENT, "%s: B / X is NULL", fn);
  NGPDE_REQUIRE(status_out && iterations_out && residual_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: an info array is NULL", fn);
  if (int32_t st = check_workspace(fn, workspace, workspace_bytes, cg_bytes(n, n_graphs, n_rhs), 1)) return st;
  Workspace w(workspace);
  CgView V;
  cg_layout(w, n, n_graphs, n_rhs, V);
  V.max_iter = max_iter;
  V.row_ptr = row_ptr, V.cols = cols, V.graph_of = graph_of, V.vals = vals;
  V.shift = shift, V.scale = scale, V.rtol = rtol, V.atol = atol;
  V.X = X, V.residual = residual_out, V.status = status_out, V.iterations = iterations_out;

  // ---- setup: the lists checked, the graphs' ranges and chunk counts, the diagonal, the pairs' state
  NGPDE_HIP_CHECK(hipMemsetAsync(V.words, 0, kCgWords * sizeof(int32_t), stream));
  hipLaunchKernelGGL(cg_check_kernel, dim3(blocks_for(std::max<int64_t>(std::max(n, nnz), 1))), dim3(kB), 0, stream, n, nnz, row_ptr, cols, n_graphs,
                     graph_of, V.words);
  NGPDE_LAUNCH_CHECK("cg_check_kernel");
  hipLaunchKernelGGL(cg_setup_kernel, dim3(blocks_for(std::max<int64_t>(n, (int64_t)n_graphs + 1))), dim3(kB), 0, stream, V,
                     precondition == NGPDE_CG_JACOBI ? 1 : 0);
  NGPDE_LAUNCH_CHECK("cg_setup_kernel");
  hipLaunchKernelGGL(cg_pairs_kernel, dim3(1), dim3(kBlock), 0, stream, V);
  NGPDE_LAUNCH_CHECK("cg_pairs_kernel");
  const dim3 grid((unsigned)V.max_chunks, (unsigned)V.n_slabs), block(kBlock);
  if (n > 0) {
    // ---- step 0: r = b - A x0, z, rho, the stop of a start that already solves the system, p = z
    hipLaunchKernelGGL(cg_load_kernel, grid, block, 0, stream, V, B, x0);
    NGPDE_LAUNCH_CHECK("cg_load_kernel");
    if (x0) {
      hipLaunchKernelGGL(cg_product_kernel, grid, block, 0, stream, V, 0, (const float *)V.x);
      NGPDE_LAUNCH_CHECK("cg_product_kernel");
    }
    hipLaunchKernelGGL(cg_update_kernel, grid, block, 0, stream, V, 0, x0 ? mResidual : mStart);
    NGPDE_LAUNCH_CHECK("cg_update_kernel");
    hipLaunchKernelGGL(cg_direction_kernel, grid, block, 0, stream, V, 0);
    NGPDE_LAUNCH_CHECK("cg_direction_kernel");
  }
  int32_t h[kCgWords] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (check_every > 0) {
    NGPDE_HIP_CHECK(hipMemcpyAsync(h, V.words, sizeof(h), hipMemcpyDeviceToHost, stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    NGPDE_REQUIRE(!h[fCsr], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: a column or a row pointer lies outside the %lld x %lld matrix",
                  fn, (long long)n, (long long)n);
    NGPDE_REQUIRE(!h[fBad], NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of holds an id outside 0:%d", fn, n_graphs - 1);
    NGPDE_REQUIRE(!h[fOrder], NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of is not non-decreasing: the nodes of a graph must be contiguous", fn);
    NGPDE_REQUIRE(!h[fDiag], NGPDE_ERR_INVALID_ARGUMENT,
                  "%s: the diagonal shift + scale * M[i][i] of node %lld is not positive: the Jacobi preconditioner divides by it (precondition "
                  "none, or another shift)",
                  fn, (long long)(n - h[fDiag]));
    if (h[fRunning] == 0) return NGPDE_OK;
  }
  // ---- the steps: three launches each; a stopped pair is frozen on the device
  for (int it = 1; n > 0 && it <= max_iter; ++it) {
    hipLaunchKernelGGL(cg_product_kernel, grid, block, 0, stream, V, it, (const float *)V.p);
    NGPDE_LAUNCH_CHECK("cg_product_kernel");
    hipLaunchKernelGGL(cg_update_kernel, grid, block, 0, stream, V, it, (int)mStep);
    NGPDE_LAUNCH_CHECK("cg_update_kernel");
    hipLaunchKernelGGL(cg_direction_kernel, grid, block, 0, stream, V, it);
    NGPDE_LAUNCH_CHECK("cg_direction_kernel");
    if (check_every > 0 && it % check_every == 0 && it < max_iter) {
      int32_t running = 0;
      NGPDE_HIP_CHECK(hipMemcpyAsync(&running, V.words + fRunning, sizeof(running), hipMemcpyDeviceToHost, stream));
      NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
      if (running == 0) break;
    }
  }
  return NGPDE_OK;
}

}  // extern "C"
