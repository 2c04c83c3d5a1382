// neighbors.hip -- neighbour search on the device: the COO lists GNNGraphs.radius_graph / knn_graph produce on the host
// with NearestNeighbors.jl trees ([UPSTREAM] GraphNeuralNetworks.jl, re-exported at /root/reference/src/NeuralGraphPDE.jl:4),
// and a space-filling-curve node order that serves as the locality schedule of a never-seen point-cloud graph without a
// host traversal.
//
// Semantics (the tests compare bit for bit with a brute-force float32 restatement):
//   d2(i, j) = sum over the coordinates, in order, of (p_i - p_j)^2, every operation rounded to float (no fused
//   multiply-add: the library is compiled with -ffp-contract=off); radius graph: j is a neighbour of i iff
//   d2 <= r*r (float product) and, with graph_id, both belong to the same graph; k-NN: the k smallest (d2, j) pairs.
//   dir = :in (default): neighbours are SOURCES, i the target; the list is ordered by i, neighbours ascending by index
//   (radius) or by (d2, index) (k-NN).  The reference's tree searches return an implementation-defined order of the
//   same edge set.
//   The float rule holds at every magnitude: any call with finite coordinates and a valid r or k returns the brute-force
//   list bit for bit or is refused by name before the grid is sized.
//     r*r = inf (r = inf, or a finite r above 1.8e19): d2 <= inf accepts every pair of a graph; the grid is one cell.
//     squares that underflow (coordinates or r below ~1e-19): df*df and r*r round to multiples of 2^-149, d2 <= r*r then
//       accepts pairs further apart than r (all of them where both sides round to 0); the cell edge never goes below
//       kMinCell = 2^-69, which covers every such pair (derivation above kMinCell in neighbor_grid.h).
//     a coordinate whose span hi - lo is not finite (e.g. -3e38 .. 3e38): refused, NGPDE_ERR_INVALID_ARGUMENT, like a
//       non-finite coordinate; so is the space-filling-curve order.  That order treats an extent below kMinCell as 0.
// Method: uniform cell grid over the bounding box (cell >= 1.01 r, so the 3^dim block around a point's cell holds its
// neighbours), points sorted by (graph, cell) with a stable radix sort, one thread per point walking contiguous cell
// ranges; counts -> scan -> fill -> per-row sort.  k-NN walks rings of cells until the k-th distance is proven.
// The grid's sizing, cell_of and the curve quantisation are host code in neighbor_grid.h, checked on the host by
// tests/host/neighbor_grid_check.cpp.
// Two-set search (ngpde_knn_query, ngpde_radius_query; include/ngpde_interp.h): the same rule and the same kernels with a point of a
// SECOND set as the searcher (template parameter QUERY, struct Searcher).  The grid is the data points'; a query's cell is clamped
// to it (cell_of_query; neighbor_grid.h's header says why covering and the ring bound survive that), results are indexed by the
// caller's query order, which is also the order the queries are processed in (a regular target grid is already coherent).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/ngpde_interp.h"
#include "common.h"
#include "device_scratch.h"
#include "neighbor_cells.h"
#include "neighbor_grid.h"

namespace ngpde {
namespace {

__device__ __forceinline__ unsigned ordered_bits(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
inline float from_ordered_bits(unsigned u) {
  const unsigned b = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

// box[0..2] = min, box[3..5] = max (ordered-bit encoding); also checks graph ids
__global__ void bbox_kernel(int64_t n, int dim, const float *__restrict__ pts, const int32_t *__restrict__ gid, int id_base,
                            int n_graphs, unsigned *__restrict__ box, int *__restrict__ bad_id) {
  unsigned mn[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, mx[3] = {0u, 0u, 0u};
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    for (int d = 0; d < dim; ++d) {
      const unsigned u = ordered_bits(pts[i * dim + d]);
      mn[d] = min(mn[d], u);
      mx[d] = max(mx[d], u);
    }
    if (gid) {
      const int g = gid[i] - id_base;
      bad |= (g < 0 || g >= n_graphs);
    }
  }
  for (int d = 0; d < dim; ++d) {
    for (int off = 32; off > 0; off >>= 1) {
      mn[d] = min(mn[d], (unsigned)__shfl_xor((int)mn[d], off));
      mx[d] = max(mx[d], (unsigned)__shfl_xor((int)mx[d], off));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(&box[d], mn[d]);
      atomicMax(&box[3 + d], mx[d]);
    }
  }
  if (bad) atomicOr(bad_id, 1);
}

template <int DIM>
__global__ void cell_key_kernel(int64_t n, Grid g, const float *__restrict__ pts, const int32_t *__restrict__ gid, int id_base,
                                unsigned *__restrict__ key, int32_t *__restrict__ iota) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float p[DIM];
  int c[DIM];
#pragma unroll
  for (int d = 0; d < DIM; ++d) p[d] = pts[i * DIM + d];
  cell_of<DIM>(g, p, c);
  const int graph = gid ? gid[i] - id_base : 0;
  key[i] = (unsigned)graph * (unsigned)g.cells + (unsigned)linear_cell<DIM>(g, c);
  iota[i] = (int32_t)i;
}

template <int DIM>
__global__ void gather_points_kernel(int64_t n, const float *__restrict__ pts, const int32_t *__restrict__ idx,
                                     float *__restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const int64_t i = idx[p];
#pragma unroll
  for (int d = 0; d < DIM; ++d) out[p * DIM + d] = pts[i * DIM + d];
}

// start[c] = first sorted position whose key is >= c   (c = 0 .. total)
__global__ void cell_start_kernel(int64_t total, int64_t n, const unsigned *__restrict__ key_sorted, int32_t *__restrict__ start) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > total) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)key_sorted[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  start[c] = (int32_t)lo;
}

template <int DIM>
__device__ __forceinline__ float dist2(const float *a, const float *b) {
  float d2 = 0.f;
#pragma unroll
  for (int d = 0; d < DIM; ++d) {
    const float df = a[d] - b[d];
    d2 = d2 + df * df;     // not contracted: -ffp-contract=off
  }
  return d2;
}

// Visits every sorted position q in the 3^DIM block of cells around point p's cell (the cells along the last
// coordinate are contiguous in key order: one range per row of the block).
template <int DIM, class F>
__device__ __forceinline__ void for_block(const Grid &g, int graph, const int *c, const int32_t *__restrict__ start, F &&f) {
  const int base = graph * g.cells;
  const int l0 = max(c[DIM - 1] - 1, 0), l1 = min(c[DIM - 1] + 1, g.nc[DIM - 1] - 1);
  if constexpr (DIM == 1) {
    for (int q = start[base + l0], e = start[base + l1 + 1]; q < e; ++q) f(q);
  } else if constexpr (DIM == 2) {
    for (int a = max(c[0] - 1, 0); a <= min(c[0] + 1, g.nc[0] - 1); ++a) {
      const int row = base + a * g.nc[1];
      for (int q = start[row + l0], e = start[row + l1 + 1]; q < e; ++q) f(q);
    }
  } else {
    for (int a = max(c[0] - 1, 0); a <= min(c[0] + 1, g.nc[0] - 1); ++a)
      for (int b = max(c[1] - 1, 0); b <= min(c[1] + 1, g.nc[1] - 1); ++b) {
        const int row = base + (a * g.nc[1] + b) * g.nc[2];
        for (int q = start[row + l0], e = start[row + l1 + 1]; q < e; ++q) f(q);
      }
  }
}

// Who searches the sorted points.  QUERY = false: one of them, p its sorted position (the one-set graphs).  QUERY = true: point p of a
// second set, in the caller's order (`from` = the queries, qgid their graph ids or NULL): its cell is clamped to the data's grid,
// its graph is its own indicator's, and no sorted position is "itself".
template <int DIM, bool QUERY>
struct Searcher {
  float a[DIM];
  int c[DIM];
  int graph;
  int32_t i;   // the row the results belong to: the point's original index, or the query's
  __device__ __forceinline__ Searcher(int64_t p, const Grid &g, const float *__restrict__ from, const int32_t *__restrict__ sidx,
                                      const unsigned *__restrict__ key_sorted, const int32_t *__restrict__ qgid, int id_base) {
#pragma unroll
    for (int d = 0; d < DIM; ++d) a[d] = from[p * DIM + d];
    if constexpr (QUERY) {
      cell_of_query<DIM>(g, a, c);
      graph = qgid ? qgid[p] - id_base : 0;
      i = (int32_t)p;
    } else {
      cell_of<DIM>(g, a, c);
      graph = (int)(key_sorted[p] / (unsigned)g.cells);
      i = sidx[p];
    }
  }
};

// FILL = false: deg[i] = number of neighbours; FILL = true: writes them (unsorted) at rowptr[i].  n = the number of searchers
// (`from`: the sorted points themselves, or the queries with their graph ids qgid); QUERY rows have no `self` list.
template <int DIM, bool FILL, bool QUERY>
__global__ void radius_kernel(int64_t n, Grid g, float r2, int self_loops, int out_base, const float *__restrict__ spts,
                              const int32_t *__restrict__ sidx, const unsigned *__restrict__ key_sorted,
                              const int32_t *__restrict__ start, int32_t *__restrict__ deg, unsigned long long *__restrict__ total,
                              const int32_t *__restrict__ rowptr, int32_t *__restrict__ nbr, int32_t *__restrict__ self,
                              const float *__restrict__ from, const int32_t *__restrict__ qgid, int id_base) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int cnt = 0;
  if (p < n) {
    const Searcher<DIM, QUERY> me(p, g, from, sidx, key_sorted, qgid, id_base);
    const float *a = me.a;
    const int32_t i = me.i;
    int32_t w = FILL ? rowptr[i] : 0;
    for_block<DIM>(g, me.graph, me.c, start, [&](int q) {
      float b[DIM];
#pragma unroll
      for (int d = 0; d < DIM; ++d) b[d] = spts[(int64_t)q * DIM + d];
      const bool hit = dist2<DIM>(a, b) <= r2 && (QUERY || self_loops || q != (int)p);
      if (hit) {
        if constexpr (FILL) {
          nbr[w] = sidx[q] + out_base;
          if constexpr (!QUERY) self[w] = i + out_base;
          ++w;
        }
        ++cnt;
      }
    });
    if constexpr (!FILL) deg[i] = cnt;
  }
  if constexpr (!FILL) {
    unsigned long long s = (unsigned long long)cnt;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(total, s);
  }
}

// k nearest (d2, index) pairs per point; the running list lives in LDS, one column per thread:
// list entry m of thread l at [m * 64 + l]
constexpr int kKnnThreads = 64;
// QUERY = false writes the COO lists s_out / t_out and ORs 1 into *short_rows; QUERY = true writes s_out = idx [n][k] and, where
// given, d2_out [n][k] (t_out unused) and keeps the smallest graph of a short row in *short_rows (atomicMin).
template <int DIM, bool QUERY>
__global__ void knn_kernel(int64_t n, Grid g, int k, int self_loops, int out_base, int dir_out, const float *__restrict__ spts,
                           const int32_t *__restrict__ sidx, const unsigned *__restrict__ key_sorted,
                           const int32_t *__restrict__ start, int32_t *__restrict__ s_out, int32_t *__restrict__ t_out,
                           int *__restrict__ short_rows, const float *__restrict__ from, const int32_t *__restrict__ qgid, int id_base,
                           float *__restrict__ d2_out) {
  extern __shared__ float knn_lds[];
  float *ld = knn_lds + threadIdx.x;                        // distances
  int *li = (int *)(knn_lds + (size_t)k * kKnnThreads) + threadIdx.x;   // original indices
  const int64_t p = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;
  if (p >= n) return;
  const Searcher<DIM, QUERY> me(p, g, from, sidx, key_sorted, qgid, id_base);
  const float *a = me.a;
  const int *c = me.c;
  const int base = me.graph * g.cells;
  const int32_t i = me.i;
  int have = 0;
  int max_ring = 0;
#pragma unroll
  for (int d = 0; d < DIM; ++d) max_ring = max(max_ring, max(c[d], g.nc[d] - 1 - c[d]));
  auto offer = [&](int q) {
    if (!QUERY && !self_loops && q == (int)p) return;
    float b[DIM];
#pragma unroll
    for (int d = 0; d < DIM; ++d) b[d] = spts[(int64_t)q * DIM + d];
    const float d2 = dist2<DIM>(a, b);
    const int j = sidx[q];
    if (have == k) {
      const float wd = ld[(k - 1) * kKnnThreads];
      const int wj = li[(k - 1) * kKnnThreads];
      if (!(d2 < wd || (d2 == wd && j < wj))) return;
    }
    int m = (have < k) ? have : k - 1;                       // slot that opens up
    while (m > 0) {
      const float pd = ld[(m - 1) * kKnnThreads];
      const int pj = li[(m - 1) * kKnnThreads];
      if (pd < d2 || (pd == d2 && pj < j)) break;
      ld[m * kKnnThreads] = pd;
      li[m * kKnnThreads] = pj;
      --m;
    }
    ld[m * kKnnThreads] = d2;
    li[m * kKnnThreads] = j;
    if (have < k) ++have;
  };
  for (int ring = 0; ring <= max_ring; ++ring) {
    // cells at Chebyshev distance exactly `ring` from the home cell
    if constexpr (DIM == 1) {
      for (int s = -1; s <= 1; s += 2) {
        const int x = c[0] + s * ring;
        if (x < 0 || x >= g.nc[0] || (ring == 0 && s > 0)) continue;
        for (int q = start[base + x], e = start[base + x + 1]; q < e; ++q) offer(q);
      }
    } else if constexpr (DIM == 2) {
      // the two end columns x = c0 -+ ring in full, then the two end cells of every column between them; a column or a row
      // outside the grid costs nothing, so a walk along a thin grid is linear in the rings, not quadratic
      auto span = [&](int x, int ya, int yb) {   // cells (x, ya..yb) clipped to the grid: one range of sorted positions
        ya = max(ya, 0);
        yb = min(yb, g.nc[1] - 1);
        if (x < 0 || x >= g.nc[0] || ya > yb) return;
        const int row = base + x * g.nc[1];
        for (int q = start[row + ya], e = start[row + yb + 1]; q < e; ++q) offer(q);
      };
      span(c[0] - ring, c[1] - ring, c[1] + ring);
      if (ring > 0) {
        span(c[0] + ring, c[1] - ring, c[1] + ring);
        const bool y_lo = c[1] - ring >= 0, y_hi = c[1] + ring < g.nc[1];
        if (y_lo || y_hi)
          for (int x = max(c[0] - ring + 1, 0); x <= min(c[0] + ring - 1, g.nc[0] - 1); ++x) {
            if (y_lo) span(x, c[1] - ring, c[1] - ring);
            if (y_hi) span(x, c[1] + ring, c[1] + ring);
          }
      }
    } else {
      // the shell by faces: |dx| = ring; |dx| < ring and |dy| = ring; |dx|, |dy| < ring and |dz| = ring.  Only faces and
      // cells inside the grid are looped over.
      auto span = [&](int x, int y, int za, int zb) {   // cells (x, y, za..zb) clipped to the grid
        za = max(za, 0);
        zb = min(zb, g.nc[2] - 1);
        if (x < 0 || x >= g.nc[0] || y < 0 || y >= g.nc[1] || za > zb) return;
        const int row = base + (x * g.nc[1] + y) * g.nc[2];
        for (int q = start[row + za], e = start[row + zb + 1]; q < e; ++q) offer(q);
      };
      if (c[0] - ring >= 0 || c[0] + ring < g.nc[0])
        for (int y = max(c[1] - ring, 0); y <= min(c[1] + ring, g.nc[1] - 1); ++y) {
          span(c[0] - ring, y, c[2] - ring, c[2] + ring);
          if (ring > 0) span(c[0] + ring, y, c[2] - ring, c[2] + ring);
        }
      if (ring > 0) {
        const int xa = max(c[0] - ring + 1, 0), xb = min(c[0] + ring - 1, g.nc[0] - 1);
        const int ya = max(c[1] - ring + 1, 0), yb = min(c[1] + ring - 1, g.nc[1] - 1);
        for (int side = -1; side <= 1; side += 2) {
          const int y = c[1] + side * ring;
          if (y >= 0 && y < g.nc[1])
            for (int x = xa; x <= xb; ++x) span(x, y, c[2] - ring, c[2] + ring);
          const int z = c[2] + side * ring;
          if (z >= 0 && z < g.nc[2])
            for (int x = xa; x <= xb; ++x)
              for (int yy = ya; yy <= yb; ++yy) span(x, yy, z, z);
        }
      }
    }
    // every unvisited point is at least ring * cell away (the point lies inside its home cell)
    if (have == k && ring > 0 && ld[(k - 1) * kKnnThreads] < ring_reach2(g, ring)) break;
  }
  if constexpr (QUERY) {
    if (have < k) atomicMin(short_rows, me.graph);
    for (int m = 0; m < k; ++m) {
      s_out[(int64_t)i * k + m] = (m < have ? li[m * kKnnThreads] : 0) + out_base;
      if (d2_out) d2_out[(int64_t)i * k + m] = m < have ? ld[m * kKnnThreads] : INFINITY;
    }
  } else {
    if (have < k) atomicOr(short_rows, 1);
    int32_t *nb = dir_out ? t_out : s_out, *own = dir_out ? s_out : t_out;
    for (int m = 0; m < k; ++m) {
      nb[(int64_t)i * k + m] = (m < have ? li[m * kKnnThreads] : i) + out_base;
      own[(int64_t)i * k + m] = i + out_base;
    }
  }
}

// ---- space-filling-curve keys ---------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned hilbert2(unsigned x, unsigned y, int bits) {   // position along the Hilbert curve
  unsigned d = 0;
  const unsigned side = 1u << bits;
  for (unsigned s = side >> 1; s > 0; s >>= 1) {
    const unsigned rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
    d += s * s * ((3u * rx) ^ ry);
    if (ry == 0) {
      if (rx == 1) {
        x = side - 1 - x;
        y = side - 1 - y;
      }
      const unsigned tmp = x;
      x = y;
      y = tmp;
    }
  }
  return d;
}

__device__ __forceinline__ unsigned spread3(unsigned v) {   // 10 bits -> every third bit
  v &= 0x3ffu;
  v = (v | (v << 16)) & 0x030000ffu;
  v = (v | (v << 8)) & 0x0300f00fu;
  v = (v | (v << 4)) & 0x030c30c3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}

template <int DIM>
__global__ void curve_key_kernel(int64_t n, Quant qz, const float *__restrict__ pts, const int32_t *__restrict__ gid, int id_base,
                                 unsigned long long *__restrict__ key, int32_t *__restrict__ iota) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned q[DIM];
  const int top = (int)((1u << qz.bits) - 1u);
#pragma unroll
  for (int d = 0; d < DIM; ++d) q[d] = (unsigned)min(top, max(0, (int)((pts[i * DIM + d] - qz.lo[d]) * qz.scale[d])));
  unsigned code;
  if constexpr (DIM == 1) code = q[0];
  else if constexpr (DIM == 2) code = hilbert2(q[0], q[1], qz.bits);
  else code = (spread3(q[0]) << 2) | (spread3(q[1]) << 1) | spread3(q[2]);
  const unsigned long long graph = gid ? (unsigned long long)(gid[i] - id_base) : 0ull;
  key[i] = (graph << 32) | code;
  iota[i] = (int32_t)i;
}

int32_t bounding_box(int64_t n, int dim, const float *pts, const int32_t *gid, int id_base, int n_graphs, hipStream_t stream,
                     Scratch &sc, float *lo, float *hi, const char *what = "points", const char *ids = "graph_indicator") {
  unsigned *box = nullptr;
  int *bad = nullptr;
  int32_t st;
  if ((st = sc.get(&box, 6)) || (st = sc.get(&bad, 1))) return st;
  const unsigned init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
  NGPDE_HIP_CHECK(hipMemcpyAsync(box, init, sizeof(init), hipMemcpyHostToDevice, stream));
  NGPDE_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int), stream));
  hipLaunchKernelGGL(bbox_kernel, dim3(std::min<unsigned>(blocks_for(n), 1024u)), dim3(kB), 0, stream, n, dim, pts, gid, id_base,
                     n_graphs, box, bad);
  NGPDE_LAUNCH_CHECK("bbox_kernel");
  unsigned h[6];
  int h_bad = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(h, box, sizeof(h), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  NGPDE_REQUIRE(!h_bad, NGPDE_ERR_INVALID_ARGUMENT, "%s holds an id outside %d:%d", ids, id_base, id_base + n_graphs - 1);
  for (int d = 0; d < 3; ++d) {
    lo[d] = d < dim ? from_ordered_bits(h[d]) : 0.f;
    hi[d] = d < dim ? from_ordered_bits(h[3 + d]) : 0.f;
    NGPDE_REQUIRE(std::isfinite(lo[d]) && std::isfinite(hi[d]), NGPDE_ERR_INVALID_ARGUMENT, "%s hold a non-finite coordinate", what);
  }
  NGPDE_REQUIRE(span_is_finite(dim, lo, hi), NGPDE_ERR_INVALID_ARGUMENT, "%s span more than the largest finite float in a coordinate",
                what);
  return NGPDE_OK;
}

struct Sorted {
  unsigned *key = nullptr;    // sorted (graph, cell) keys
  int32_t *idx = nullptr;     // original index per sorted position
  float *pts = nullptr;       // points in sorted order
  int32_t *start = nullptr;   // [total cells + 1]
};

template <int DIM>
int32_t sort_into_cells(int64_t n, const Grid &g, int n_graphs, const float *pts, const int32_t *gid, int id_base,
                        hipStream_t stream, Scratch &sc, Sorted &out) {
  const int64_t total = (int64_t)g.cells * n_graphs;
  unsigned *key = nullptr;
  int32_t *iota = nullptr;
  int32_t st;
  if ((st = sc.get(&key, (size_t)n)) || (st = sc.get(&iota, (size_t)n)) || (st = sc.get(&out.key, (size_t)n)) ||
      (st = sc.get(&out.idx, (size_t)n)) || (st = sc.get(&out.pts, (size_t)n * DIM)) || (st = sc.get(&out.start, (size_t)total + 1)))
    return st;
  hipLaunchKernelGGL(cell_key_kernel<DIM>, dim3(blocks_for(n)), dim3(kB), 0, stream, n, g, pts, gid, id_base, key, iota);
  NGPDE_LAUNCH_CHECK("cell_key_kernel");
  const unsigned end_bit = bits_for(std::max<int64_t>(total, 2));
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, key, out.key, iota, out.idx, (size_t)n, 0u, end_bit, stream);
  };
  if ((st = with_temp(sc, sort))) return st;
  hipLaunchKernelGGL(gather_points_kernel<DIM>, dim3(blocks_for(n)), dim3(kB), 0, stream, n, pts, out.idx, out.pts);
  NGPDE_LAUNCH_CHECK("gather_points_kernel");
  hipLaunchKernelGGL(cell_start_kernel, dim3(blocks_for(total + 1)), dim3(kB), 0, stream, total, n, out.key, out.start);
  NGPDE_LAUNCH_CHECK("cell_start_kernel");
  return NGPDE_OK;
}

template <int DIM>
int32_t radius_graph_impl(int64_t n, const float *pts, float r, const int32_t *gid, int n_graphs, int id_base, int self_loops,
                          int dir_out, int out_base, int64_t capacity, int32_t *s, int32_t *t, int64_t *n_edges,
                          hipStream_t stream) {
  Scratch sc;
  float lo[3], hi[3];
  int32_t st;
  if ((st = bounding_box(n, DIM, pts, gid, id_base, n_graphs, stream, sc, lo, hi))) return st;
  const Grid g = make_grid(DIM, lo, hi, radius_want(r), cell_budget(n), n_graphs);
  Sorted so;
  if ((st = sort_into_cells<DIM>(n, g, n_graphs, pts, gid, id_base, stream, sc, so))) return st;
  int32_t *deg = nullptr, *rowptr = nullptr;
  unsigned long long *total = nullptr;
  if ((st = sc.get(&deg, (size_t)n + 1)) || (st = sc.get(&rowptr, (size_t)n + 1)) || (st = sc.get(&total, 1))) return st;
  NGPDE_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(unsigned long long), stream));
  NGPDE_HIP_CHECK(hipMemsetAsync(deg, 0, ((size_t)n + 1) * sizeof(int32_t), stream));
  const float r2 = r * r;
  hipLaunchKernelGGL((radius_kernel<DIM, false, false>), dim3(blocks_for(n)), dim3(kB), 0, stream, n, g, r2, self_loops, out_base, so.pts,
                     so.idx, so.key, so.start, deg, total, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr,
                     (const float *)so.pts, (const int32_t *)nullptr, 0);
  NGPDE_LAUNCH_CHECK("radius_kernel(count)");
  unsigned long long h_total = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_total, total, sizeof(h_total), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  *n_edges = (int64_t)h_total;
  if (!s && !t) return NGPDE_OK;   // count only
  NGPDE_REQUIRE(h_total <= 0x7fffffffull, NGPDE_ERR_UNSUPPORTED, "radius graph has %llu edges: more than int32 positions", h_total);
  NGPDE_REQUIRE((int64_t)h_total <= capacity, NGPDE_ERR_INVALID_ARGUMENT,
                "radius graph has %llu edges, the output arrays hold %lld", h_total, (long long)capacity);
  if (h_total == 0) return NGPDE_OK;
  auto scan = [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, deg, rowptr, 0, (size_t)n + 1, rocprim::plus<int32_t>(), stream);
  };
  if ((st = with_temp(sc, scan))) return st;
  int32_t *nbr = nullptr;
  if ((st = sc.get(&nbr, (size_t)h_total))) return st;
  int32_t *nb_out = dir_out ? t : s, *me_out = dir_out ? s : t;
  hipLaunchKernelGGL((radius_kernel<DIM, true, false>), dim3(blocks_for(n)), dim3(kB), 0, stream, n, g, r2, self_loops, out_base, so.pts,
                     so.idx, so.key, so.start, (int32_t *)nullptr, (unsigned long long *)nullptr, (const int32_t *)rowptr, nbr, me_out,
                     (const float *)so.pts, (const int32_t *)nullptr, 0);
  NGPDE_LAUNCH_CHECK("radius_kernel(fill)");
  const unsigned end_bit = bits_for(std::max<int64_t>(n + out_base + 1, 2));
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::segmented_radix_sort_keys(tmp, bytes, nbr, nb_out, (unsigned)h_total, (unsigned)n, rowptr, rowptr + 1, 0u, end_bit, stream);
  };
  if ((st = with_temp(sc, sort))) return st;
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  return NGPDE_OK;
}

template <int DIM>
int32_t knn_graph_impl(int64_t n, const float *pts, int k, const int32_t *gid, int n_graphs, int id_base, int self_loops, int dir_out,
                       int out_base, int32_t *s, int32_t *t, hipStream_t stream) {
  Scratch sc;
  float lo[3], hi[3];
  int32_t st;
  if ((st = bounding_box(n, DIM, pts, gid, id_base, n_graphs, stream, sc, lo, hi))) return st;
  const float want = knn_want(DIM, lo, hi, n, n_graphs, k);
  const Grid g = make_grid(DIM, lo, hi, want, cell_budget(n), n_graphs);
  Sorted so;
  if ((st = sort_into_cells<DIM>(n, g, n_graphs, pts, gid, id_base, stream, sc, so))) return st;
  int *short_rows = nullptr;
  if ((st = sc.get(&short_rows, 1))) return st;
  NGPDE_HIP_CHECK(hipMemsetAsync(short_rows, 0, sizeof(int), stream));
  const size_t lds = (size_t)k * kKnnThreads * 8;
  NGPDE_HIP_CHECK(hipFuncSetAttribute((const void *)knn_kernel<DIM, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((knn_kernel<DIM, false>), dim3((unsigned)((n + kKnnThreads - 1) / kKnnThreads)), dim3(kKnnThreads), lds, stream, n, g, k,
                     self_loops, out_base, dir_out, so.pts, so.idx, so.key, so.start, s, t, short_rows, (const float *)so.pts,
                     (const int32_t *)nullptr, 0, (float *)nullptr);
  NGPDE_LAUNCH_CHECK("knn_kernel");
  int h_short = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_short, short_rows, sizeof(int), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  NGPDE_REQUIRE(!h_short, NGPDE_ERR_INVALID_ARGUMENT, "knn_graph: a graph has fewer than k%s points", self_loops ? "" : " + 1");
  return NGPDE_OK;
}

template <int DIM>
int32_t spatial_order_impl(int64_t n, const float *pts, const int32_t *gid, int n_graphs, int id_base, int32_t *order,
                           hipStream_t stream) {
  Scratch sc;
  float lo[3], hi[3];
  int32_t st;
  if ((st = bounding_box(n, DIM, pts, gid, id_base, n_graphs, stream, sc, lo, hi))) return st;
  const Quant qz = make_quant(DIM, lo, hi);
  unsigned long long *key = nullptr, *key_sorted = nullptr;
  int32_t *iota = nullptr;
  if ((st = sc.get(&key, (size_t)n)) || (st = sc.get(&key_sorted, (size_t)n)) || (st = sc.get(&iota, (size_t)n))) return st;
  hipLaunchKernelGGL(curve_key_kernel<DIM>, dim3(blocks_for(n)), dim3(kB), 0, stream, n, qz, pts, gid, id_base, key, iota);
  NGPDE_LAUNCH_CHECK("curve_key_kernel");
  const unsigned end_bit = 32u + bits_for(std::max<int64_t>(n_graphs, 2));
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, key, key_sorted, iota, order, (size_t)n, 0u, end_bit, stream);
  };
  if ((st = with_temp(sc, sort))) return st;
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  return NGPDE_OK;
}

// ---- two-set search: the data points are boxed, gridded and sorted as above, the queries are boxed for their checks alone ------
// boxes of both sets with their id and finiteness checks; the span that must be finite is the union's (q - lo is formed in float)
int32_t two_boxes(int64_t n, int64_t m, int dim, const float *pts, const float *qs, const int32_t *gid, const int32_t *qgid, int id_base,
                  int n_graphs, hipStream_t stream, Scratch &sc, float *lo, float *hi) {
  float qlo[3], qhi[3], ulo[3], uhi[3];
  int32_t st;
  if ((st = bounding_box(n, dim, pts, gid, id_base, n_graphs, stream, sc, lo, hi, "points", "point_graph_id")) ||
      (st = bounding_box(m, dim, qs, qgid, id_base, n_graphs, stream, sc, qlo, qhi, "queries", "query_graph_id")))
    return st;
  for (int d = 0; d < 3; ++d) {
    ulo[d] = std::min(lo[d], qlo[d]);
    uhi[d] = std::max(hi[d], qhi[d]);
  }
  NGPDE_REQUIRE(span_is_finite(dim, ulo, uhi), NGPDE_ERR_INVALID_ARGUMENT,
                "points and queries together span more than the largest finite float in a coordinate");
  return NGPDE_OK;
}

constexpr int kNoShortGraph = 0x7f7f7f7f;   // (what hipMemset writes byte by byte; above every graph number)

template <int DIM>
int32_t knn_query_impl(int64_t n, int64_t m, const float *pts, const float *qs, int k, const int32_t *gid, const int32_t *qgid,
                       int n_graphs, int id_base, int out_base, int32_t *idx, float *d2, hipStream_t stream) {
  Scratch sc;
  float lo[3], hi[3];
  int32_t st;
  if ((st = two_boxes(n, m, DIM, pts, qs, gid, qgid, id_base, n_graphs, stream, sc, lo, hi))) return st;
  const float want = knn_want(DIM, lo, hi, n, n_graphs, k);
  const Grid g = make_grid(DIM, lo, hi, want, cell_budget(n), n_graphs);
  Sorted so;
  if ((st = sort_into_cells<DIM>(n, g, n_graphs, pts, gid, id_base, stream, sc, so))) return st;
  int *short_graph = nullptr;
  if ((st = sc.get(&short_graph, 1))) return st;
  NGPDE_HIP_CHECK(hipMemsetAsync(short_graph, 0x7f, sizeof(int), stream));
  const size_t lds = (size_t)k * kKnnThreads * 8;
  NGPDE_HIP_CHECK(hipFuncSetAttribute((const void *)knn_kernel<DIM, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((knn_kernel<DIM, true>), dim3((unsigned)((m + kKnnThreads - 1) / kKnnThreads)), dim3(kKnnThreads), lds, stream, m, g, k,
                     1, out_base, 0, so.pts, so.idx, so.key, so.start, idx, (int32_t *)nullptr, short_graph, qs, qgid, id_base, d2);
  NGPDE_LAUNCH_CHECK("knn_kernel(query)");
  int h_short = kNoShortGraph;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_short, short_graph, sizeof(int), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  if (h_short != kNoShortGraph) {
    int32_t bounds[2] = {0, 0};   // the graph's points are the sorted positions start[graph * cells] .. start[(graph + 1) * cells]
    NGPDE_HIP_CHECK(hipMemcpy(&bounds[0], so.start + (size_t)h_short * g.cells, sizeof(int32_t), hipMemcpyDeviceToHost));
    NGPDE_HIP_CHECK(hipMemcpy(&bounds[1], so.start + ((size_t)h_short + 1) * g.cells, sizeof(int32_t), hipMemcpyDeviceToHost));
    return fail(NGPDE_ERR_INVALID_ARGUMENT, "knn_query: graph %d has queries and %d points, fewer than k = %d", h_short + id_base,
                bounds[1] - bounds[0], k);
  }
  return NGPDE_OK;
}

template <int DIM>
int32_t radius_query_impl(int64_t n, int64_t m, const float *pts, const float *qs, float r, const int32_t *gid, const int32_t *qgid,
                          int n_graphs, int id_base, int out_base, int64_t capacity, int32_t *ptr, int32_t *nbr_out, int64_t *n_found,
                          hipStream_t stream) {
  Scratch sc;
  float lo[3], hi[3];
  int32_t st;
  if ((st = two_boxes(n, m, DIM, pts, qs, gid, qgid, id_base, n_graphs, stream, sc, lo, hi))) return st;
  const Grid g = make_grid(DIM, lo, hi, radius_want(r), cell_budget(n), n_graphs);
  Sorted so;
  if ((st = sort_into_cells<DIM>(n, g, n_graphs, pts, gid, id_base, stream, sc, so))) return st;
  int32_t *deg = nullptr;
  unsigned long long *total = nullptr;
  if ((st = sc.get(&deg, (size_t)m + 1)) || (st = sc.get(&total, 1))) return st;
  NGPDE_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(unsigned long long), stream));
  NGPDE_HIP_CHECK(hipMemsetAsync(deg, 0, ((size_t)m + 1) * sizeof(int32_t), stream));
  const float r2 = r * r;
  hipLaunchKernelGGL((radius_kernel<DIM, false, true>), dim3(blocks_for(m)), dim3(kB), 0, stream, m, g, r2, 1, out_base, so.pts, so.idx,
                     so.key, so.start, deg, total, (const int32_t *)nullptr, (int32_t *)nullptr, (int32_t *)nullptr, qs, qgid, id_base);
  NGPDE_LAUNCH_CHECK("radius_kernel(query count)");
  unsigned long long h_total = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_total, total, sizeof(h_total), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  *n_found = (int64_t)h_total;
  if (!nbr_out) return NGPDE_OK;   // count only
  NGPDE_REQUIRE(h_total <= 0x7fffffffull, NGPDE_ERR_UNSUPPORTED, "radius_query found %llu pairs: more than int32 positions", h_total);
  NGPDE_REQUIRE((int64_t)h_total <= capacity, NGPDE_ERR_INVALID_ARGUMENT, "radius_query found %llu pairs, the output array holds %lld",
                h_total, (long long)capacity);
  auto scan = [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, deg, ptr, 0, (size_t)m + 1, rocprim::plus<int32_t>(), stream);
  };
  if ((st = with_temp(sc, scan))) return st;
  if (h_total > 0) {
    int32_t *nbr = nullptr;
    if ((st = sc.get(&nbr, (size_t)h_total))) return st;
    hipLaunchKernelGGL((radius_kernel<DIM, true, true>), dim3(blocks_for(m)), dim3(kB), 0, stream, m, g, r2, 1, out_base, so.pts, so.idx,
                       so.key, so.start, (int32_t *)nullptr, (unsigned long long *)nullptr, (const int32_t *)ptr, nbr, (int32_t *)nullptr,
                       qs, qgid, id_base);
    NGPDE_LAUNCH_CHECK("radius_kernel(query fill)");
    const unsigned end_bit = bits_for(std::max<int64_t>(n + out_base + 1, 2));
    auto sort = [&](void *tmp, size_t &bytes) {
      return rocprim::segmented_radix_sort_keys(tmp, bytes, nbr, nbr_out, (unsigned)h_total, (unsigned)m, ptr, ptr + 1, 0u, end_bit, stream);
    };
    if ((st = with_temp(sc, sort))) return st;
  }
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  return NGPDE_OK;
}

int32_t check_query(const char *fn, int64_t n, int64_t m, int32_t dim, const float *pts, const float *qs, const int32_t *gid,
                    const int32_t *qgid, int32_t n_graphs) {
  NGPDE_REQUIRE(n >= 0 && n <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: number of points %lld outside 0:2^31-1", fn, (long long)n);
  NGPDE_REQUIRE(m >= 0 && m <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: number of queries %lld outside 0:2^31-1", fn, (long long)m);
  NGPDE_REQUIRE(dim >= 1 && dim <= 3, NGPDE_ERR_UNSUPPORTED, "%s: neighbour search supports 1, 2 or 3 coordinates, got %d", fn, dim);
  NGPDE_REQUIRE(n == 0 || pts != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: points is NULL", fn);
  NGPDE_REQUIRE(m == 0 || qs != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: queries is NULL", fn);
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_graphs must be >= 1", fn);
  NGPDE_REQUIRE((gid != nullptr || n == 0) && (qgid != nullptr || m == 0) || n_graphs == 1, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: n_graphs > 1 needs point_graph_id and query_graph_id", fn);
  return NGPDE_OK;
}

int32_t check_common(int64_t n, int32_t dim, const float *pts, const int32_t *gid, int32_t n_graphs) {
  NGPDE_REQUIRE(n >= 0 && n <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "number of points %lld outside 0:2^31-1", (long long)n);
  NGPDE_REQUIRE(dim >= 1 && dim <= 3, NGPDE_ERR_UNSUPPORTED, "neighbour search supports 1, 2 or 3 coordinates, got %d", dim);
  NGPDE_REQUIRE(n == 0 || pts != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "points is NULL");
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "n_graphs must be >= 1");
  NGPDE_REQUIRE(gid != nullptr || n_graphs == 1, NGPDE_ERR_INVALID_ARGUMENT, "n_graphs > 1 needs a graph_indicator");
  return NGPDE_OK;
}

}  // namespace

// (neighbor_cells.h) the sorted grid for delaunay.hip
int32_t point_cells_2d(int64_t n, const float *pts, const int32_t *gid, int n_graphs, int id_base, int k, hipStream_t stream,
                       std::vector<void *> &owned, Grid *g, PointCells *out) {
  Scratch sc;
  float lo[3], hi[3];
  Sorted so;
  int32_t st = bounding_box(n, 2, pts, gid, id_base, n_graphs, stream, sc, lo, hi);
  if (!st) {
    *g = make_grid(2, lo, hi, knn_want(2, lo, hi, n, n_graphs, k), cell_budget(n), n_graphs);
    st = sort_into_cells<2>(n, *g, n_graphs, pts, gid, id_base, stream, sc, so);
  }
  if (st) return st;   // (sc frees what it holds)
  *out = PointCells{so.key, so.idx, so.pts, so.start};
  owned.insert(owned.end(), sc.ptrs.begin(), sc.ptrs.end());
  sc.ptrs.clear();
  return NGPDE_OK;
}

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_radius_graph(int64_t n, int32_t dim, const float *points, float r, const int32_t *graph_id, int32_t n_graphs,
                           int32_t id_base, int32_t self_loops, int32_t dir_out, int32_t index_base, int64_t capacity, int32_t *s,
                           int32_t *t, int64_t *n_edges, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_common(n, dim, points, graph_id, n_graphs);
  if (st) return st;
  NGPDE_REQUIRE(n_edges != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "n_edges is NULL");
  NGPDE_REQUIRE(r >= 0.f, NGPDE_ERR_INVALID_ARGUMENT, "radius must be >= 0 (got %g)", (double)r);
  NGPDE_REQUIRE((s == nullptr) == (t == nullptr), NGPDE_ERR_INVALID_ARGUMENT, "s and t must both be given or both be NULL");
  *n_edges = 0;
  if (n == 0) return NGPDE_OK;
  hipStream_t hs = (hipStream_t)stream;
  switch (dim) {
    case 1: return radius_graph_impl<1>(n, points, r, graph_id, n_graphs, id_base, self_loops, dir_out, index_base, capacity, s, t, n_edges, hs);
    case 2: return radius_graph_impl<2>(n, points, r, graph_id, n_graphs, id_base, self_loops, dir_out, index_base, capacity, s, t, n_edges, hs);
    default: return radius_graph_impl<3>(n, points, r, graph_id, n_graphs, id_base, self_loops, dir_out, index_base, capacity, s, t, n_edges, hs);
  }
}

int32_t ngpde_knn_graph(int64_t n, int32_t dim, const float *points, int32_t k, const int32_t *graph_id, int32_t n_graphs,
                        int32_t id_base, int32_t self_loops, int32_t dir_out, int32_t index_base, int32_t *s, int32_t *t,
                        ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_common(n, dim, points, graph_id, n_graphs);
  if (st) return st;
  NGPDE_REQUIRE(k >= 0 && k <= NGPDE_KNN_MAX_K, NGPDE_ERR_UNSUPPORTED, "knn_graph supports 0 <= k <= %d, got %d", NGPDE_KNN_MAX_K, k);
  NGPDE_REQUIRE(n * (int64_t)k <= 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "knn graph has more than int32 positions");
  if (n == 0 || k == 0) return NGPDE_OK;
  NGPDE_REQUIRE(s != nullptr && t != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "s or t is NULL");
  NGPDE_REQUIRE(n >= (int64_t)k + (self_loops ? 0 : 1), NGPDE_ERR_INVALID_ARGUMENT, "knn_graph: a graph has fewer than k%s points",
                self_loops ? "" : " + 1");
  hipStream_t hs = (hipStream_t)stream;
  switch (dim) {
    case 1: return knn_graph_impl<1>(n, points, k, graph_id, n_graphs, id_base, self_loops, dir_out, index_base, s, t, hs);
    case 2: return knn_graph_impl<2>(n, points, k, graph_id, n_graphs, id_base, self_loops, dir_out, index_base, s, t, hs);
    default: return knn_graph_impl<3>(n, points, k, graph_id, n_graphs, id_base, self_loops, dir_out, index_base, s, t, hs);
  }
}

int32_t ngpde_spatial_order(int64_t n, int32_t dim, const float *points, const int32_t *graph_id, int32_t n_graphs, int32_t id_base,
                            int32_t *order, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_common(n, dim, points, graph_id, n_graphs);
  if (st) return st;
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(order != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "order is NULL");
  hipStream_t hs = (hipStream_t)stream;
  switch (dim) {
    case 1: return spatial_order_impl<1>(n, points, graph_id, n_graphs, id_base, order, hs);
    case 2: return spatial_order_impl<2>(n, points, graph_id, n_graphs, id_base, order, hs);
    default: return spatial_order_impl<3>(n, points, graph_id, n_graphs, id_base, order, hs);
  }
}

int32_t ngpde_knn_query(int64_t n, int64_t m, int32_t dim, const float *points, const float *queries, int32_t k,
                        const int32_t *point_graph_id, const int32_t *query_graph_id, int32_t n_graphs, int32_t id_base,
                        int32_t index_base, int32_t *idx, float *d2, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_query("knn_query", n, m, dim, points, queries, point_graph_id, query_graph_id, n_graphs);
  if (st) return st;
  NGPDE_REQUIRE(k >= 0, NGPDE_ERR_INVALID_ARGUMENT, "knn_query: k must be >= 0 (got %d)", k);
  NGPDE_REQUIRE(k <= NGPDE_KNN_MAX_K, NGPDE_ERR_UNSUPPORTED, "knn_query supports k <= %d, got %d", NGPDE_KNN_MAX_K, k);
  NGPDE_REQUIRE(m * (int64_t)k <= 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "knn_query: more than int32 positions");
  if (m == 0 || k == 0) return NGPDE_OK;
  NGPDE_REQUIRE(idx != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "knn_query: idx is NULL");
  NGPDE_REQUIRE(n >= (int64_t)k, NGPDE_ERR_INVALID_ARGUMENT, "knn_query: %lld points in all, fewer than k = %d", (long long)n, k);
  hipStream_t hs = (hipStream_t)stream;
  switch (dim) {
    case 1: return knn_query_impl<1>(n, m, points, queries, k, point_graph_id, query_graph_id, n_graphs, id_base, index_base, idx, d2, hs);
    case 2: return knn_query_impl<2>(n, m, points, queries, k, point_graph_id, query_graph_id, n_graphs, id_base, index_base, idx, d2, hs);
    default: return knn_query_impl<3>(n, m, points, queries, k, point_graph_id, query_graph_id, n_graphs, id_base, index_base, idx, d2, hs);
  }
}

int32_t ngpde_radius_query(int64_t n, int64_t m, int32_t dim, const float *points, const float *queries, float r,
                           const int32_t *point_graph_id, const int32_t *query_graph_id, int32_t n_graphs, int32_t id_base,
                           int32_t index_base, int64_t capacity, int32_t *ptr, int32_t *nbr, int64_t *n_found, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_query("radius_query", n, m, dim, points, queries, point_graph_id, query_graph_id, n_graphs);
  if (st) return st;
  NGPDE_REQUIRE(n_found != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "radius_query: n_found is NULL");
  NGPDE_REQUIRE(r >= 0.f, NGPDE_ERR_INVALID_ARGUMENT, "radius_query: radius must be >= 0 (got %g)", (double)r);
  NGPDE_REQUIRE(nbr == nullptr || (ptr != nullptr && capacity >= 0), NGPDE_ERR_INVALID_ARGUMENT,
                "radius_query: a fill call needs ptr and a capacity >= 0");
  *n_found = 0;
  hipStream_t hs = (hipStream_t)stream;
  if (n == 0 || m == 0) {   // nothing to find: every row is empty
    if (nbr) {
      NGPDE_HIP_CHECK(hipMemsetAsync(ptr, 0, ((size_t)m + 1) * sizeof(int32_t), hs));
      NGPDE_HIP_CHECK(hipStreamSynchronize(hs));
    }
    return NGPDE_OK;
  }
  switch (dim) {
    case 1: return radius_query_impl<1>(n, m, points, queries, r, point_graph_id, query_graph_id, n_graphs, id_base, index_base, capacity, ptr, nbr, n_found, hs);
    case 2: return radius_query_impl<2>(n, m, points, queries, r, point_graph_id, query_graph_id, n_graphs, id_base, index_base, capacity, ptr, nbr, n_found, hs);
    default: return radius_query_impl<3>(n, m, points, queries, r, point_graph_id, query_graph_id, n_graphs, id_base, index_base, capacity, ptr, nbr, n_found, hs);
  }
}

}  // extern "C"
