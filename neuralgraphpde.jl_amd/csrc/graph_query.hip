// graph_query.hip -- neighbourhood queries and random-walk encodings on a COO list that lives in HBM (include/ngpde.h, "graph queries
// by node and by pair"): has_edge, adjacency_list / neighbors, intersect and random_walk_pe of the GNNGraphs re-export
// (src/NeuralGraphPDE.jl:4 of the reference).  The lookups a script does between radius_graph, sample_neighbors, negative_sample and
// updategraph, without the lists leaving the device.
//
// Order guarantees, all by construction (no float atomics anywhere; the flag words use integer atomics, which commute):
//   key plan        one stable LSD radix sort (rocPRIM) of the 64-bit keys s * n + t with the COO position as the payload: equal keys
//                   ascend by COO position, so the first sorted copy of a key is its smallest position
//   has_edge        a lane per query bisects the sorted keys for the first key >= its own
//   adjacency_list  the by-node rows of coo_rows.h (what sample_neighbors builds): a row lists its edges in COO order; a lane per
//                   OUTPUT ELEMENT finds its row by bisection in the scanned counts
//   intersect       a lane per edge of g1 decides from the two plans; flags -> exclusive scan -> scatter (coo_compact.h) keeps COO order
//   random_walk_pe  Y = RW X row by row: a wave per (row, chunk of columns), the row's entries front to back (ascending column) from
//                   0.0f, every term one multiply and one add; columns are independent, so neither the block of seeds, the grid nor
//                   the row range a launch covers changes a bit
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "coo_compact.h"
#include "coo_rows.h"

namespace ngpde {

namespace {

// device flag words of one call (int32; words 0 and 1 are ONE 64-bit word, 8-byte aligned: the smallest offending id)
enum { fOffender = 0, fBadEdge = 2, fCsr = 3, fGraph = 4, fOrder = 5 };

constexpr int kWave = 64;
constexpr int kRwFixedBytes = 256;                       // the flag words of ngpde_csr_random_walk_pe, at the end of its workspace
constexpr size_t kRwWorkspaceCap = (size_t)256 << 20;    // what the library's own choice of `block` keeps the two state buffers under

inline unsigned long long offender_of(const int32_t *h) {
  unsigned long long w;
  std::memcpy(&w, h + fOffender, sizeof(w));
  return w;
}

int32_t check_sizes(const char *fn, int64_t n_nodes, int64_t n_edges) {
  NGPDE_REQUIRE(n_nodes >= 0 && n_edges >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n_nodes %lld, n_edges %lld)", fn,
                (long long)n_nodes, (long long)n_edges);
  NGPDE_REQUIRE(n_nodes <= 0x7fffffffLL && n_edges <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: a size above 2^31 - 1 (n_nodes %lld, n_edges %lld)", fn, (long long)n_nodes, (long long)n_edges);
  return NGPDE_OK;
}

// ---- the key plan ---------------------------------------------------------------------------------------------------------------
// key[e] = s * n + t; an end outside the node range is reported and the edge takes key 0
__global__ void pair_keys_kernel(int64_t m, int64_t n, int base, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                                 unsigned long long *__restrict__ key, int32_t *__restrict__ iota, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    report_offender(reinterpret_cast<unsigned long long *>(flags + fOffender), (a < 0 || a >= n) ? a : b);
    a = b = 0;
  }
  key[e] = (unsigned long long)a * (unsigned long long)n + (unsigned long long)b;
  iota[e] = (int32_t)e;
}

// ---- has_edge -------------------------------------------------------------------------------------------------------------------
__global__ void has_edge_kernel(int64_t n_queries, int64_t n, int64_t m, int base, const unsigned long long *__restrict__ keys,
                                const int32_t *__restrict__ positions, const int64_t *__restrict__ qs, const int64_t *__restrict__ qt,
                                uint8_t *__restrict__ found, int32_t *__restrict__ eid, unsigned long long *__restrict__ status) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n_queries) return;
  const int64_t a = qs[q] - base, b = qt[q] - base;
  int32_t at = -1;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    report_offender(status, (a < 0 || a >= n) ? a : b);
  } else {
    const unsigned long long k = (unsigned long long)a * (unsigned long long)n + (unsigned long long)b;
    const int64_t p = lower_bound_dev(keys, m, k);
    if (p < m && keys[p] == k) at = positions[p];
  }
  if (found) found[q] = at >= 0 ? 1 : 0;
  if (eid) eid[q] = at;
}

// ---- adjacency_list -------------------------------------------------------------------------------------------------------------
// cnt[i] = the length of the row of listed node i (cnt[n_rows] = 0: the scan's total); a listed id outside the node range is reported
__global__ void adjacency_count_kernel(int64_t n_rows, int64_t n, const int64_t *__restrict__ nodes, const int32_t *__restrict__ rowptr,
                                       long long *__restrict__ cnt, int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_rows) return;
  long long c = 0;
  if (i < n_rows) {
    const int64_t v = nodes ? nodes[i] : i;
    if (v < 0 || v >= n) report_offender(reinterpret_cast<unsigned long long *>(flags + fOffender), v);
    else c = rowptr[v + 1] - rowptr[v];
  }
  cnt[i] = c;
}

__global__ void narrow_offsets_kernel(int64_t count, const long long *__restrict__ off, int32_t *__restrict__ ptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) ptr[i] = (int32_t)std::min<long long>(off[i], 0x7fffffffLL);
}

// A lane per output element x: its row i is the last with ptr[i] <= x, so a hub's row is spread over as many lanes as it has
// neighbours.  ptr, row_ptr and row_eid are the caller's: a place that does not exist raises fCsr and nothing is read through it.
__global__ void adjacency_fill_kernel(int64_t total, int64_t n_rows, int64_t n, int64_t m, int dir, const int64_t *__restrict__ nodes,
                                      const int32_t *__restrict__ s, const int32_t *__restrict__ t, const int32_t *__restrict__ row_ptr,
                                      const int32_t *__restrict__ row_eid, const int32_t *__restrict__ ptr,
                                      int32_t *__restrict__ neighbors, int32_t *__restrict__ eid, int32_t *__restrict__ flags) {
  const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (x >= total) return;
  if (x == 0 && (ptr[n_rows] != total || ptr[0] != 0)) atomicOr(&flags[fCsr], 1);
  int64_t lo = 0, hi = n_rows;   // the last i with ptr[i] <= x
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (ptr[mid] <= x) lo = mid;
    else hi = mid;
  }
  const int64_t r = x - ptr[lo], v = nodes ? nodes[lo] : lo;
  int64_t e = -1;
  if (v >= 0 && v < n && r >= 0) {
    const int64_t b = row_ptr[v], end = row_ptr[v + 1];
    if (b >= 0 && end <= m && b + r < end) {
      e = row_eid[b + r];
      if (e < 0 || e >= m) e = -1;
    }
  }
  if (e < 0) atomicOr(&flags[fCsr], 1);
  neighbors[x] = e < 0 ? -1 : (dir == NGPDE_DIR_IN ? s[e] : t[e]);
  eid[x] = (int32_t)e;
}

// ---- intersect ------------------------------------------------------------------------------------------------------------------
// keep[e] = edge e of g1 is the first copy of its pair in g1 (its position is the one g1's plan lists first for the key) and the
// key occurs in g2's plan
__global__ void intersect_flags_kernel(int64_t m1, int64_t n, int base, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                                       const unsigned long long *__restrict__ keys1, const int32_t *__restrict__ pos1, int64_t m2,
                                       const unsigned long long *__restrict__ keys2, int32_t *__restrict__ keep, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m1) return;
  const int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  int32_t k = 0;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    report_offender(reinterpret_cast<unsigned long long *>(flags + fOffender), (a < 0 || a >= n) ? a : b);
  } else {
    const unsigned long long key = (unsigned long long)a * (unsigned long long)n + (unsigned long long)b;
    const int64_t p = lower_bound_dev(keys1, m1, key);
    if (p >= m1 || keys1[p] != key) {
      atomicOr(&flags[fCsr], 1);   // (the plan is not this list's)
    } else if (pos1[p] == (int32_t)e) {
      const int64_t q = lower_bound_dev(keys2, m2, key);
      k = (q < m2 && keys2[q] == key) ? 1 : 0;
    }
  }
  keep[e] = k;
}

// ---- random_walk_pe -------------------------------------------------------------------------------------------------------------
// what the step kernels rely on: row pointers inside the matrix, columns and graph ids in range; is graph_of non-decreasing?
__global__ void rw_check_kernel(int64_t n, int64_t nnz, const int32_t *__restrict__ row_ptr, const int32_t *__restrict__ cols,
                                int32_t n_graphs, const int32_t *__restrict__ graph_of, int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < nnz && (cols[p] < 0 || cols[p] >= n)) report_offender(reinterpret_cast<unsigned long long *>(flags + fOffender), cols[p]);
  if (p < n) {
    if (row_ptr[p] > row_ptr[p + 1] || row_ptr[p] < 0 || row_ptr[p + 1] > nnz) atomicOr(&flags[fCsr], 1);
    if (graph_of) {
      if (graph_of[p] < 0 || graph_of[p] >= n_graphs) atomicOr(&flags[fGraph], 1);
      if (p > 0 && graph_of[p] < graph_of[p - 1]) atomicOr(&flags[fOrder], 1);
    }
  }
  if (p == 0 && (row_ptr[0] != 0 || row_ptr[n] != nnz)) atomicOr(&flags[fCsr], 1);
}

// inv[j] = d[j] == 0 ? 0 : 1 / d[j], d[j] = row j's entries front to back from 0.0f
__global__ void rw_inverse_kernel(int64_t n, int64_t nnz, const int32_t *__restrict__ row_ptr, const float *__restrict__ vals,
                                  float *__restrict__ inv) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  int64_t b = row_ptr[j], e = row_ptr[j + 1];
  b = b < 0 ? 0 : b;
  e = e > nnz ? nnz : e;
  float d = 0.f;
  for (int64_t p = b; p < e; ++p) d += vals[p];
  inv[j] = d == 0.f ? 0.f : 1.0f / d;
}

// range[2 b], range[2 b + 1] = the rows of the graphs that the seeds of block b lie in (graph_of non-decreasing)
__global__ void rw_ranges_kernel(int64_t n, int32_t block, int32_t n_blocks, const int32_t *__restrict__ graph_of, int32_t *__restrict__ range) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_blocks) return;
  const int64_t first = (int64_t)b * block, last = std::min<int64_t>(first + block, n) - 1;
  range[2 * b] = (int32_t)lower_bound_dev(graph_of, n, graph_of[first]);
  range[2 * b + 1] = (int32_t)lower_bound_dev(graph_of, n, graph_of[last] + 1);
}

// X0[i][c] = (i == b0 + c) over the rows r0 .. r1 - 1: column c is the walk started at node b0 + c
__global__ void rw_init_kernel(int32_t r0, int32_t r1, int32_t b0, int32_t block, float *__restrict__ x) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t row = r0 + idx / block;
  const int c = (int)(idx % block);
  if (row < r1) x[(size_t)row * block + c] = row == (int64_t)b0 + c ? 1.0f : 0.f;
}

// One step Y = RW X over the rows r0 .. r1 - 1 and the first n_chunks chunks of 64 V columns.  A wave per (row, chunk), V adjacent
// columns per lane: an entry's row of X is one contiguous read of the wave (1 KiB at V = 4).  The wave loads up to 64 entries of
// its row at once -- column and RW value = vals * inv[col], rounded once -- and walks them in order; every lane adds the same terms
// in the same order, a multiply and an add each.  A column outside the matrix (reported by rw_check_kernel) contributes nothing
// and nothing is read through it.  The wave that holds column row - b0 of a seed row stores the diagonal to pe_row[row].
template <int V>
__global__ __launch_bounds__(256) void rw_step_kernel(int64_t n, int64_t nnz, int32_t r0, int32_t r1, int32_t b0, int32_t block,
                                                      int32_t n_chunks, const int32_t *__restrict__ row_ptr,
                                                      const int32_t *__restrict__ cols, const float *__restrict__ vals,
                                                      const float *__restrict__ inv, const float *__restrict__ x, float *__restrict__ y,
                                                      float *__restrict__ pe_row) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave));   // (row, chunk and the loop bounds are scalars)
  const int64_t item = (int64_t)blockIdx.x * (256 / kWave) + wave;
  const int64_t row = r0 + item / n_chunks;
  const int chunk = (int)(item % n_chunks);
  if (row >= r1) return;
  int64_t begin = row_ptr[row], end = row_ptr[row + 1];
  begin = begin < 0 ? 0 : begin;
  end = end > nnz ? nnz : end;
  const size_t col0 = (size_t)chunk * (kWave * V) + (size_t)lane * V;
  const float *__restrict__ xc = x + col0;
  float acc[V];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v] = 0.f;
  // entry j of the 64 the wave holds: its column and value from lane j (scalars), its row of X read by all lanes
  auto row_of_x = [&](int32_t c, int j) { return xc + (size_t)__builtin_amdgcn_readlane(c, j) * block; };
  auto add_term = [&](float w, int j, const float (&xv)[V]) {
    const float wj = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(w), j));
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = acc[v] + wj * xv[v];
  };
  auto load_row = [&](const float *__restrict__ xr, float (&xv)[V]) {
    if constexpr (V == 4) {
      const float4 q = *reinterpret_cast<const float4 *>(xr);
      xv[0] = q.x, xv[1] = q.y, xv[2] = q.z, xv[3] = q.w;
    } else {
      xv[0] = xr[0];
    }
  };
  for (int64_t p0 = begin; p0 < end; p0 += kWave) {
    const int cnt = (int)std::min<int64_t>(kWave, end - p0);
    int32_t c = 0;
    float w = 0.f;
    if (lane < cnt) {
      c = cols[p0 + lane];
      if (c < 0 || c >= n) c = 0;   // (w stays 0: the term is + 0 * X[0], and row 0 exists)
      else w = vals[p0 + lane] * inv[c];
    }
    int j = 0;
    for (; j + 4 <= cnt; j += 4) {   // four rows of X in flight; the terms are still added one after the other, in order
      float x0[V], x1[V], x2[V], x3[V];
      load_row(row_of_x(c, j), x0);
      load_row(row_of_x(c, j + 1), x1);
      load_row(row_of_x(c, j + 2), x2);
      load_row(row_of_x(c, j + 3), x3);
      add_term(w, j, x0);
      add_term(w, j + 1, x1);
      add_term(w, j + 2, x2);
      add_term(w, j + 3, x3);
    }
    for (; j < cnt; ++j) {
      float x0[V];
      load_row(row_of_x(c, j), x0);
      add_term(w, j, x0);
    }
  }
  float *__restrict__ yr = y + (size_t)row * block + col0;
  if constexpr (V == 4) *reinterpret_cast<float4 *>(yr) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  else yr[0] = acc[0];
  const int64_t d = row - b0;   // the seed column of this row, if it is a seed of the block
  if (d >= 0 && d < block && d / (kWave * V) == chunk && (d % (kWave * V)) / V == lane) {
    float diag = acc[0];
#pragma unroll
    for (int v = 1; v < V; ++v) diag = (d % V) == v ? acc[v] : diag;
    pe_row[row] = diag;
  }
}

// the library's choice of block: 256 columns (a float4 per lane), fewer where the graph has fewer nodes or the two state buffers
// would pass kRwWorkspaceCap
int32_t rw_choose_block(int64_t n) {
  int64_t b = std::min<int64_t>(256, ((std::max<int64_t>(n, 1) + 63) / 64) * 64);
  while (b > 64 && (size_t)2 * (size_t)n * (size_t)b * 4 > kRwWorkspaceCap) b -= 64;
  return (int32_t)b;
}

struct RwWs {
  float *xbuf[2], *inv;   // the two state buffers [n][block], the inverse row sums
  int32_t *flags;         // the last kRwFixedBytes
};
void rw_layout(Workspace &w, int64_t n, int32_t block, RwWs &p) {
  p.xbuf[0] = w.take<float>((size_t)n * (size_t)block);
  p.xbuf[1] = w.take<float>((size_t)n * (size_t)block);
  p.inv = w.take<float>((size_t)n);
  p.flags = w.take<int32_t>(kRwFixedBytes / sizeof(int32_t));
}
size_t rw_bytes(int64_t n, int32_t block) {
  RwWs p;
  return measure(rw_layout, n, block, p);
}

template <int V>
int32_t rw_launch_step(int64_t n, int64_t nnz, int32_t r0, int32_t r1, int32_t b0, int32_t block, const int32_t *row_ptr, const int32_t *cols,
                       const float *vals, const float *inv, const float *x, float *y, float *pe_row, hipStream_t stream) {
  const int64_t width = std::min<int64_t>(block, n - b0);   // the seeds of this block
  const int32_t n_chunks = (int32_t)((width + kWave * V - 1) / (kWave * V));
  const int64_t items = (int64_t)(r1 - r0) * n_chunks;
  const int64_t grid = (items + (256 / kWave) - 1) / (256 / kWave);
  NGPDE_REQUIRE(grid <= 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "ngpde_csr_random_walk_pe: %lld workgroups in one launch", (long long)grid);
  hipLaunchKernelGGL((rw_step_kernel<V>), dim3((unsigned)grid), dim3(256), 0, stream, n, nnz, r0, r1, b0, block, n_chunks, row_ptr, cols, vals, inv,
                     x, y, pe_row);
  NGPDE_LAUNCH_CHECK("rw_step_kernel");
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_coo_sort_keys(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, uint64_t *keys_out,
                            int32_t *positions_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_sort_keys";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_sizes(fn, n_nodes, n_edges)) return st;
  if (n_edges == 0) return NGPDE_OK;
  NGPDE_REQUIRE(s && t, NGPDE_ERR_INVALID_ARGUMENT, "%s: s / t is NULL", fn);
  NGPDE_REQUIRE(keys_out && positions_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: keys_out / positions_out is NULL", fn);
  NGPDE_REQUIRE(n_nodes > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %lld edges on a graph without nodes", fn, (long long)n_edges);
  Scratch sc;
  int32_t *flags = nullptr, *iota = nullptr;
  unsigned long long *key = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&key, (size_t)n_edges)) || (st = sc.get(&iota, (size_t)n_edges))) return st;
  hipLaunchKernelGGL(pair_keys_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, s, t, key, iota, flags);
  NGPDE_LAUNCH_CHECK("pair_keys_kernel");
  const unsigned end_bit = bits_for((unsigned long long)n_nodes * (unsigned long long)n_nodes);
  unsigned long long *sorted = reinterpret_cast<unsigned long long *>(keys_out);
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, key, sorted, iota, positions_out, (size_t)n_edges, 0u, end_bit, stream);
  };
  if ((st = with_temp(sc, sort))) return st;
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;   // (the temporaries are freed on return: the stream must be done with them)
  NGPDE_REQUIRE(!offender_of(h), NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references node %lld, outside the %lld nodes", fn,
                (long long)decode_offender(offender_of(h)), (long long)n_nodes);
  return NGPDE_OK;
}

int32_t ngpde_coo_has_edge(int64_t n_nodes, int64_t n_edges, const uint64_t *keys, const int32_t *positions, int64_t n_queries,
                           const int64_t *qs, const int64_t *qt, int32_t index_base, uint8_t *found_out, int32_t *eid_out, uint64_t *status,
                           ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_has_edge";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_sizes(fn, n_nodes, n_edges)) return st;
  NGPDE_REQUIRE(n_queries >= 0 && n_queries <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_queries %lld outside 0 : 2^31 - 1", fn,
                (long long)n_queries);
  if (n_queries == 0) return NGPDE_OK;
  NGPDE_REQUIRE(n_edges == 0 || (keys && positions), NGPDE_ERR_INVALID_ARGUMENT, "%s: keys / positions is NULL", fn);
  NGPDE_REQUIRE(qs && qt, NGPDE_ERR_INVALID_ARGUMENT, "%s: qs / qt is NULL", fn);
  NGPDE_REQUIRE(found_out || eid_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: found_out and eid_out are both NULL", fn);
  NGPDE_REQUIRE(status != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: status is NULL", fn);
  unsigned long long *word = reinterpret_cast<unsigned long long *>(status);
  if (int32_t st = launch_zero(word, sizeof(unsigned long long), stream)) return st;
  hipLaunchKernelGGL(has_edge_kernel, dim3(blocks_for(n_queries)), dim3(kB), 0, stream, n_queries, n_nodes, n_edges, index_base,
                     reinterpret_cast<const unsigned long long *>(keys), positions, qs, qt, found_out, eid_out, word);
  NGPDE_LAUNCH_CHECK("has_edge_kernel");
  if (capturing(stream)) return NGPDE_OK;   // (no read-back inside a capture: the word stays with the caller)
  unsigned long long h = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h, word, sizeof(h), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  NGPDE_REQUIRE(!h, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: a query names node %lld, outside the %lld nodes", fn,
                (long long)decode_offender(h), (long long)n_nodes);
  return NGPDE_OK;
}

int32_t ngpde_coo_adjacency_count(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                                  int64_t n_listed, const int64_t *nodes, int32_t *row_ptr_out, int32_t *row_eid_out, int32_t *ptr_out,
                                  int64_t *total_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_adjacency_count";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_sizes(fn, n_nodes, n_edges)) return st;
  NGPDE_REQUIRE(total_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: total_out is NULL", fn);
  *total_out = 0;
  NGPDE_REQUIRE(dir == NGPDE_DIR_OUT || dir == NGPDE_DIR_IN, NGPDE_ERR_INVALID_ARGUMENT, "%s: dir %d is neither NGPDE_DIR_OUT nor NGPDE_DIR_IN", fn,
                dir);
  NGPDE_REQUIRE(n_listed >= 0 && n_listed <= 0x7fffffffLL - 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_listed %lld outside 0 : 2^31 - 2", fn,
                (long long)n_listed);
  NGPDE_REQUIRE(nodes || n_listed == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: nodes is NULL with n_listed %lld", fn, (long long)n_listed);
  NGPDE_REQUIRE(n_edges == 0 || (s && t), NGPDE_ERR_INVALID_ARGUMENT, "%s: s / t is NULL", fn);
  NGPDE_REQUIRE(n_edges == 0 || n_nodes > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %lld edges on a graph without nodes", fn,
                (long long)n_edges);
  NGPDE_REQUIRE(row_ptr_out && ptr_out && (n_edges == 0 || row_eid_out), NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  const int64_t n_rows = nodes ? n_listed : n_nodes;
  Scratch sc;
  int32_t *flags = nullptr;
  long long *cnt = nullptr, *off = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&cnt, (size_t)n_rows + 1)) || (st = sc.get(&off, (size_t)n_rows + 1))) return st;
  if (n_edges > 0) {
    Rows rows;
    rows.eid = row_eid_out;
    rows.rowptr = row_ptr_out;
    if ((st = build_rows(n_nodes, n_edges, s, t, index_base, dir, &rows, flags + fBadEdge, sc, stream))) return st;
  } else {
    NGPDE_HIP_CHECK(hipMemsetAsync(row_ptr_out, 0, ((size_t)n_nodes + 1) * sizeof(int32_t), stream));
  }
  hipLaunchKernelGGL(adjacency_count_kernel, dim3(blocks_for(n_rows + 1)), dim3(kB), 0, stream, n_rows, n_nodes, nodes, row_ptr_out, cnt, flags);
  NGPDE_LAUNCH_CHECK("adjacency_count_kernel");
  auto scan = [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, cnt, off, 0ll, (size_t)n_rows + 1, rocprim::plus<long long>(), stream);
  };
  if ((st = with_temp(sc, scan))) return st;
  hipLaunchKernelGGL(narrow_offsets_kernel, dim3(blocks_for(n_rows + 1)), dim3(kB), 0, stream, n_rows + 1, off, ptr_out);
  NGPDE_LAUNCH_CHECK("narrow_offsets_kernel");
  long long total = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&total, off + n_rows, sizeof(total), hipMemcpyDeviceToHost, stream));
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[fBadEdge], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references a node outside the %lld nodes", fn,
                (long long)n_nodes);
  NGPDE_REQUIRE(!offender_of(h), NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: nodes lists node %lld, outside the %lld nodes", fn,
                (long long)decode_offender(offender_of(h)), (long long)n_nodes);
  NGPDE_REQUIRE(total <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: the listed rows hold %lld neighbours, at most 2^31 - 1", fn, total);
  *total_out = total;
  return NGPDE_OK;
}

int32_t ngpde_coo_adjacency_fill(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t dir, int64_t n_listed,
                                 const int64_t *nodes, const int32_t *row_ptr, const int32_t *row_eid, const int32_t *ptr, int64_t total,
                                 int32_t *neighbors_out, int32_t *eid_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_adjacency_fill";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_sizes(fn, n_nodes, n_edges)) return st;
  NGPDE_REQUIRE(dir == NGPDE_DIR_OUT || dir == NGPDE_DIR_IN, NGPDE_ERR_INVALID_ARGUMENT, "%s: dir %d is neither NGPDE_DIR_OUT nor NGPDE_DIR_IN", fn,
                dir);
  NGPDE_REQUIRE(n_listed >= 0 && n_listed <= 0x7fffffffLL - 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_listed %lld outside 0 : 2^31 - 2", fn,
                (long long)n_listed);
  NGPDE_REQUIRE(nodes || n_listed == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: nodes is NULL with n_listed %lld", fn, (long long)n_listed);
  NGPDE_REQUIRE(total >= 0 && total <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: total %lld outside 0 : 2^31 - 1", fn, (long long)total);
  if (total == 0) return NGPDE_OK;
  const int64_t n_rows = nodes ? n_listed : n_nodes;
  NGPDE_REQUIRE(n_rows > 0 && n_edges > 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld neighbours of a list without rows or edges", fn, (long long)total);
  NGPDE_REQUIRE(s && t, NGPDE_ERR_INVALID_ARGUMENT, "%s: s / t is NULL", fn);
  NGPDE_REQUIRE(row_ptr && row_eid && ptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: row_ptr / row_eid / ptr is NULL", fn);
  NGPDE_REQUIRE(neighbors_out && eid_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  Scratch sc;
  int32_t *flags = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream))) return st;
  hipLaunchKernelGGL(adjacency_fill_kernel, dim3(blocks_for(total)), dim3(kB), 0, stream, total, n_rows, n_nodes, n_edges, dir, nodes, s, t, row_ptr,
                     row_eid, ptr, neighbors_out, eid_out, flags);
  NGPDE_LAUNCH_CHECK("adjacency_fill_kernel");
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[fCsr], NGPDE_ERR_INVALID_ARGUMENT, "%s: ptr / row_ptr / row_eid are not what ngpde_coo_adjacency_count wrote for this list", fn);
  return NGPDE_OK;
}

int32_t ngpde_coo_intersect(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, const uint64_t *keys,
                            const int32_t *positions, int64_t n_edges2, const uint64_t *keys2, int32_t *s_out, int32_t *t_out, int64_t *kept,
                            int64_t *n_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_intersect";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_sizes(fn, n_nodes, n_edges)) return st;
  NGPDE_REQUIRE(n_edges2 >= 0 && n_edges2 <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_edges2 %lld outside 0 : 2^31 - 1 (negative, or too large)",
                fn, (long long)n_edges2);
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_out is NULL", fn);
  *n_out = 0;
  if (n_edges == 0) return NGPDE_OK;
  NGPDE_REQUIRE(s && t, NGPDE_ERR_INVALID_ARGUMENT, "%s: s / t is NULL", fn);
  NGPDE_REQUIRE(keys && positions && (n_edges2 == 0 || keys2), NGPDE_ERR_INVALID_ARGUMENT, "%s: keys / positions / keys2 is NULL", fn);
  NGPDE_REQUIRE(s_out && t_out && kept, NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  NGPDE_REQUIRE(n_nodes > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %lld edges on a graph without nodes", fn, (long long)n_edges);
  Scratch sc;
  int32_t *flags = nullptr, *keep = nullptr, *pos = nullptr, *count = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&keep, (size_t)n_edges)) || (st = sc.get(&pos, (size_t)n_edges)) ||
      (st = sc.get(&count, 1)))
    return st;
  hipLaunchKernelGGL(intersect_flags_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, s, t,
                     reinterpret_cast<const unsigned long long *>(keys), positions, n_edges2, reinterpret_cast<const unsigned long long *>(keys2),
                     keep, flags);
  NGPDE_LAUNCH_CHECK("intersect_flags_kernel");
  if ((st = compact_flagged(n_edges, index_base, s, t, nullptr, keep, pos, s_out, t_out, kept, count, sc, stream))) return st;
  int32_t h_count = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_count, count, sizeof(h_count), hipMemcpyDeviceToHost, stream));
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!offender_of(h), NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references node %lld, outside the %lld nodes", fn,
                (long long)decode_offender(offender_of(h)), (long long)n_nodes);
  NGPDE_REQUIRE(!h[fCsr], NGPDE_ERR_INVALID_ARGUMENT, "%s: keys / positions are not the plan ngpde_coo_sort_keys made of this list", fn);
  *n_out = h_count;
  return NGPDE_OK;
}

size_t ngpde_csr_random_walk_pe_workspace_bytes(int64_t n, int32_t block) {
  if (n < 0 || n > 0x7fffffffLL || block < 0 || block % kWave != 0) return 0;
  if (block == 0) block = rw_choose_block(n);
  if ((uint64_t)n * (uint64_t)block > (uint64_t)1 << 40) return 0;
  return rw_bytes(n, block);
}

int32_t ngpde_csr_random_walk_pe(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *cols, const float *vals, int32_t n_graphs,
                                 const int32_t *graph_of, int32_t walk_length, int32_t block, float *pe, void *workspace, size_t workspace_bytes,
                                 ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_random_walk_pe";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(n >= 0 && nnz >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n %lld, nnz %lld)", fn, (long long)n, (long long)nnz);
  NGPDE_REQUIRE(n <= 0x7fffffffLL && nnz <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: a size above 2^31 - 1 (n %lld, nnz %lld)", fn,
                (long long)n, (long long)nnz);
  NGPDE_REQUIRE(walk_length >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: walk_length %d, at least 1", fn, walk_length);
  NGPDE_REQUIRE(block >= 0 && block % kWave == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: block %d is not a multiple of 64 (0: the library's choice)", fn,
                block);
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_graphs %d, at least 1", fn, n_graphs);
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(row_ptr && (nnz == 0 || (cols && vals)), NGPDE_ERR_INVALID_ARGUMENT, "%s: row_ptr / cols / vals is NULL", fn);
  NGPDE_REQUIRE(pe != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: pe is NULL", fn);
  if (block == 0) block = rw_choose_block(n);
  NGPDE_REQUIRE((uint64_t)n * (uint64_t)block <= (uint64_t)1 << 40, NGPDE_ERR_UNSUPPORTED, "%s: %lld nodes x block %d: the state is too large", fn,
                (long long)n, block);
  int32_t st;
  if ((st = check_workspace(fn, workspace, workspace_bytes, rw_bytes(n, block), 16))) return st;
  Workspace w(workspace);
  RwWs p;
  rw_layout(w, n, block, p);
  float *const *xbuf = p.xbuf, *const inv = p.inv;
  int32_t *const flags = p.flags;
  const int32_t n_blocks = (int32_t)((n + block - 1) / block);
  if ((st = launch_zero(flags, kFlagWords * sizeof(int32_t), stream))) return st;
  hipLaunchKernelGGL(rw_check_kernel, dim3(blocks_for(std::max(n, nnz))), dim3(kB), 0, stream, n, nnz, row_ptr, cols, n_graphs, graph_of, flags);
  NGPDE_LAUNCH_CHECK("rw_check_kernel");
  hipLaunchKernelGGL(rw_inverse_kernel, dim3(blocks_for(n)), dim3(kB), 0, stream, n, nnz, row_ptr, vals, inv);
  NGPDE_LAUNCH_CHECK("rw_inverse_kernel");
  // The row range of a block's launches: the graphs its seeds lie in, when graph_of is non-decreasing.  That is known on the device;
  // it is read back once, with the flags, unless the stream is being captured -- then every launch covers all rows (the same bits).
  const bool in_capture = capturing(stream);
  std::vector<int32_t> range;
  if (!in_capture) {
    const bool ranged = graph_of && n_graphs > 1;
    if (ranged) {
      range.resize(2 * (size_t)n_blocks);
      int32_t *range_dev = (int32_t *)xbuf[0];   // (2 n_blocks words of a buffer of n * block: free until the first init launch)
      hipLaunchKernelGGL(rw_ranges_kernel, dim3(blocks_for(n_blocks)), dim3(kB), 0, stream, n, block, n_blocks, graph_of, range_dev);
      NGPDE_LAUNCH_CHECK("rw_ranges_kernel");
      NGPDE_HIP_CHECK(hipMemcpyAsync(range.data(), range_dev, range.size() * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    }
    int32_t h[kFlagWords];
    if ((st = read_flags(flags, h, stream))) return st;
    NGPDE_REQUIRE(!h[fCsr], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: a row pointer lies outside the %lld entries", fn, (long long)nnz);
    NGPDE_REQUIRE(!offender_of(h), NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an entry names column %lld, outside the %lld nodes", fn,
                  (long long)decode_offender(offender_of(h)), (long long)n);
    NGPDE_REQUIRE(!h[fGraph], NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of holds an id outside 0:%d", fn, n_graphs - 1);
    if (h[fOrder]) range.clear();   // the nodes of a graph are not contiguous: every launch covers all rows
  }
  for (int32_t b = 0; b < n_blocks; ++b) {
    const int32_t b0 = b * block;
    int32_t r0 = 0, r1 = (int32_t)n;
    if (!range.empty()) {
      r0 = std::max(0, range[2 * (size_t)b]);
      r1 = std::min((int32_t)n, range[2 * (size_t)b + 1]);
      if (r0 >= r1) continue;
    }
    const int64_t cells = (int64_t)(r1 - r0) * block;
    NGPDE_REQUIRE(blocks_for(cells) <= 0x7fffffffu && cells / kB <= 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "%s: %lld cells in one launch", fn,
                  (long long)cells);
    hipLaunchKernelGGL(rw_init_kernel, dim3(blocks_for(cells)), dim3(kB), 0, stream, r0, r1, b0, block, xbuf[0]);
    NGPDE_LAUNCH_CHECK("rw_init_kernel");
    for (int32_t k = 0; k < walk_length; ++k) {
      const float *x = xbuf[k & 1];
      float *y = xbuf[(k + 1) & 1];
      float *pe_row = pe + (size_t)k * (size_t)n;
      if (block % 256 == 0) st = rw_launch_step<4>(n, nnz, r0, r1, b0, block, row_ptr, cols, vals, inv, x, y, pe_row, stream);
      else st = rw_launch_step<1>(n, nnz, r0, r1, b0, block, row_ptr, cols, vals, inv, x, y, pe_row, stream);
      if (st) return st;
    }
  }
  return NGPDE_OK;
}

}  // extern "C"
