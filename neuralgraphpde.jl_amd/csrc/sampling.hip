// sampling.hip -- random parts of a COO list that lives in HBM (include/ngpde.h, "random graph sampling"): sample_neighbors and
// rand_edge_split of the GNNGraphs re-export (src/NeuralGraphPDE.jl:4 of the reference), and the counter-based generator under them.
// The sibling of graph_ops.hip: a fresh sub-sample of every neighbourhood per epoch, or a random hold-out of the edges, without the
// COO lists leaving the device.
//
// Randomness: Philox4x32-10 (philox.h; Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), stateless.  A value is a pure
// function of (seed, stream, counter) -- never of the thread, the launch geometry or the call order -- so a call gives the same bits
// on every run and a test restates the generator in numpy.
//
// Order guarantees, all by construction (no float anywhere; the int32 flag words use integer atomics, which commute):
//   rows             stable LSD radix sort (rocPRIM) of the COO positions by target (or source): a row lists its edges in COO order
//   selection        an edge is kept iff fewer than K edges of its row have a smaller (key, COO position): one order statistic,
//                    evaluated by exact rank counting on keys staged in LDS (rows up to NGPDE_SAMPLE_LDS_ROW_MAX) or by a stable
//                    segmented radix sort of the keys (longer rows) -- the two agree bit for bit
//   compaction       flags -> exclusive scan -> scatter: kept edges stay in COO order
//   with replacement output slot (listed node i, draw j) is computed, not raced for
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "coo_rows.h"
#include "philox.h"

namespace ngpde {

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = kB / kWave;                                // a wave per short row
constexpr int kWaveRowMax = NGPDE_SAMPLE_LDS_ROW_MAX / kRowsPerBlock;    // 512: the four waves' rows share the block row's LDS
static_assert(NGPDE_SAMPLE_LDS_ROW_MAX % kB == 0 && NGPDE_SAMPLE_LDS_ROW_MAX * 8 <= 64 * 1024, "the staged keys of a row must fit LDS");

// device flag words of one call
enum { kBadEdge = 0, kBadNode = 1, kBadCount = 2, kCount = 4 };

// ---- the generator (philox.h) -----------------------------------------------------------------------------------------------
__global__ void random_keys_kernel(unsigned long long seed, uint32_t stream, uint32_t c1, unsigned long long first, int64_t n,
                                   unsigned long long *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = philox_draw(seed, stream, (uint32_t)(first + (unsigned long long)i), c1);
}

// ---- rows: coo_rows.h (row_keys_kernel, rowptr_kernel, Rows, build_rows), shared with graph_query.hip ---------------------------

// listed[v] = 1 for every listed node; an entry out of range or listed twice raises kBadNode
__global__ void mark_listed_kernel(int64_t n_listed, int64_t n, const int64_t *__restrict__ nodes, int32_t *__restrict__ listed,
                                   int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_listed) return;
  const int64_t v = nodes[i];
  if (v < 0 || v >= n) atomicOr(&flags[kBadNode], 1);
  else if (atomicExch(&listed[v], 1) != 0) atomicOr(&flags[kBadNode], 1);
}

// ---- selection without replacement --------------------------------------------------------------------------------------------
// the rows that are copied through without drawing: keep[e] = its row is listed and (k < 0 or deg <= k); everything else starts at 0
__global__ void keep_short_kernel(int64_t m, int k, const uint32_t *__restrict__ row_of, const int32_t *__restrict__ eid,
                                  const int32_t *__restrict__ rowptr, const int32_t *__restrict__ listed, int32_t *__restrict__ keep) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const uint32_t v = row_of[p];
  const int deg = rowptr[v + 1] - rowptr[v];
  keep[eid[p]] = ((!listed || listed[v]) && (k < 0 || deg <= k)) ? 1 : 0;
}

// entry i of a row staged in `keys` (deg of them): kept iff fewer than k entries have a smaller (key, position).  Every lane reads
// the same keys[j] -- an LDS broadcast -- and counts for its own entry.
__device__ __forceinline__ bool among_k_smallest(const unsigned long long *keys, int deg, int i, int k) {
  const unsigned long long ki = keys[i];
  int smaller = 0;
#pragma unroll 4
  for (int j = 0; j < deg; ++j) {
    const unsigned long long kj = keys[j];
    smaller += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
  }
  return smaller < k;
}

// One launch for every row with k < deg <= NGPDE_SAMPLE_LDS_ROW_MAX.  A workgroup of four waves takes four consecutive nodes: first
// each wave selects its own node's row if that has at most kWaveRowMax edges (the keys of the four rows side by side in LDS), then the
// whole workgroup takes the longer rows of the four one after the other.  The keys are drawn here and never written to memory.  The
// branches between the barriers depend on the degrees of the workgroup's four nodes alone, which every thread reads alike.
__global__ __launch_bounds__(kB) void select_rows_kernel(int64_t n, int k, unsigned long long seed, const int32_t *__restrict__ rowptr,
                                                         const int32_t *__restrict__ eid, const int32_t *__restrict__ listed,
                                                         int32_t *__restrict__ keep) {
  __shared__ unsigned long long keys[NGPDE_SAMPLE_LDS_ROW_MAX];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int64_t v0 = (int64_t)blockIdx.x * kRowsPerBlock;
  {
    const int64_t v = v0 + wave;
    int begin = 0, deg = 0;
    if (v < n && (!listed || listed[v])) {
      begin = rowptr[v];
      deg = rowptr[v + 1] - begin;
    }
    if (deg <= k || deg > kWaveRowMax) deg = 0;   // copied through already / a workgroup's row
    unsigned long long *wk = keys + wave * kWaveRowMax;
    for (int i = lane; i < deg; i += kWave) wk[i] = philox_draw(seed, kStreamNeighbor, (uint32_t)eid[begin + i], 0u);
    __syncthreads();
    for (int i = lane; i < deg; i += kWave)
      if (among_k_smallest(wk, deg, i, k)) keep[eid[begin + i]] = 1;
  }
  for (int r = 0; r < kRowsPerBlock; ++r) {
    const int64_t v = v0 + r;
    if (v >= n || (listed && !listed[v])) continue;
    const int begin = rowptr[v], deg = rowptr[v + 1] - begin;
    if (deg <= k || deg <= kWaveRowMax || deg > NGPDE_SAMPLE_LDS_ROW_MAX) continue;
    __syncthreads();   // the previous use of `keys` is over
    for (int i = threadIdx.x; i < deg; i += kB) keys[i] = philox_draw(seed, kStreamNeighbor, (uint32_t)eid[begin + i], 0u);
    __syncthreads();
    for (int i = threadIdx.x; i < deg; i += kB)
      if (among_k_smallest(keys, deg, i, k)) keep[eid[begin + i]] = 1;
  }
}

// rows beyond the LDS bound: the segments of the segmented sort (every other row is an empty segment) ...
__global__ void long_segments_kernel(int64_t n, int k, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ listed,
                                     int32_t *__restrict__ seg_begin, int32_t *__restrict__ seg_end) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int begin = rowptr[v], deg = rowptr[v + 1] - begin;
  const bool is_long = (!listed || listed[v]) && deg > k && deg > NGPDE_SAMPLE_LDS_ROW_MAX;
  seg_begin[v] = begin;
  seg_end[v] = is_long ? begin + deg : begin;
}

// ... their keys, written in row order (COO order inside a row: the stable sort then breaks ties by position) ...
__global__ void long_keys_kernel(int64_t m, unsigned long long seed, const uint32_t *__restrict__ row_of, const int32_t *__restrict__ eid,
                                 const int32_t *__restrict__ seg_begin, const int32_t *__restrict__ seg_end,
                                 unsigned long long *__restrict__ key) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const uint32_t v = row_of[p];
  if (seg_end[v] > seg_begin[v]) key[p] = philox_draw(seed, kStreamNeighbor, (uint32_t)eid[p], 0u);
}

// ... and the first k of every sorted segment
__global__ void long_take_kernel(int64_t m, int k, const uint32_t *__restrict__ row_of, const int32_t *__restrict__ eid_sorted,
                                 const int32_t *__restrict__ seg_begin, const int32_t *__restrict__ seg_end, int32_t *__restrict__ keep) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const uint32_t v = row_of[p];
  if (seg_end[v] > seg_begin[v] && p - seg_begin[v] < k) keep[eid_sorted[p]] = 1;
}

__global__ void compact_kernel(int64_t m, const int32_t *__restrict__ s, const int32_t *__restrict__ t, const int32_t *__restrict__ keep,
                               const int32_t *__restrict__ pos, int32_t *__restrict__ s_out, int32_t *__restrict__ t_out,
                               int64_t *__restrict__ eid_out, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int32_t p = pos[e];
  if (keep[e]) {
    s_out[p] = s[e];
    t_out[p] = t[e];
    eid_out[p] = e;
  }
  if (e == m - 1) flags[kCount] = p + keep[e];
}

// ---- with replacement ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t listed_node(const int64_t *__restrict__ nodes, int64_t i, int64_t n) {
  const int64_t v = nodes ? nodes[i] : i;
  return (v < 0 || v >= n) ? -1 : v;   // (an entry out of range was reported by mark_listed_kernel)
}

__global__ void draw_counts_kernel(int64_t n_listed, int64_t n, int k, const int64_t *__restrict__ nodes, const int32_t *__restrict__ rowptr,
                                   int32_t *__restrict__ cnt) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_listed) return;
  const int64_t v = listed_node(nodes, i, n);
  cnt[i] = (v >= 0 && rowptr[v + 1] > rowptr[v]) ? k : 0;
}

// draw j of listed node i: entry (draw * deg) >> 64 of its row
__global__ void draw_kernel(int64_t n_listed, int64_t n, int k, unsigned long long seed, const int64_t *__restrict__ nodes,
                            const int32_t *__restrict__ rowptr, const int32_t *__restrict__ eid, const int32_t *__restrict__ cnt,
                            const int32_t *__restrict__ off, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                            int32_t *__restrict__ s_out, int32_t *__restrict__ t_out, int64_t *__restrict__ eid_out,
                            int32_t *__restrict__ flags) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_listed * k) return;
  const int64_t i = idx / k;
  const int j = (int)(idx - i * k);
  if (cnt[i]) {
    const int64_t v = listed_node(nodes, i, n);
    const int begin = rowptr[v], deg = rowptr[v + 1] - begin;
    const unsigned long long d = philox_draw(seed, kStreamReplace, (uint32_t)v, (uint32_t)j);
    const int e = eid[begin + (int)__umul64hi(d, (unsigned long long)deg)];
    const int64_t o = (int64_t)off[i] + j;
    s_out[o] = s[e];
    t_out[o] = t[e];
    eid_out[o] = e;
  }
  if (idx == n_listed * k - 1) flags[kCount] = off[i] + cnt[i];
}

// ---- split ----------------------------------------------------------------------------------------------------------------------
// by_pair == 0: the key belongs to the COO position; by_pair: to the unordered pair of ends, and upper[e] = (s <= t) marks the ranked edges
__global__ void split_keys_kernel(int64_t m, int64_t n, int base, int by_pair, unsigned long long seed, const int32_t *__restrict__ s,
                                  const int32_t *__restrict__ t, unsigned long long *__restrict__ key, int32_t *__restrict__ iota,
                                  int32_t *__restrict__ upper, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    atomicOr(&flags[kBadEdge], 1);
    a = b = 0;
  }
  key[e] = by_pair ? philox_draw(seed, kStreamSplit, (uint32_t)(a < b ? a : b), (uint32_t)(a < b ? b : a))
                   : philox_draw(seed, kStreamSplit, (uint32_t)e, 0u);
  iota[e] = (int32_t)e;
  if (by_pair) upper[e] = a <= b ? 1 : 0;
}

__global__ void side_by_rank_kernel(int64_t m, int64_t n_first, const int32_t *__restrict__ eid_sorted, int32_t *__restrict__ side) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < m) side[eid_sorted[r]] = r < n_first ? 0 : 1;
}

__global__ void upper_sorted_kernel(int64_t m, const int32_t *__restrict__ eid_sorted, const int32_t *__restrict__ upper,
                                    int32_t *__restrict__ upper_sorted) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < m) upper_sorted[r] = upper[eid_sorted[r]];
}

// tau = the key of the ranked edge of rank n_first - 1 (incl = the inclusive scan of the ranked flags in sorted order); fewer ranked
// edges than n_first raises kBadCount
__global__ void threshold_kernel(int64_t m, int64_t n_first, const unsigned long long *__restrict__ key_sorted,
                                 const int32_t *__restrict__ upper_sorted, const int32_t *__restrict__ incl, unsigned long long *__restrict__ tau,
                                 int32_t *__restrict__ flags) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  if (upper_sorted[r] && incl[r] == n_first) *tau = key_sorted[r];
  if (r == m - 1 && incl[r] < n_first) atomicOr(&flags[kBadCount], 1);
}

__global__ void side_by_threshold_kernel(int64_t m, int64_t n_first, const unsigned long long *__restrict__ key,
                                         const unsigned long long *__restrict__ tau, int32_t *__restrict__ side) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < m) side[e] = (n_first > 0 && key[e] <= *tau) ? 0 : 1;
}

__global__ void first_flags_kernel(int64_t m, const int32_t *__restrict__ side, int32_t *__restrict__ first) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < m) first[e] = side[e] == 0 ? 1 : 0;
}

__global__ void split_compact_kernel(int64_t m, const int32_t *__restrict__ first, const int32_t *__restrict__ pos, int64_t *__restrict__ kept0,
                                     int64_t *__restrict__ kept1, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int32_t p = pos[e];
  if (first[e]) kept0[p] = e;
  else kept1[e - p] = e;
  if (e == m - 1) flags[kCount] = p + first[e];
}

// ---- host helpers -------------------------------------------------------------------------------------------------------------
int32_t exclusive_scan_i32(const int32_t *in, int32_t *out, size_t count, Scratch &sc, hipStream_t stream) {
  return with_temp(sc, [&](void *tmp, size_t &bytes) { return rocprim::exclusive_scan(tmp, bytes, in, out, 0, count, rocprim::plus<int32_t>(), stream); });
}

int32_t inclusive_scan_i32(const int32_t *in, int32_t *out, size_t count, Scratch &sc, hipStream_t stream) {
  return with_temp(sc, [&](void *tmp, size_t &bytes) { return rocprim::inclusive_scan(tmp, bytes, in, out, count, rocprim::plus<int32_t>(), stream); });
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_random_keys(uint64_t seed, uint32_t stream_id, uint32_t c1, uint64_t first, int64_t n, uint64_t *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(n >= 0, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_random_keys: negative count %lld", (long long)n);
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_random_keys: out is NULL");
  NGPDE_REQUIRE(n <= 0x7fffffffLL * (int64_t)kB, NGPDE_ERR_UNSUPPORTED, "ngpde_random_keys: more keys than one launch covers");
  hipLaunchKernelGGL(random_keys_kernel, dim3(blocks_for(n)), dim3(kB), 0, (hipStream_t)stream, (unsigned long long)seed, stream_id, c1,
                     (unsigned long long)first, n, reinterpret_cast<unsigned long long *>(out));
  NGPDE_LAUNCH_CHECK("random_keys_kernel");
  return NGPDE_OK;
}

int32_t ngpde_coo_sample_neighbors(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                                   int64_t n_listed, const int64_t *nodes, int32_t k, int32_t replace, uint64_t seed, int32_t *s_out,
                                   int32_t *t_out, int64_t *eid_out, int64_t *n_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const char *fn = "ngpde_coo_sample_neighbors";
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_out is NULL", fn);
  *n_out = 0;
  NGPDE_REQUIRE(dir == NGPDE_DIR_OUT || dir == NGPDE_DIR_IN, NGPDE_ERR_INVALID_ARGUMENT, "%s: dir %d is neither NGPDE_DIR_OUT nor NGPDE_DIR_IN", fn,
                dir);
  NGPDE_REQUIRE(k >= -1, NGPDE_ERR_INVALID_ARGUMENT, "%s: k is %d; -1 keeps every edge, 0 none", fn, k);
  NGPDE_REQUIRE(!replace || k >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: k = -1 (every edge) with replacement", fn);
  NGPDE_REQUIRE(n_listed >= 0 && n_listed <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_listed %lld outside 0 : 2^31 - 1", fn,
                (long long)n_listed);
  NGPDE_REQUIRE(nodes || n_listed == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: nodes is NULL with n_listed %lld", fn, (long long)n_listed);
  const int64_t n_rows = nodes ? n_listed : n_nodes;   // the listed nodes
  const int64_t bound = replace ? n_rows * (int64_t)k : n_edges;
  NGPDE_REQUIRE(bound <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld draws, at most 2^31 - 1", fn, (long long)bound);
  NGPDE_REQUIRE(bound == 0 || n_edges == 0 || (s_out && t_out && eid_out), NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  if (n_edges == 0 && !nodes) return NGPDE_OK;
  Scratch sc;
  int32_t *flags = nullptr, *listed = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream))) return st;
  if (nodes) {
    if ((st = sc.get(&listed, (size_t)n_nodes))) return st;
    NGPDE_HIP_CHECK(hipMemsetAsync(listed, 0, std::max<size_t>((size_t)n_nodes, 1) * sizeof(int32_t), stream));
    if (n_listed > 0) {
      hipLaunchKernelGGL(mark_listed_kernel, dim3(blocks_for(n_listed)), dim3(kB), 0, stream, n_listed, n_nodes, nodes, listed, flags);
      NGPDE_LAUNCH_CHECK("mark_listed_kernel");
    }
  }
  if (n_edges > 0) {
    Rows rows;
    if ((st = build_rows(n_nodes, n_edges, s, t, index_base, dir, &rows, flags + kBadEdge, sc, stream))) return st;
    if (!replace) {
      int32_t *keep = nullptr, *pos = nullptr;
      if ((st = sc.get(&keep, (size_t)n_edges)) || (st = sc.get(&pos, (size_t)n_edges))) return st;
      hipLaunchKernelGGL(keep_short_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, k, rows.row_of, rows.eid, rows.rowptr, listed,
                         keep);
      NGPDE_LAUNCH_CHECK("keep_short_kernel");
      if (k > 0 && n_edges > k) {   // some row may be longer than k
        hipLaunchKernelGGL(select_rows_kernel, dim3((unsigned)((n_nodes + kRowsPerBlock - 1) / kRowsPerBlock)), dim3(kB), 0, stream, n_nodes, k,
                           (unsigned long long)seed, rows.rowptr, rows.eid, listed, keep);
        NGPDE_LAUNCH_CHECK("select_rows_kernel");
      }
      if (k > 0 && n_edges > NGPDE_SAMPLE_LDS_ROW_MAX) {   // some row may be longer than the LDS bound: whether one is, only the device
        int32_t *seg_begin = nullptr, *seg_end = nullptr, *eid_sorted = nullptr;   // knows; a list without one sorts empty segments
        unsigned long long *key = nullptr, *key_sorted = nullptr;
        if ((st = sc.get(&seg_begin, (size_t)n_nodes)) || (st = sc.get(&seg_end, (size_t)n_nodes)) || (st = sc.get(&key, (size_t)n_edges)) ||
            (st = sc.get(&key_sorted, (size_t)n_edges)) || (st = sc.get(&eid_sorted, (size_t)n_edges)))
          return st;
        hipLaunchKernelGGL(long_segments_kernel, dim3(blocks_for(n_nodes)), dim3(kB), 0, stream, n_nodes, k, rows.rowptr, listed, seg_begin, seg_end);
        NGPDE_LAUNCH_CHECK("long_segments_kernel");
        hipLaunchKernelGGL(long_keys_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, (unsigned long long)seed, rows.row_of, rows.eid,
                           seg_begin, seg_end, key);
        NGPDE_LAUNCH_CHECK("long_keys_kernel");
        auto sort = [&](void *tmp, size_t &bytes) {
          return rocprim::segmented_radix_sort_pairs(tmp, bytes, key, key_sorted, rows.eid, eid_sorted, (unsigned)n_edges, (unsigned)n_nodes,
                                                     seg_begin, seg_end, 0u, 64u, stream);
        };
        if ((st = with_temp(sc, sort))) return st;
        hipLaunchKernelGGL(long_take_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, k, rows.row_of, eid_sorted, seg_begin, seg_end,
                           keep);
        NGPDE_LAUNCH_CHECK("long_take_kernel");
      }
      if ((st = exclusive_scan_i32(keep, pos, (size_t)n_edges, sc, stream))) return st;
      hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, s, t, keep, pos, s_out, t_out, eid_out, flags);
      NGPDE_LAUNCH_CHECK("compact_kernel");
    } else if (bound > 0) {
      int32_t *cnt = nullptr, *off = nullptr;
      if ((st = sc.get(&cnt, (size_t)n_rows)) || (st = sc.get(&off, (size_t)n_rows))) return st;
      hipLaunchKernelGGL(draw_counts_kernel, dim3(blocks_for(n_rows)), dim3(kB), 0, stream, n_rows, n_nodes, k, nodes, rows.rowptr, cnt);
      NGPDE_LAUNCH_CHECK("draw_counts_kernel");
      if ((st = exclusive_scan_i32(cnt, off, (size_t)n_rows, sc, stream))) return st;
      hipLaunchKernelGGL(draw_kernel, dim3(blocks_for(bound)), dim3(kB), 0, stream, n_rows, n_nodes, k, (unsigned long long)seed, nodes, rows.rowptr,
                         rows.eid, cnt, off, s, t, s_out, t_out, eid_out, flags);
      NGPDE_LAUNCH_CHECK("draw_kernel");
    }
    int32_t h[kFlagWords];
    if ((st = read_flags(flags, h, stream))) return st;   // (the temporaries are freed on return: the stream must be done with them)
    NGPDE_REQUIRE(!h[kBadNode], NGPDE_ERR_INVALID_ARGUMENT, "%s: nodes holds an entry outside 0:%lld or a repeated one", fn, (long long)n_nodes - 1);
    NGPDE_REQUIRE(!h[kBadEdge], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references a node outside the %lld nodes", fn,
                  (long long)n_nodes);
    *n_out = h[kCount];
    return NGPDE_OK;
  }
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[kBadNode], NGPDE_ERR_INVALID_ARGUMENT, "%s: nodes holds an entry outside 0:%lld or a repeated one", fn, (long long)n_nodes - 1);
  return NGPDE_OK;
}

int32_t ngpde_coo_rand_split(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_first,
                             int32_t by_pair, uint64_t seed, int32_t *side_out, int64_t *kept0, int64_t *kept1, int64_t *n0_out,
                             ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const char *fn = "ngpde_coo_rand_split";
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(n0_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: n0_out is NULL", fn);
  *n0_out = 0;
  NGPDE_REQUIRE(n_first >= 0 && n_first <= n_edges, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_first %lld outside 0 : n_edges = %lld", fn,
                (long long)n_first, (long long)n_edges);
  NGPDE_REQUIRE(n_edges == 0 || (side_out && kept0 && kept1), NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  if (n_edges == 0) return NGPDE_OK;
  Scratch sc;
  int32_t *flags = nullptr, *iota = nullptr, *eid_sorted = nullptr, *upper = nullptr, *first = nullptr, *pos = nullptr;
  unsigned long long *key = nullptr, *key_sorted = nullptr;
  const size_t m = (size_t)n_edges;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&key, m)) || (st = sc.get(&key_sorted, m)) || (st = sc.get(&iota, m)) ||
      (st = sc.get(&eid_sorted, m)) || (st = sc.get(&first, m)) || (st = sc.get(&pos, m)) || (by_pair && (st = sc.get(&upper, m))))
    return st;
  hipLaunchKernelGGL(split_keys_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, by_pair,
                     (unsigned long long)seed, s, t, key, iota, upper, flags);
  NGPDE_LAUNCH_CHECK("split_keys_kernel");
  auto sort = [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_pairs(tmp, bytes, key, key_sorted, iota, eid_sorted, m, 0u, 64u, stream); };
  if ((st = with_temp(sc, sort))) return st;
  if (!by_pair) {
    hipLaunchKernelGGL(side_by_rank_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_first, eid_sorted, side_out);
    NGPDE_LAUNCH_CHECK("side_by_rank_kernel");
  } else {
    int32_t *upper_sorted = nullptr, *incl = nullptr;
    unsigned long long *tau = nullptr;
    if ((st = sc.get(&upper_sorted, m)) || (st = sc.get(&incl, m)) || (st = sc.get(&tau, 1))) return st;
    NGPDE_HIP_CHECK(hipMemsetAsync(tau, 0, sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(upper_sorted_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, eid_sorted, upper, upper_sorted);
    NGPDE_LAUNCH_CHECK("upper_sorted_kernel");
    if ((st = inclusive_scan_i32(upper_sorted, incl, m, sc, stream))) return st;
    hipLaunchKernelGGL(threshold_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_first, key_sorted, upper_sorted, incl, tau, flags);
    NGPDE_LAUNCH_CHECK("threshold_kernel");
    hipLaunchKernelGGL(side_by_threshold_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_first, key, tau, side_out);
    NGPDE_LAUNCH_CHECK("side_by_threshold_kernel");
  }
  hipLaunchKernelGGL(first_flags_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, side_out, first);
  NGPDE_LAUNCH_CHECK("first_flags_kernel");
  if ((st = exclusive_scan_i32(first, pos, m, sc, stream))) return st;
  hipLaunchKernelGGL(split_compact_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, first, pos, kept0, kept1, flags);
  NGPDE_LAUNCH_CHECK("split_compact_kernel");
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[kBadEdge], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references a node outside the %lld nodes", fn,
                (long long)n_nodes);
  NGPDE_REQUIRE(!h[kBadCount], NGPDE_ERR_INVALID_ARGUMENT, "%s: n_first %lld exceeds the number of edges with s <= t", fn, (long long)n_first);
  *n0_out = h[kCount];
  return NGPDE_OK;
}

}  // extern "C"
