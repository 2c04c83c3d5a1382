// graph_edit.hip -- edits of a COO list that lives in HBM (include/ngpde.h, "graph editing"): the transforms of the GNNGraphs re-export
// (src/NeuralGraphPDE.jl:4 of the reference) that CHANGE a graph -- add_edges, remove_edges, remove_nodes, to_unidirected -- and
// negative_sample.  The sibling of graph_ops.hip and sampling.hip: a cloud refined or cut between two updategraph calls, or the
// non-edges an edge predictor trains against, without the COO lists leaving the device.
//
// Order guarantees, all by construction (no float anywhere; the int32 flag words use integer atomics, which commute):
//   append           slot i of the output is computed, not raced for: the old edges in order, then the new ones in the order given
//   removal          flags -> exclusive scan -> scatter (coo_compact.h, shared with ngpde_coo_compact): kept edges stay in COO order
//   complement       the same scan over the nodes: ascending
//   negative sample  the FIRST n_target distinct negatives of one fixed candidate sequence, in sequence order (below)
//
// Negative sampling.  Candidate j = 0, 1, 2, ... is a pure function of (seed, j): the code c_j = (draw(stream 4, counter j) * U) >> 64
// with U = N (N - 1) decodes to an ordered pair without a loop.  The sequence is walked in chunks.  A chunk's candidates are looked up
// in the sorted keys of the graph and in the keys accepted so far (binary searches), the survivors are sorted stably by key with j as
// the payload -- so the head of every key group is that pair's first occurrence in the chunk -- and the heads are merged into the
// accepted set, which therefore holds, after any number of chunks of any size, every distinct negative among the candidates walked so
// far with the position of its first occurrence.  Sorting that set by j and cutting at n_target gives the same bits for every chunk size.
#include <algorithm>
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
enum { kBadEnd = 0, kCross = 1, kBadListed = 2, kBadEdge = 3, kCount = 4, kPairs = 5 };

using u64 = unsigned long long;

// is v among the m ascending keys?
__device__ __forceinline__ bool contains_u64(const u64 *__restrict__ key, int64_t m, u64 v) {
  const int64_t lo = lower_bound_dev(key, m, v);
  return lo < m && key[lo] == v;
}

// ---- append -------------------------------------------------------------------------------------------------------------------
// slot i < m: old edge i, copied; slot m + k: new edge k, whose ends are checked against the node range (kBadEnd) and, with graph_of,
// against each other's graph (kCross).  A bad end is copied as it is: the call fails and nothing indexes by it.
__global__ void append_kernel(int64_t m, int64_t n_new, int64_t n, int base, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                              const int32_t *__restrict__ s_new, const int32_t *__restrict__ t_new, const int32_t *__restrict__ graph_of,
                              int32_t *__restrict__ s_out, int32_t *__restrict__ t_out, int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m + n_new) return;
  if (i < m) {
    s_out[i] = s[i];
    t_out[i] = t[i];
    return;
  }
  const int32_t sa = s_new[i - m], tb = t_new[i - m];
  const int64_t a = (int64_t)sa - base, b = (int64_t)tb - base;
  if (a < 0 || a >= n || b < 0 || b >= n) atomicOr(&flags[kBadEnd], 1);
  else if (graph_of && graph_of[a] != graph_of[b]) atomicOr(&flags[kCross], 1);
  s_out[i] = sa;
  t_out[i] = tb;
}

// ---- removal ------------------------------------------------------------------------------------------------------------------
__global__ void fill_i32_kernel(int64_t m, int32_t v, int32_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = v;
}

// keep[p] = 0 for every listed position p (a repeat stores the same 0 again); an entry outside 0 : m - 1 raises kBadListed
__global__ void drop_positions_kernel(int64_t n_listed, int64_t m, const int64_t *__restrict__ positions, int32_t *__restrict__ keep,
                                      int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_listed) return;
  const int64_t p = positions[i];
  if (p < 0 || p >= m) atomicOr(&flags[kBadListed], 1);
  else keep[p] = 0;
}

// the 64-bit key a * n + b of every pair of a list (canonical != 0: of (min, max)); an end outside the node range raises flags[bad]
// and the pair takes key 0
__global__ void pair_keys_kernel(int64_t m, int64_t n, int base, int canonical, int bad, const int32_t *__restrict__ s,
                                 const int32_t *__restrict__ t, u64 *__restrict__ key, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    atomicOr(&flags[bad], 1);
    a = b = 0;
  }
  if (canonical && a > b) {
    const int64_t x = a;
    a = b;
    b = x;
  }
  key[e] = (u64)a * (u64)n + (u64)b;
}

// keep[e] = the pair of edge e is not among the sorted listed keys
__global__ void drop_pairs_kernel(int64_t m, int64_t n, int base, int64_t n_listed, const u64 *__restrict__ listed,
                                  const int32_t *__restrict__ s, const int32_t *__restrict__ t, int32_t *__restrict__ keep,
                                  int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    atomicOr(&flags[kBadEdge], 1);
    keep[e] = 0;
    return;
  }
  keep[e] = contains_u64(listed, n_listed, (u64)a * (u64)n + (u64)b) ? 0 : 1;
}

// ---- complement ---------------------------------------------------------------------------------------------------------------
__global__ void drop_nodes_kernel(int64_t n_listed, int64_t n, const int64_t *__restrict__ nodes, int32_t *__restrict__ keep,
                                  int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_listed) return;
  const int64_t v = nodes[i];
  if (v < 0 || v >= n) atomicOr(&flags[kBadListed], 1);
  else keep[v] = 0;
}

__global__ void iota_compact_kernel(int64_t n, const int32_t *__restrict__ keep, const int32_t *__restrict__ pos, int64_t *__restrict__ out,
                                    int32_t *__restrict__ count) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= n) return;
  const int32_t p = pos[v];
  if (keep[v]) out[p] = v;
  if (v == n - 1) *count = p + keep[v];
}

// ---- orient -------------------------------------------------------------------------------------------------------------------
__global__ void orient_kernel(int64_t m, const int32_t *__restrict__ s, const int32_t *__restrict__ t, int32_t *__restrict__ s_out,
                              int32_t *__restrict__ t_out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int32_t a = s[e], b = t[e];
  s_out[e] = a < b ? a : b;
  t_out[e] = a < b ? b : a;
}

// ---- negative sampling --------------------------------------------------------------------------------------------------------
// flags[kPairs] = the number of distinct keys a * n + b with a != b among the m ascending keys
__global__ void count_pairs_kernel(int64_t m, u64 n, const u64 *__restrict__ key, int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool is = false;
  if (p < m) {
    const u64 k = key[p];
    is = (k / n != k % n) && (p == 0 || key[p - 1] != k);
  }
  const u64 mask = __ballot(is);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&flags[kPairs], __popcll(mask));
}

// candidate j = first + i: its key, or `none` (one past the largest key) if the pair is an edge of the graph or already accepted
__global__ void candidates_kernel(int64_t c, u64 first, u64 seed, u64 n, u64 n_codes, int canonical, const u64 *__restrict__ graph,
                                  int64_t n_graph, const u64 *__restrict__ accepted, int64_t n_accepted, u64 none, u64 *__restrict__ key,
                                  u64 *__restrict__ seq) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  const u64 j = first + (u64)i;
  const u64 code = __umul64hi(philox_draw(seed, kStreamNegative, (uint32_t)j, (uint32_t)(j >> 32)), n_codes);
  u64 a = code / (n - 1);
  u64 b = code % (n - 1);
  b += b >= a ? 1 : 0;
  if (canonical && a > b) {
    const u64 x = a;
    a = b;
    b = x;
  }
  const u64 k = a * n + b;
  key[i] = (contains_u64(graph, n_graph, k) || contains_u64(accepted, n_accepted, k)) ? none : k;
  seq[i] = j;
}

__global__ void new_heads_kernel(int64_t c, u64 none, const u64 *__restrict__ key, int32_t *__restrict__ head) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < c) head[p] = (key[p] != none && (p == 0 || key[p] != key[p - 1])) ? 1 : 0;
}

__global__ void take_heads_kernel(int64_t c, const u64 *__restrict__ key, const u64 *__restrict__ seq, const int32_t *__restrict__ head,
                                  const int32_t *__restrict__ pos, u64 *__restrict__ key_new, u64 *__restrict__ seq_new,
                                  int32_t *__restrict__ count) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= c) return;
  const int32_t q = pos[p];
  if (head[p]) {
    key_new[q] = key[p];
    seq_new[q] = seq[p];
  }
  if (p == c - 1) *count = q + head[p];
}

// merge by rank of two ascending key lists without a common key: the n_a accepted and the *n_new (<= c) new ones
__global__ void merge_kernel(int64_t n_a, int64_t c, const u64 *__restrict__ key_a, const u64 *__restrict__ seq_a,
                             const u64 *__restrict__ key_new, const u64 *__restrict__ seq_new, const int32_t *__restrict__ n_new_,
                             u64 *__restrict__ key_out, u64 *__restrict__ seq_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_a + c) return;
  const int64_t n_new = *n_new_;
  if (i < n_a) {
    const int64_t o = i + lower_bound_dev(key_new, n_new, key_a[i]);
    key_out[o] = key_a[i];
    seq_out[o] = seq_a[i];
  } else if (i - n_a < n_new) {
    const int64_t k = i - n_a;
    const int64_t o = k + lower_bound_dev(key_a, n_a, key_new[k]);
    key_out[o] = key_new[k];
    seq_out[o] = seq_new[k];
  }
}

// the accepted pairs in sequence order: slot i holds (a, b); with `both`, slot n_target + i holds (b, a)
__global__ void decode_kernel(int64_t n_target, u64 n, int base, int both, const u64 *__restrict__ key, int32_t *__restrict__ s_out,
                              int32_t *__restrict__ t_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_target) return;
  const int32_t a = (int32_t)(key[i] / n) + base, b = (int32_t)(key[i] % n) + base;
  s_out[i] = a;
  t_out[i] = b;
  if (both) {
    s_out[n_target + i] = b;
    t_out[n_target + i] = a;
  }
}

int32_t sort_keys_u64(const u64 *in, u64 *out, size_t count, unsigned end_bit, Scratch &sc, hipStream_t stream) {
  return with_temp(sc, [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_keys(tmp, bytes, in, out, count, 0u, end_bit, stream); });
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_coo_append(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_new,
                         const int32_t *s_new, const int32_t *t_new, const int32_t *graph_of, int32_t *s_out, int32_t *t_out,
                         ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const char *fn = "ngpde_coo_append";
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(n_new >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative number of new edges %lld", fn, (long long)n_new);
  NGPDE_REQUIRE(n_edges + n_new <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld edges after the append, at most 2^31 - 1", fn,
                (long long)(n_edges + n_new));
  NGPDE_REQUIRE(n_new == 0 || (s_new && t_new), NGPDE_ERR_INVALID_ARGUMENT, "%s: s_new / t_new is NULL", fn);
  NGPDE_REQUIRE(n_new == 0 || n_nodes > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %lld new edges on a graph without nodes", fn,
                (long long)n_new);
  if (n_edges + n_new == 0) return NGPDE_OK;
  NGPDE_REQUIRE(s_out && t_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: s_out / t_out is NULL", fn);
  Scratch sc;
  int32_t *flags = nullptr;
  if (int32_t st = new_flags(sc, &flags, stream)) return st;
  hipLaunchKernelGGL(append_kernel, dim3(blocks_for(n_edges + n_new)), dim3(kB), 0, stream, n_edges, n_new, n_nodes, index_base, s, t, s_new,
                     t_new, graph_of, s_out, t_out, flags);
  NGPDE_LAUNCH_CHECK("append_kernel");
  int32_t h[kFlagWords];
  if (int32_t st = read_flags(flags, h, stream)) return st;
  NGPDE_REQUIRE(!h[kBadEnd], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: a new edge references a node outside the %lld nodes", fn,
                (long long)n_nodes);
  NGPDE_REQUIRE(!h[kCross], NGPDE_ERR_INVALID_ARGUMENT, "%s: a new edge joins nodes of two different graphs of the batch", fn);
  return NGPDE_OK;
}

int32_t ngpde_coo_remove_edges(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_listed,
                               const int64_t *positions, const int32_t *ls, const int32_t *lt, int32_t *s_out, int32_t *t_out, int64_t *kept,
                               int64_t *n_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const char *fn = "ngpde_coo_remove_edges";
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_out is NULL", fn);
  *n_out = 0;
  NGPDE_REQUIRE(n_listed >= 0 && n_listed <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_listed %lld outside 0 : 2^31 - 1", fn,
                (long long)n_listed);
  NGPDE_REQUIRE(!positions || (!ls && !lt), NGPDE_ERR_INVALID_ARGUMENT, "%s: both positions and pairs are given (one form per call)", fn);
  NGPDE_REQUIRE((ls != nullptr) == (lt != nullptr), NGPDE_ERR_INVALID_ARGUMENT, "%s: one of ls / lt is NULL", fn);
  NGPDE_REQUIRE(n_listed == 0 || positions || ls, NGPDE_ERR_INVALID_ARGUMENT, "%s: the list is NULL with n_listed %lld", fn, (long long)n_listed);
  NGPDE_REQUIRE(n_edges == 0 || (s_out && t_out && kept), NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  const bool by_pair = n_listed > 0 && ls;
  NGPDE_REQUIRE(!by_pair || n_nodes > 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: listed pairs on a graph without nodes", fn);
  Scratch sc;
  int32_t *flags = nullptr, *keep = nullptr, *pos = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream))) return st;
  u64 *listed = nullptr;
  if (by_pair) {   // (checked and sorted even without edges: a listed end out of range is an error of its own)
    u64 *key = nullptr;
    if ((st = sc.get(&key, (size_t)n_listed)) || (st = sc.get(&listed, (size_t)n_listed))) return st;
    hipLaunchKernelGGL(pair_keys_kernel, dim3(blocks_for(n_listed)), dim3(kB), 0, stream, n_listed, n_nodes, index_base, 0, (int)kBadListed, ls, lt,
                       key, flags);
    NGPDE_LAUNCH_CHECK("pair_keys_kernel");
    if ((st = sort_keys_u64(key, listed, (size_t)n_listed, bits_for((u64)n_nodes * (u64)n_nodes), sc, stream))) return st;
  }
  if (n_edges > 0) {
    if ((st = sc.get(&keep, (size_t)n_edges)) || (st = sc.get(&pos, (size_t)n_edges))) return st;
    if (by_pair) {
      hipLaunchKernelGGL(drop_pairs_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, n_listed, listed, s, t,
                         keep, flags);
      NGPDE_LAUNCH_CHECK("drop_pairs_kernel");
    } else {
      hipLaunchKernelGGL(fill_i32_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, 1, keep);
      NGPDE_LAUNCH_CHECK("fill_i32_kernel");
    }
  }
  if (n_listed > 0 && !by_pair) {   // (with n_edges == 0 every entry is out of range: keep is not written)
    hipLaunchKernelGGL(drop_positions_kernel, dim3(blocks_for(n_listed)), dim3(kB), 0, stream, n_listed, n_edges, positions, keep, flags);
    NGPDE_LAUNCH_CHECK("drop_positions_kernel");
  }
  if (n_edges > 0 &&
      (st = compact_flagged(n_edges, index_base, s, t, nullptr, keep, pos, s_out, t_out, kept, flags + kCount, sc, stream)))
    return st;
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[kBadListed], NGPDE_ERR_INVALID_ARGUMENT,
                by_pair ? "%s: a listed pair has an end outside 0:%lld" : "%s: a listed position lies outside 0:%lld", fn,
                (long long)(by_pair ? n_nodes : n_edges) - 1);
  NGPDE_REQUIRE(!h[kBadEdge], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references a node outside the %lld nodes", fn,
                (long long)n_nodes);
  *n_out = h[kCount];
  return NGPDE_OK;
}

int32_t ngpde_coo_complement_nodes(int64_t n_nodes, int64_t n_listed, const int64_t *nodes, int64_t *out, int64_t *n_out,
                                   ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const char *fn = "ngpde_coo_complement_nodes";
  NGPDE_REQUIRE(n_nodes >= 0 && n_listed >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n_nodes %lld, n_listed %lld)", fn,
                (long long)n_nodes, (long long)n_listed);
  NGPDE_REQUIRE(n_nodes <= 0x7fffffffLL && n_listed <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: sizes outside 0 : 2^31 - 1", fn);
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_out is NULL", fn);
  *n_out = 0;
  NGPDE_REQUIRE(nodes || n_listed == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: nodes is NULL with n_listed %lld", fn, (long long)n_listed);
  NGPDE_REQUIRE(out || n_nodes == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: out is NULL", fn);
  if (n_nodes == 0 && n_listed == 0) return NGPDE_OK;
  Scratch sc;
  int32_t *flags = nullptr, *keep = nullptr, *pos = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&keep, (size_t)n_nodes)) || (st = sc.get(&pos, (size_t)n_nodes))) return st;
  if (n_nodes > 0) {
    hipLaunchKernelGGL(fill_i32_kernel, dim3(blocks_for(n_nodes)), dim3(kB), 0, stream, n_nodes, 1, keep);
    NGPDE_LAUNCH_CHECK("fill_i32_kernel");
  }
  if (n_listed > 0) {
    hipLaunchKernelGGL(drop_nodes_kernel, dim3(blocks_for(n_listed)), dim3(kB), 0, stream, n_listed, n_nodes, nodes, keep, flags);
    NGPDE_LAUNCH_CHECK("drop_nodes_kernel");
  }
  if (n_nodes > 0) {
    if ((st = scan_i32(false, keep, pos, (size_t)n_nodes, sc, stream))) return st;
    hipLaunchKernelGGL(iota_compact_kernel, dim3(blocks_for(n_nodes)), dim3(kB), 0, stream, n_nodes, keep, pos, out, flags + kCount);
    NGPDE_LAUNCH_CHECK("iota_compact_kernel");
  }
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[kBadListed], NGPDE_ERR_INVALID_ARGUMENT, "%s: nodes holds an entry outside 0:%lld", fn, (long long)n_nodes - 1);
  *n_out = h[kCount];
  return NGPDE_OK;
}

int32_t ngpde_coo_orient(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t *s_out, int32_t *t_out,
                         ngpde_stream_t stream) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_orient";
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  if (n_edges == 0) return NGPDE_OK;
  NGPDE_REQUIRE(s_out && t_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: s_out / t_out is NULL", fn);
  hipLaunchKernelGGL(orient_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, (hipStream_t)stream, n_edges, s, t, s_out, t_out);
  NGPDE_LAUNCH_CHECK("orient_kernel");
  return NGPDE_OK;
}

int32_t ngpde_coo_negative_sample(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_target,
                                  int32_t bidirected, uint64_t seed, int64_t chunk, int32_t *s_out, int32_t *t_out, int64_t *n_out,
                                  ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  const char *fn = "ngpde_coo_negative_sample";
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_out is NULL", fn);
  *n_out = 0;
  const int copies = bidirected ? 2 : 1;
  NGPDE_REQUIRE(n_target >= 0 && n_target <= 0x7fffffffLL / copies, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_target %lld outside 0 : %lld", fn,
                (long long)n_target, 0x7fffffffLL / copies);
  NGPDE_REQUIRE(chunk >= 0 && chunk <= (1LL << 24), NGPDE_ERR_INVALID_ARGUMENT, "%s: chunk %lld outside 0 : 2^24 (0: the library's choice)", fn,
                (long long)chunk);
  if (n_target == 0) return NGPDE_OK;
  NGPDE_REQUIRE(s_out && t_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: s_out / t_out is NULL", fn);
  const u64 n = (u64)n_nodes;
  const u64 n_codes = n > 1 ? n * (n - 1) : 0;            // U: the ordered pairs without a loop, < 2^62
  const u64 n_eff = bidirected ? n_codes / 2 : n_codes;   // U_eff
  NGPDE_REQUIRE((u64)n_target <= n_eff, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld negatives asked of %lld nodes, which have %llu pairs", fn,
                (long long)n_target, (long long)n_nodes, n_eff);
  Scratch sc;
  int32_t *flags = nullptr;
  int32_t st, h[kFlagWords];
  if ((st = new_flags(sc, &flags, stream))) return st;
  // the graph's keys, ascending (of the canonical pairs with `bidirected`: a candidate is canonical too, so one search answers both
  // orientations), and K, the number of distinct non-loop ones
  const unsigned key_bits = bits_for(n * n + 1);   // the keys and `none`
  u64 *graph = nullptr;
  if (n_edges > 0) {
    u64 *key = nullptr;
    if ((st = sc.get(&key, (size_t)n_edges)) || (st = sc.get(&graph, (size_t)n_edges))) return st;
    hipLaunchKernelGGL(pair_keys_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, bidirected ? 1 : 0,
                       (int)kBadEdge, s, t, key, flags);
    NGPDE_LAUNCH_CHECK("pair_keys_kernel");
    if ((st = sort_keys_u64(key, graph, (size_t)n_edges, key_bits, sc, stream))) return st;
    hipLaunchKernelGGL(count_pairs_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n, graph, flags);
    NGPDE_LAUNCH_CHECK("count_pairs_kernel");
  }
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[kBadEdge], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references a node outside the %lld nodes", fn,
                (long long)n_nodes);
  const u64 n_pairs = (u64)h[kPairs];   // K <= U_eff
  NGPDE_REQUIRE((u64)n_target <= n_eff - n_pairs, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: %lld negatives asked, but only %llu of the %llu pairs are not edges of the graph", fn, (long long)n_target, n_eff - n_pairs,
                n_eff);
  const u64 n_free = n_eff - n_pairs;
  const unsigned __int128 cap128 = (unsigned __int128)64 * ((n_eff + n_free - 1) / n_free) * (u64)(n_target + 16);
  const u64 cap = cap128 > (unsigned __int128)0x7fffffffffffffffULL ? 0x7fffffffffffffffULL : (u64)cap128;
  if (chunk == 0) {   // enough for one round in nearly every call: the expected number of candidates per negative, and a margin
    const double expect = (double)n_target * ((double)n_eff / (double)n_free);
    chunk = (int64_t)std::min(std::max(1.25 * expect + 64.0, 256.0), (double)(1 << 22));
  }
  const size_t c = (size_t)chunk, room = (size_t)n_target + c;   // the accepted set stops growing once it holds n_target
  u64 *key = nullptr, *seq = nullptr, *key_sorted = nullptr, *seq_sorted = nullptr, *key_new = nullptr, *seq_new = nullptr;
  u64 *key_acc[2] = {nullptr, nullptr}, *seq_acc[2] = {nullptr, nullptr};
  int32_t *head = nullptr, *pos = nullptr;
  void *sort_tmp = nullptr, *scan_tmp = nullptr;   // one allocation each for all the rounds
  size_t sort_bytes = 0, scan_bytes = 0;
  // (by reference: the lists are allocated below, and a size query reads none of them)
  auto sort = [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_pairs(tmp, bytes, key, key_sorted, seq, seq_sorted, c, 0u, key_bits, stream); };
  auto scan = [&](void *tmp, size_t &bytes) { return rocprim::exclusive_scan(tmp, bytes, head, pos, 0, c, rocprim::plus<int32_t>(), stream); };
  if ((st = temp_bytes(&sort_bytes, sort)) || (st = temp_bytes(&scan_bytes, scan))) return st;
  if ((st = sc.get(&key, c)) || (st = sc.get(&seq, c)) || (st = sc.get(&key_sorted, c)) || (st = sc.get(&seq_sorted, c)) ||
      (st = sc.get(&key_new, c)) || (st = sc.get(&seq_new, c)) || (st = sc.get(&head, c)) || (st = sc.get(&pos, c)) ||
      (st = sc.get(&key_acc[0], room)) || (st = sc.get(&seq_acc[0], room)) || (st = sc.get(&key_acc[1], room)) ||
      (st = sc.get(&seq_acc[1], room)) || (st = sc.get((char **)&sort_tmp, sort_bytes)) || (st = sc.get((char **)&scan_tmp, scan_bytes)))
    return st;
  const u64 none = n * n;
  int64_t n_acc = 0;
  u64 done = 0;
  int cur = 0;
  while (n_acc < n_target) {
    NGPDE_REQUIRE(done < cap, NGPDE_ERR_STATE, "%s: %llu candidates gave %lld of the %lld negatives asked (the cap on the walk is reached)", fn, done,
                  (long long)n_acc, (long long)n_target);
    hipLaunchKernelGGL(candidates_kernel, dim3(blocks_for(chunk)), dim3(kB), 0, stream, chunk, done, (u64)seed, n, n_codes, bidirected ? 1 : 0, graph,
                       n_edges, key_acc[cur], n_acc, none, key, seq);
    NGPDE_LAUNCH_CHECK("candidates_kernel");
    NGPDE_HIP_CHECK(sort(sort_tmp, sort_bytes));
    hipLaunchKernelGGL(new_heads_kernel, dim3(blocks_for(chunk)), dim3(kB), 0, stream, chunk, none, key_sorted, head);
    NGPDE_LAUNCH_CHECK("new_heads_kernel");
    NGPDE_HIP_CHECK(scan(scan_tmp, scan_bytes));
    hipLaunchKernelGGL(take_heads_kernel, dim3(blocks_for(chunk)), dim3(kB), 0, stream, chunk, key_sorted, seq_sorted, head, pos, key_new, seq_new,
                       flags + kCount);
    NGPDE_LAUNCH_CHECK("take_heads_kernel");
    hipLaunchKernelGGL(merge_kernel, dim3(blocks_for(n_acc + chunk)), dim3(kB), 0, stream, n_acc, chunk, key_acc[cur], seq_acc[cur], key_new, seq_new,
                       flags + kCount, key_acc[cur ^ 1], seq_acc[cur ^ 1]);
    NGPDE_LAUNCH_CHECK("merge_kernel");
    if ((st = read_flags(flags, h, stream))) return st;
    n_acc += h[kCount];
    done += (u64)chunk;
    cur ^= 1;
  }
  // the accepted set in sequence order, cut at n_target
  {
    u64 *seq_by = nullptr, *key_by = nullptr;
    const unsigned seq_bits = bits_for(done + 1);
    if ((st = sc.get(&seq_by, (size_t)n_acc)) || (st = sc.get(&key_by, (size_t)n_acc))) return st;
    auto by_seq = [&](void *tmp, size_t &bytes) {
      return rocprim::radix_sort_pairs(tmp, bytes, seq_acc[cur], seq_by, key_acc[cur], key_by, (size_t)n_acc, 0u, seq_bits, stream);
    };
    if ((st = with_temp(sc, by_seq))) return st;
    hipLaunchKernelGGL(decode_kernel, dim3(blocks_for(n_target)), dim3(kB), 0, stream, n_target, n, index_base, bidirected ? 1 : 0, key_by, s_out,
                       t_out);
    NGPDE_LAUNCH_CHECK("decode_kernel");
  }
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));   // (the temporaries are freed on return: the stream must be done with them)
  *n_out = n_target * copies;
  return NGPDE_OK;
}

}  // extern "C"
