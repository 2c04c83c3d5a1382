// graph_ops.hip -- queries and transforms on a COO list that lives in HBM (include/ngpde.h, "graph queries and transforms"): degree, the
// self-loop / multi-edge / bidirected predicates, stable compaction (self-loop removal, induced subgraph), coalescing with an optional
// symmetrisation (remove_multi_edges, to_bidirected), the reduction of the coalesced edges' features with its pullback, and the
// self-loop append.  The step between the neighbour search (neighbors.hip) and the handle builder (graph_device.hip): a minibatch of
// unseen clouds never leaves the device on its way to updategraph (docs/src/tutorials/VMH.md:132-134 of the reference).
//
// Order guarantees, all by construction (no float atomics anywhere; the int32 counts use integer atomics, which commute):
//   compaction       flags -> exclusive scan -> scatter: kept edges stay in COO order
//   coalesce         stable LSD radix sort (rocPRIM) of the copies by the 64-bit key s*n + t: groups ascend by (s, t), the members of a
//                    group ascend by copy number, i.e. by COO position
//   weighted degree  stable sort of the COO positions by node, one thread per node adds its run front to back
//   group reduce     one lane walks a group's members in that order
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "coo_compact.h"
#include "row_lanes.h"

namespace ngpde {

namespace {

// device flag words of one call
enum { kBad = 0, kSelf = 1, kMulti = 2, kAsym = 3, kCount = 4 };

// ---- keys ---------------------------------------------------------------------------------------------------------------------
// copy c < E is edge c, copy c >= E edge c - E reversed; `reverse` flips every copy.  An end outside the node range raises kBad and
// the copy takes key 0.
__global__ void pair_keys_kernel(int64_t n_copies, int64_t n_edges, int64_t n, int base, int reverse, const int32_t *__restrict__ s,
                                 const int32_t *__restrict__ t, unsigned long long *__restrict__ key, int32_t *__restrict__ iota,
                                 int32_t *__restrict__ flags) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_copies) return;
  const int64_t e = c < n_edges ? c : c - n_edges;
  int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    atomicOr(&flags[kBad], 1);
    a = b = 0;
  } else if (a == b) {
    atomicOr(&flags[kSelf], 1);
  }
  if ((c >= n_edges) != (reverse != 0)) {
    const int64_t x = a;
    a = b;
    b = x;
  }
  key[c] = (unsigned long long)a * (unsigned long long)n + (unsigned long long)b;
  if (iota) iota[c] = (int32_t)c;
}

__global__ void flags_kernel(int64_t m, const unsigned long long *__restrict__ fwd, const unsigned long long *__restrict__ rev,
                             int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  if (p > 0 && fwd[p] == fwd[p - 1]) atomicOr(&flags[kMulti], 1);
  if (fwd[p] != rev[p]) atomicOr(&flags[kAsym], 1);
}

// ---- degree -------------------------------------------------------------------------------------------------------------------
__global__ void degree_count_kernel(int64_t m, int64_t n, int base, int dir, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                                    int32_t *__restrict__ deg, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    atomicOr(&flags[kBad], 1);
    return;
  }
  if (dir != NGPDE_DIR_IN) atomicAdd(&deg[a], 1);
  if (dir != NGPDE_DIR_OUT) atomicAdd(&deg[b], 1);
}

__global__ void node_keys_kernel(int64_t m, int64_t n, int base, const int32_t *__restrict__ end, uint32_t *__restrict__ key,
                                 int32_t *__restrict__ iota, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  int64_t a = (int64_t)end[e] - base;
  if (a < 0 || a >= n) {
    atomicOr(&flags[kBad], 1);
    a = 0;
  }
  key[e] = (uint32_t)a;
  iota[e] = (int32_t)e;
}

// one thread per node: its run of the sorted positions, added front to back (COO order: the sort is stable)
__global__ void degree_sum_kernel(int64_t n, int64_t m, const uint32_t *__restrict__ key, const int32_t *__restrict__ eid,
                                  const float *__restrict__ w, int accumulate, float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t p = lower_bound_dev(key, m, (uint32_t)i);
  float acc = 0.f;
  for (; p < m && key[p] == (uint32_t)i; ++p) acc += w[eid[p]];
  out[i] = accumulate ? out[i] + acc : acc;
}

// ---- compaction ---------------------------------------------------------------------------------------------------------------
__global__ void relabel_kernel(int64_t n_keep, int64_t n, const int64_t *__restrict__ nodes, int32_t *__restrict__ relabel,
                               int32_t *__restrict__ flags) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_keep) return;
  const int64_t v = nodes[k];
  if (v < 0 || v >= n) atomicOr(&flags[kBad], 1);
  else if (atomicCAS(&relabel[v], -1, (int32_t)k) != -1) atomicOr(&flags[kBad], 1);   // listed twice
}

__global__ void keep_kernel(int64_t m, int64_t n, int base, int drop_self_loops, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                            const int32_t *__restrict__ relabel, int32_t *__restrict__ keep, int32_t *__restrict__ flags) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  int k = 1;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    atomicOr(&flags[kSelf], 1);   // (kBad is the node list's here)
    k = 0;
  } else {
    if (drop_self_loops && a == b) k = 0;
    if (relabel && (relabel[a] < 0 || relabel[b] < 0)) k = 0;
  }
  keep[e] = k;
}

// ---- coalesce -----------------------------------------------------------------------------------------------------------------
__global__ void heads_kernel(int64_t m, const unsigned long long *__restrict__ key, int32_t *__restrict__ head) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < m) head[p] = (p == 0 || key[p] != key[p - 1]) ? 1 : 0;
}

// incl = inclusive scan of the heads: the sorted copy p lies in group incl[p] - 1
__global__ void groups_kernel(int64_t m, int64_t n_edges, int64_t n, int base, const unsigned long long *__restrict__ key,
                              const int32_t *__restrict__ copy, const int32_t *__restrict__ head, const int32_t *__restrict__ incl,
                              int32_t *__restrict__ s_out, int32_t *__restrict__ t_out, int32_t *__restrict__ group_ptr,
                              int32_t *__restrict__ member, int32_t *__restrict__ group_of, int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int32_t g = incl[p] - 1;
  const int32_t c = copy[p];
  member[p] = (int32_t)(c < n_edges ? c : c - n_edges);
  group_of[c] = g;
  if (head[p]) {
    const unsigned long long k = key[p];
    s_out[g] = (int32_t)(k / (unsigned long long)n) + base;
    t_out[g] = (int32_t)(k % (unsigned long long)n) + base;
    group_ptr[g] = (int32_t)p;
  }
  if (p == m - 1) {
    group_ptr[g + 1] = (int32_t)m;
    flags[kCount] = g + 1;
  }
}

// ---- group reduce -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float vdiv(float a, float c) { return a / c; }
__device__ __forceinline__ float4 vdiv(float4 a, float c) { return make_float4(a.x / c, a.y / c, a.z / c, a.w / c); }

// a lane per (group, column chunk): T = float4 covers 4 columns, T = float one; w = chunks per row.  Adjacent lanes take adjacent
// chunks of the same group, so a member row is read as one contiguous run.
template <typename T>
__global__ void group_reduce_fwd_kernel(int64_t n_groups, int w, int aggr, const int32_t *__restrict__ group_ptr,
                                        const int32_t *__restrict__ member, const T *__restrict__ src, T *__restrict__ out) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_groups * w) return;
  const int64_t g = idx / w;
  const int c = (int)(idx - g * w);
  const int32_t begin = group_ptr[g], end = group_ptr[g + 1];
  T acc = vzero(T());
  if (begin < end) {
    acc = src[(size_t)member[begin] * w + c];
    for (int32_t p = begin + 1; p < end; ++p) {
      const T v = src[(size_t)member[p] * w + c];
      acc = aggr == NGPDE_AGGR_MAX ? vmax(acc, v) : aggr == NGPDE_AGGR_MIN ? vmin(acc, v) : vadd(acc, v);
    }
    if (aggr == NGPDE_AGGR_MEAN) acc = vdiv(acc, (float)(end - begin));
  }
  out[idx] = acc;
}

template <typename T>
__global__ void group_reduce_bwd_kernel(int64_t n_rows, int copies, int w, int aggr, const int32_t *__restrict__ group_ptr,
                                        const int32_t *__restrict__ group_of, const T *__restrict__ src, const T *__restrict__ out,
                                        const T *__restrict__ dout, T *__restrict__ dsrc) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n_rows * w) return;
  const int64_t r = idx / w;
  const int c = (int)(idx - r * w);
  T acc = vzero(T());
  for (int k = 0; k < copies; ++k) {
    const int32_t g = group_of[r + (int64_t)k * n_rows];
    T term = dout[(size_t)g * w + c];
    if (aggr == NGPDE_AGGR_MEAN) term = vdiv(term, (float)(group_ptr[g + 1] - group_ptr[g]));
    if (aggr == NGPDE_AGGR_MAX || aggr == NGPDE_AGGR_MIN) term = vsel_eq(src[idx], out[(size_t)g * w + c], term);
    acc = k == 0 ? term : vadd(acc, term);
  }
  dsrc[idx] = acc;
}

// ---- self-loop append ---------------------------------------------------------------------------------------------------------
__global__ void add_self_loops_kernel(int64_t n, int64_t m, int base, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                                      const float *__restrict__ w, int32_t *__restrict__ s_out, int32_t *__restrict__ t_out,
                                      float *__restrict__ w_out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m + n) return;
  if (i < m) {
    s_out[i] = s[i];
    t_out[i] = t[i];
    if (w_out) w_out[i] = w[i];
  } else {
    const int32_t v = (int32_t)(i - m) + base;
    s_out[i] = v;
    t_out[i] = v;
    if (w_out) w_out[i] = 1.0f;
  }
}

// ---- host helpers -------------------------------------------------------------------------------------------------------------
// the keys of the copies, sorted; with `copy_sorted`, the stable permutation too
int32_t sorted_pair_keys(int64_t n_copies, int64_t n_edges, int64_t n, int base, int reverse, const int32_t *s, const int32_t *t,
                         unsigned long long **key_sorted, int32_t **copy_sorted, bool want_copies, int32_t *flags, Scratch &sc,
                         hipStream_t stream) {
  unsigned long long *key = nullptr;
  int32_t *iota = nullptr;
  int32_t st;
  if ((st = sc.get(&key, (size_t)n_copies)) || (st = sc.get(key_sorted, (size_t)n_copies))) return st;
  if (want_copies && ((st = sc.get(&iota, (size_t)n_copies)) || (st = sc.get(copy_sorted, (size_t)n_copies)))) return st;
  hipLaunchKernelGGL(pair_keys_kernel, dim3(blocks_for(n_copies)), dim3(kB), 0, stream, n_copies, n_edges, n, base, reverse, s, t, key, iota,
                     flags);
  NGPDE_LAUNCH_CHECK("pair_keys_kernel");
  const unsigned end_bit = bits_for((unsigned long long)n * (unsigned long long)n);
  return with_temp(sc, [&](void *tmp, size_t &bytes) {
    return want_copies ? rocprim::radix_sort_pairs(tmp, bytes, key, *key_sorted, iota, *copy_sorted, (size_t)n_copies, 0u, end_bit, stream)
                       : rocprim::radix_sort_keys(tmp, bytes, key, *key_sorted, (size_t)n_copies, 0u, end_bit, stream);
  });
}

int32_t check_reduce(const char *fn, int64_t n_groups, int64_t n_rows, int32_t d, int32_t aggr) {
  NGPDE_REQUIRE(n_groups >= 0 && n_rows >= 0 && n_groups <= 0x7fffffffLL && n_rows <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: sizes outside 0 : 2^31 - 1 (n_groups %lld, n_rows %lld)", fn, (long long)n_groups, (long long)n_rows);
  NGPDE_REQUIRE(d >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative width %d", fn, d);
  NGPDE_REQUIRE(aggr == NGPDE_AGGR_SUM || aggr == NGPDE_AGGR_MEAN || aggr == NGPDE_AGGR_MAX || aggr == NGPDE_AGGR_MIN, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: aggregation %d not supported (+, mean, max and min are)", fn, aggr);
  NGPDE_REQUIRE(std::max(n_groups, n_rows) * (int64_t)std::max(d, 1) <= 0x7fffffffLL * (int64_t)kB, NGPDE_ERR_UNSUPPORTED,
                "%s: more elements than one launch covers", fn);
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_coo_degree(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                         const float *w, int32_t *out_counts, float *out_sums, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_coo("ngpde_coo_degree", n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(dir == NGPDE_DIR_OUT || dir == NGPDE_DIR_IN || dir == NGPDE_DIR_BOTH, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_coo_degree: dir %d is none of NGPDE_DIR_OUT / IN / BOTH", dir);
  NGPDE_REQUIRE(n_nodes == 0 || ((out_counts != nullptr) != (out_sums != nullptr)), NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_coo_degree: output is NULL or both are given (exactly one of out_counts / out_sums is written)");
  NGPDE_REQUIRE(!out_sums || w || n_edges == 0, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_degree: out_sums without w");
  if (n_nodes == 0) return NGPDE_OK;
  Scratch sc;
  int32_t *flags = nullptr;
  if (int32_t st = new_flags(sc, &flags, stream)) return st;
  if (!out_sums) {
    NGPDE_HIP_CHECK(hipMemsetAsync(out_counts, 0, (size_t)n_nodes * sizeof(int32_t), stream));
    if (n_edges > 0) {
      hipLaunchKernelGGL(degree_count_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, dir, s, t, out_counts,
                         flags);
      NGPDE_LAUNCH_CHECK("degree_count_kernel");
    }
  } else {
    uint32_t *key = nullptr, *key_sorted = nullptr;
    int32_t *iota = nullptr, *eid = nullptr;
    int32_t st;
    if ((st = sc.get(&key, (size_t)n_edges)) || (st = sc.get(&key_sorted, (size_t)n_edges)) || (st = sc.get(&iota, (size_t)n_edges)) ||
        (st = sc.get(&eid, (size_t)n_edges)))
      return st;
    const unsigned end_bit = bits_for(std::max<int64_t>(n_nodes, 2));
    auto sort = [&](void *tmp, size_t &bytes) {
      return rocprim::radix_sort_pairs(tmp, bytes, key, key_sorted, iota, eid, (size_t)n_edges, 0u, end_bit, stream);
    };
    size_t sort_bytes = 0;
    void *sort_tmp = nullptr;   // one temporary for the sorts of both directions
    if (n_edges > 0 && ((st = temp_bytes(&sort_bytes, sort)) || (st = sc.get((char **)&sort_tmp, sort_bytes)))) return st;
    int pass = 0;
    for (int which : {NGPDE_DIR_OUT, NGPDE_DIR_IN}) {
      if (dir != NGPDE_DIR_BOTH && dir != which) continue;
      if (n_edges > 0) {
        hipLaunchKernelGGL(node_keys_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base,
                           which == NGPDE_DIR_OUT ? s : t, key, iota, flags);
        NGPDE_LAUNCH_CHECK("node_keys_kernel");
        NGPDE_HIP_CHECK(sort(sort_tmp, sort_bytes));
      }
      hipLaunchKernelGGL(degree_sum_kernel, dim3(blocks_for(n_nodes)), dim3(kB), 0, stream, n_nodes, n_edges, key_sorted, eid, w, pass, out_sums);
      NGPDE_LAUNCH_CHECK("degree_sum_kernel");
      ++pass;
    }
  }
  int32_t h[kFlagWords];
  if (int32_t st = read_flags(flags, h, stream)) return st;   // (the temporaries are freed on return: the stream must be done with them)
  NGPDE_REQUIRE(!h[kBad], NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_coo_degree: DimensionMismatch: an edge references a node outside the %lld nodes",
                (long long)n_nodes);
  return NGPDE_OK;
}

int32_t ngpde_coo_flags(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t *has_self_loops,
                        int32_t *has_multi_edges, int32_t *is_bidirected, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_coo("ngpde_coo_flags", n_nodes, n_edges, s, t)) return st;
  int32_t h[kFlagWords] = {0};
  if (n_edges > 0) {
    Scratch sc;
    int32_t *flags = nullptr;
    unsigned long long *fwd = nullptr, *rev = nullptr;
    int32_t st;
    if ((st = new_flags(sc, &flags, stream)) ||
        (st = sorted_pair_keys(n_edges, n_edges, n_nodes, index_base, 0, s, t, &fwd, nullptr, false, flags, sc, stream)) ||
        (st = sorted_pair_keys(n_edges, n_edges, n_nodes, index_base, 1, s, t, &rev, nullptr, false, flags, sc, stream)))
      return st;
    hipLaunchKernelGGL(flags_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, fwd, rev, flags);
    NGPDE_LAUNCH_CHECK("flags_kernel");
    if ((st = read_flags(flags, h, stream))) return st;
  }
  NGPDE_REQUIRE(!h[kBad], NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_coo_flags: DimensionMismatch: an edge references a node outside the %lld nodes",
                (long long)n_nodes);
  if (has_self_loops) *has_self_loops = h[kSelf] ? 1 : 0;
  if (has_multi_edges) *has_multi_edges = h[kMulti] ? 1 : 0;
  if (is_bidirected) *is_bidirected = h[kAsym] ? 0 : 1;
  return NGPDE_OK;
}

int32_t ngpde_coo_compact(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_keep,
                          const int64_t *nodes, int32_t drop_self_loops, int32_t *s_out, int32_t *t_out, int64_t *kept, int64_t *n_out,
                          ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_coo("ngpde_coo_compact", n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_compact: n_out is NULL");
  *n_out = 0;
  NGPDE_REQUIRE(n_keep >= 0 && n_keep <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_compact: n_keep %lld outside 0 : 2^31 - 1",
                (long long)n_keep);
  NGPDE_REQUIRE(nodes || n_keep == 0, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_compact: nodes is NULL with n_keep %lld", (long long)n_keep);
  NGPDE_REQUIRE(n_edges == 0 || (s_out && t_out && kept), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_compact: an output is NULL");
  Scratch sc;
  int32_t *flags = nullptr, *relabel = nullptr, *keep = nullptr, *pos = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream))) return st;
  if (nodes) {
    if ((st = sc.get(&relabel, (size_t)n_nodes))) return st;
    NGPDE_HIP_CHECK(hipMemsetAsync(relabel, 0xff, (size_t)n_nodes * sizeof(int32_t), stream));   // -1: dropped
    if (n_keep > 0) {
      hipLaunchKernelGGL(relabel_kernel, dim3(blocks_for(n_keep)), dim3(kB), 0, stream, n_keep, n_nodes, nodes, relabel, flags);
      NGPDE_LAUNCH_CHECK("relabel_kernel");
    }
  }
  if (n_edges > 0) {
    if ((st = sc.get(&keep, (size_t)n_edges)) || (st = sc.get(&pos, (size_t)n_edges))) return st;
    hipLaunchKernelGGL(keep_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, drop_self_loops, s, t, relabel,
                       keep, flags);
    NGPDE_LAUNCH_CHECK("keep_kernel");
    if ((st = compact_flagged(n_edges, index_base, s, t, relabel, keep, pos, s_out, t_out, kept, flags + kCount, sc, stream))) return st;
  }
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[kBad], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_compact: nodes holds an entry outside 0:%lld or a repeated one",
                (long long)n_nodes - 1);
  NGPDE_REQUIRE(!h[kSelf], NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_coo_compact: DimensionMismatch: an edge references a node outside the %lld nodes",
                (long long)n_nodes);
  *n_out = h[kCount];
  return NGPDE_OK;
}

int32_t ngpde_coo_coalesce(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t symmetrize,
                           int32_t *s_out, int32_t *t_out, int32_t *group_ptr, int32_t *member, int32_t *group_of, int64_t *n_out,
                           ngpde_stream_t stream_) {
  NGPDE_RANGE();
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_coo("ngpde_coo_coalesce", n_nodes, n_edges, s, t, symmetrize ? 2 : 1)) return st;
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_coalesce: n_out is NULL");
  *n_out = 0;
  NGPDE_REQUIRE(group_ptr != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_coalesce: group_ptr is NULL");
  NGPDE_REQUIRE(n_edges == 0 || (s_out && t_out && member && group_of), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_coalesce: an output is NULL");
  const int64_t m = n_edges * (symmetrize ? 2 : 1);
  if (m == 0) {
    NGPDE_HIP_CHECK(hipMemsetAsync(group_ptr, 0, sizeof(int32_t), stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    return NGPDE_OK;
  }
  Scratch sc;
  int32_t *flags = nullptr, *copy = nullptr, *head = nullptr, *incl = nullptr;
  unsigned long long *key = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) ||
      (st = sorted_pair_keys(m, n_edges, n_nodes, index_base, 0, s, t, &key, &copy, true, flags, sc, stream)) ||
      (st = sc.get(&head, (size_t)m)) || (st = sc.get(&incl, (size_t)m)))
    return st;
  hipLaunchKernelGGL(heads_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, key, head);
  NGPDE_LAUNCH_CHECK("heads_kernel");
  if ((st = scan_i32(true, head, incl, (size_t)m, sc, stream))) return st;
  hipLaunchKernelGGL(groups_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, n_edges, n_nodes, index_base, key, copy, head, incl, s_out, t_out,
                     group_ptr, member, group_of, flags);
  NGPDE_LAUNCH_CHECK("groups_kernel");
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[kBad], NGPDE_ERR_DIMENSION_MISMATCH, "ngpde_coo_coalesce: DimensionMismatch: an edge references a node outside the %lld nodes",
                (long long)n_nodes);
  *n_out = h[kCount];
  return NGPDE_OK;
}

int32_t ngpde_group_reduce_forward(int64_t n_groups, int64_t n_rows, int32_t d, int32_t aggr, const int32_t *group_ptr,
                                   const int32_t *member, const float *src, float *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_reduce("ngpde_group_reduce_forward", n_groups, n_rows, d, aggr)) return st;
  if (d == 0 || n_groups == 0) return NGPDE_OK;
  NGPDE_REQUIRE(group_ptr && member && src && out, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_group_reduce_forward: NULL argument");
  if (d % 4 == 0 && al16(src) && al16(out)) {
    const int w = d / 4;
    hipLaunchKernelGGL(group_reduce_fwd_kernel<float4>, dim3(blocks_for(n_groups * w)), dim3(kB), 0, (hipStream_t)stream, n_groups, w, aggr,
                       group_ptr, member, reinterpret_cast<const float4 *>(src), reinterpret_cast<float4 *>(out));
  } else {
    hipLaunchKernelGGL(group_reduce_fwd_kernel<float>, dim3(blocks_for(n_groups * d)), dim3(kB), 0, (hipStream_t)stream, n_groups, d, aggr,
                       group_ptr, member, src, out);
  }
  NGPDE_LAUNCH_CHECK("group_reduce_fwd_kernel");
  return NGPDE_OK;
}

int32_t ngpde_group_reduce_backward(int64_t n_groups, int64_t n_rows, int32_t copies, int32_t d, int32_t aggr, const int32_t *group_ptr,
                                    const int32_t *group_of, const float *src, const float *out, const float *dout, float *dsrc,
                                    ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_reduce("ngpde_group_reduce_backward", n_groups, n_rows, d, aggr)) return st;
  NGPDE_REQUIRE(copies == 1 || copies == 2, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_group_reduce_backward: copies is %d, not 1 or 2", copies);
  if (d == 0 || n_rows == 0) return NGPDE_OK;
  const bool ext = aggr == NGPDE_AGGR_MAX || aggr == NGPDE_AGGR_MIN;
  NGPDE_REQUIRE(group_ptr && group_of && dout && dsrc && (!ext || (src && out)), NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_group_reduce_backward: NULL argument");
  if (d % 4 == 0 && al16(src) && al16(out) && al16(dout) && al16(dsrc)) {
    const int w = d / 4;
    hipLaunchKernelGGL(group_reduce_bwd_kernel<float4>, dim3(blocks_for(n_rows * w)), dim3(kB), 0, (hipStream_t)stream, n_rows, copies, w, aggr,
                       group_ptr, group_of, reinterpret_cast<const float4 *>(src), reinterpret_cast<const float4 *>(out),
                       reinterpret_cast<const float4 *>(dout), reinterpret_cast<float4 *>(dsrc));
  } else {
    hipLaunchKernelGGL(group_reduce_bwd_kernel<float>, dim3(blocks_for(n_rows * d)), dim3(kB), 0, (hipStream_t)stream, n_rows, copies, d, aggr,
                       group_ptr, group_of, src, out, dout, dsrc);
  }
  NGPDE_LAUNCH_CHECK("group_reduce_bwd_kernel");
  return NGPDE_OK;
}

int32_t ngpde_coo_add_self_loops(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, const float *w,
                                 int32_t *s_out, int32_t *t_out, float *w_out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_coo("ngpde_coo_add_self_loops", n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(n_edges + n_nodes <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_add_self_loops: %lld edges with the loops, at most 2^31 - 1",
                (long long)(n_edges + n_nodes));
  if (n_edges + n_nodes == 0) return NGPDE_OK;
  NGPDE_REQUIRE(s_out && t_out, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_add_self_loops: s_out / t_out is NULL");
  NGPDE_REQUIRE(!w_out || w || n_edges == 0, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_coo_add_self_loops: w_out without w");
  hipLaunchKernelGGL(add_self_loops_kernel, dim3(blocks_for(n_edges + n_nodes)), dim3(kB), 0, (hipStream_t)stream, n_nodes, n_edges, index_base, s, t,
                     w, s_out, t_out, w_out);
  NGPDE_LAUNCH_CHECK("add_self_loops_kernel");
  return NGPDE_OK;
}

}  // extern "C"
