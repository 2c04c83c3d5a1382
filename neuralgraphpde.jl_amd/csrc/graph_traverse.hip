// graph_traverse.hip -- the questions whose answer needs a traversal of a COO list that lives in HBM (include/ngpde.h, "graph
// traversal"): connected_components / is_connected and gdistances / neighborhood of the Graphs.jl interface a GNNGraph answers
// (src/NeuralGraphPDE.jl:4 re-exports GNNGraphs, :16 `using Graphs` of the reference).  Every result is an integer; the only atomics
// are integer min / or / add, which commute, so the bits depend neither on the COO order, the launch geometry nor the run.  Kernel
// boundaries are the only synchronisation: no lane ever waits for another lane's progress, no grid barrier, no cooperative launch.
//
// COMPONENTS: root hooking with compression on ONE int32 word per node, parent[] (the caller's labels_out), parent[i] = i to start.
//   invariant    parent[x] <= x at every instant (values only ever decrease, and every value written to parent[x] is below x), so there
//                is no cycle and the root of a tree is its smallest member.  Between rounds every parent[x] IS x's root.
//   hook         one lane per edge (a, b): ra = parent[a], rb = parent[b]; where they differ, atomicMin(parent[max], min) at agent
//                scope, and the round's `hooked` word is set with a plain store.
//   compress     parent[i] <- the ancestor reached after kJumpLinks further links, in place, in launches of their own: every launch
//                divides the depth of the forest by kJumpLinks + 1 at least.
//                HAZARD 1, long chains: after the first hook round on a sequentially numbered path every parent[i + 1] is i -- ONE chain
//                of depth N.  A lane that walked to its root link by link would serialise N loads; here a lane reads at most
//                kJumpLinks + 2 words per launch and ceil(log2 N / 3) launches reach depth 1 (each exits at once when the launch
//                before found every node at its root).
//   HAZARD 2, stale reads inside a launch: a plain load may return a value of parent[x] that another compute unit or XCD has since
//   lowered (plain loads are not coherent across XCDs inside a kernel).  The code is correct for EVERY such value:
//     hook       the words of nodes that are not roots cannot change during the launch (only a start-of-round root is the target of an
//                atomicMin); the word of a start-of-round root r reads as r or as one of the start-of-round roots some lane has
//                hooked it under.  Either way ra and rb are start-of-round roots of the TRUE components of a and b and the edge
//                joins them, so the lane's atomicMin hooks a start-of-round root under a smaller node of its own true component:
//                trees stay subsets of true components and parent[x] <= x holds.  A link an even smaller hook overwrites is not
//                lost: its edge sees two roots again next round.  A lane never has to decide "this is a root" in this launch.
//     compress   every value parent[x] holds during the launches of a compression is an ancestor of x in the forest the hook left
//                (a word is only ever replaced by an ancestor of its value), so a stale read is an ancestor too and the lane merely
//                climbs less.  "p is a root" is decided from parent[p] == p, and a root's word cannot change in a compress launch
//                (no lane writes a value that differs from a root's own), nor can another word become a root.
//   stop         a round that hooks nothing changed no word, so all its reads were current: every edge has both ends under one root,
//                and every root is the smallest member of its component -- the labels are a function of the edge SET alone.
//
// HOP DISTANCES: level-synchronous pull on 64-bit source masks.  Bit b of seen[v] / frontier[v] belongs to source b of the pass (all
// sources share bit 0 when one distance to the NEAREST source is asked).  One level is one launch with a lane per node: it ORs the
// frontier words of the other ends of its row(s), keeps the bits it has not seen, stores level for each and writes seen[v],
// next[v] -- a lane writes its own node only: no atomics in the level loop, no race, the same bits whatever the geometry.  Rows of
// NGPDE_HOP_WAVE_ROW entries or more take the hub-row walk of traverse_rounds.h (which also holds the stop words and the round loop).
#include <algorithm>
#include <cstdint>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "coo_compact.h"
#include "coo_rows.h"
#include "traverse_rounds.h"

namespace ngpde {

namespace {

constexpr int kJumpLinks = 7;   // links a compress lane follows beyond parent[i]: a launch divides the depth by 8

// flag words of the calls that take their temporaries from Scratch (device_scratch.h)
enum { fOffender = 0, fBad = 2, fLabel = 3, fGraph = 4, fRowsBad = 5 };

int32_t edge_error(const char *fn, const int32_t *h, int at, int64_t n_nodes) {   // the 64-bit word at h[at]: the smallest offending end
  NGPDE_REQUIRE(!word_of(h, at), NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: an edge references node %lld, outside the %lld nodes", fn,
                (long long)decode_offender(word_of(h, at)), (long long)n_nodes);
  return NGPDE_OK;
}

inline int jumps_for(int64_t n) { return std::max(1, ((int)bits_for((unsigned long long)std::max<int64_t>(n, 2)) + 2) / 3); }

// ---- components -----------------------------------------------------------------------------------------------------------------
// every control word cleared but the first cTurn word: "round 0 hooked", so that round 1 runs (each word has ONE writer)
__global__ void cc_init_kernel(int64_t n, int32_t *__restrict__ parent, int32_t *__restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = (int32_t)i;
  if (i < kCtlRead) ctl[i] = i == cTurn ? 1 : 0;
}

// Round `round` >= 1; its cTurn word says "this round hooked".
__global__ void cc_hook_kernel(int64_t m, int64_t n, int base, int round, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                               int32_t *parent, int32_t *ctl) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int go = round_go(ctl, cTurn, round, e == 0);
  if (e == 0) {
    ctl[cMore] = 0;   // (the first compress launch of the round sets it)
    if (go) ctl[cRounds] = round;
  }
  if (!go || e >= m) return;
  const int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  if (a < 0 || a >= n || b < 0 || b >= n) {   // reported; nothing is read or written through it
    if (round == 1) report_offender(reinterpret_cast<unsigned long long *>(ctl + cOffender), (a < 0 || a >= n) ? a : b);
    return;
  }
  const int32_t ra = parent[a], rb = parent[b];   // start-of-round roots of the true components of a and b, whatever is read (above)
  if (ra == rb) return;
  __hip_atomic_fetch_min(&parent[ra > rb ? ra : rb], ra > rb ? rb : ra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  round_mark(ctl, cTurn, round);
}

// Launch j of the compression of round `round`: runs if the round hooked (j = 0) or the launch before left a node short of its root.
// The cMore words rotate over j as the cTurn words do over the rounds.
__global__ void cc_compress_kernel(int64_t n, int round, int j, int32_t *parent, int32_t *ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int go = ctl[j == 0 ? round_word(cTurn, round) : round_word(cMore, j + 2)];   // (round_go, but launch 0 follows the hook)
  if (i == 0) ctl[round_word(cMore, j + 1)] = 0;
  if (!go || i >= n) return;
  const int32_t p0 = parent[i];
  int32_t p = p0;
  bool root = false;
  for (int k = 0; k <= kJumpLinks; ++k) {   // (the last read only asks whether p is a root)
    const int32_t gp = parent[p];
    if (gp >= p) {   // gp == p: a root, and a root's word does not change in this launch
      root = true;
      break;
    }
    if (k == kJumpLinks) break;
    p = gp;
  }
  if (p != p0) parent[i] = p;   // an ancestor of p0: a lane that reads the old or the new word climbs the same tree
  if (!root) round_mark(ctl, cMore, j);
}

// rounds_out[0] = the rounds run (the confirming one included), rounds_out[1] = did the last enqueued round still hook?
__global__ void cc_finish_kernel(int last_round, const int32_t *__restrict__ ctl, int32_t *__restrict__ rounds_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    rounds_out[0] = ctl[cRounds];
    rounds_out[1] = ctl[round_word(cTurn, last_round)] ? 1 : 0;
  }
}

// ---- ranking --------------------------------------------------------------------------------------------------------------------
// isroot[i] = labels[i] == i.  A label that is not a root at or below its node is reported (nothing is read through it); every root
// counts for its graph (integer atomicAdd: commutes).
__global__ void rank_roots_kernel(int64_t n, const int32_t *__restrict__ labels, int32_t n_graphs, const int32_t *__restrict__ graph_of,
                                  int32_t *__restrict__ isroot, int32_t *__restrict__ per_graph, int32_t *__restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int64_t l = labels[i];
  int32_t r = 0;
  if (l < 0 || l > i || labels[l] != l) {
    atomicOr(&flags[fLabel], 1);
  } else if (l == i) {
    r = 1;
    if (per_graph) {
      const int64_t g = graph_of ? graph_of[i] : 0;
      if (g < 0 || g >= n_graphs) atomicOr(&flags[fGraph], 1);
      else atomicAdd(&per_graph[g], 1);
    }
  }
  isroot[i] = r;
}

// rank[i] = the number of roots below i's root = the rank of its component among the components ordered by smallest member
__global__ void rank_nodes_kernel(int64_t n, const int32_t *__restrict__ labels, const int32_t *__restrict__ isroot,
                                  const int32_t *__restrict__ below, int32_t *__restrict__ rank, int32_t *__restrict__ iota,
                                  int32_t *__restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t l = labels[i];
  if (l < 0 || l > i) l = i;   // (reported by rank_roots_kernel)
  rank[i] = below[l];
  iota[i] = (int32_t)i;
  if (i == n - 1) *count = below[i] + isroot[i];
}

// ptr[k] = the first sorted position whose rank is >= k, k = 0 .. count; sizes[k] = ptr[k + 1] - ptr[k]
__global__ void rank_ptr_kernel(int64_t n, const int32_t *__restrict__ sorted_rank, const int32_t *__restrict__ count,
                                int32_t *__restrict__ ptr, int32_t *__restrict__ sizes) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t c = *count;
  if (k > c) return;
  const int32_t at = (int32_t)lower_bound_dev(sorted_rank, n, (int32_t)k);
  ptr[k] = at;
  if (k < c) sizes[k] = (int32_t)lower_bound_dev(sorted_rank, n, (int32_t)(k + 1)) - at;
}

// ---- the rows plan --------------------------------------------------------------------------------------------------------------
// other[p] = the 0-based other end of the edge at sorted position p of the rows coo_rows.h built; both ends are checked here, so
// that the smallest offending id can be named
__global__ void rows_other_kernel(int64_t m, int64_t n, int base, int dir, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                                  const int32_t *__restrict__ eid, int32_t *__restrict__ other, int32_t *__restrict__ flags) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= m) return;
  const int64_t e = eid[p];
  int64_t o = 0;
  if (e < 0 || e >= m) {
    atomicOr(&flags[fBad], 1);
  } else {
    const int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
    if (a < 0 || a >= n || b < 0 || b >= n) report_offender(reinterpret_cast<unsigned long long *>(flags + fOffender), (a < 0 || a >= n) ? a : b);
    else o = dir == NGPDE_DIR_IN ? a : b;
  }
  other[p] = (int32_t)o;
}

// ---- hop distances --------------------------------------------------------------------------------------------------------------
// a pass starts: nothing seen, an empty frontier; "level 0 found something" (the sources), so that level 1 runs
__global__ void hop_init_kernel(int64_t n, u64 *__restrict__ seen, u64 *__restrict__ frontier, int32_t *__restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) seen[i] = 0, frontier[i] = 0;
  rounds_arm(ctl, cTurn, i);
}

// source i of the pass takes bit i (bit 0 in union mode) of its node's words and distance 0 in its row of dist; integer atomicOr
// commutes, and two lanes that store the same 0 do not race for a value
__global__ void hop_sources_kernel(int64_t cnt, int64_t n, int base, int separate, int64_t row0, const int64_t *__restrict__ sources,
                                   u64 *__restrict__ seen, u64 *__restrict__ frontier, int32_t *__restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const int64_t v = sources[i] - base;
  if (v < 0 || v >= n) return;   // (reported by fill_sources_kernel)
  const u64 bit = separate ? 1ull << i : 1ull;
  atomicOr(&seen[v], bit);
  atomicOr(&frontier[v], bit);
  dist[source_cell(separate, row0, i, n, v)] = 0;
}

__device__ __forceinline__ u64 wave_or(u64 v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v |= __shfl_xor(v, off, kWave);
  return v;
}

// the frontier words of the other ends of positions b .. e - 1, every `step`-th from `first`; a place outside the lists raises cCsr
// and nothing is read through it
__device__ __forceinline__ u64 or_entries(const HopRows &r, int64_t first, int64_t e, int step, int64_t n, const u64 *__restrict__ cur,
                                          int32_t *ctl) {
  u64 acc = 0;
  for (int64_t p = first; p < e; p += step) {
    const int64_t u = r.other[p];
    if (u < 0 || u >= n) ctl[cCsr] = 1;
    else acc |= cur[u];
  }
  return acc;
}

// Level `level` >= 1 of a pass: node v gets distance `level` from every source whose bit reaches it now; its cTurn word says "this
// level found a new bit".  cur is not written by this launch and every other word a lane reads or writes is its own node's, so the
// launch has no race.  A node that has seen every source of the pass reads no row.
__global__ __launch_bounds__(256) void hop_level_kernel(int64_t n, int level, HopRows ra, HopRows rb, u64 pass_mask, int64_t row0,
                                                        const u64 *__restrict__ cur, u64 *__restrict__ next, u64 *__restrict__ seen,
                                                        int32_t *__restrict__ dist, int32_t *ctl) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  if (!round_go(ctl, cTurn, level, v == 0)) return;   // (the whole grid: the level before found nothing new)
  const bool live = v < n;
  const u64 mine = live ? seen[v] : 0;
  const u64 want = live ? pass_mask & ~mine : 0;
  u64 acc = 0;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const HopRows &r = k == 0 ? ra : rb;
    if (!r.ptr) continue;   // (uniform)
    int64_t b, e;
    row_span(r, v, want != 0, b, e, ctl);
    const bool wide = e - b >= NGPDE_HOP_WAVE_ROW;
    if (!wide) acc |= or_entries(r, b, e, 1, n, cur, ctl);
    for_wide_rows(wide, b, e, [&](int owner, int64_t wb, int64_t we) {
      const u64 part = wave_or(or_entries(r, wb + lane, we, kWave, n, cur, ctl));
      if (lane == owner) acc |= part;
    });
  }
  if (!live) return;
  const u64 fresh = acc & want;
  next[v] = fresh;
  if (!fresh) return;
  seen[v] = mine | fresh;
  for (u64 bits = fresh; bits; bits &= bits - 1) {
    const int bit = __ffsll((long long)bits) - 1;
    dist[(size_t)(row0 + bit) * (size_t)n + (size_t)v] = level;
  }
  round_mark(ctl, cTurn, level);
}

// keep[i] = node i was reached
__global__ void reached_flags_kernel(int64_t n, const int32_t *__restrict__ dist, int32_t *__restrict__ keep) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keep[i] = dist[i] >= 0 ? 1 : 0;
}

// the scatter of coo_compact.h's compaction, over nodes: kept nodes stay in ascending order
__global__ void reached_scatter_kernel(int64_t n, int base, const int32_t *__restrict__ keep, const int32_t *__restrict__ pos,
                                       int64_t *__restrict__ nodes, int32_t *__restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (keep[i]) nodes[pos[i]] = i + base;
  if (i == n - 1) *count = pos[i] + keep[i];
}

// the workspace: seen, the two frontiers -- a 64-bit word per node each -- and the control block
struct HopWs {
  u64 *seen, *fr[2];
  int32_t *ctl;
};
void hop_layout(Workspace &w, int64_t n, HopWs &p) {
  p.seen = w.take<u64>((size_t)n);
  p.fr[0] = w.take<u64>((size_t)n);
  p.fr[1] = w.take<u64>((size_t)n);
  p.ctl = take_ctl(w);
}

int32_t check_rows(const char *fn, const char *what, int64_t nnz, const int32_t *ptr, const int32_t *other) {
  NGPDE_REQUIRE(nnz >= 0 && nnz <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: %s %lld outside 0 : 2^31 - 1 (negative, or too large)", fn, what,
                (long long)nnz);
  NGPDE_REQUIRE(ptr && (nnz == 0 || other), NGPDE_ERR_INVALID_ARGUMENT, "%s: a row list is NULL", fn);
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

size_t ngpde_coo_components_workspace_bytes(int64_t n_nodes) {
  if (n_nodes < 0 || n_nodes > 0x7fffffffLL) return 0;
  return kCtlBytes;
}

int32_t ngpde_coo_components(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t max_rounds,
                             int32_t check_every, int32_t *labels_out, int32_t *rounds_out, void *workspace, size_t workspace_bytes,
                             ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_coo_components";
  hipStream_t stream = (hipStream_t)stream_;
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(max_rounds >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: max_rounds %d is negative (0: the library's choice)", fn, max_rounds);
  NGPDE_REQUIRE(check_every >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: check_every %d is negative (0: no read-back)", fn, check_every);
  NGPDE_REQUIRE(labels_out || n_nodes == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: labels_out is NULL", fn);
  if (int32_t st = check_workspace(fn, workspace, workspace_bytes, kCtlBytes, 8)) return st;
  if (max_rounds == 0) {   // 2 ceil(log2 N) + 8, in whole groups
    max_rounds = 2 * (int32_t)bits_for((unsigned long long)std::max<int64_t>(n_nodes, 2)) + 8;
    if (check_every > 0) max_rounds = (max_rounds + check_every - 1) / check_every * check_every;
  }
  const int jumps = jumps_for(n_nodes);
  NGPDE_REQUIRE(check_every > 0 || (int64_t)max_rounds * (jumps + 1) <= kMaxUncheckedLaunches, NGPDE_ERR_UNSUPPORTED,
                "%s: max_rounds %d with check_every 0 would enqueue %lld launches", fn, max_rounds, (long long)max_rounds * (jumps + 1));
  int32_t *ctl = (int32_t *)workspace;
  hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_for(n_nodes)), dim3(kB), 0, stream, n_nodes, labels_out, ctl);
  NGPDE_LAUNCH_CHECK("cc_init_kernel");
  auto round = [&](int64_t r) -> int32_t {
    hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, (int)r, s, t, labels_out, ctl);
    NGPDE_LAUNCH_CHECK("cc_hook_kernel");
    for (int j = 0; j < jumps; ++j) {
      hipLaunchKernelGGL(cc_compress_kernel, dim3(blocks_for(n_nodes)), dim3(kB), 0, stream, n_nodes, (int)r, j, labels_out, ctl);
      NGPDE_LAUNCH_CHECK("cc_compress_kernel");
    }
    return NGPDE_OK;
  };
  Rounds rounds = {check_every, ctl, stream};
  if (int32_t st = rounds.run(max_rounds, round, [&](const int32_t *h) { return edge_error(fn, h, cOffender, n_nodes); })) return st;
  if (rounds_out) {
    hipLaunchKernelGGL(cc_finish_kernel, dim3(1), dim3(kWave), 0, stream, (int)rounds.last, ctl, rounds_out);
    NGPDE_LAUNCH_CHECK("cc_finish_kernel");
  }
  NGPDE_REQUIRE(check_every == 0 || rounds.done, NGPDE_ERR_STATE,
                "%s: still hooking after max_rounds = %d rounds: the labels are not final (raise max_rounds)", fn, max_rounds);
  return NGPDE_OK;
}

int32_t ngpde_components_rank(int64_t n_nodes, const int32_t *labels, int32_t n_graphs, const int32_t *graph_of, int32_t *rank_out,
                              int32_t *sizes_out, int32_t *order_out, int32_t *ptr_out, int64_t *count_out, int32_t *per_graph_out,
                              ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_components_rank";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(count_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: count_out is NULL", fn);
  *count_out = 0;
  NGPDE_REQUIRE(n_nodes >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n_nodes %lld)", fn, (long long)n_nodes);
  NGPDE_REQUIRE(n_nodes <= 0x7fffffffLL - 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld nodes, at most 2^31 - 2", fn, (long long)n_nodes);
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_graphs %d, at least 1", fn, n_graphs);
  NGPDE_REQUIRE(graph_of || n_graphs == 1 || n_nodes == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of is NULL with n_graphs %d", fn, n_graphs);
  NGPDE_REQUIRE(ptr_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: ptr_out is NULL", fn);
  NGPDE_REQUIRE(n_nodes == 0 || (labels && rank_out && sizes_out && order_out), NGPDE_ERR_INVALID_ARGUMENT,
                "%s: labels / rank_out / sizes_out / order_out is NULL", fn);
  if (per_graph_out) NGPDE_HIP_CHECK(hipMemsetAsync(per_graph_out, 0, (size_t)n_graphs * sizeof(int32_t), stream));
  if (n_nodes == 0) {
    NGPDE_HIP_CHECK(hipMemsetAsync(ptr_out, 0, sizeof(int32_t), stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    return NGPDE_OK;
  }
  const int64_t n = n_nodes;
  Scratch sc;
  int32_t *flags = nullptr, *isroot = nullptr, *below = nullptr, *iota = nullptr, *sorted = nullptr, *count = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream)) || (st = sc.get(&isroot, (size_t)n)) || (st = sc.get(&below, (size_t)n)) ||
      (st = sc.get(&iota, (size_t)n)) || (st = sc.get(&sorted, (size_t)n)) || (st = sc.get(&count, 1)))
    return st;
  hipLaunchKernelGGL(rank_roots_kernel, dim3(blocks_for(n)), dim3(kB), 0, stream, n, labels, n_graphs, graph_of, isroot, per_graph_out, flags);
  NGPDE_LAUNCH_CHECK("rank_roots_kernel");
  if ((st = scan_i32(false, isroot, below, (size_t)n, sc, stream))) return st;
  hipLaunchKernelGGL(rank_nodes_kernel, dim3(blocks_for(n)), dim3(kB), 0, stream, n, labels, isroot, below, rank_out, iota, count);
  NGPDE_LAUNCH_CHECK("rank_nodes_kernel");
  // the nodes grouped by rank, ascending inside a group: ONE stable radix sort of the ranks with the node ids as the payload
  const unsigned end_bit = bits_for((unsigned long long)std::max<int64_t>(n, 2));
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, reinterpret_cast<const uint32_t *>(rank_out), reinterpret_cast<uint32_t *>(sorted), iota, order_out,
                                     (size_t)n, 0u, end_bit, stream);
  };
  if ((st = with_temp(sc, sort))) return st;
  hipLaunchKernelGGL(rank_ptr_kernel, dim3(blocks_for(n + 1)), dim3(kB), 0, stream, n, sorted, count, ptr_out, sizes_out);
  NGPDE_LAUNCH_CHECK("rank_ptr_kernel");
  int32_t h_count = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_count, count, sizeof(h_count), hipMemcpyDeviceToHost, stream));
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  NGPDE_REQUIRE(!h[fLabel], NGPDE_ERR_INVALID_ARGUMENT, "%s: labels are not what ngpde_coo_components wrote (a label that is no root at or below its node)",
                fn);
  NGPDE_REQUIRE(!h[fGraph], NGPDE_ERR_INVALID_ARGUMENT, "%s: graph_of holds an id outside 0:%d", fn, n_graphs - 1);
  *count_out = h_count;
  return NGPDE_OK;
}

// ngpde_coo_rows and ngpde_coo_rows_eid: the rows of coo_rows.h with the other end of every entry; with_eid keeps the COO positions
static int32_t coo_rows_entry(const char *fn, bool with_eid, int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t,
                              int32_t index_base, int32_t dir, int32_t *row_ptr_out, int32_t *row_other_out, int32_t *row_eid_out,
                              hipStream_t stream) {
  if (int32_t st = check_coo(fn, n_nodes, n_edges, s, t)) return st;
  NGPDE_REQUIRE(dir == NGPDE_DIR_OUT || dir == NGPDE_DIR_IN, NGPDE_ERR_INVALID_ARGUMENT, "%s: dir %d is neither NGPDE_DIR_OUT nor NGPDE_DIR_IN", fn,
                dir);
  NGPDE_REQUIRE(row_ptr_out && (n_edges == 0 || (row_other_out && (row_eid_out || !with_eid))), NGPDE_ERR_INVALID_ARGUMENT, "%s: an output is NULL", fn);
  if (n_edges == 0) {
    NGPDE_HIP_CHECK(hipMemsetAsync(row_ptr_out, 0, ((size_t)n_nodes + 1) * sizeof(int32_t), stream));
    return NGPDE_OK;
  }
  Scratch sc;
  int32_t *flags = nullptr;
  int32_t st;
  if ((st = new_flags(sc, &flags, stream))) return st;
  Rows rows;
  rows.rowptr = row_ptr_out;
  rows.eid = row_eid_out;   // (NULL: a temporary)
  if ((st = build_rows(n_nodes, n_edges, s, t, index_base, dir, &rows, flags + fRowsBad, sc, stream))) return st;
  hipLaunchKernelGGL(rows_other_kernel, dim3(blocks_for(n_edges)), dim3(kB), 0, stream, n_edges, n_nodes, index_base, dir, s, t, rows.eid,
                     row_other_out, flags);
  NGPDE_LAUNCH_CHECK("rows_other_kernel");
  int32_t h[kFlagWords];
  if ((st = read_flags(flags, h, stream))) return st;
  if ((st = edge_error(fn, h, fOffender, n_nodes))) return st;
  NGPDE_REQUIRE(!h[fBad], NGPDE_ERR_HIP, "%s: the sort returned a position outside the list", fn);
  return NGPDE_OK;
}

int32_t ngpde_coo_rows(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                       int32_t *row_ptr_out, int32_t *row_other_out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  return coo_rows_entry("ngpde_coo_rows", false, n_nodes, n_edges, s, t, index_base, dir, row_ptr_out, row_other_out, nullptr, (hipStream_t)stream);
}

int32_t ngpde_coo_rows_eid(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                           int32_t *row_ptr_out, int32_t *row_other_out, int32_t *row_eid_out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  return coo_rows_entry("ngpde_coo_rows_eid", true, n_nodes, n_edges, s, t, index_base, dir, row_ptr_out, row_other_out, row_eid_out,
                        (hipStream_t)stream);
}

size_t ngpde_csr_hop_distance_workspace_bytes(int64_t n) {
  if (n < 0 || n > 0x7fffffffLL) return 0;
  HopWs p;
  return measure(hop_layout, n, p);
}

int32_t ngpde_csr_hop_distance(int64_t n, int64_t nnz_a, const int32_t *row_ptr_a, const int32_t *other_a, int64_t nnz_b,
                               const int32_t *row_ptr_b, const int32_t *other_b, int64_t n_sources, const int64_t *sources, int32_t index_base,
                               int32_t separate, int64_t max_hops, int32_t check_every, int32_t *dist_out, void *workspace,
                               size_t workspace_bytes, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_hop_distance";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(n >= 0 && n_sources >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n %lld, n_sources %lld)", fn, (long long)n,
                (long long)n_sources);
  NGPDE_REQUIRE(n <= 0x7fffffffLL && n_sources <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: a size above 2^31 - 1 (n %lld, n_sources %lld)", fn,
                (long long)n, (long long)n_sources);
  if (int32_t st = check_rows(fn, "nnz_a", nnz_a, row_ptr_a, other_a)) return st;
  if (row_ptr_b || other_b || nnz_b)
    if (int32_t st = check_rows(fn, "nnz_b", nnz_b, row_ptr_b, other_b)) return st;
  NGPDE_REQUIRE(sources || n_sources == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: sources is NULL with n_sources %lld", fn, (long long)n_sources);
  NGPDE_REQUIRE(check_every >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: check_every %d is negative (0: no read-back)", fn, check_every);
  NGPDE_REQUIRE(check_every > 0 || max_hops >= 0, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: check_every 0 enqueues exactly max_hops levels: max_hops must be given (not negative)", fn);
  int64_t total;
  if (int32_t st = check_result(fn, n, n_sources, separate, dist_out, &total)) return st;
  if (total == 0) return NGPDE_OK;
  if (int32_t st = check_workspace(fn, workspace, workspace_bytes, ngpde_csr_hop_distance_workspace_bytes(n), 8)) return st;
  const int64_t levels = std::min<int64_t>(max_hops < 0 ? n - 1 : max_hops, n - 1);   // (a shortest path has fewer than n edges)
  const int64_t per = pass_sources(n_sources, separate), passes = (n_sources + per - 1) / per;
  NGPDE_REQUIRE(check_every > 0 || levels * passes <= kMaxUncheckedLaunches, NGPDE_ERR_UNSUPPORTED,
                "%s: max_hops %lld with check_every 0 would enqueue %lld launches", fn, (long long)max_hops, (long long)(levels * passes));
  Workspace w(workspace);
  HopWs p;
  hop_layout(w, n, p);
  u64 *const seen = p.seen, *const *fr = p.fr;
  int32_t *const ctl = p.ctl;
  if (int32_t st = launch_zero(ctl, kCtlBytes, stream)) return st;
  NGPDE_REQUIRE(blocks_for(total) <= 0x7fffffffu && total / kB <= 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "%s: %lld cells in one launch", fn,
                (long long)total);
  hipLaunchKernelGGL(fill_sources_kernel<int32_t>, dim3(blocks_for(std::max(total, n_sources))), dim3(kB), 0, stream, total, -1, dist_out, nullptr,
                     nullptr, n_sources, sources, index_base, n, ctl);
  NGPDE_LAUNCH_CHECK("fill_sources_kernel");
  const HopRows ra = {row_ptr_a, other_a, nnz_a}, rb = {row_ptr_b, other_b, nnz_b};
  auto errors = [&](const int32_t *h) { return named_errors(fn, h, n, "a row pointer or a row entry"); };
  Rounds rounds = {check_every, ctl, stream};
  for (int64_t row0 = 0; row0 < n_sources; row0 += per) {
    const int64_t cnt = std::min(per, n_sources - row0);
    const u64 pass_mask = !separate ? 1ull : (cnt == 64 ? ~0ull : (1ull << cnt) - 1);
    hipLaunchKernelGGL(hop_init_kernel, dim3(blocks_for(n)), dim3(kB), 0, stream, n, seen, fr[0], ctl);
    NGPDE_LAUNCH_CHECK("hop_init_kernel");
    hipLaunchKernelGGL(hop_sources_kernel, dim3(blocks_for(cnt)), dim3(kB), 0, stream, cnt, n, index_base, separate ? 1 : 0, row0, sources + row0,
                       seen, fr[0], dist_out);
    NGPDE_LAUNCH_CHECK("hop_sources_kernel");
    auto level = [&](int64_t l) -> int32_t {
      hipLaunchKernelGGL(hop_level_kernel, dim3(blocks_for(n)), dim3(kB), 0, stream, n, (int)l, ra, rb, pass_mask, row0, fr[(l - 1) & 1], fr[l & 1],
                         seen, dist_out, ctl);
      NGPDE_LAUNCH_CHECK("hop_level_kernel");
      return NGPDE_OK;
    };
    if (int32_t st = rounds.run(levels, level, errors)) return st;
  }
  return rounds.answer(errors);   // (no level ran: the sources are still to be answered for)
}

int32_t ngpde_hop_reached_nodes(int64_t n, const int32_t *dist, int32_t index_base, int64_t *nodes_out, int64_t *n_out, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_hop_reached_nodes";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(n_out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_out is NULL", fn);
  *n_out = 0;
  NGPDE_REQUIRE(n >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n %lld)", fn, (long long)n);
  NGPDE_REQUIRE(n <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld nodes, at most 2^31 - 1", fn, (long long)n);
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(dist && nodes_out, NGPDE_ERR_INVALID_ARGUMENT, "%s: dist / nodes_out is NULL", fn);
  Scratch sc;
  int32_t *keep = nullptr, *pos = nullptr, *count = nullptr;
  int32_t st;
  if ((st = sc.get(&keep, (size_t)n)) || (st = sc.get(&pos, (size_t)n)) || (st = sc.get(&count, 1))) return st;
  hipLaunchKernelGGL(reached_flags_kernel, dim3(blocks_for(n)), dim3(kB), 0, stream, n, dist, keep);
  NGPDE_LAUNCH_CHECK("reached_flags_kernel");
  if ((st = scan_i32(false, keep, pos, (size_t)n, sc, stream))) return st;
  hipLaunchKernelGGL(reached_scatter_kernel, dim3(blocks_for(n)), dim3(kB), 0, stream, n, index_base, keep, pos, nodes_out, count);
  NGPDE_LAUNCH_CHECK("reached_scatter_kernel");
  int32_t h_count = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_count, count, sizeof(h_count), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  *n_out = h_count;
  return NGPDE_OK;
}

}  // extern "C"
