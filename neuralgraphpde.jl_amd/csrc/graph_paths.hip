// graph_paths.hip -- weighted shortest paths on the rows of a device COO list (include/ngpde.h, "graph traversal":
// ngpde_csr_shortest_paths): dijkstra_shortest_paths / bellman_ford_shortest_paths of the Graphs.jl interface a GNNGraph answers
// (src/NeuralGraphPDE.jl:4 re-exports GNNGraphs, :16 `using Graphs` of the reference), where graph_traverse.hip counts edges only.
//
// SYNCHRONOUS ROUNDS.  d_0 = 0 at the sources, +inf elsewhere; round r writes, for every node v and source i,
//     d_r[v] = min(d_{r-1}[v], min over the entries p of v's rows of fl32(d_{r-1}[other[p]] + w[p]))
// from the values of round r - 1 ONLY: two buffers of the workspace alternate, a lane writes the cells of its own (node, source
// group) and nothing else.  There is no atomic and no race, so d_r is defined for every r, whatever the launch geometry or the order
// in which lanes run.  The first round that lowers nothing ends the pass.  A lane that lowers a distance also stores it, and the
// tree edge, into the caller's arrays: they hold the last value of every cell, which is the result.
//   the value    w >= 0 and fl32(a + w) is monotone in a, so every d_r[v] is the fp32 length of a walk from a source (added up from
//                the source) and the limit is the greatest fixed point below d_0: what a float32 heap Dijkstra returns, bit for bit.
//   the parents  written when, and only when, the node's distance STRICTLY decreases; among the equal candidates of a round the
//                first in row order wins (set a before set b, COO order inside a row: the rows of coo_rows.h are a stable sort).
//                tight  d[u] never rises, so the candidate of the recorded edge never rises; at the fixed point it is not below
//                       d[v] either: fl32(d[parent] + w) == d[v], also when u was lowered later by an amount w absorbs.
//                tree   let t(v) be the round of v's last decrease and u its parent: d[v] >= d_{t(v)-1}[u] >= d[u].  On a parent
//                       cycle every one of these holds with equality, so u already had its final value in round t(v) - 1:
//                       t(u) < t(v) all the way round the cycle, which cannot be.  Zero and absorbed weights included.
//   the buffers  the caller's dist_out is [sources][nodes]: what a lane stores there for its node is contiguous across the wave.
//                What a round READS is the distance of the other end of every row entry, a gather; the two round buffers are
//                therefore one slab [nodes][kLane] per group of kLane sources (the last group padded): the kLane distances a lane
//                needs of a neighbour are ONE aligned 16-byte load, not kLane loads from kLane rows, a wave's own cells are one
//                contiguous KiB, and a group's lanes touch their slab only.  A padded column stays +inf and is never stored.
//   hub rows     a row of NGPDE_SSSP_WAVE_ROW entries or more is walked by the whole wave (traverse_rounds.h, the hub-row walk); the
//                wave reduces (distance, row position) lexicographically, so the first-in-row rule holds for them too.
//   max_dist     a candidate above it is dropped.  Distances do not decrease along a path, so every node within max_dist keeps
//                its exact distance and parent.
// Kernel boundaries are the only synchronisation: no spin-wait, no grid barrier (stop words and round loop: traverse_rounds.h).
#include <climits>
#include <cmath>

#include "traverse_rounds.h"

namespace ngpde {

namespace {

constexpr int kLane = NGPDE_SSSP_LANE_SOURCES;   // the sources a lane relaxes from one read of its row (1 when the call has one row)

static_assert(kLane == 4, "a lane's sources of one neighbour are one float4");
static_assert(NGPDE_SSSP_PASS == kPassSources && NGPDE_SSSP_PASS % NGPDE_SSSP_LANE_SOURCES == 0, "a pass is a whole number of lane groups");

struct PathRows : HopRows {   // HopRows with, per position, the COO position eid and the weight w
  const int32_t *eid;
  const float *w;   // in row order; NULL: 1 per entry
};

// w_rows[p] = weights[eid[p]] for the positions of set a, then of set b.  A negative or NaN weight is reported by its COO position
// and stored as +inf, so that nothing is relaxed through it; a COO position outside the list raises cCsr.
__global__ void sssp_weights_kernel(int64_t nnz_a, int64_t nnz_b, int64_t m, const int32_t *__restrict__ eid_a,
                                    const int32_t *__restrict__ eid_b, const float *__restrict__ weights, float *__restrict__ w_a,
                                    float *__restrict__ w_b, int32_t *__restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nnz_a + nnz_b) return;
  const bool second = i >= nnz_a;
  const int64_t p = second ? i - nnz_a : i;
  const int64_t e = second ? eid_b[p] : eid_a[p];
  float w = INFINITY;
  if (e < 0 || e >= m) {
    ctl[cCsr] = 1;
  } else {
    const float x = weights[e];
    if (x >= 0.f) w = x;   // (false for a NaN)
    else report_offender(reinterpret_cast<unsigned long long *>(ctl + cWeight), e);
  }
  (second ? w_b : w_a)[p] = w;
}

// a pass starts: its first round buffer is +inf; "round 0 changed something" (the sources), so that round 1 runs
__global__ void sssp_pass_kernel(int64_t cells, float *__restrict__ buf, int32_t *__restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < cells) buf[i] = INFINITY;
  rounds_arm(ctl, cTurn, i);
}

// source i of the pass gets distance 0 in its cell of the round buffer (the layout of sssp_round_kernel) and in its row of dist (all
// in column / row 0 when one distance to the NEAREST source is asked); two lanes that store the same 0 do not race for a value
__global__ void sssp_sources_kernel(int64_t cnt, int64_t n, int base, int separate, int64_t row0, int width, const int64_t *__restrict__ sources,
                                    float *__restrict__ buf, float *__restrict__ dist) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const int64_t v = sources[i] - base;
  if (v < 0 || v >= n) return;   // (reported by fill_sources_kernel)
  const int64_t col = separate ? i : 0, k = width > 1 ? kLane : 1;   // slab col / k, column col % k of the node's cells
  buf[((size_t)(col / k) * (size_t)n + (size_t)v) * (size_t)k + (size_t)(col % k)] = 0.f;
  dist[source_cell(separate, row0, i, n, v)] = 0.f;
}

template <int K>
struct Cells {   // the K distances of one node that a lane works on: one aligned load / store
  float d[K];
};

template <int K>
__device__ __forceinline__ Cells<K> load_cells(const float *__restrict__ at) {
  Cells<K> c;
  if constexpr (K == 4) {
    const float4 x = *reinterpret_cast<const float4 *>(at);
    c.d[0] = x.x, c.d[1] = x.y, c.d[2] = x.z, c.d[3] = x.w;
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) c.d[k] = at[k];
  }
  return c;
}

template <int K>
__device__ __forceinline__ void store_cells(float *__restrict__ at, const Cells<K> &c) {
  if constexpr (K == 4) {
    *reinterpret_cast<float4 *>(at) = make_float4(c.d[0], c.d[1], c.d[2], c.d[3]);
  } else {
#pragma unroll
    for (int k = 0; k < K; ++k) at[k] = c.d[k];
  }
}

template <int K>
struct Best {   // per source of the lane's group: the smallest candidate so far and the position (in its set) that gave it, -1: none
  float d[K];
  int32_t p[K];
};

// positions first, first + step, .. below e of one set: candidate k = fl32(prev[other][k] + w), kept when it is within max_dist and
// STRICTLY below the best so far -- the first position wins a tie
template <int K>
__device__ __forceinline__ void relax_entries(const PathRows &r, int64_t first, int64_t e, int step, int64_t n, float max_dist,
                                              const float *__restrict__ prev, Best<K> &best, int32_t *ctl) {
  for (int64_t p = first; p < e; p += step) {
    const int64_t u = r.other[p];
    if (u < 0 || u >= n) {
      ctl[cCsr] = 1;
      continue;
    }
    const float w = r.w ? r.w[p] : 1.f;
    const Cells<K> du = load_cells<K>(prev + (size_t)u * K);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float c = du.d[k] + w;
      if (c <= max_dist && c < best.d[k]) best.d[k] = c, best.p[k] = (int32_t)p;
    }
  }
}

// the lexicographic minimum of (d, p) over the wave, in every lane
__device__ __forceinline__ void wave_first_min(float &d, int32_t &p) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float od = __shfl_xor(d, off, kWave);
    const int32_t op = __shfl_xor(p, off, kWave);
    if (od < d || (od == d && op < p)) d = od, p = op;
  }
}

// Round `round` >= 1 of a pass.  prev / next: [gridDim.y][n][K] -- a slab per group of K sources --, blockIdx.y the lane's group, v
// its node; dist / parent_eid / parent: the pass's `cnt` rows of the caller's arrays, row stride n.  prev is not written by this launch and
// every cell a lane writes is its own, so the launch has no race.  Its cTurn word says "this round lowered a distance".
template <int K>
__global__ __launch_bounds__(256) void sssp_round_kernel(int64_t n, int round, PathRows ra, PathRows rb, int cnt, float max_dist,
                                                         const float *__restrict__ prev, float *__restrict__ next, float *__restrict__ dist,
                                                         int32_t *__restrict__ parent_eid, int32_t *__restrict__ parent, int32_t *ctl) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & (kWave - 1);
  const int go = round_go(ctl, cTurn, round, v == 0 && blockIdx.y == 0);
  if (v == 0 && blockIdx.y == 0 && go && round > ctl[cRounds]) ctl[cRounds] = round;
  if (!go) return;   // (the whole grid: the round before lowered nothing)
  const int k0 = (int)blockIdx.y * K;
  const size_t slab = (size_t)blockIdx.y * (size_t)n * K;
  prev += slab, next += slab;
  const bool mine = v < n;
  Cells<K> old;
#pragma unroll
  for (int k = 0; k < K; ++k) old.d[k] = INFINITY;
  if (mine) old = load_cells<K>(prev + (size_t)v * K);
  Best<K> best;   // starts at the node's own distance: only a candidate STRICTLY below it is ever kept
  int set[K];
#pragma unroll
  for (int k = 0; k < K; ++k) best.d[k] = old.d[k], best.p[k] = -1, set[k] = 0;
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const PathRows &r = s == 0 ? ra : rb;
    if (!r.ptr) continue;   // (uniform)
    int64_t b, e;
    row_span(r, v, mine, b, e, ctl);
    Best<K> here;   // this set's own first minimum below what the earlier set left
#pragma unroll
    for (int k = 0; k < K; ++k) here.d[k] = best.d[k], here.p[k] = -1;
    const bool wide = e - b >= NGPDE_SSSP_WAVE_ROW;
    if (!wide) relax_entries<K>(r, b, e, 1, n, max_dist, prev, here, ctl);
    for_wide_rows(wide, b, e, [&](int owner, int64_t wb, int64_t we) {
      Best<K> part;   // (every lane starts from the owner's bound)
#pragma unroll
      for (int k = 0; k < K; ++k) part.d[k] = __shfl(best.d[k], owner, kWave), part.p[k] = -1;
      relax_entries<K>(r, wb + lane, we, kWave, n, max_dist, prev, part, ctl);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (part.p[k] < 0) part.p[k] = INT_MAX;   // (no candidate of its own below the bound: loses every comparison)
        wave_first_min(part.d[k], part.p[k]);
        if (lane == owner && part.p[k] != INT_MAX) here.d[k] = part.d[k], here.p[k] = part.p[k];
      }
    });
#pragma unroll
    for (int k = 0; k < K; ++k)
      if (here.p[k] >= 0) best.d[k] = here.d[k], best.p[k] = here.p[k], set[k] = s;
  }
  if (!mine) return;
  Cells<K> now;
  bool lowered = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    now.d[k] = best.d[k];   // (= old.d[k] where nothing was kept)
    if (best.p[k] >= 0 && k0 + k < cnt) {
      const PathRows &r = set[k] == 0 ? ra : rb;
      const size_t at = (size_t)(k0 + k) * (size_t)n + (size_t)v;
      dist[at] = best.d[k];
      if (parent_eid) parent_eid[at] = r.eid[best.p[k]];
      if (parent) parent[at] = r.other[best.p[k]];
      lowered = true;
    }
  }
  store_cells<K>(next + (size_t)v * K, now);
  if (lowered) round_mark(ctl, cTurn, round);
}

// a pass ends: did its last enqueued round still lower a distance?  rounds_out[0] = the rounds run so far (the largest over the passes)
__global__ void sssp_pass_end_kernel(int last_round, int32_t *__restrict__ ctl, int32_t *__restrict__ rounds_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (last_round > 0 && ctl[round_word(cTurn, last_round)]) ctl[cState] = 1;
    if (rounds_out) rounds_out[0] = ctl[cRounds], rounds_out[1] = ctl[cState];
  }
}

// the columns of a round buffer for `rows` sources: 1, or the next multiple of kLane
inline int64_t width_for(int64_t rows) { return rows <= 1 ? 1 : (rows + kLane - 1) / kLane * kLane; }

struct PathWs {
  float *buf[2];   // round r reads buf[(r - 1) & 1] and writes buf[r & 1]
  float *w_a, *w_b;
  int32_t *ctl;
};
void path_layout(Workspace &w, int64_t n, int64_t nnz_a, int64_t nnz_b, int64_t n_sources, int separate, PathWs &p) {
  const size_t cells = (size_t)n * (size_t)width_for(separate ? std::min<int64_t>(n_sources, NGPDE_SSSP_PASS) : 1);
  p.buf[0] = w.take<float>(cells);
  p.buf[1] = w.take<float>(cells);
  p.w_a = w.take<float>((size_t)nnz_a);
  p.w_b = w.take<float>((size_t)nnz_b);
  p.ctl = take_ctl(w);
}

bool sizes_ok(int64_t n, int64_t nnz_a, int64_t nnz_b, int64_t n_sources) {
  const int64_t top = 0x7fffffffLL;
  return n >= 0 && n <= top && nnz_a >= 0 && nnz_a <= top && nnz_b >= 0 && nnz_b <= top && n_sources >= 0 && n_sources <= top;
}

int32_t check_rows(const char *fn, const char *what, const int32_t *ptr, const int32_t *other, const int32_t *eid, int64_t nnz) {
  NGPDE_REQUIRE(ptr && (nnz == 0 || (other && eid)), NGPDE_ERR_INVALID_ARGUMENT, "%s: a row list of set %s is NULL", fn, what);
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde

using namespace ngpde;

extern "C" {

size_t ngpde_csr_shortest_paths_workspace_bytes(int64_t n, int64_t nnz_a, int64_t nnz_b, int64_t n_sources, int32_t separate) {
  if (!sizes_ok(n, nnz_a, nnz_b, n_sources)) return 0;
  PathWs p;
  return measure(path_layout, n, nnz_a, nnz_b, n_sources, separate, p);
}

int32_t ngpde_csr_shortest_paths(int64_t n, int64_t nnz_a, const int32_t *row_ptr_a, const int32_t *other_a, const int32_t *eid_a,
                                 int64_t nnz_b, const int32_t *row_ptr_b, const int32_t *other_b, const int32_t *eid_b, int64_t n_sources,
                                 const int64_t *sources, int32_t index_base, int32_t separate, const float *weights, float max_dist,
                                 int32_t max_rounds, int32_t check_every, float *dist_out, int32_t *parent_eid_out, int32_t *parent_out,
                                 int32_t *rounds_out, void *workspace, size_t workspace_bytes, ngpde_stream_t stream_) {
  NGPDE_RANGE();
  const char *fn = "ngpde_csr_shortest_paths";
  hipStream_t stream = (hipStream_t)stream_;
  NGPDE_REQUIRE(n >= 0 && n_sources >= 0 && nnz_a >= 0 && nnz_b >= 0, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: negative size (n %lld, n_sources %lld, nnz_a %lld, nnz_b %lld)", fn, (long long)n, (long long)n_sources, (long long)nnz_a,
                (long long)nnz_b);
  NGPDE_REQUIRE(sizes_ok(n, nnz_a, nnz_b, n_sources), NGPDE_ERR_INVALID_ARGUMENT,
                "%s: a size above 2^31 - 1 (n %lld, n_sources %lld, nnz_a %lld, nnz_b %lld)", fn, (long long)n, (long long)n_sources,
                (long long)nnz_a, (long long)nnz_b);
  if (int32_t st = check_rows(fn, "a", row_ptr_a, other_a, eid_a, nnz_a)) return st;
  const bool two = row_ptr_b || other_b || eid_b || nnz_b;
  if (two) {
    if (int32_t st = check_rows(fn, "b", row_ptr_b, other_b, eid_b, nnz_b)) return st;
    NGPDE_REQUIRE(nnz_b == nnz_a, NGPDE_ERR_INVALID_ARGUMENT, "%s: nnz_b %lld is not nnz_a %lld: the two sets are the rows of ONE list", fn,
                  (long long)nnz_b, (long long)nnz_a);
  }
  NGPDE_REQUIRE(sources || n_sources == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: sources is NULL with n_sources %lld", fn, (long long)n_sources);
  NGPDE_REQUIRE(max_dist >= 0.f, NGPDE_ERR_INVALID_ARGUMENT, "%s: max_dist %g is negative or NaN (+inf: no bound)", fn, (double)max_dist);
  NGPDE_REQUIRE(max_rounds >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: max_rounds %d is negative (0: the library's choice)", fn, max_rounds);
  NGPDE_REQUIRE(check_every >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: check_every %d is negative (0: no read-back)", fn, check_every);
  NGPDE_REQUIRE(check_every > 0 || max_rounds > 0, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: check_every 0 enqueues exactly max_rounds rounds: max_rounds must be given (positive)", fn);
  int64_t total;
  if (int32_t st = check_result(fn, n, n_sources, separate, dist_out, &total)) return st;
  if (int32_t st = check_workspace(fn, workspace, workspace_bytes, ngpde_csr_shortest_paths_workspace_bytes(n, nnz_a, nnz_b, n_sources, separate), 16))
    return st;
  const int64_t max_r = max_rounds > 0 ? max_rounds : std::max<int64_t>(n, 1);
  const int64_t per = pass_sources(n_sources, separate), passes = total == 0 ? 0 : (n_sources + per - 1) / per;
  NGPDE_REQUIRE(check_every > 0 || max_r * passes <= kMaxUncheckedLaunches, NGPDE_ERR_UNSUPPORTED,
                "%s: max_rounds %d with check_every 0 would enqueue %lld launches", fn, max_rounds, (long long)(max_r * passes));
  const int64_t most = std::max({total, nnz_a + nnz_b, n * width_for(std::min<int64_t>(separate ? n_sources : 1, NGPDE_SSSP_PASS))});
  NGPDE_REQUIRE(most / kB < 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "%s: %lld cells in one launch", fn, (long long)most);

  Workspace w(workspace);
  PathWs p;
  path_layout(w, n, nnz_a, nnz_b, n_sources, separate, p);
  float *const *buf = p.buf, *const w_a = p.w_a, *const w_b = p.w_b;
  int32_t *const ctl = p.ctl;
  int32_t st;
  if ((st = launch_zero(ctl, kCtlBytes, stream))) return st;
  if (weights && nnz_a > 0) {
    const int64_t cells = nnz_a + (two ? nnz_b : 0);
    hipLaunchKernelGGL(sssp_weights_kernel, dim3(blocks_for(cells)), dim3(kB), 0, stream, nnz_a, two ? nnz_b : 0, nnz_a, eid_a, eid_b, weights, w_a,
                       w_b, ctl);
    NGPDE_LAUNCH_CHECK("sssp_weights_kernel");
  }
  if (std::max(total, n_sources) > 0) {
    hipLaunchKernelGGL(fill_sources_kernel<float>, dim3(blocks_for(std::max(total, n_sources))), dim3(kB), 0, stream, total, INFINITY, dist_out,
                       parent_eid_out, parent_out, n_sources, sources, index_base, n, ctl);
    NGPDE_LAUNCH_CHECK("fill_sources_kernel");
  }
  const PathRows ra = {{row_ptr_a, other_a, nnz_a}, eid_a, weights ? w_a : nullptr};
  const PathRows rb = {{two ? row_ptr_b : nullptr, other_b, nnz_b}, eid_b, weights ? w_b : nullptr};
  auto errors = [&](const int32_t *h) { return named_errors(fn, h, n, "a row pointer, a row entry or a COO position"); };
  Rounds rounds = {check_every, ctl, stream};
  bool unfinished = false;
  for (int64_t row0 = 0; row0 < passes * per && !unfinished; row0 += per) {
    const int64_t cnt = std::min(per, n_sources - row0);
    const int rows_here = separate ? (int)cnt : 1;
    const int width = (int)width_for(rows_here);
    const size_t at = (size_t)row0 * (size_t)n;
    float *dist = dist_out + at;
    int32_t *pe = parent_eid_out ? parent_eid_out + at : nullptr, *pa = parent_out ? parent_out + at : nullptr;
    hipLaunchKernelGGL(sssp_pass_kernel, dim3(blocks_for(n * width)), dim3(kB), 0, stream, n * width, buf[0], ctl);
    NGPDE_LAUNCH_CHECK("sssp_pass_kernel");
    hipLaunchKernelGGL(sssp_sources_kernel, dim3(blocks_for(cnt)), dim3(kB), 0, stream, cnt, n, index_base, separate ? 1 : 0, row0, width,
                       sources + row0, buf[0], dist_out);
    NGPDE_LAUNCH_CHECK("sssp_sources_kernel");
    auto round = [&](int64_t r) -> int32_t {
      if (width == 1)
        hipLaunchKernelGGL(sssp_round_kernel<1>, dim3(blocks_for(n), 1), dim3(kB), 0, stream, n, (int)r, ra, rb, rows_here, max_dist,
                           buf[(r - 1) & 1], buf[r & 1], dist, pe, pa, ctl);
      else
        hipLaunchKernelGGL(sssp_round_kernel<kLane>, dim3(blocks_for(n), (unsigned)(width / kLane)), dim3(kB), 0, stream, n, (int)r, ra, rb,
                           rows_here, max_dist, buf[(r - 1) & 1], buf[r & 1], dist, pe, pa, ctl);
      NGPDE_LAUNCH_CHECK("sssp_round_kernel");
      return NGPDE_OK;
    };
    if ((st = rounds.run(max_r, round, errors))) return st;
    unfinished = check_every > 0 && !rounds.done;
    hipLaunchKernelGGL(sssp_pass_end_kernel, dim3(1), dim3(kWave), 0, stream, (int)rounds.last, ctl, rounds_out);
    NGPDE_LAUNCH_CHECK("sssp_pass_end_kernel");
  }
  if (passes == 0 && rounds_out) {   // (no pass ran: no rounds)
    hipLaunchKernelGGL(sssp_pass_end_kernel, dim3(1), dim3(kWave), 0, stream, 0, ctl, rounds_out);
    NGPDE_LAUNCH_CHECK("sssp_pass_end_kernel");
  }
  // (no round ran: the sources and the weights are still to be answered for)
  if ((st = rounds.answer(errors))) return st;
  NGPDE_REQUIRE(!unfinished, NGPDE_ERR_STATE,
                "%s: still changing after max_rounds = %lld rounds: the distances are not final (raise max_rounds)", fn, (long long)max_r);
  return NGPDE_OK;
}

}  // extern "C"
