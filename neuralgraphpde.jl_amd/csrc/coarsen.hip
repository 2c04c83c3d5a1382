// coarsen.hip -- choosing the coarse cloud (include/ngpde_coarsen.h): farthest-point sampling on two paths, grid clusters, pooling of
// node features over clusters and its pullback.  [UPSTREAM torch_geometric's fps, voxel_grid, avg_pool / max_pool.]  Every decision
// (which candidate wins, the distance, which graph takes which path and where its slices lie, the cell and its key) is
// coarsen_rule.h's; the kernels here only carry it out.
//   fps, tile path   one workgroup of 1 024 threads per graph, the graph's keys and coordinates in registers (1, 4 or 16 points per thread),
//                    all k rounds in one launch; per round: update the own keys, keep the own best, reduce the wave by shuffles, hand the
//                    wave's best with its coordinates through a double-buffered LDS slot, ONE barrier, read the 16 slots.
//   fps, round path  one launch per round; a workgroup per slice of 2 048 points reduces the previous round's partials of its graph,
//                    updates its slice's keys in the workspace and leaves its partial in the other half of a double buffer.
//   grid_cluster     cells -> extents and refusals (one read-back) -> keys -> one stable radix sort -> head flags -> scan -> rows.
//   pool             one wave per cluster, lanes (slot, column) as in row_lanes.h, fixed xor butterfly; the pullback is a gather.
// The library is compiled with -ffp-contract=off: no product below is fused into its sum.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include <rocprim/rocprim.hpp>

#include "../../include/ngpde_coarsen.h"
#include "common.h"
#include "coarsen_rule.h"
#include "coo_compact.h"
#include "device_scratch.h"
#include "row_lanes.h"
#include "workspace.h"

static_assert(NGPDE_FPS_TILE_MAX_POINTS == ngpde::coarsen::kFpsTileMaxPoints, "the header's cap is the rule's");
static_assert(NGPDE_FPS_TILE_THREADS == ngpde::coarsen::kFpsTileThreads, "the header's workgroup is the rule's");

struct ngpde_fps_plan {
  ngpde::coarsen::FpsLayout lay;
  int32_t dim = 0;
  ngpde::coarsen::FpsGraph *graphs = nullptr;   // device: tile classes 0, 1, 2, then the round path's
  int32_t *wg_graph = nullptr;                  // device [lay.wg_graph.size()]
  size_t first[4] = {0, 0, 0, 0};               // where each list starts in `graphs`
};

namespace ngpde {
namespace {

using namespace coarsen;

__device__ __forceinline__ Cand wave_best(Cand c) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    Cand other;
    other.key = __shfl_xor(c.key, o);
    other.idx = __shfl_xor(c.idx, o);
    c = pick(c, other);
  }
  return c;
}

__device__ __forceinline__ int start_of(const FpsGraph &G, const int32_t *__restrict__ start, int index_base) {
  const int s = start ? start[G.g] - index_base - G.lo : 0;
  return min(max(s, 0), G.n - 1);   // (documented precondition: inside the graph; clamped, so never out of bounds)
}

// ---- the tile path ----------------------------------------------------------------------------------------------------------------
template <int DIM, int PPT>
__global__ __launch_bounds__(kFpsTileThreads) void fps_tile_kernel(const FpsGraph *__restrict__ graphs, const float *__restrict__ points,
                                                                   const int32_t *__restrict__ start, int index_base,
                                                                   int32_t *__restrict__ idx, float *__restrict__ d2out) {
  constexpr int W = kFpsTileThreads, NW = W / 64;
  __shared__ float4 slot[2][NW];   // a wave's best of a round: {key, index bits, x, y}
  __shared__ float slot_z[2][NW];
  const FpsGraph G = graphs[blockIdx.x];   // read once; n and k are workgroup-uniform, and so is every loop bound below
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = G.n, k = G.k;              // 1 <= k <= n <= PPT * W (the plan's layout)

  float key[PPT], px[PPT], py[PPT], pz[PPT];
#pragma unroll
  for (int j = 0; j < PPT; ++j) {
    const int i = tid + j * W;
    const bool real = i < n;
    const float *p = points + (size_t)(G.lo + (real ? i : 0)) * DIM;
    key[j] = real ? INFINITY : kKeyNone;
    px[j] = p[0];
    py[j] = DIM > 1 ? p[1] : 0.f;
    pz[j] = DIM > 2 ? p[2] : 0.f;
  }

  int s = start_of(G, start, index_base);
  float skey = INFINITY;
  float sp[3];
  {
    const float *p = points + (size_t)(G.lo + s) * DIM;
    sp[0] = p[0];
    sp[1] = DIM > 1 ? p[1] : 0.f;
    sp[2] = DIM > 2 ? p[2] : 0.f;
  }
  for (int r = 0;; ++r) {
    if (tid == 0) {
      idx[G.out + r] = G.lo + s + index_base;
      if (d2out) d2out[G.out + r] = skey;
    }
    if (r == k - 1) break;   // uniform: the last round has nothing to prepare
    Cand mine = {kKeyNone, kIdxNone};
    float bx = 0.f, by = 0.f, bz = 0.f;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
      const int i = tid + j * W;
      float kj = key[j];
      if (kj >= 0.f) {   // a real, unselected point
        const float q[3] = {px[j], py[j], pz[j]};
        kj = i == s ? kKeySelected : updated_key(kj, dist2<DIM>(q, sp));
        key[j] = kj;
      }
      if (kj >= 0.f && better(kj, i, mine.key, mine.idx)) {
        mine.key = kj;
        mine.idx = i;
        bx = px[j];
        by = py[j];
        bz = pz[j];
      }
    }
    const Cand wb = wave_best(mine);
    const int b = r & 1;
    if (mine.idx == wb.idx && (mine.idx != kIdxNone || lane == 0)) {   // the one lane that holds the wave's best
      slot[b][wave] = make_float4(wb.key, __int_as_float(wb.idx), bx, by);
      if (DIM > 2) slot_z[b][wave] = bz;
    }
    __syncthreads();   // the round's only barrier: round r + 1 writes the other buffer, round r + 2 lies behind the next barrier
    Cand best = {kKeyNone, kIdxNone};
    int bw = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const float4 v = slot[b][w];
      const int vi = __float_as_int(v.y);
      if (better(v.x, vi, best.key, best.idx)) {
        best.key = v.x;
        best.idx = vi;
        sp[0] = v.z;
        sp[1] = v.w;
        bw = w;
      }
    }
    if (DIM > 2) sp[2] = slot_z[b][bw];
    s = min(max(best.idx, 0), n - 1);
    skey = best.key;
  }
}

// ---- the round path ---------------------------------------------------------------------------------------------------------------
template <int DIM>
__global__ __launch_bounds__(kFpsRoundThreads) void fps_round_kernel(int r, const FpsGraph *__restrict__ graphs,
                                                                     const int32_t *__restrict__ wg_graph, const float *__restrict__ points,
                                                                     const int32_t *__restrict__ start, int index_base,
                                                                     int32_t *__restrict__ idx, float *__restrict__ d2out,
                                                                     float *__restrict__ keys, Cand *__restrict__ partials, int n_parts_all) {
  constexpr int T = kFpsRoundThreads, NW = T / 64;
  __shared__ Cand prev_best[NW], my_best[NW];
  const FpsGraph G = graphs[wg_graph[blockIdx.x]];
  if (r >= G.k) return;   // uniform over the workgroup
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slice = blockIdx.x - G.first_part, n = G.n;
  Cand sel;
  if (r == 0) {
    sel.key = INFINITY;
    sel.idx = start_of(G, start, index_base);
  } else {   // every workgroup of the graph reduces the same partials of round r - 1
    const Cand *prev = partials + (size_t)((r - 1) & 1) * n_parts_all + G.first_part;
    Cand c = {kKeyNone, kIdxNone};
    for (int p = tid; p < G.n_parts; p += T) c = pick(c, prev[p]);
    c = wave_best(c);
    if (lane == 0) prev_best[wave] = c;
    __syncthreads();
    sel = prev_best[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) sel = pick(sel, prev_best[w]);
  }
  const int s = min(max(sel.idx, 0), n - 1);
  if (slice == 0 && tid == 0) {
    idx[G.out + r] = G.lo + s + index_base;
    if (d2out) d2out[G.out + r] = sel.key;
  }
  if (r == G.k - 1) return;   // uniform
  float sp[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int c = 0; c < DIM; ++c) sp[c] = points[(size_t)(G.lo + s) * DIM + c];
  float *key = keys + G.key_off;
  Cand mine = {kKeyNone, kIdxNone};
#pragma unroll
  for (int j = 0; j < kFpsRoundPerThread; ++j) {
    const int i = slice * kFpsSlice + j * T + tid;
    if (i < n) {
      float kj = r == 0 ? INFINITY : key[i];
      if (kj >= 0.f) {
        float q[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DIM; ++c) q[c] = points[(size_t)(G.lo + i) * DIM + c];
        kj = i == s ? kKeySelected : updated_key(kj, dist2<DIM>(q, sp));
        key[i] = kj;
        if (kj >= 0.f && better(kj, i, mine.key, mine.idx)) {
          mine.key = kj;
          mine.idx = i;
        }
      }
    }
  }
  mine = wave_best(mine);
  if (lane == 0) my_best[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    Cand c = my_best[0];
#pragma unroll
    for (int w = 1; w < NW; ++w) c = pick(c, my_best[w]);
    partials[(size_t)(r & 1) * n_parts_all + blockIdx.x] = c;
  }
}

struct FpsWs {
  float *keys;
  Cand *partials;
};
void fps_ws_layout(Workspace &ws, int64_t round_points, int64_t n_parts, FpsWs *out) {
  out->keys = ws.take<float>((size_t)round_points);
  out->partials = ws.take<Cand>((size_t)(2 * n_parts));
}

template <int DIM>
int32_t launch_fps(const ngpde_fps_plan *pl, const float *points, const int32_t *start, int index_base, int32_t *idx, float *d2, const FpsWs &w,
                   hipStream_t hs) {
  const FpsLayout &L = pl->lay;
  if (!L.tile[0].empty())
    hipLaunchKernelGGL((fps_tile_kernel<DIM, 1>), dim3((unsigned)L.tile[0].size()), dim3(kFpsTileThreads), 0, hs, pl->graphs + pl->first[0], points,
                       start, index_base, idx, d2);
  if (!L.tile[1].empty())
    hipLaunchKernelGGL((fps_tile_kernel<DIM, 4>), dim3((unsigned)L.tile[1].size()), dim3(kFpsTileThreads), 0, hs, pl->graphs + pl->first[1], points,
                       start, index_base, idx, d2);
  if (!L.tile[2].empty())
    hipLaunchKernelGGL((fps_tile_kernel<DIM, kFpsTileMaxPerThread>), dim3((unsigned)L.tile[2].size()), dim3(kFpsTileThreads), 0, hs,
                       pl->graphs + pl->first[2], points, start, index_base, idx, d2);
  NGPDE_LAUNCH_CHECK("fps_tile_kernel");
  const int n_parts = (int)L.wg_graph.size();
  for (int r = 0; r < L.round_launches; ++r)
    hipLaunchKernelGGL((fps_round_kernel<DIM>), dim3((unsigned)n_parts), dim3(kFpsRoundThreads), 0, hs, r, pl->graphs + pl->first[3], pl->wg_graph,
                       points, start, index_base, idx, d2, w.keys, w.partials, n_parts);
  NGPDE_LAUNCH_CHECK("fps_round_kernel");
  return NGPDE_OK;
}

// ---- grid clusters ----------------------------------------------------------------------------------------------------------------
struct GridArgs {
  int dim, n_graphs, own_origin;
  float size[3], origin[3];
  unsigned bits[3];
};
enum { kMaxCell0 = 0, kBadNonFinite = 3, kBadBelow = 4, kBadCell = 5, kStatWords = 8 };

// the minimum of every graph's own points per coordinate: one workgroup per graph
__global__ __launch_bounds__(256) void grid_origin_kernel(int dim, const int32_t *__restrict__ gptr, const float *__restrict__ points,
                                                          float *__restrict__ origin) {
  __shared__ float part[4][3];
  const int g = blockIdx.x, lo = gptr[g], hi = gptr[g + 1];
  float m[3] = {INFINITY, INFINITY, INFINITY};
  for (int i = lo + threadIdx.x; i < hi; i += blockDim.x)
    for (int c = 0; c < dim; ++c) m[c] = fminf(m[c], points[(size_t)i * dim + c]);
  for (int c = 0; c < 3; ++c)
    for (int o = 1; o < 64; o <<= 1) m[c] = fminf(m[c], __shfl_xor(m[c], o));
  if ((threadIdx.x & 63) == 0)
    for (int c = 0; c < 3; ++c) part[threadIdx.x >> 6][c] = m[c];
  __syncthreads();
  if (threadIdx.x < 3) origin[g * 3 + threadIdx.x] = fminf(fminf(part[0][threadIdx.x], part[1][threadIdx.x]), fminf(part[2][threadIdx.x], part[3][threadIdx.x]));
}

// pass 0: the refusals and the largest cell of every coordinate; pass 1: the keys
__global__ void grid_cells_kernel(int pass, int64_t n, GridArgs a, const int32_t *__restrict__ gptr, const float *__restrict__ points,
                                  const float *__restrict__ origin, unsigned long long *__restrict__ stats, unsigned long long *__restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int lo = 0, hi = a.n_graphs;   // the graph of point i: the last g with gptr[g] <= i
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gptr[mid] <= i) lo = mid;
    else hi = mid;
  }
  const int g = lo;
  int32_t c[3] = {0, 0, 0};
  bool ok = true;
  for (int d = 0; d < a.dim; ++d) {
    const float p = points[(size_t)i * a.dim + d];
    const float o = a.own_origin ? origin[g * 3 + d] : a.origin[d];
    const float q = cell_quotient(p, o, a.size[d]);
    if (!isfinite(p)) {
      if (pass == 0) report_offender(stats + kBadNonFinite, i);
      ok = false;
    } else if (q < 0.f) {
      if (pass == 0) report_offender(stats + kBadBelow, i);
      ok = false;
    } else if (!cell_fits(q)) {
      if (pass == 0) report_offender(stats + kBadCell, i);
      ok = false;
    } else {
      c[d] = (int32_t)q;
    }
  }
  if (pass == 0) {
    if (ok)
      for (int d = 0; d < a.dim; ++d) atomicMax(stats + kMaxCell0 + d, (unsigned long long)c[d]);
  } else {
    keys[i] = cell_key(a.dim, c, g, a.bits[0], a.bits[1], a.bits[2]);
  }
}

__global__ void grid_heads_kernel(int64_t n, const unsigned long long *__restrict__ key_sorted, int32_t *__restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) head[i] = i == 0 || key_sorted[i] != key_sorted[i - 1];
}

// rank[i] = the inclusive scan of the head flags: sorted position i lies in cluster rank[i] - 1
__global__ void grid_rows_kernel(int64_t n, unsigned cell_bits, const unsigned long long *__restrict__ key_sorted, const int32_t *__restrict__ head,
                                 const int32_t *__restrict__ rank, const int32_t *__restrict__ order, int32_t *__restrict__ labels,
                                 int32_t *__restrict__ ptr, int32_t *__restrict__ cluster_graph, int32_t *__restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int32_t c = rank[i] - 1;
  labels[order[i]] = c;
  if (head[i]) {
    ptr[c] = (int32_t)i;
    cluster_graph[c] = (int32_t)(key_sorted[i] >> cell_bits) + 1;
  }
  if (i == n - 1) {
    ptr[c + 1] = (int32_t)n;
    *count = c + 1;
  }
}

// ---- pooling ----------------------------------------------------------------------------------------------------------------------
template <int AGGR>
__device__ __forceinline__ float pool_identity() {
  return AGGR == NGPDE_AGGR_MAX ? -INFINITY : AGGR == NGPDE_AGGR_MIN ? INFINITY : 0.f;
}
template <int AGGR>
__device__ __forceinline__ float pool_combine(float a, float b) {
  return AGGR == NGPDE_AGGR_MAX ? fmaxf(a, b) : AGGR == NGPDE_AGGR_MIN ? fminf(a, b) : a + b;
}

template <int AGGR>
__global__ __launch_bounds__(256) void pool_forward_kernel(int n, int nc, int d, const int32_t *__restrict__ ptr, const int32_t *__restrict__ order,
                                                           const float *__restrict__ x, float *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= nc) return;
  const int rs = min(max(ptr[row], 0), n), re = min(max(ptr[row + 1], rs), n);
  const int dpl = lanes_per_entry(d), slots = 64 / dpl, sl = lane / dpl, cl = lane % dpl;
  for (int c0 = 0; c0 < d; c0 += dpl) {
    const int c = min(c0 + cl, d - 1);
    float a = pool_identity<AGGR>();
    for (int p0 = rs + sl; p0 < re; p0 += 4 * slots) {   // four gathers in flight, combined in ascending order
      float v[4];
      bool use[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = p0 + u * slots;
        const int i = p < re ? order[p] : -1;
        use[u] = (unsigned)i < (unsigned)n;
        v[u] = use[u] ? x[(size_t)i * d + c] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (use[u]) a = pool_combine<AGGR>(a, v[u]);
    }
    for (int o = dpl; o < 64; o <<= 1) a = pool_combine<AGGR>(a, __shfl_xor(a, o));
    if (AGGR == NGPDE_AGGR_MEAN) a = re > rs ? a / (float)(re - rs) : 0.f;
    if (sl == 0 && c0 + cl < d) out[(size_t)row * d + c] = a;
  }
}

__global__ void pool_backward_kernel(int64_t total, int nc, int d, int aggr, const int32_t *__restrict__ labels, const int32_t *__restrict__ ptr,
                                     const float *__restrict__ x, const float *__restrict__ out, const float *__restrict__ dout,
                                     float *__restrict__ dx) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int64_t i = e / d;
  const int c = (int)(e - i * d);
  const int l = labels[i];
  float g = 0.f;
  if ((unsigned)l < (unsigned)nc) {
    g = dout[(size_t)l * d + c];
    if (aggr == NGPDE_AGGR_MEAN) g = g / (float)(ptr[l + 1] - ptr[l]);
    else if (aggr == NGPDE_AGGR_MAX || aggr == NGPDE_AGGR_MIN) g = x[e] == out[(size_t)l * d + c] ? g : 0.f;
  }
  dx[e] = g;
}

int32_t check_pool(const char *fn, int64_t n, int64_t c, int32_t d, int32_t aggr) {
  NGPDE_REQUIRE(d >= 1, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: the feature width must be >= 1 (got %d)", fn, d);
  NGPDE_REQUIRE(aggr == NGPDE_AGGR_SUM || aggr == NGPDE_AGGR_MEAN || aggr == NGPDE_AGGR_MAX || aggr == NGPDE_AGGR_MIN, NGPDE_ERR_INVALID_ARGUMENT,
                "%s: aggr must be NGPDE_AGGR_SUM, MEAN, MAX or MIN (got %d)", fn, aggr);
  NGPDE_REQUIRE(n >= 0 && n <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: number of points %lld outside 0:2^31-1", fn, (long long)n);
  NGPDE_REQUIRE(c >= 0 && c <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: number of clusters %lld outside 0:2^31-1", fn, (long long)c);
  return NGPDE_OK;
}

}  // namespace
}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_fps_plan_create(int32_t n_graphs, const int64_t *graph_ptr, const int64_t *sample_ptr, int32_t dim, int32_t path,
                              ngpde_stream_t stream, ngpde_fps_plan_t **plan) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(plan != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: plan is NULL");
  *plan = nullptr;
  NGPDE_REQUIRE(n_graphs >= 0, NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: n_graphs must be >= 0 (got %d)", n_graphs);
  NGPDE_REQUIRE(graph_ptr != nullptr && sample_ptr != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: graph_ptr or sample_ptr is NULL");
  NGPDE_REQUIRE(dim >= 1 && dim <= 3, NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: dim must be 1, 2 or 3 (got %d)", dim);
  NGPDE_REQUIRE(path >= 0 && path <= 2, NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: path must be 0 (auto), 1 (tile) or 2 (round), got %d", path);
  ngpde_fps_plan *pl = new (std::nothrow) ngpde_fps_plan;
  NGPDE_REQUIRE(pl != nullptr, NGPDE_ERR_HIP, "fps_plan_create: out of host memory");
  int32_t where = 0;
  const FpsRefusal why = fps_layout(n_graphs, graph_ptr, sample_ptr, path, &pl->lay, &where);
  if (why != kFpsOk) {
    const long long n = (long long)(graph_ptr[where + 1] - graph_ptr[where]), k = (long long)(sample_ptr[where + 1] - sample_ptr[where]);
    delete pl;
    switch (why) {
      case kFpsBadStart: return fail(NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: graph_ptr and sample_ptr must start at 0");
      case kFpsDecreasing: return fail(NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: graph_ptr decreases at graph %d", where);
      case kFpsSamplesDecreasing: return fail(NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: sample_ptr decreases at graph %d", where);
      case kFpsTooMany: return fail(NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: graph %d has %lld points, %lld samples asked for", where, n, k);
      case kFpsOverCap:
        return fail(NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: graph %d has %lld points, more than NGPDE_FPS_TILE_MAX_POINTS = %d of the tile path",
                    where, n, kFpsTileMaxPoints);
      default: return fail(NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_create: graph %d ends beyond 2^31 - 1 points", where);
    }
  }
  pl->dim = dim;
  const FpsLayout &L = pl->lay;
  std::vector<FpsGraph> all;
  for (int c = 0; c < 3; ++c) {
    pl->first[c] = all.size();
    all.insert(all.end(), L.tile[c].begin(), L.tile[c].end());
  }
  pl->first[3] = all.size();
  all.insert(all.end(), L.round.begin(), L.round.end());
  if (!all.empty()) {   // (a plan without work touches no device)
    hipStream_t hs = (hipStream_t)stream;
    int32_t st = dev_alloc(&pl->graphs, all.size());
    if (!st) st = dev_alloc(&pl->wg_graph, L.wg_graph.size());
    if (st) {
      ngpde_fps_plan_destroy(pl);
      return st;
    }
    hipError_t e = hipMemcpyAsync(pl->graphs, all.data(), all.size() * sizeof(FpsGraph), hipMemcpyHostToDevice, hs);
    if (e == hipSuccess && !L.wg_graph.empty())
      e = hipMemcpyAsync(pl->wg_graph, L.wg_graph.data(), L.wg_graph.size() * sizeof(int32_t), hipMemcpyHostToDevice, hs);
    if (e == hipSuccess) e = hipStreamSynchronize(hs);
    if (e != hipSuccess) {
      ngpde_fps_plan_destroy(pl);
      return fail(NGPDE_ERR_HIP, "fps_plan_create: copying the plan's tables failed: %s", hipGetErrorString(e));
    }
  }
  *plan = pl;
  return NGPDE_OK;
}

int32_t ngpde_fps_plan_destroy(ngpde_fps_plan_t *plan) {
  if (!plan) return NGPDE_OK;
  if (plan->graphs) (void)hipFree(plan->graphs);
  if (plan->wg_graph) (void)hipFree(plan->wg_graph);
  delete plan;
  return NGPDE_OK;
}

int32_t ngpde_fps_plan_info(const ngpde_fps_plan_t *plan, int64_t *info) {
  NGPDE_REQUIRE(plan != nullptr && info != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "fps_plan_info: plan or info is NULL");
  const FpsLayout &L = plan->lay;
  info[0] = L.n_points;
  info[1] = L.n_samples;
  info[2] = L.n_tile_graphs();
  info[3] = (int64_t)L.round.size();
  info[4] = L.round_launches;
  info[5] = (int64_t)!L.tile[0].empty() + (int64_t)!L.tile[1].empty() + (int64_t)!L.tile[2].empty();
  return NGPDE_OK;
}

size_t ngpde_fps_workspace_bytes(const ngpde_fps_plan_t *plan) {
  if (!plan || plan->lay.round.empty()) return 0;
  FpsWs w;
  return measure(fps_ws_layout, plan->lay.round_points, (int64_t)plan->lay.wg_graph.size(), &w);
}

int32_t ngpde_fps(const ngpde_fps_plan_t *plan, const float *points, const int32_t *start, int32_t index_base, int32_t *idx, float *d2,
                  void *workspace, size_t workspace_bytes, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(plan != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "fps: plan is NULL");
  const FpsLayout &L = plan->lay;
  if (L.n_samples == 0) return NGPDE_OK;
  NGPDE_REQUIRE(points != nullptr && idx != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "fps: points or idx is NULL");
  FpsWs w = {nullptr, nullptr};
  if (!L.round.empty()) {
    const size_t needed = ngpde_fps_workspace_bytes(plan);
    if (int32_t st = check_workspace("fps", workspace, workspace_bytes, needed, 8)) return st;
    Workspace ws(workspace);
    fps_ws_layout(ws, L.round_points, (int64_t)L.wg_graph.size(), &w);
  }
  hipStream_t hs = (hipStream_t)stream;
  switch (plan->dim) {
    case 1: return launch_fps<1>(plan, points, start, index_base, idx, d2, w, hs);
    case 2: return launch_fps<2>(plan, points, start, index_base, idx, d2, w, hs);
    default: return launch_fps<3>(plan, points, start, index_base, idx, d2, w, hs);
  }
}

int32_t ngpde_grid_cluster(int64_t n, int32_t dim, const float *points, int32_t n_graphs, const int64_t *graph_ptr, const float *size,
                           const float *origin, int32_t *labels, int32_t *ptr, int32_t *order, int32_t *cluster_graph,
                           int64_t *n_clusters, ngpde_stream_t stream) {
  NGPDE_RANGE();
  NGPDE_REQUIRE(n_clusters != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: the count pointer is NULL");
  NGPDE_REQUIRE(n >= 0 && n <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: number of points %lld outside 0:2^31-1", (long long)n);
  NGPDE_REQUIRE(dim >= 1 && dim <= 3, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: dim must be 1, 2 or 3 (got %d)", dim);
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: n_graphs must be >= 1 (got %d)", n_graphs);
  NGPDE_REQUIRE(graph_ptr != nullptr && size != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: graph_ptr or size is NULL");
  NGPDE_REQUIRE(graph_ptr[0] == 0 && graph_ptr[n_graphs] == n, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: graph_ptr must run from 0 to n = %lld",
                (long long)n);
  for (int32_t g = 0; g < n_graphs; ++g)
    NGPDE_REQUIRE(graph_ptr[g + 1] >= graph_ptr[g], NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: graph_ptr decreases at graph %d", g);
  GridArgs a;
  std::memset(&a, 0, sizeof(a));
  a.dim = dim;
  a.n_graphs = n_graphs;
  a.own_origin = origin == nullptr;
  for (int d = 0; d < dim; ++d) {
    NGPDE_REQUIRE(std::isfinite(size[d]) && size[d] > 0.f, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: size[%d] = %g must be finite and > 0", d,
                  (double)size[d]);
    a.size[d] = size[d];
    if (origin) {
      NGPDE_REQUIRE(std::isfinite(origin[d]), NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: origin[%d] = %g is not finite", d, (double)origin[d]);
      a.origin[d] = origin[d];
    }
  }
  if (n == 0) {
    *n_clusters = 0;
    if (ptr) {
      hipStream_t hs0 = (hipStream_t)stream;
      NGPDE_HIP_CHECK(hipMemsetAsync(ptr, 0, sizeof(int32_t), hs0));
      NGPDE_HIP_CHECK(hipStreamSynchronize(hs0));
    }
    return NGPDE_OK;
  }
  NGPDE_REQUIRE(points && labels && ptr && order && cluster_graph, NGPDE_ERR_INVALID_ARGUMENT,
                "grid_cluster: points, labels, ptr, order or cluster_graph is NULL");
  hipStream_t hs = (hipStream_t)stream;
  Scratch sc;
  int32_t st;
  int32_t *gptr = nullptr, *head = nullptr, *rank = nullptr, *count = nullptr;
  float *own = nullptr;
  unsigned long long *stats = nullptr, *keys = nullptr, *key_sorted = nullptr;
  if ((st = sc.get(&gptr, (size_t)n_graphs + 1)) || (st = sc.get(&own, (size_t)n_graphs * 3)) || (st = sc.get(&stats, kStatWords)) ||
      (st = sc.get(&keys, (size_t)n)) || (st = sc.get(&key_sorted, (size_t)n)) || (st = sc.get(&head, (size_t)n)) ||
      (st = sc.get(&rank, (size_t)n)) || (st = sc.get(&count, 1)))
    return st;
  std::vector<int32_t> h_gptr((size_t)n_graphs + 1);
  for (int32_t g = 0; g <= n_graphs; ++g) h_gptr[g] = (int32_t)graph_ptr[g];
  NGPDE_HIP_CHECK(hipMemcpyAsync(gptr, h_gptr.data(), h_gptr.size() * sizeof(int32_t), hipMemcpyHostToDevice, hs));
  NGPDE_HIP_CHECK(hipMemsetAsync(stats, 0, kStatWords * sizeof(unsigned long long), hs));
  if (a.own_origin) {
    hipLaunchKernelGGL(grid_origin_kernel, dim3((unsigned)n_graphs), dim3(256), 0, hs, dim, gptr, points, own);
    NGPDE_LAUNCH_CHECK("grid_origin_kernel");
  }
  hipLaunchKernelGGL(grid_cells_kernel, dim3(blocks_for(n)), dim3(kB), 0, hs, 0, n, a, gptr, points, own, stats, keys);
  NGPDE_LAUNCH_CHECK("grid_cells_kernel");
  unsigned long long h[kStatWords];
  NGPDE_HIP_CHECK(hipMemcpyAsync(h, stats, sizeof(h), hipMemcpyDeviceToHost, hs));
  NGPDE_HIP_CHECK(hipStreamSynchronize(hs));   // (the one read-back of the refusals and the extents)
  NGPDE_REQUIRE(h[kBadNonFinite] == 0, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: point %lld has a non-finite coordinate",
                (long long)decode_offender(h[kBadNonFinite]));
  NGPDE_REQUIRE(h[kBadBelow] == 0, NGPDE_ERR_INVALID_ARGUMENT, "grid_cluster: point %lld lies below the origin",
                (long long)decode_offender(h[kBadBelow]));
  NGPDE_REQUIRE(h[kBadCell] == 0, NGPDE_ERR_INVALID_ARGUMENT,
                "grid_cluster: cell size too small for the cloud's extent (point %lld lies in a cell beyond int32)",
                (long long)decode_offender(h[kBadCell]));
  int64_t max_cell[3] = {(int64_t)h[0], (int64_t)h[1], (int64_t)h[2]};
  const KeyBits kb = key_bits(dim, max_cell, n_graphs);
  NGPDE_REQUIRE(kb.total() <= 63, NGPDE_ERR_INVALID_ARGUMENT,
                "grid_cluster: cell size too small for the cloud's extent (the cluster key needs %u bits, at most 63)", kb.total());
  for (int d = 0; d < 3; ++d) a.bits[d] = kb.c[d];
  hipLaunchKernelGGL(grid_cells_kernel, dim3(blocks_for(n)), dim3(kB), 0, hs, 1, n, a, gptr, points, own, stats, keys);
  NGPDE_LAUNCH_CHECK("grid_cells_kernel");
  // one stable sort of the positions by key: equal keys keep their order, so a cluster's members ascend
  const unsigned end_bit = std::max(kb.total(), 1u);
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, keys, key_sorted, rocprim::counting_iterator<int32_t>(0), order, (size_t)n, 0u, end_bit, hs);
  };
  if ((st = with_temp(sc, sort))) return st;
  hipLaunchKernelGGL(grid_heads_kernel, dim3(blocks_for(n)), dim3(kB), 0, hs, n, key_sorted, head);
  NGPDE_LAUNCH_CHECK("grid_heads_kernel");
  if ((st = scan_i32(true, head, rank, (size_t)n, sc, hs))) return st;
  hipLaunchKernelGGL(grid_rows_kernel, dim3(blocks_for(n)), dim3(kB), 0, hs, n, kb.c[0] + kb.c[1] + kb.c[2], key_sorted, head, rank, order, labels, ptr,
                     cluster_graph, count);
  NGPDE_LAUNCH_CHECK("grid_rows_kernel");
  int32_t h_count = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_count, count, sizeof(int32_t), hipMemcpyDeviceToHost, hs));
  NGPDE_HIP_CHECK(hipStreamSynchronize(hs));
  *n_clusters = h_count;
  return NGPDE_OK;
}

int32_t ngpde_cluster_pool_forward(int64_t n, int64_t c, int32_t d, int32_t aggr, const int32_t *ptr, const int32_t *order, const float *x,
                                   float *out, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_pool("cluster_pool_forward", n, c, d, aggr)) return st;
  if (c == 0) return NGPDE_OK;
  NGPDE_REQUIRE(ptr != nullptr && out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "cluster_pool_forward: ptr or out is NULL");
  NGPDE_REQUIRE(n == 0 || (order != nullptr && x != nullptr), NGPDE_ERR_INVALID_ARGUMENT, "cluster_pool_forward: order or x is NULL");
  hipStream_t hs = (hipStream_t)stream;
  const dim3 grid((unsigned)((c + 3) / 4)), block(256);
  switch (aggr) {
    case NGPDE_AGGR_SUM: hipLaunchKernelGGL((pool_forward_kernel<NGPDE_AGGR_SUM>), grid, block, 0, hs, (int)n, (int)c, d, ptr, order, x, out); break;
    case NGPDE_AGGR_MEAN: hipLaunchKernelGGL((pool_forward_kernel<NGPDE_AGGR_MEAN>), grid, block, 0, hs, (int)n, (int)c, d, ptr, order, x, out); break;
    case NGPDE_AGGR_MAX: hipLaunchKernelGGL((pool_forward_kernel<NGPDE_AGGR_MAX>), grid, block, 0, hs, (int)n, (int)c, d, ptr, order, x, out); break;
    default: hipLaunchKernelGGL((pool_forward_kernel<NGPDE_AGGR_MIN>), grid, block, 0, hs, (int)n, (int)c, d, ptr, order, x, out); break;
  }
  NGPDE_LAUNCH_CHECK("pool_forward_kernel");
  return NGPDE_OK;
}

int32_t ngpde_cluster_pool_backward(int64_t n, int64_t c, int32_t d, int32_t aggr, const int32_t *labels, const int32_t *ptr,
                                    const float *x, const float *out, const float *dout, float *dx, ngpde_stream_t stream) {
  NGPDE_RANGE();
  if (int32_t st = check_pool("cluster_pool_backward", n, c, d, aggr)) return st;
  if (n == 0) return NGPDE_OK;
  NGPDE_REQUIRE(labels != nullptr && dx != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "cluster_pool_backward: labels or dx is NULL");
  NGPDE_REQUIRE(c == 0 || dout != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "cluster_pool_backward: dout is NULL");
  NGPDE_REQUIRE(c == 0 || aggr != NGPDE_AGGR_MEAN || ptr != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "cluster_pool_backward: ptr is NULL (MEAN)");
  NGPDE_REQUIRE(c == 0 || (aggr != NGPDE_AGGR_MAX && aggr != NGPDE_AGGR_MIN) || (x != nullptr && out != nullptr), NGPDE_ERR_INVALID_ARGUMENT,
                "cluster_pool_backward: x or out is NULL (MAX / MIN)");
  const int64_t total = n * (int64_t)d;
  NGPDE_REQUIRE(total / kB < 0x7fffffffLL, NGPDE_ERR_UNSUPPORTED, "cluster_pool_backward: n * d = %lld is more than one launch covers", (long long)total);
  hipLaunchKernelGGL(pool_backward_kernel, dim3(blocks_for(total)), dim3(kB), 0, (hipStream_t)stream, total, (int)c, d, aggr, labels, ptr, x, out, dout,
                     dx);
  NGPDE_LAUNCH_CHECK("pool_backward_kernel");
  return NGPDE_OK;
}

}  // extern "C"
