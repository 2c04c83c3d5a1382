// delaunay.hip -- Delaunay neighbour graphs and triangles of 2-D point clouds on the device (include/ngpde_mesh.h): the graphs of
// the reference's VMH tutorial ("Neighbors for each node were selected by applying Delaunay triangulation to the measurement
// positions", /root/reference/docs/src/tutorials/VMH.md:53-55), which the tutorial reads from a file.
//
// Each point computes its own star as its Voronoi cell: the geometry, its error bound and the stop are csrc/delaunay_star.h (host
// code, checked by tests/host/delaunay_star_check.cpp); the candidates come ring by ring from the neighbour search's sorted cell
// grid (neighbor_cells.h).  star_lane_kernel: one lane per point, kLaneCap vertices in LDS columns, at most kLaneRings rings.
// star_wave_kernel: one wave per point that overflowed either, up to NGPDE_DELAUNAY_MAX_DEGREE vertices in LDS, 64 candidates
// classified at once and the ones that cut applied in candidate order (by ring, by span of cells, by sorted position); a point not
// certified within kWaveRings rings sweeps the sorted positions of its whole graph once.  Both run twice, to count and to fill (the protocol of radius_kernel).  The stars are symmetrised
// by one radix sort of 64-bit (point, neighbour) keys and rocprim::unique; triangle_kernel reads the triangles off the rows.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "../../include/ngpde_mesh.h"
#include "common.h"
#include "delaunay_star.h"
#include "device_scratch.h"
#include "neighbor_cells.h"
#include "neighbor_grid.h"

namespace ngpde {
namespace {

using namespace star;

constexpr int kLaneCap = 24;      // vertices of a first-pass cell (the largest degree on the bench clouds is 16)
constexpr int kLaneRings = 6;     // rings a first-pass point may walk
constexpr int kLaneThreads = 64;
constexpr int kWaveRings = 8;     // rings a second-pass point walks before it sweeps its whole graph
constexpr int kWaveCap = NGPDE_DELAUNAY_MAX_DEGREE;
constexpr int kGridK = 4;         // grid of about 2 points per cell
constexpr unsigned long long kNoPair = ~0ull;
constexpr int kNoPoint = INT_MAX;

struct Words {                    // the words a call reads back
  unsigned long long pair;        // smallest coincident pair (lo << 32 | hi), kNoPair
  int over;                       // smallest point whose star overflows, kNoPoint
  int wave_points;                // points that took the second pass
};

struct Cloud {
  Grid g;
  const float *spts;
  const int32_t *sidx;
  const unsigned *key;
  const int32_t *start;
  float r2;                       // max_edge_length^2 in float (inf: no limit)
};

// the cells at Chebyshev distance exactly `ring` from c, as ranges [q0, q1) of sorted positions: the two end columns in full, then
// the two end cells of every column between them (knn_kernel's walk)
template <class F>
__device__ __forceinline__ void ring_spans(const Grid &g, int base, const int *c, int ring, const int32_t *__restrict__ start, F &&f) {
  auto span = [&](int x, int ya, int yb) {
    ya = max(ya, 0);
    yb = min(yb, g.nc[1] - 1);
    if (x < 0 || x >= g.nc[0] || ya > yb) return;
    const int row = base + x * g.nc[1];
    f(start[row + ya], start[row + yb + 1]);
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
}

struct Me {   // the point whose star is built
  float a[2];
  int c[2];
  int base;       // first cell of its graph
  int max_ring;   // the ring that exhausts the grid
  int32_t i;      // original index
  __device__ __forceinline__ Me(int64_t p, const Cloud &cl) {
    a[0] = cl.spts[p * 2];
    a[1] = cl.spts[p * 2 + 1];
    cell_of<2>(cl.g, a, c);
    base = (int)(cl.key[p] / (unsigned)cl.g.cells) * cl.g.cells;
    max_ring = max(max(c[0], cl.g.nc[0] - 1 - c[0]), max(c[1], cl.g.nc[1] - 1 - c[1]));
    i = cl.sidx[p];
  }
  __device__ __forceinline__ Line line(const Cloud &cl, int q) const {
    return line_to(a[0], a[1], cl.spts[(int64_t)q * 2], cl.spts[(int64_t)q * 2 + 1], q);
  }
  // the neighbour search's float rule, unchanged (neighbors.hip: dist2)
  __device__ __forceinline__ bool within(const Cloud &cl, int q) const {
    const float dx = a[0] - cl.spts[(int64_t)q * 2], dy = a[1] - cl.spts[(int64_t)q * 2 + 1];
    float d2 = 0.f;
    d2 = d2 + dx * dx;
    d2 = d2 + dy * dy;
    return d2 <= cl.r2;
  }
};

__device__ __forceinline__ void report_pair(Words *words, int32_t i, int32_t j) {
  const unsigned long long lo = (unsigned)min(i, j), hi = (unsigned)max(i, j);
  atomicMin(&words->pair, (lo << 32) | hi);
}
__device__ __forceinline__ void write_edge(unsigned long long *__restrict__ keys, int64_t w, int32_t i, int32_t j) {
  keys[2 * w] = ((unsigned long long)(unsigned)i << 32) | (unsigned)j;
  keys[2 * w + 1] = ((unsigned long long)(unsigned)j << 32) | (unsigned)i;
}

// a first-pass cell: vertex k of thread l at [k * kLaneThreads + l] of every column
struct LaneCell {
  double *x, *y, *w;
  float *ab, *abs;
  int32_t *tag;
  __device__ __forceinline__ Vertex get(int k) const {
    const int o = k * kLaneThreads;
    Vertex v;
    v.x = x[o];
    v.y = y[o];
    v.w = w[o];
    v.ab = ab[o];
    v.abs = abs[o];
    v.tag = tag[o];
    return v;
  }
  __device__ __forceinline__ void set(int k, const Vertex &v) {
    const int o = k * kLaneThreads;
    x[o] = v.x;
    y[o] = v.y;
    w[o] = v.w;
    ab[o] = v.ab;
    abs[o] = v.abs;
    tag[o] = v.tag;
  }
};

// FILL = false: deg[i] = size of the star, second[p] = 1 where the point needs the second pass (deg 0).
// FILL = true: writes the star's two keys per entry from rowptr[i] on.
template <bool FILL>
__global__ __launch_bounds__(kLaneThreads) void star_lane_kernel(int64_t n, Cloud cl, int32_t *__restrict__ deg, int32_t *__restrict__ second,
                                                                 const int32_t *__restrict__ rowptr, unsigned long long *__restrict__ keys,
                                                                 Words *__restrict__ words) {
  __shared__ double lx[kLaneCap * kLaneThreads], ly[kLaneCap * kLaneThreads], lw[kLaneCap * kLaneThreads];
  __shared__ float lab[kLaneCap * kLaneThreads], labs[kLaneCap * kLaneThreads];
  __shared__ int32_t ltag[kLaneCap * kLaneThreads];
  const int64_t p = (int64_t)blockIdx.x * kLaneThreads + threadIdx.x;
  if (p >= n) return;
  if (FILL && second[p]) return;
  const int t = threadIdx.x;
  LaneCell P{lx + t, ly + t, lw + t, lab + t, labs + t, ltag + t};
  const Me me(p, cl);
  int m = 4;
  for (int k = 0; k < 4; ++k) P.set(k, plane_corner(k));
  auto line_of = [&](int32_t tag) { return me.line(cl, tag); };
  bool overflow = false;
  int stop_ring = -1;
  const int last = min(me.max_ring, kLaneRings);
  for (int ring = 0; ring <= last && !overflow; ++ring) {
    ring_spans(cl.g, me.base, me.c, ring, cl.start, [&](int q0, int q1) {
      for (int q = q0; q < q1 && !overflow; ++q) {
        if (q == (int)p) continue;
        const Line l = me.line(cl, q);
        if (coincident(l)) {
          if (!FILL) report_pair(words, me.i, cl.sidx[q]);
          continue;
        }
        overflow = clip(P, &m, kLaneCap, l, line_of) == kOverflow;
      }
    });
    if (overflow) break;
    if (ring == me.max_ring) {
      stop_ring = ring;
      break;
    }
    if (ring > 0) {
      double r2max = 0.0;
      for (int k = 0; k < m; ++k) r2max = fmax(r2max, rho2(P.get(k)));
      if (certified(r2max, ring_reach2(cl.g, ring))) {
        stop_ring = ring;
        break;
      }
    }
  }
  if (stop_ring < 0) {
    if (!FILL) {
      second[p] = 1;
      deg[me.i] = 0;
    }
    return;
  }
  int cnt = 0;
  int64_t w = FILL ? rowptr[me.i] : 0;
  for (int ring = 0; ring <= stop_ring; ++ring)
    ring_spans(cl.g, me.base, me.c, ring, cl.start, [&](int q0, int q1) {
      for (int q = q0; q < q1; ++q) {
        if (q == (int)p) continue;
        const Line l = me.line(cl, q);
        if (coincident(l)) continue;
        bool hit = false;
        for (int k = 0; k < m && !hit; ++k) hit = touches(P.get(k), P.get(k + 1 == m ? 0 : k + 1), l);
        if (hit && me.within(cl, q)) {
          if (FILL) write_edge(keys, w++, me.i, cl.sidx[q]);
          ++cnt;
        }
      }
    });
  if (!FILL) {
    second[p] = 0;
    deg[me.i] = cnt;
    if (cnt > NGPDE_DELAUNAY_MAX_DEGREE) atomicMin(&words->over, me.i);
  }
}

// ---- second pass: one wave per point ---------------------------------------------------------------------------------------------
struct WaveLds {
  Vertex v[kWaveCap];
  unsigned char cut[kWaveCap];
  int first, far;
};

// moves cnt vertices from src to dst (overlapping), the whole wave; chunks in the order that never overwrites what is still to be read
__device__ __forceinline__ void wave_move(Vertex *V, int dst, int src, int cnt, int lane) {
  if (dst == src || cnt <= 0) return;
  const int chunks = (cnt + 63) / 64;
  for (int ci = 0; ci < chunks; ++ci) {
    const int k = (dst < src ? ci : chunks - 1 - ci) * 64 + lane;
    Vertex tmp;
    if (k < cnt) tmp = V[src + k];
    __syncthreads();
    if (k < cnt) V[dst + k] = tmp;
    __syncthreads();
  }
}

// star::clip by the whole wave: the same run (cut_run), the same two new vertices, the same resulting list
template <class LineOf>
__device__ __forceinline__ ClipResult wave_clip(WaveLds &L, int *m_io, const Line &l, LineOf &&line_of, int lane) {
  const int m = *m_io;
  Vertex *V = L.v;
  __syncthreads();
  if (lane == 0) {
    L.first = INT_MAX;
    L.far = 0;
  }
  for (int k = lane; k < m; k += 64) L.cut[k] = is_cut(V[k == 0 ? m - 1 : k - 1], V[k], l, line_of);
  __syncthreads();
  for (int k = lane; k < m; k += 64)
    if (L.cut[k] && !L.cut[k == 0 ? m - 1 : k - 1]) atomicMin(&L.first, k);
  __syncthreads();
  const int a = L.first;
  if (a == INT_MAX) return kUnchanged;
  for (int k = lane; k < m; k += 64)
    if (L.cut[k]) {
      const int t = k >= a ? k - a : k - a + m;
      if (t < m - 1) atomicMax(&L.far, t);
    }
  __syncthreads();
  const int len = L.far + 1, m_new = m - len + 2;
  if (m_new > kWaveCap) return kOverflow;
  int b = a + len - 1;
  const bool wraps = b >= m;
  if (wraps) b -= m;
  const Vertex u = V[a == 0 ? m - 1 : a - 1], va = V[a], vb = V[b], vn = V[b + 1 == m ? 0 : b + 1];
  const Line eu = u.tag == kTagInfinity ? Line{0, 0, 0, 0, kTagInfinity} : line_of(u.tag);
  const Line eb = vb.tag == kTagInfinity ? Line{0, 0, 0, 0, kTagInfinity} : line_of(vb.tag);
  const Vertex A = cross_vertex(eu, l, u, va, l.tag);
  const Vertex B = cross_vertex(eb, l, vn, vb, vb.tag);
  __syncthreads();
  int at;
  if (wraps) {
    at = m - len;
    wave_move(V, 0, b + 1, at, lane);
  } else {
    at = a;
    wave_move(V, a + 2, b + 1, m - 1 - b, lane);
  }
  if (lane == 0) {
    V[at] = A;
    V[at + 1] = B;
  }
  __syncthreads();
  *m_io = m_new;
  return kClipped;
}

__device__ __forceinline__ Line broadcast(const Line &l, int src) {
  Line r;
  r.x = __shfl(l.x, src);
  r.y = __shfl(l.y, src);
  r.h = __shfl(l.h, src);
  r.n = __shfl(l.n, src);
  r.tag = __shfl(l.tag, src);
  return r;
}

template <bool FILL>
__global__ __launch_bounds__(64) void star_wave_kernel(int64_t n, Cloud cl, int32_t *__restrict__ deg, const int32_t *__restrict__ second,
                                                       const int32_t *__restrict__ rowptr, unsigned long long *__restrict__ keys,
                                                       Words *__restrict__ words) {
  extern __shared__ __align__(16) unsigned char wave_lds_raw[];
  WaveLds &L = *reinterpret_cast<WaveLds *>(wave_lds_raw);
  const int64_t p = blockIdx.x;
  if (!second[p]) return;
  const int lane = threadIdx.x;
  const Me me(p, cl);
  Vertex *V = L.v;
  int m = 4;
  if (lane < 4) V[lane] = plane_corner(lane);
  __syncthreads();
  auto line_of = [&](int32_t tag) { return me.line(cl, tag); };
  bool overflow = false;
  int stop_ring = -1;
  auto clip_span = [&](int q0, int q1) {   // 64 candidates at once; the ones that cut are applied in candidate order
    for (int qb = q0; qb < q1 && !overflow; qb += 64) {
      const int q = qb + lane;
      bool valid = q < q1 && q != (int)p;
      Line l{0, 0, 0, 0, 0};
      if (valid) {
        l = me.line(cl, q);
        if (coincident(l)) {
          if (!FILL) report_pair(words, me.i, cl.sidx[q]);
          valid = false;
        }
      }
      bool cuts = false;
      if (valid)
        for (int k = 0; k < m && !cuts; ++k) cuts = is_cut(V[k == 0 ? m - 1 : k - 1], V[k], l, line_of);
      unsigned long long mask = __ballot(cuts);
      while (mask && !overflow) {
        const int src = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        overflow = wave_clip(L, &m, broadcast(l, src), line_of, lane) == kOverflow;
      }
    }
  };
  const int last = min(me.max_ring, kWaveRings);
  for (int ring = 0; ring <= last && !overflow; ++ring) {
    ring_spans(cl.g, me.base, me.c, ring, cl.start, clip_span);
    if (overflow) break;
    if (ring == me.max_ring) {
      stop_ring = ring;
      break;
    }
    if (ring > 0) {
      double r2max = 0.0;
      for (int k = lane; k < m; k += 64) r2max = fmax(r2max, rho2(V[k]));
      for (int off = 32; off > 0; off >>= 1) r2max = fmax(r2max, __shfl_xor(r2max, off));
      if (certified(r2max, ring_reach2(cl.g, ring))) {
        stop_ring = ring;
        break;
      }
    }
  }
  // Not certified within kWaveRings (a hull point's cell never is): the rest of the graph in ONE sweep of its sorted positions
  // instead of ring by ring -- the far rings of a large grid are thousands of one-cell spans, each behind two dependent loads.
  // Candidates seen before come again and change nothing: their line's own vertices are ties, which are kept.
  const int g0 = cl.start[me.base], g1 = cl.start[me.base + cl.g.cells];
  if (stop_ring < 0 && !overflow) clip_span(g0, g1);
  if (overflow) {
    if (!FILL && lane == 0) {
      atomicMin(&words->over, me.i);
      deg[me.i] = 0;
    }
    return;
  }
  int cnt = 0;
  const int64_t w0 = FILL ? rowptr[me.i] : 0;
  auto decide_span = [&](int q0, int q1) {
    for (int qb = q0; qb < q1; qb += 64) {
      const int q = qb + lane;
      bool hit = false;
      if (q < q1 && q != (int)p) {
        const Line l = me.line(cl, q);
        if (!coincident(l)) {
          for (int k = 0; k < m && !hit; ++k) hit = touches(V[k], V[k + 1 == m ? 0 : k + 1], l);
          hit = hit && me.within(cl, q);
        }
      }
      const unsigned long long mask = __ballot(hit);
      if (FILL && hit) write_edge(keys, w0 + cnt + __popcll(mask & ((1ull << lane) - 1ull)), me.i, cl.sidx[q]);
      cnt += __popcll(mask);
    }
  };
  if (stop_ring < 0) decide_span(g0, g1);
  else
    for (int ring = 0; ring <= stop_ring; ++ring) ring_spans(cl.g, me.base, me.c, ring, cl.start, decide_span);
  if (!FILL && lane == 0) {
    deg[me.i] = cnt;
    if (cnt > NGPDE_DELAUNAY_MAX_DEGREE) atomicMin(&words->over, me.i);
    atomicAdd(&words->wave_points, 1);
  }
}

// ---- the symmetric rows and the triangles ----------------------------------------------------------------------------------------
__global__ void split_keys_kernel(int64_t e, const unsigned long long *__restrict__ keys, int base, int32_t *__restrict__ nb,
                                  int32_t *__restrict__ own) {
  const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= e) return;
  own[k] = (int32_t)(keys[k] >> 32) + base;
  nb[k] = (int32_t)(keys[k] & 0xffffffffull) + base;
}

// row[i] = first key of point i (i = 0 .. n)
__global__ void row_start_kernel(int64_t n, int64_t e, const unsigned long long *__restrict__ keys, int32_t *__restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n) return;
  row[i] = (int32_t)lower_bound_dev(keys, e, (unsigned long long)i << 32);
}

// One thread per directed edge (i, j) with i < j: the neighbour k of i that follows j counter-clockwise.  Among the neighbours
// strictly to the left of i -> j (orientation > 0, so the angle is below 180 degrees) it is the one no other is to the right of;
// both signs are those of a x b = a_x b_y - a_y b_x in double on the translated float coordinates.  third[e] = k, or -1.
__global__ void triangle_kernel(int64_t e, const unsigned long long *__restrict__ keys, const int32_t *__restrict__ row,
                                const float *__restrict__ pts, float r2, int32_t *__restrict__ third) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= e) return;
  const int32_t i = (int32_t)(keys[pos] >> 32), j = (int32_t)(keys[pos] & 0xffffffffull);
  int32_t best = -1;
  if (i < j) {
    const float ix = pts[(int64_t)i * 2], iy = pts[(int64_t)i * 2 + 1];
    const double jx = (double)pts[(int64_t)j * 2] - (double)ix, jy = (double)pts[(int64_t)j * 2 + 1] - (double)iy;
    double bx = 0.0, by = 0.0;
    for (int32_t c = row[i]; c < row[i + 1]; ++c) {
      const int32_t k = (int32_t)(keys[c] & 0xffffffffull);
      if (k == j) continue;
      const double kx = (double)pts[(int64_t)k * 2] - (double)ix, ky = (double)pts[(int64_t)k * 2 + 1] - (double)iy;
      if (!(jx * ky - jy * kx > 0.0)) continue;
      if (best < 0 || kx * by - ky * bx > 0.0) {   // k is to the right of the best so far: it comes first
        best = k;
        bx = kx;
        by = ky;
      }
    }
    if (best >= 0) {
      bool ok = best > i;
      if (ok) {   // k in j's row
        const unsigned long long want = ((unsigned long long)(unsigned)j << 32) | (unsigned)best;
        const int64_t at = lower_bound_dev(keys + row[j], (int64_t)(row[j + 1] - row[j]), want);
        ok = at < row[j + 1] - row[j] && keys[row[j] + at] == want;
      }
      if (ok && r2 < INFINITY) {   // max_edge_length: every edge of the triangle under the float rule
        const int32_t tri[3] = {i, j, best};
        for (int s = 0; s < 3 && ok; ++s) {
          const int32_t u = tri[s], v = tri[(s + 1) % 3];
          const float dx = pts[(int64_t)u * 2] - pts[(int64_t)v * 2], dy = pts[(int64_t)u * 2 + 1] - pts[(int64_t)v * 2 + 1];
          float d2 = 0.f;
          d2 = d2 + dx * dx;
          d2 = d2 + dy * dy;
          ok = d2 <= r2;
        }
      }
      if (!ok) best = -1;
    }
  }
  third[pos] = best;
}

__global__ void triangle_flag_kernel(int64_t e, const int32_t *__restrict__ third, int32_t *__restrict__ flag) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos <= e) flag[pos] = pos < e && third[pos] >= 0;
}

// the edges are sorted by (i, j) and every (i, j) leads at most one triangle, so the scanned positions are the lexicographic order
__global__ void triangle_write_kernel(int64_t e, const unsigned long long *__restrict__ keys, const int32_t *__restrict__ third,
                                      const int32_t *__restrict__ at, int base, int32_t *__restrict__ tri) {
  const int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (pos >= e || third[pos] < 0) return;
  int32_t *o = tri + (int64_t)at[pos] * 3;
  o[0] = (int32_t)(keys[pos] >> 32) + base;
  o[1] = (int32_t)(keys[pos] & 0xffffffffull) + base;
  o[2] = third[pos] + base;
}

thread_local int64_t last_lane_points = 0, last_wave_points = 0;

// the sorted, deduplicated (point << 32 | neighbour) keys of the symmetric graph, 0-based; *n_dir of them (0: *keys stays NULL)
int32_t build_edges(int64_t n, const float *pts, const int32_t *gid, int n_graphs, int id_base, float r, int index_base, hipStream_t stream,
                    Scratch &sc, unsigned long long **keys_out, int64_t *n_dir) {
  *keys_out = nullptr;
  *n_dir = 0;
  Cloud cl{};
  PointCells cells;
  int32_t st;
  if ((st = point_cells_2d(n, pts, gid, n_graphs, id_base, kGridK, stream, sc.ptrs, &cl.g, &cells))) return st;
  cl.spts = cells.pts;
  cl.sidx = cells.idx;
  cl.key = cells.key;
  cl.start = cells.start;
  cl.r2 = r * r;
  if (std::isnan(cl.r2)) cl.r2 = INFINITY;   // (r = inf; NaN itself is refused by the entries)
  int32_t *deg = nullptr, *rowptr = nullptr, *second = nullptr;
  Words *words = nullptr;
  if ((st = sc.get(&deg, (size_t)n + 1)) || (st = sc.get(&rowptr, (size_t)n + 1)) || (st = sc.get(&second, (size_t)n)) ||
      (st = sc.get(&words, 1)))
    return st;
  const Words init{kNoPair, kNoPoint, 0};
  NGPDE_HIP_CHECK(hipMemcpyAsync(words, &init, sizeof(init), hipMemcpyHostToDevice, stream));
  NGPDE_HIP_CHECK(hipMemsetAsync(deg, 0, ((size_t)n + 1) * sizeof(int32_t), stream));
  const dim3 lane_grid((unsigned)((n + kLaneThreads - 1) / kLaneThreads)), wave_grid((unsigned)n);
  const size_t wave_lds = sizeof(WaveLds);
  NGPDE_HIP_CHECK(hipFuncSetAttribute((const void *)star_wave_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wave_lds));
  NGPDE_HIP_CHECK(hipFuncSetAttribute((const void *)star_wave_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)wave_lds));
  hipLaunchKernelGGL(star_lane_kernel<false>, lane_grid, dim3(kLaneThreads), 0, stream, n, cl, deg, second, (const int32_t *)nullptr,
                     (unsigned long long *)nullptr, words);
  NGPDE_LAUNCH_CHECK("star_lane_kernel(count)");
  hipLaunchKernelGGL(star_wave_kernel<false>, wave_grid, dim3(64), wave_lds, stream, n, cl, deg, (const int32_t *)second,
                     (const int32_t *)nullptr, (unsigned long long *)nullptr, words);
  NGPDE_LAUNCH_CHECK("star_wave_kernel(count)");
  auto scan = [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, deg, rowptr, 0, (size_t)n + 1, rocprim::plus<int32_t>(), stream);
  };
  if ((st = with_temp(sc, scan))) return st;
  Words h{};
  int32_t h_total = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h, words, sizeof(h), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_total, rowptr + n, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  last_wave_points = h.wave_points;
  last_lane_points = n - h.wave_points;
  NGPDE_REQUIRE(h.pair == kNoPair, NGPDE_ERR_INVALID_ARGUMENT, "delaunay: points %lld and %lld coincide (%s index)",
                (long long)(h.pair >> 32) + index_base, (long long)(h.pair & 0xffffffffull) + index_base, index_base ? "1-based" : "0-based");
  NGPDE_REQUIRE(h.over == kNoPoint, NGPDE_ERR_INVALID_ARGUMENT,
                "delaunay: the star of point %lld exceeds NGPDE_DELAUNAY_MAX_DEGREE = %d (%s index)", (long long)h.over + index_base,
                NGPDE_DELAUNAY_MAX_DEGREE, index_base ? "1-based" : "0-based");
  NGPDE_REQUIRE(h_total >= 0 && h_total <= 0x3fffffff, NGPDE_ERR_UNSUPPORTED, "delaunay: the stars hold more than 2^30 entries");
  if (h_total == 0) return NGPDE_OK;
  const size_t pairs = 2 * (size_t)h_total;
  unsigned long long *keys = nullptr, *sorted = nullptr, *uniq = nullptr;
  size_t *n_uniq = nullptr;
  if ((st = sc.get(&keys, pairs)) || (st = sc.get(&sorted, pairs)) || (st = sc.get(&uniq, pairs)) || (st = sc.get(&n_uniq, 1))) return st;
  hipLaunchKernelGGL(star_lane_kernel<true>, lane_grid, dim3(kLaneThreads), 0, stream, n, cl, (int32_t *)nullptr, second,
                     (const int32_t *)rowptr, keys, words);
  NGPDE_LAUNCH_CHECK("star_lane_kernel(fill)");
  hipLaunchKernelGGL(star_wave_kernel<true>, wave_grid, dim3(64), wave_lds, stream, n, cl, (int32_t *)nullptr, (const int32_t *)second,
                     (const int32_t *)rowptr, keys, words);
  NGPDE_LAUNCH_CHECK("star_wave_kernel(fill)");
  const unsigned end_bit = 32u + bits_for((unsigned long long)std::max<int64_t>(n, 2));
  auto sort = [&](void *tmp, size_t &bytes) { return rocprim::radix_sort_keys(tmp, bytes, keys, sorted, pairs, 0u, end_bit, stream); };
  if ((st = with_temp(sc, sort))) return st;
  auto unique = [&](void *tmp, size_t &bytes) {
    return rocprim::unique(tmp, bytes, sorted, uniq, n_uniq, pairs, rocprim::equal_to<unsigned long long>(), stream);
  };
  if ((st = with_temp(sc, unique))) return st;
  size_t h_uniq = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_uniq, n_uniq, sizeof(size_t), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  *keys_out = uniq;
  *n_dir = (int64_t)h_uniq;
  return NGPDE_OK;
}

int32_t check_cloud(const char *fn, int64_t n, const float *pts, const int32_t *gid, int32_t n_graphs, float r, int64_t capacity,
                    const void *count) {
  NGPDE_REQUIRE(n >= 0 && n <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: number of points %lld outside 0:2^31-1", fn, (long long)n);
  NGPDE_REQUIRE(n == 0 || pts != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: points is NULL", fn);
  NGPDE_REQUIRE(n_graphs >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_graphs must be >= 1", fn);
  NGPDE_REQUIRE(gid != nullptr || n_graphs == 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_graphs > 1 needs a graph_id", fn);
  NGPDE_REQUIRE(r >= 0.f, NGPDE_ERR_INVALID_ARGUMENT, "%s: max_edge_length must be >= 0 or +inf (got %g)", fn, (double)r);
  NGPDE_REQUIRE(capacity >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: capacity %lld is negative", fn, (long long)capacity);
  NGPDE_REQUIRE(count != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: the count pointer is NULL", fn);
  return NGPDE_OK;
}

}  // namespace
}  // namespace ngpde

using namespace ngpde;

extern "C" {

int32_t ngpde_delaunay_graph(int64_t n, const float *points, const int32_t *graph_id, int32_t n_graphs, int32_t id_base,
                             float max_edge_length, int32_t dir_out, int32_t index_base, int64_t capacity, int32_t *s, int32_t *t,
                             int64_t *n_edges, ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_cloud("delaunay_graph", n, points, graph_id, n_graphs, max_edge_length, capacity, n_edges);
  if (st) return st;
  NGPDE_REQUIRE((s == nullptr) == (t == nullptr), NGPDE_ERR_INVALID_ARGUMENT, "delaunay_graph: s and t must both be given or both be NULL");
  *n_edges = 0;
  last_lane_points = last_wave_points = 0;
  if (n == 0) return NGPDE_OK;
  hipStream_t hs = (hipStream_t)stream;
  Scratch sc;
  unsigned long long *keys = nullptr;
  int64_t e = 0;
  if ((st = build_edges(n, points, graph_id, n_graphs, id_base, max_edge_length, index_base, hs, sc, &keys, &e))) return st;
  *n_edges = e;
  if (!s) return NGPDE_OK;
  NGPDE_REQUIRE(e <= capacity, NGPDE_ERR_INVALID_ARGUMENT, "delaunay_graph: the graph has %lld edges, the output arrays hold %lld",
                (long long)e, (long long)capacity);
  if (e == 0) return NGPDE_OK;
  hipLaunchKernelGGL(split_keys_kernel, dim3(blocks_for(e)), dim3(kB), 0, hs, e, (const unsigned long long *)keys, index_base,
                     dir_out ? t : s, dir_out ? s : t);
  NGPDE_LAUNCH_CHECK("split_keys_kernel");
  NGPDE_HIP_CHECK(hipStreamSynchronize(hs));
  return NGPDE_OK;
}

int32_t ngpde_delaunay_triangles(int64_t n, const float *points, const int32_t *graph_id, int32_t n_graphs, int32_t id_base,
                                 float max_edge_length, int32_t index_base, int64_t capacity, int32_t *tri, int64_t *n_triangles,
                                 ngpde_stream_t stream) {
  NGPDE_RANGE();
  int32_t st = check_cloud("delaunay_triangles", n, points, graph_id, n_graphs, max_edge_length, capacity, n_triangles);
  if (st) return st;
  *n_triangles = 0;
  last_lane_points = last_wave_points = 0;
  if (n == 0) return NGPDE_OK;
  hipStream_t hs = (hipStream_t)stream;
  Scratch sc;
  unsigned long long *keys = nullptr;
  int64_t e = 0;
  // the rows WITHOUT the limit: a dropped edge must not make two of a point's neighbours adjacent
  if ((st = build_edges(n, points, graph_id, n_graphs, id_base, INFINITY, index_base, hs, sc, &keys, &e))) return st;
  if (e == 0) return NGPDE_OK;
  int32_t *row = nullptr, *third = nullptr, *flag = nullptr, *at = nullptr;
  if ((st = sc.get(&row, (size_t)n + 1)) || (st = sc.get(&third, (size_t)e)) || (st = sc.get(&flag, (size_t)e + 1)) ||
      (st = sc.get(&at, (size_t)e + 1)))
    return st;
  float r2 = max_edge_length * max_edge_length;
  if (std::isnan(r2)) r2 = INFINITY;
  hipLaunchKernelGGL(row_start_kernel, dim3(blocks_for(n + 1)), dim3(kB), 0, hs, n, e, (const unsigned long long *)keys, row);
  NGPDE_LAUNCH_CHECK("row_start_kernel");
  hipLaunchKernelGGL(triangle_kernel, dim3(blocks_for(e)), dim3(kB), 0, hs, e, (const unsigned long long *)keys, (const int32_t *)row,
                     points, r2, third);
  NGPDE_LAUNCH_CHECK("triangle_kernel");
  hipLaunchKernelGGL(triangle_flag_kernel, dim3(blocks_for(e + 1)), dim3(kB), 0, hs, e, (const int32_t *)third, flag);
  NGPDE_LAUNCH_CHECK("triangle_flag_kernel");
  auto scan = [&](void *tmp, size_t &bytes) {
    return rocprim::exclusive_scan(tmp, bytes, flag, at, 0, (size_t)e + 1, rocprim::plus<int32_t>(), hs);
  };
  if ((st = with_temp(sc, scan))) return st;
  int32_t h_t = 0;
  NGPDE_HIP_CHECK(hipMemcpyAsync(&h_t, at + e, sizeof(int32_t), hipMemcpyDeviceToHost, hs));
  NGPDE_HIP_CHECK(hipStreamSynchronize(hs));
  *n_triangles = h_t;
  if (!tri) return NGPDE_OK;
  NGPDE_REQUIRE(h_t <= capacity, NGPDE_ERR_INVALID_ARGUMENT, "delaunay_triangles: %lld triangles, the output array holds %lld",
                (long long)h_t, (long long)capacity);
  if (h_t == 0) return NGPDE_OK;
  hipLaunchKernelGGL(triangle_write_kernel, dim3(blocks_for(e)), dim3(kB), 0, hs, e, (const unsigned long long *)keys, (const int32_t *)third,
                     (const int32_t *)at, index_base, tri);
  NGPDE_LAUNCH_CHECK("triangle_write_kernel");
  NGPDE_HIP_CHECK(hipStreamSynchronize(hs));
  return NGPDE_OK;
}

int32_t ngpde_delaunay_last_passes(int64_t *lane_points, int64_t *wave_points) {
  if (lane_points) *lane_points = last_lane_points;
  if (wave_points) *wave_points = last_wave_points;
  return NGPDE_OK;
}

}  // extern "C"
