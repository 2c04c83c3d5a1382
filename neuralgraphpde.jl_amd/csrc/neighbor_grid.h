// neighbor_grid.h -- the host side of the neighbour search's cell grid (neighbors.hip): how the grid is sized, which cell a
// point falls in, the k-NN cell edge and the quantisation of the space-filling-curve keys.  Includes nothing from HIP, so
// tests/host/neighbor_grid_check.cpp checks it as a stand-alone host program.
//
// What the kernels need of a grid (the decision rule itself is the float rule of neighbors.hip's header):
//   covering    every pair whose float d2 is <= the float r*r lies in cells that differ by at most 1 per dimension
//               (radius_kernel reads the 3^dim block around a point's cell and nothing else);
//   ring bound  a point in a cell at Chebyshev distance > ring from the home cell has a float d2 >= reach*reach, where
//               reach = ((float)ring - 0.02f) * cell as knn_kernel forms it (a ring stop never cuts off one of the k smallest).
// Both hold when (1) the cell edge is >= 1.01 * the largest |p_i - p_j| per coordinate that the float rule can accept,
// (2) a cell coordinate is wrong by at most 1e-3 cells, and (3) cell and 1 / cell are finite and positive.  (1) fails for
// a cell of 1.01 r where squares leave the float range, which is what the three rules below are for.
//
// Two-set search (ngpde_knn_query / ngpde_radius_query, include/ngpde_interp.h).  The grid is sized over the DATA points alone
// (their box, their count): a grid over the union would be coarsened by a handful of far queries until the cells of the data no
// longer separate anything, and the data's grid is the one the one-set entries already prove.  A query may then lie anywhere, and
// cell_of_query clamps its cell coordinate to the grid.  Covering and the ring bound survive the clamp: let q' be q with every
// coordinate clamped to the data's [lo, hi].  Every data coordinate lies in [lo, hi], so |p - q'| <= |p - q| per coordinate for
// every data point p -- a clamped query is at least as far from every point, hence from every cell, as its clamped position is.
//   the cell   q' lies in the box, and the clamped cell of q is a cell condition (2) allows for q': below lo the float difference
//              is negative, the cell is 0 and q' = lo has coordinate exactly 0; above hi the float coordinate is monotone in q, so
//              it is >= the one of q' = hi, and the clamp returns either that cell or the top cell, whose exact lower edge
//              top <= ext / cell is within the same 1e-3 of hi's coordinate;
//   covering   a pair (q, p) the float rule accepts has |p - q| <= the bound of (1) per coordinate, so |p - q'| has it too, and
//              the argument for two points of the box puts p within one cell of q''s cell per dimension;
//   ring bound a point p in a cell at Chebyshev distance > ring from q's clamped cell is >= (ring - 0.002) cells from q' in one
//              coordinate, so at least as far from q in that coordinate, and its float d2 (a sum of non-negative terms, each
//              rounded monotonically) is >= reach^2 as for two points of the box.
// A far query pays for this in time, not in correctness: its k-th distance exceeds every ring's reach until the walk has seen
// the whole grid of its graph.  What must hold of the two sets TOGETHER is the span: q - lo is formed in float, so span_is_finite is
// asked of the union's box.  tests/host/neighbor_query_check.cpp checks covering and the ring bound for clamped queries by brute force.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <limits>

#if defined(__HIPCC__)
#define NGPDE_GRID_HD __host__ __device__ __forceinline__
#else
#define NGPDE_GRID_HD inline
#endif

namespace ngpde {

struct Grid {
  float lo[3];
  float inv;        // 1 / cell edge
  float cell;       // cell edge
  int nc[3];        // cells per dimension
  int cells;        // per graph
};

// (p - lo) * inv in float, clamped to the grid.  With at most kMaxCellsPerDim cells per dimension the two roundings (the
// difference, the product) move the coordinate by at most 8192 * 2^-23 < 1e-3 cells from the same expression evaluated
// exactly; the rounding of inv = 1 / cell itself is one common factor of every coordinate, i.e. a grid whose cell is
// 2^-24 shorter or longer.
template <int DIM>
NGPDE_GRID_HD void cell_of(const Grid &g, const float *p, int *c) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int d = 0; d < DIM; ++d) {
    const int x = (int)((p[d] - g.lo[d]) * g.inv);
    const int top = g.nc[d] - 1;
    c[d] = x < 0 ? 0 : (x > top ? top : x);
  }
}
// cell_of for a point of a second set (a query), which may lie anywhere relative to the grid: the same expression, clamped as a
// float BEFORE the conversion (a coordinate thousands of boxes away, or inf after the product, has no int value).  For a coordinate
// inside the grid the result is cell_of's.  The header comment says why a clamped cell serves.
template <int DIM>
NGPDE_GRID_HD void cell_of_query(const Grid &g, const float *p, int *c) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int d = 0; d < DIM; ++d) {
    const float x = (p[d] - g.lo[d]) * g.inv;
    const int top = g.nc[d] - 1;
    c[d] = x >= (float)top ? top : (x > 0.f ? (int)x : 0);
  }
}
template <int DIM>
NGPDE_GRID_HD int linear_cell(const Grid &g, const int *c) {
  int l = c[0];
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int d = 1; d < DIM; ++d) l = l * g.nc[d] + c[d];
  return l;
}

// k-NN ring stop: after ring `ring` every unvisited point is at least ring cells minus the coordinates' rounding away
// (the point lies inside its home cell); a k-th distance below this value is final
NGPDE_GRID_HD float ring_reach2(const Grid &g, int ring) {
  const float reach = ((float)ring - 0.02f) * g.cell;
  return reach * reach;
}

constexpr int kMaxCellsPerDim = 8192;

// Lower bound of the cell edge.  Where squares underflow, the float rule accepts pairs that are further apart than r:
// a product df*df below FLT_MIN is rounded to a multiple of the smallest denormal u = 2^-149, so it is wrong by up to u/2
// in absolute terms (sums of such values are exact), and so is r*r.  A pair with float d2 <= float r*r therefore has, in
// exact arithmetic, d2 <= r^2 (1 + 2^-22) + (dim + 1) u/2, and every |p_i - p_j| <= sqrt(r^2 + A) with
// A = (dim + 1) u/2 <= 2u = 2^-148 for dim <= 3, sqrt(A) <= 2^-74 (5.3e-23).  With kMinCell = 32 sqrt(A) = 2^-69 (1.7e-21):
//   1.01 r >= kMinCell:  sqrt(r^2 + A) <= r sqrt(1 + 1.0201 / 1024) < 1.0005 r, so the cell 1.01 r keeps a margin of 0.9 %;
//   1.01 r <  kMinCell:  sqrt(r^2 + A) <  kMinCell sqrt(1 / 1.0201 + 1 / 1024) < 0.9908 kMinCell, the ordinary margin.
// Either is above the 2e-3 cells two coordinates are wrong by together.  The same bound keeps the k-NN ring stop sound:
// an unvisited point is >= (ring - 0.002) cells away in one coordinate, reach^2 is ((ring - 0.02) cell)^2, and the gap
// 0.035 cell^2 >= 0.035 * 2^-138 is far above the 2u the roundings can move the two sides by.  And 1 / kMinCell = 2^69 and
// 2^30 / kMinCell = 2^99 (the finest curve quantisation) are finite, where 1 / (a denormal) is inf.
constexpr float kMinCell = 0x1p-69f;

// `want` of the radius grid: 1 % above r.  A finite r whose float square is inf accepts every pair (d2 <= inf), exactly
// as r = inf does, so the grid is sized as for r = inf: one cell.
inline float radius_want(float r) {
  const float r2 = r * r;
  return std::isfinite(r2) ? r * 1.01f : std::numeric_limits<float>::infinity();
}

// `want` of the k-NN grid: about k/2 points per cell on average, so the first ring usually settles a point
inline float knn_want(int dim, const float *lo, const float *hi, int64_t n, int n_graphs, int k) {
  double vol = 1.0;
  for (int d = 0; d < dim; ++d) vol *= std::max((double)hi[d] - (double)lo[d], 1e-30);
  const double per_graph = std::max(1.0, (double)n / n_graphs);
  const double want = std::pow(vol * std::max(1.0, 0.5 * k) / per_graph, 1.0 / dim);
  return want < (double)FLT_MAX ? (float)want : std::numeric_limits<float>::infinity();
}

// hi - lo is finite in every dimension (two finite coordinates can be more than FLT_MAX apart; no cell edge covers that)
inline bool span_is_finite(int dim, const float *lo, const float *hi) {
  for (int d = 0; d < dim; ++d)
    if (!std::isfinite(hi[d] - lo[d])) return false;
  return true;
}

// cell edge >= max(want, kMinCell), at most ~budget cells in total over all graphs, at most kMaxCellsPerDim per dimension
// (which bounds the rounding of a cell coordinate, see cell_of).  Needs a finite span (span_is_finite).
//   want = inf or NaN (r = inf, r*r = inf)  -> one cell;
//   want <= 0 (r = 0)                       -> the finest grid the caps allow;
//   coarsening multiplies the edge by 1.26 (a factor 2 in the cells of a 3-D grid) until the budget holds; the edge starts
//   at >= ext_max / 8192 and one cell is reached above ext_max, so the loop ends within 40 steps.  An edge that would leave
//   the float range on the way ends it at once with one cell.  *coarsenings (optional) receives the number of steps.
inline Grid make_grid(int dim, const float *lo, const float *hi, float want, int64_t budget, int n_graphs,
                      int *coarsenings = nullptr) {
  Grid g{};
  float ext[3] = {0.f, 0.f, 0.f};
  float ext_max = 0.f;
  for (int d = 0; d < dim; ++d) {
    ext[d] = hi[d] - lo[d];
    ext_max = std::max(ext_max, ext[d]);
  }
  for (int d = 0; d < 3; ++d) g.lo[d] = d < dim ? lo[d] : 0.f;
  int steps = 0;
  float cell = want;
  bool one_cell = !std::isfinite(cell) || !std::isfinite(ext_max);
  if (!one_cell) {
    if (!(cell > 0.f)) cell = ext_max > 0.f ? ext_max / (float)kMaxCellsPerDim : 1.f;
    cell = std::max(std::max(cell, ext_max / (float)kMaxCellsPerDim), kMinCell);
    for (;;) {
      int64_t cells = 1;
      for (int d = 0; d < 3; ++d) {
        g.nc[d] = 1;
        if (d < dim) g.nc[d] = (int)std::min<double>((double)kMaxCellsPerDim, std::floor((double)ext[d] / cell) + 1.0);
        cells *= g.nc[d];
      }
      if (cells * n_graphs <= budget || cells == 1) {
        g.cells = (int)cells;
        break;
      }
      if (!(cell < FLT_MAX / 1.26f)) {
        one_cell = true;
        break;
      }
      cell *= 1.26f;
      ++steps;
    }
  }
  if (one_cell) {   // every coordinate clamps to cell 0 whatever inv is; the largest edge whose inverse is not 0
    cell = std::isfinite(ext_max) ? std::min(std::max(std::max(ext_max, 1.f) * 2.f, kMinCell), 0x1p126f) : 0x1p126f;
    g.nc[0] = g.nc[1] = g.nc[2] = 1;
    g.cells = 1;
  }
  g.cell = cell;
  g.inv = 1.0f / cell;
  if (coarsenings) *coarsenings = steps;
  return g;
}

// total cells over all graphs: ~4 per point, and (graph, cell) keys must fit 32 bits
inline int64_t cell_budget(int64_t n) { return std::min<int64_t>(std::max<int64_t>(4 * n, 1 << 16), (int64_t)1 << 30); }

// ---- quantisation of the space-filling-curve keys: q = (p - lo) * scale, clamped to 0 .. 2^bits - 1 ------------------------
struct Quant {
  float lo[3];
  float scale[3];
  int bits;
};

// An extent below kMinCell quantises as extent 0 (every point at q = 0 in that dimension): 2^bits / ext is inf for
// ext < 2^bits / FLT_MAX, and (p - lo) * inf is NaN at p = lo.  oracle.ngpde_oracle.spatial_order states the same rule.
inline Quant make_quant(int dim, const float *lo, const float *hi) {
  Quant qz{};
  qz.bits = dim == 1 ? 30 : (dim == 2 ? 16 : 10);
  for (int d = 0; d < dim; ++d) {
    const float ext = hi[d] - lo[d];
    qz.lo[d] = lo[d];
    qz.scale[d] = ext >= kMinCell ? (float)(1u << qz.bits) / ext : 0.f;
  }
  return qz;
}

}  // namespace ngpde
