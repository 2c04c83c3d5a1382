// coarsen_rule.h -- the decision rules of the coarsening block (include/ngpde_coarsen.h; kernels: coarsen.hip): which of two
// farthest-point candidates wins, the squared distance both FPS kernels use, how a batch's graphs are laid out over the two FPS
// paths, and the cell / key rule of grid_cluster.  Plain C++: it compiles with a host compiler alone (tests/host/coarsen_rule_check.cpp
// holds every function here to a brute force under ASan + UBSan) and, with NGPDE_HD, inside the kernels -- one definition of each.
// The library is compiled with -ffp-contract=off, and so is the check: no product below is fused into a sum.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define NGPDE_HD __host__ __device__ __forceinline__
#else
#define NGPDE_HD inline
#endif

namespace ngpde {
namespace coarsen {

// ---- farthest-point sampling ---------------------------------------------------------------------------------------------------
constexpr int kFpsTileThreads = 1024;       // W: the tile path's workgroup
constexpr int kFpsTileMaxPerThread = 16;    // points a thread of the tile path holds in registers
constexpr int kFpsTileMaxPoints = kFpsTileThreads * kFpsTileMaxPerThread;   // = NGPDE_FPS_TILE_MAX_POINTS (16 384)
constexpr int kFpsRoundThreads = 256;       // the round path's workgroup
constexpr int kFpsRoundPerThread = 8;
constexpr int kFpsSlice = kFpsRoundThreads * kFpsRoundPerThread;   // points of one round-path workgroup (2 048)

constexpr float kKeySelected = -1.f;   // the key of a point once it has been selected
constexpr float kKeyNone = -2.f;       // below every key of a real point: a lane or slot without a candidate
constexpr int32_t kIdxNone = 0x7fffffff;

struct Cand {   // a candidate of a round: the key and the position inside the graph
  float key;
  int32_t idx;
};

// "larger key, then smaller index": a total order on candidates with distinct indices, so the maximum does not depend on the
// order or the shape of the reduction
NGPDE_HD bool better(float ka, int32_t ia, float kb, int32_t ib) { return ka > kb || (ka == kb && ia < ib); }
NGPDE_HD Cand pick(Cand a, Cand b) { return better(b.key, b.idx, a.key, a.idx) ? b : a; }

// the neighbour search's float rule: the sum over the coordinates, in order, of (p - q)^2, every operation rounded to float
template <int DIM>
NGPDE_HD float dist2(const float *p, const float *q) {
  float dx = p[0] - q[0];
  float s = dx * dx;
  if (DIM > 1) {
    float dy = p[1] - q[1];
    s = s + dy * dy;
  }
  if (DIM > 2) {
    float dz = p[2] - q[2];
    s = s + dz * dz;
  }
  return s;
}
NGPDE_HD float dist2(int dim, const float *p, const float *q) {
  return dim == 1 ? dist2<1>(p, q) : dim == 2 ? dist2<2>(p, q) : dist2<3>(p, q);
}

// the key of an unselected point after the round that selected s: min(key, d2(p, p_s)); a NaN distance leaves the key as it is
NGPDE_HD float updated_key(float key, float d2) { return d2 < key ? d2 : key; }

// the tile path's points per thread for a graph of n points: 1, 4 or 16 (the three instantiations of the kernel)
NGPDE_HD int tile_per_thread(int64_t n) { return n <= kFpsTileThreads ? 1 : n <= 4 * kFpsTileThreads ? 4 : kFpsTileMaxPerThread; }
NGPDE_HD int tile_class(int64_t n) { return n <= kFpsTileThreads ? 0 : n <= 4 * kFpsTileThreads ? 1 : 2; }

// One graph with work (n > 0 and k > 0) on either path.  lo: its first point; out: where its samples start in idx / d2
struct FpsGraph {
  int32_t lo, n, k, out, g;
  int32_t first_part;   // round path: its first slice's position among the partials (= its first workgroup); tile path: 0
  int32_t n_parts;      // round path: its slices, ceil(n / kFpsSlice); tile path: 0
  int32_t key_off;      // round path: where its keys start in the workspace; tile path: 0
};

struct FpsLayout {
  int64_t n_points = 0, n_samples = 0;
  std::vector<FpsGraph> tile[3];   // by tile_class
  std::vector<FpsGraph> round;
  std::vector<int32_t> wg_graph;   // round path: workgroup b works on round[wg_graph[b]], slice b - round[..].first_part
  int32_t round_launches = 0;      // the largest k of a round-path graph
  int64_t round_points = 0;        // keys in the workspace
  int32_t n_tile_graphs() const { return (int32_t)(tile[0].size() + tile[1].size() + tile[2].size()); }
};

// what refuses a plan, found before any device is touched; 0: fine.  *where: the graph (0-based) the refusal names
enum FpsRefusal { kFpsOk = 0, kFpsBadStart, kFpsDecreasing, kFpsSamplesDecreasing, kFpsTooMany, kFpsOverCap, kFpsTooLarge };

// path: 0 auto (the tile path where the graph fits), 1 tile, 2 round
inline FpsRefusal fps_layout(int32_t n_graphs, const int64_t *graph_ptr, const int64_t *sample_ptr, int path, FpsLayout *out, int32_t *where) {
  *out = FpsLayout();
  *where = 0;
  if (graph_ptr[0] != 0 || sample_ptr[0] != 0) return kFpsBadStart;
  for (int32_t g = 0; g < n_graphs; ++g) {
    *where = g;
    const int64_t n = graph_ptr[g + 1] - graph_ptr[g], k = sample_ptr[g + 1] - sample_ptr[g];
    if (n < 0) return kFpsDecreasing;
    if (k < 0) return kFpsSamplesDecreasing;
    if (k > n) return kFpsTooMany;
    if (graph_ptr[g + 1] > 0x7fffffffLL) return kFpsTooLarge;
    if (path == 1 && n > kFpsTileMaxPoints) return kFpsOverCap;
    if (k == 0) continue;
    FpsGraph f = {(int32_t)graph_ptr[g], (int32_t)n, (int32_t)k, (int32_t)sample_ptr[g], g, 0, 0, 0};
    const bool tile = path == 1 || (path == 0 && n <= kFpsTileMaxPoints);
    if (tile) {
      out->tile[tile_class(n)].push_back(f);
    } else {
      f.first_part = (int32_t)out->wg_graph.size();
      f.n_parts = (int32_t)((n + kFpsSlice - 1) / kFpsSlice);
      f.key_off = (int32_t)out->round_points;
      out->round_points += n;
      for (int32_t s = 0; s < f.n_parts; ++s) out->wg_graph.push_back((int32_t)out->round.size());
      if (f.k > out->round_launches) out->round_launches = f.k;
      out->round.push_back(f);
    }
  }
  out->n_points = graph_ptr[n_graphs];
  out->n_samples = sample_ptr[n_graphs];
  return kFpsOk;
}

// ---- grid clusters -------------------------------------------------------------------------------------------------------------
// the cell of coordinate p over the origin o with cell size h: floorf((p - o) / h), one float subtraction and one correctly rounded
// float division.  ok = false where the quotient is not a cell an int32 holds (non-finite, negative, or 2^31 and beyond).
NGPDE_HD float cell_quotient(float p, float o, float h) { return floorf((p - o) / h); }
NGPDE_HD bool cell_fits(float q) { return q >= 0.f && q < 2147483648.f; }

NGPDE_HD unsigned bits_holding(uint64_t top) {   // bits that hold every value 0 .. top
  unsigned b = 0;
  while (b < 64 && (top >> b) != 0) ++b;
  return b;
}

// The key of (graph, c_z, c_y, c_x), x fastest: fields of bits[d] bits for coordinate d (what holds the cloud's largest cell of that
// coordinate) under a field of bits_holding(n_graphs - 1) bits for the 0-based graph.  More than 63 bits in all is refused.
struct KeyBits {
  unsigned c[3] = {0, 0, 0}, g = 0;
  unsigned total() const { return c[0] + c[1] + c[2] + g; }
};
inline KeyBits key_bits(int dim, const int64_t *max_cell, int32_t n_graphs) {
  KeyBits kb;
  for (int d = 0; d < dim; ++d) kb.c[d] = bits_holding((uint64_t)max_cell[d]);
  kb.g = bits_holding((uint64_t)(n_graphs > 0 ? n_graphs - 1 : 0));
  return kb;
}
NGPDE_HD uint64_t cell_key(int dim, const int32_t *c, int32_t g, unsigned b0, unsigned b1, unsigned b2) {
  uint64_t key = (uint64_t)g;
  if (dim > 2) key = (key << b2) | (uint64_t)c[2];
  if (dim > 1) key = (key << b1) | (uint64_t)c[1];
  key = (key << b0) | (uint64_t)c[0];
  return key;
}

}  // namespace coarsen
}  // namespace ngpde
