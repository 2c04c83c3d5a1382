// neighbor_query_check.cpp -- stand-alone check of the two-set part of csrc/neighbor_grid.h on the host (built with ASan + UBSan and
// -ffp-contract=off by tests/test_interp_host.py, as tests/test_neighbor_grid_host.py builds neighbor_grid_check.cpp).  The grid is
// sized over the DATA points; a query may lie anywhere and cell_of_query clamps its cell to the grid.  By brute force, on the header's
// own functions with the library's operation order:
//   same cell   cell_of_query gives a data point (a coordinate inside the grid) the cell cell_of gives it;
//   in range    every query, up to coordinates at +-1e38 and products that overflow to inf, gets cells in 0 .. nc - 1 (and the
//               conversion to int is defined: the program runs under UBSan);
//   covering    every (query, point) pair with float d2 <= r*r lies in cells that differ by at most 1 per dimension;
//   ring        a point in a cell at Chebyshev distance D >= 2 from the query's clamped cell has a float d2 >= ring_reach2(ring)
//               for every ring < D (checked at D - 1 and 1).
// Queries: inside the box, a quarter outside on every side by up to two boxes, and far ones (hundreds to 1e6 cells away, and at
// magnitudes where squares overflow).  Prints the regimes reached and "<checks> checks, <failed> failed"; exit status 1 on a failure.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "neighbor_grid.h"

using namespace ngpde;

namespace {

long checks = 0, failures = 0;
void check(bool ok, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
void check(bool ok, const char *fmt, ...) {
  ++checks;
  if (ok) return;
  if (++failures > 20) return;
  va_list ap;
  va_start(ap, fmt);
  std::fprintf(stderr, "FAILED ");
  std::vfprintf(stderr, fmt, ap);
  std::fprintf(stderr, "\n");
  va_end(ap);
}

const float kInf = std::numeric_limits<float>::infinity();

struct Rng {   // 64-bit LCG, the high 24 bits as a float in [0, 1)
  uint64_t s;
  float next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(s >> 40) * 0x1p-24f;
  }
};

template <int DIM>
float dist2(const float *a, const float *b) {   // neighbors.hip's, operation by operation
  float d2 = 0.f;
  for (int d = 0; d < DIM; ++d) {
    const float df = a[d] - b[d];
    d2 = d2 + df * df;
  }
  return d2;
}

long n_clamped = 0, n_far = 0, n_accepted = 0, n_accepted_clamped = 0, n_ring_pairs = 0, n_ring_clamped = 0;

// data: n points in lo + scale * [0, 1)^DIM (a cluster in one corner when `corner`)
template <int DIM>
void run(const char *name, int n, uint64_t seed, float scale, float offset, bool corner) {
  Rng rng{seed};
  std::vector<float> p((size_t)n * DIM);
  for (auto &v : p) v = offset + scale * (corner ? 0.1f : 1.f) * rng.next();
  if (corner)   // one point in the far corner keeps the box large while the cluster stays in the near one
    for (int d = 0; d < DIM; ++d) p[d] = offset + scale;
  float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
  for (int d = 0; d < DIM; ++d) {
    lo[d] = hi[d] = p[d];
    for (int i = 1; i < n; ++i) {
      lo[d] = std::min(lo[d], p[(size_t)i * DIM + d]);
      hi[d] = std::max(hi[d], p[(size_t)i * DIM + d]);
    }
  }
  // queries: inside, just outside on every side, far outside, and at the edge of the float range
  std::vector<float> q;
  const int m = 240;
  for (int j = 0; j < m; ++j)
    for (int d = 0; d < DIM; ++d) {
      const float ext = hi[d] - lo[d];
      float v;
      if (j % 4 != 0) v = lo[d] + ext * rng.next();                               // inside
      else if (j % 16 != 0) v = lo[d] + ext * (rng.next() * 5.f - 2.f);           // up to two boxes outside on either side
      else if (j % 32 != 0) v = lo[d] + ext * (rng.next() - 0.5f) * 2e3f;         // hundreds of boxes away
      else v = (rng.next() < 0.5f ? -1.f : 1.f) * (j % 64 ? 1e30f : 1e38f);       // squares overflow; 1e38 - lo stays finite
      q.push_back(v);
    }
  float ulo[3], uhi[3];
  for (int d = 0; d < 3; ++d) ulo[d] = lo[d], uhi[d] = hi[d];
  for (int j = 0; j < m; ++j)
    for (int d = 0; d < DIM; ++d) {
      ulo[d] = std::min(ulo[d], q[(size_t)j * DIM + d]);
      uhi[d] = std::max(uhi[d], q[(size_t)j * DIM + d]);
    }
  check(span_is_finite(DIM, ulo, uhi), "%s: the union's span is not finite", name);
  float ext_max = 0.f;
  for (int d = 0; d < DIM; ++d) ext_max = std::max(ext_max, hi[d] - lo[d]);
  std::vector<int> cp((size_t)n * DIM), cq((size_t)m * DIM);

  auto cells = [&](const Grid &g) {
    for (int i = 0; i < n; ++i) {
      cell_of<DIM>(g, &p[(size_t)i * DIM], &cp[(size_t)i * DIM]);
      int same[3];
      cell_of_query<DIM>(g, &p[(size_t)i * DIM], same);
      for (int d = 0; d < DIM; ++d)
        check(same[d] == cp[(size_t)i * DIM + d], "%s: cell_of_query puts a data point in cell %d, cell_of in %d", name, same[d],
              cp[(size_t)i * DIM + d]);
    }
    std::vector<char> clamped(m, 0);
    for (int j = 0; j < m; ++j) {
      cell_of_query<DIM>(g, &q[(size_t)j * DIM], &cq[(size_t)j * DIM]);
      for (int d = 0; d < DIM; ++d) {
        const int c = cq[(size_t)j * DIM + d];
        check(c >= 0 && c < g.nc[d], "%s: query cell %d of %d", name, c, g.nc[d]);
        const float v = q[(size_t)j * DIM + d];
        if (v < lo[d] || v > hi[d]) clamped[j] = 1;
        if (v < lo[d] - 100.f * g.cell || v > hi[d] + 100.f * g.cell) ++n_far;
      }
      n_clamped += clamped[j];
    }
    return clamped;
  };

  for (float r : {ext_max / 10.f, ext_max / 100.f, ext_max * 2e-4f, ext_max * 3.f, 0.f, kInf}) {
    const Grid g = make_grid(DIM, lo, hi, radius_want(r), cell_budget(n), 1);
    const std::vector<char> clamped = cells(g);
    const float r2 = r * r;
    long missed = 0;
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < n; ++i) {
        if (!(dist2<DIM>(&q[(size_t)j * DIM], &p[(size_t)i * DIM]) <= r2)) continue;
        ++n_accepted;
        n_accepted_clamped += clamped[j];
        for (int d = 0; d < DIM; ++d)
          if (std::abs(cq[(size_t)j * DIM + d] - cp[(size_t)i * DIM + d]) > 1) {
            ++missed;
            break;
          }
      }
    check(missed == 0, "covering: %s, r = %g: %ld accepted (query, point) pairs lie in non-adjacent cells (grid %d x %d x %d)", name,
          (double)r, missed, g.nc[0], g.nc[1], g.nc[2]);
  }
  for (int k : {1, 3, 8}) {
    const Grid g = make_grid(DIM, lo, hi, knn_want(DIM, lo, hi, n, 1, k), cell_budget(n), 1);
    const std::vector<char> clamped = cells(g);
    long cut = 0;
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < n; ++i) {
        int D = 0;
        for (int d = 0; d < DIM; ++d) D = std::max(D, std::abs(cq[(size_t)j * DIM + d] - cp[(size_t)i * DIM + d]));
        if (D < 2) continue;
        ++n_ring_pairs;
        n_ring_clamped += clamped[j];
        const float d2 = dist2<DIM>(&q[(size_t)j * DIM], &p[(size_t)i * DIM]);
        if (!(d2 >= ring_reach2(g, D - 1)) || !(d2 >= ring_reach2(g, 1))) ++cut;
      }
    check(cut == 0, "ring: %s, k = %d: %ld (query, point) pairs sort below the reach of a ring that has not visited them", name, k, cut);
  }
}

}  // namespace

int main() {
  uint64_t seed = 1;
  for (float scale : {1.f, 1e-3f, 1e4f, 1e-20f, 1e18f})
    for (float offset : {0.f, -7.7f})
      for (int corner = 0; corner < 2; ++corner) {
        const float off = offset * scale;
        char name[64];
        std::snprintf(name, sizeof(name), "scale %g offset %g%s", (double)scale, (double)off, corner ? " corner" : "");
        run<1>(name, 300, seed++, scale, off, corner);
        run<2>(name, 300, seed++, scale, off, corner);
        run<3>(name, 300, seed++, scale, off, corner);
      }
  run<2>("offset 1e6", 300, seed++, 8.f, 1e6f, false);
  check(n_clamped > 10000 && n_far > 1000, "vacuous: %ld clamped queries, %ld far coordinates", n_clamped, n_far);
  check(n_accepted_clamped > 10000 && n_ring_clamped > 100000, "vacuous: %ld accepted pairs and %ld ring pairs of clamped queries",
        n_accepted_clamped, n_ring_clamped);
  std::printf("queries: %ld clamped, %ld far coordinates; %ld accepted pairs (%ld clamped), %ld ring pairs (%ld clamped)\n", n_clamped, n_far,
              n_accepted, n_accepted_clamped, n_ring_pairs, n_ring_clamped);
  std::printf("%ld checks, %ld failed\n", checks, failures);
  return failures ? 1 : 0;
}
