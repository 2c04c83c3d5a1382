// neighbor_grid_check.cpp -- stand-alone check of csrc/neighbor_grid.h on the host (built with ASan + UBSan and -ffp-contract=off by
// tests/test_neighbor_grid_host.py).  Four properties, each on the header's own functions with the library's operation order:
//   sanity     make_grid returns within a bounded number of coarsening steps with a finite positive cell and inverse, 1..8192 cells
//              per dimension and cells * n_graphs <= budget (or one cell), over every combination of extents and `want` from 0 and
//              the smallest denormal to FLT_MAX and inf; a span above FLT_MAX is reported by span_is_finite;
//   covering   on seeded clouds (ordinary, lattice at the threshold, offset, anisotropic, flat, one outlier, magnitudes where squares
//              leave the float range), for radii that give an ordinary, a capped and a coarsened grid: every pair with float
//              d2 <= r*r lies in cells that differ by at most 1 per dimension;
//   ring       on the same clouds with the k-NN grid: a point in a cell at Chebyshev distance D >= 2 from the home cell has a float
//              d2 >= ring_reach2(ring) for every ring < D (checked at ring = D - 1 and 1: the bound grows with the ring);
//   rounding   the float cell coordinate differs from the same expression in long double by less than 1e-3 cells, at lo, hi, every
//              lo + j * cell and their two float neighbours, for 1, 2, 8191 and 8192 cells.
// Prints "<checks> checks, <failed> failed" and one line per regime reached; the exit status is 1 if a check failed.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
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
  ++failures;
  static int printed[256];
  if (++printed[(unsigned char)fmt[0]] > 12) return;   // per kind of message; the count goes on, the text does not
  va_list ap;
  va_start(ap, fmt);
  std::fprintf(stderr, "FAILED ");
  std::vfprintf(stderr, fmt, ap);
  std::fprintf(stderr, "\n");
  va_end(ap);
}

const float kInf = std::numeric_limits<float>::infinity();
const float kDenorm = std::numeric_limits<float>::denorm_min();
constexpr int kStepCap = 400;

// ---- sanity ----------------------------------------------------------------------------------------------------------------------
void check_grid(const char *what, int dim, const float *lo, const float *hi, float want, int64_t budget, int n_graphs, const Grid &g,
                int steps) {
  check(steps >= 0 && steps < kStepCap, "%s: %d coarsening steps (dim %d, ext %g %g %g, want %g)", what, steps, dim, hi[0] - lo[0],
        hi[1] - lo[1], hi[2] - lo[2], want);
  check(std::isfinite(g.cell) && g.cell > 0.f, "%s: cell %g (dim %d, ext %g %g %g, want %g)", what, g.cell, dim, hi[0] - lo[0],
        hi[1] - lo[1], hi[2] - lo[2], want);
  check(std::isfinite(g.inv) && g.inv > 0.f, "%s: inv %g (cell %g, dim %d, want %g)", what, g.inv, g.cell, dim, want);
  int64_t cells = 1;
  for (int d = 0; d < 3; ++d) {
    check(g.nc[d] >= 1 && g.nc[d] <= kMaxCellsPerDim && (d < dim || g.nc[d] == 1), "%s: nc[%d] = %d", what, d, g.nc[d]);
    cells *= g.nc[d];
  }
  check(cells == g.cells && (cells * n_graphs <= budget || cells == 1), "%s: %lld cells x %d graphs, budget %lld", what,
        (long long)cells, n_graphs, (long long)budget);
}

void sanity() {
  const float vals[] = {0.f, kDenorm, FLT_MIN, 1e-30f, 1e-3f, 1.f, 1e4f, 1e19f, 1e30f, FLT_MAX, kInf};
  const int n_ext = 10, n_want = 11;   // inf is a `want` only
  const int64_t budgets[] = {(int64_t)1 << 16, (int64_t)1 << 30};
  const int graphs[] = {1, 1000};
  for (int dim = 1; dim <= 3; ++dim) {
    int combos = 1;
    for (int d = 0; d < dim; ++d) combos *= n_ext;
    for (int e = 0; e < combos; ++e) {
      float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
      for (int d = 0, r = e; d < dim; ++d, r /= n_ext) hi[d] = vals[r % n_ext];
      check(span_is_finite(dim, lo, hi), "sanity: a finite extent is reported as a non-finite span");
      for (int w = 0; w < n_want; ++w)
        for (int64_t budget : budgets)
          for (int ng : graphs) {
            int steps = -1;
            const Grid g = make_grid(dim, lo, hi, vals[w], budget, ng, &steps);
            check_grid("sanity", dim, lo, hi, vals[w], budget, ng, g, steps);
          }
    }
  }
  // two finite coordinates further apart than FLT_MAX: no grid; the library refuses the call on this answer
  for (int dim = 1; dim <= 3; ++dim)
    for (int at = 0; at <= dim; ++at) {   // one coordinate, and (at == dim) all of them
      float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {1.f, 1.f, 1.f};
      for (int d = 0; d < dim; ++d)
        if (d == at || at == dim) {
          lo[d] = -3e38f;
          hi[d] = 3e38f;
        }
      const bool finite = span_is_finite(dim, lo, hi);
      check(!finite, "wide span: -3e38 .. 3e38 in coordinate %d of %d is not reported", at, dim);
      if (finite) {   // a grid code that does not look at the span has to size this one too (and must not spin on it)
        int steps = -1;
        const Grid g = make_grid(dim, lo, hi, 1.01f, (int64_t)1 << 16, 1, &steps);
        check_grid("wide span", dim, lo, hi, 1.01f, (int64_t)1 << 16, 1, g, steps);
      }
    }
  // the curve quantisation: a finite scale, and hi lands on 2^bits up to rounding
  for (int dim = 1; dim <= 3; ++dim)
    for (int e = 0; e < n_ext; ++e) {
      float lo[3] = {0.f, 0.f, 0.f}, hi[3] = {0.f, 0.f, 0.f};
      for (int d = 0; d < dim; ++d) hi[d] = vals[e];
      const Quant q = make_quant(dim, lo, hi);
      for (int d = 0; d < dim; ++d) {
        const float top = (hi[d] - q.lo[d]) * q.scale[d], bottom = (lo[d] - q.lo[d]) * q.scale[d];
        check(std::isfinite(q.scale[d]) && q.scale[d] >= 0.f && bottom == 0.f && top >= 0.f && top <= (float)(1u << q.bits) * 1.000001f,
              "quant: dim %d ext %g: scale %g, lo -> %g, hi -> %g", dim, vals[e], q.scale[d], bottom, top);
      }
    }
}

// ---- clouds ----------------------------------------------------------------------------------------------------------------------
struct Cloud {
  std::string name;
  int dim;
  std::vector<float> p;        // [n][dim]
  std::vector<float> radii;    // beside the generic ones
  int n() const { return (int)(p.size() / dim); }
};

struct Rng {   // 64-bit LCG, the high 24 bits as a float in [0, 1)
  uint64_t s;
  float next() {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (float)(s >> 40) * 0x1p-24f;
  }
};

Cloud uniform(const char *name, int dim, int n, uint64_t seed, float sx, float sy, float sz, float ox = 0.f, float oy = 0.f, float oz = 0.f) {
  Cloud c{name, dim, {}, {}};
  Rng rng{seed};
  const float s[3] = {sx, sy, sz}, o[3] = {ox, oy, oz};
  for (int i = 0; i < n; ++i)
    for (int d = 0; d < dim; ++d) c.p.push_back(rng.next() * s[d] + o[d]);
  return c;
}

Cloud lattice(const char *name, int dim, int side, float h, float ox, float oy, float oz) {
  Cloud c{name, dim, {}, {h}};
  const float o[3] = {ox, oy, oz};
  int n = 1;
  for (int d = 0; d < dim; ++d) n *= side;
  for (int i = 0; i < n; ++i)
    for (int d = 0, r = i; d < dim; ++d, r /= side) c.p.push_back((float)(r % side) * h + o[d]);
  return c;
}

std::vector<Cloud> clouds() {
  std::vector<Cloud> cs;
  cs.push_back(uniform("uniform 1-D", 1, 400, 1, 1.f, 1.f, 1.f));
  cs.push_back(uniform("uniform 2-D", 2, 400, 2, 1.f, 1.f, 1.f));
  cs.push_back(uniform("uniform 3-D", 3, 400, 3, 1.f, 1.f, 1.f));
  cs.push_back(lattice("lattice 2-D, spacing r", 2, 20, 0.125f, 0.f, 0.f, 0.f));
  cs.push_back(lattice("lattice 3-D, spacing r", 3, 7, 0.125f, 0.f, 0.f, 0.f));
  cs.push_back(lattice("lattice 2-D at (0.3, -7.7)", 2, 20, 0.125f, 0.3f, -7.7f, 0.f));
  cs.push_back(lattice("lattice 2-D at 1e6", 2, 20, 0.125f, 1e6f, -1e6f, 0.f));
  cs.push_back(lattice("lattice 3-D at 1e6", 3, 7, 0.125f, 1e6f, -1e6f, 5e5f));
  cs.push_back(uniform("uniform 2-D at 1.6e7", 2, 400, 4, 64.f, 64.f, 1.f, 1.6e7f, 1.6e7f, 0.f));
  cs.back().radii = {1.f, 2.f};
  cs.push_back(uniform("anisotropic 1e4 x 1e-3", 2, 400, 5, 1e4f, 1e-3f, 1.f));
  cs.back().radii = {2.f, 1e-3f};
  cs.push_back(uniform("anisotropic 1e4 x 1e-3 x 1", 3, 400, 6, 1e4f, 1e-3f, 1.f));
  cs.back().radii = {2.f, 1.f};
  cs.push_back(uniform("collinear in 3-D", 3, 400, 7, 1.f, 0.f, 0.f, 0.f, 0.5f, -2.f));
  cs.push_back(uniform("coplanar in 3-D", 3, 400, 8, 1.f, 1.f, 0.f, 0.f, 0.f, 3.f));
  cs.push_back(uniform("coincident", 3, 100, 9, 0.f, 0.f, 0.f, 1.f, 1.f, 1.f));
  cs.push_back(uniform("one outlier at 1e6", 2, 400, 10, 1e-3f, 1e-3f, 1.f));
  cs.back().p[0] = cs.back().p[1] = 1e6f;
  cs.back().radii = {1e-4f};
  const float scales[] = {1e-40f, 1e-30f, 1e-22f, 1e19f, 1e30f};
  for (float s : scales) {
    static char names[10][40];
    static int k = 0;
    std::snprintf(names[k], sizeof(names[k]), "scale %g 2-D", (double)s);
    cs.push_back(uniform(names[k++], 2, 200, 11, s, s, s));
    std::snprintf(names[k], sizeof(names[k]), "scale %g 3-D", (double)s);
    cs.push_back(uniform(names[k++], 3, 200, 12, s, s, s));
  }
  cs.push_back(uniform("3e38 x 1", 2, 200, 13, 3e38f, 1.f, 1.f));
  cs.back().radii = {1e37f, 1e19f, 1.f};
  return cs;
}

template <int DIM>
float dist2(const float *a, const float *b) {   // neighbors.hip's, operation by operation
  float d2 = 0.f;
  for (int d = 0; d < DIM; ++d) {
    const float df = a[d] - b[d];
    d2 = d2 + df * df;
  }
  return d2;
}

void bounds(const Cloud &c, float *lo, float *hi) {
  for (int d = 0; d < 3; ++d) lo[d] = hi[d] = 0.f;
  for (int d = 0; d < c.dim; ++d) {
    lo[d] = hi[d] = c.p[d];
    for (int i = 1; i < c.n(); ++i) {
      lo[d] = std::min(lo[d], c.p[(size_t)i * c.dim + d]);
      hi[d] = std::max(hi[d], c.p[(size_t)i * c.dim + d]);
    }
  }
}

long n_ordinary = 0, n_capped = 0, n_coarsened = 0, n_one_cell = 0, n_accepted = 0, n_ring_pairs = 0;

template <int DIM>
void covering_and_ring(const Cloud &c) {
  const int n = c.n();
  float lo[3], hi[3];
  bounds(c, lo, hi);
  if (!span_is_finite(DIM, lo, hi)) return;
  float ext_max = 0.f;
  for (int d = 0; d < DIM; ++d) ext_max = std::max(ext_max, hi[d] - lo[d]);
  std::vector<float> radii = {ext_max / 10.f, ext_max * 2e-4f, ext_max * 1e-6f, 0.f, kInf};
  radii.insert(radii.end(), c.radii.begin(), c.radii.end());
  std::vector<int> cell((size_t)n * DIM);
  for (float r : radii) {
    int steps = -1;
    const Grid g = make_grid(DIM, lo, hi, radius_want(r), cell_budget(n), 1, &steps);
    check_grid(c.name.c_str(), DIM, lo, hi, radius_want(r), cell_budget(n), 1, g, steps);
    if (!(steps >= 0 && steps < kStepCap && g.inv > 0.f)) continue;
    bool capped = false;
    for (int d = 0; d < DIM; ++d) capped |= g.nc[d] == kMaxCellsPerDim;
    if (steps > 0) ++n_coarsened;
    else if (capped) ++n_capped;
    else if (g.cells == 1) ++n_one_cell;
    else ++n_ordinary;
    for (int i = 0; i < n; ++i) cell_of<DIM>(g, &c.p[(size_t)i * DIM], &cell[(size_t)i * DIM]);
    const float r2 = r * r;
    long missed = 0, accepted = 0;
    for (int i = 0; i < n; ++i)
      for (int j = i + 1; j < n; ++j) {
        if (!(dist2<DIM>(&c.p[(size_t)i * DIM], &c.p[(size_t)j * DIM]) <= r2)) continue;
        ++accepted;
        for (int d = 0; d < DIM; ++d)
          if (std::abs(cell[(size_t)i * DIM + d] - cell[(size_t)j * DIM + d]) > 1) {
            ++missed;
            break;
          }
      }
    n_accepted += accepted;
    check(missed == 0, "covering: %s, r = %g: %ld of the %ld accepted pairs lie in non-adjacent cells (grid %d x %d x %d, cell %g)",
          c.name.c_str(), r, missed, accepted, g.nc[0], g.nc[1], g.nc[2], g.cell);
  }
  for (int k : {1, 6}) {
    if (n < k + 1) continue;
    int steps = -1;
    const float want = knn_want(DIM, lo, hi, n, 1, k);
    const Grid g = make_grid(DIM, lo, hi, want, cell_budget(n), 1, &steps);
    check_grid(c.name.c_str(), DIM, lo, hi, want, cell_budget(n), 1, g, steps);
    if (!(steps >= 0 && steps < kStepCap && g.inv > 0.f)) continue;
    for (int i = 0; i < n; ++i) cell_of<DIM>(g, &c.p[(size_t)i * DIM], &cell[(size_t)i * DIM]);
    long cut = 0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        int D = 0;
        for (int d = 0; d < DIM; ++d) D = std::max(D, std::abs(cell[(size_t)i * DIM + d] - cell[(size_t)j * DIM + d]));
        if (D < 2) continue;
        ++n_ring_pairs;
        const float d2 = dist2<DIM>(&c.p[(size_t)i * DIM], &c.p[(size_t)j * DIM]);
        if (!(d2 >= ring_reach2(g, D - 1)) || !(d2 >= ring_reach2(g, 1))) ++cut;
      }
    check(cut == 0, "ring: %s, k = %d: %ld pairs sort below the reach of a ring that has not visited them (grid %d x %d x %d, cell %g)",
          c.name.c_str(), k, cut, g.nc[0], g.nc[1], g.nc[2], g.cell);
  }
}

// ---- rounding ---------------------------------------------------------------------------------------------------------------------
void rounding() {
  const float boxes[][2] = {{0.f, 1.f}, {-1000.f, 2000.5f}, {-7.7f, 3.3f}, {1e6f, 8192.f}, {3e-3f, 1e-4f}, {-2e30f, 3e30f}};
  const int ncs[] = {1, 2, 8191, 8192};
  for (const auto &box : boxes)
    for (int nc : ncs) {
      const float lo[3] = {box[0], 0.f, 0.f}, hi[3] = {box[0] + box[1], 0.f, 0.f};
      const float ext = hi[0] - lo[0];
      const Grid g = make_grid(1, lo, hi, nc == 1 ? ext * 2.f : ext / ((float)nc - 0.5f), (int64_t)1 << 30, 1);
      check(g.nc[0] == nc, "rounding: box %g + %g wanted %d cells, has %d", box[0], box[1], nc, g.nc[0]);
      long double worst = 0.0L;
      auto at = [&](float p) {
        if (!(p >= lo[0] && p <= hi[0])) return;
        const float cf = (p - g.lo[0]) * g.inv;
        const long double cl = ((long double)p - (long double)g.lo[0]) * (long double)g.inv;
        worst = std::max(worst, fabsl((long double)cf - cl));
        int c = -1;
        cell_of<1>(g, &p, &c);
        check(c >= 0 && c < g.nc[0] && std::abs((long double)c - std::floor(cl)) <= 1.0L, "rounding: cell %d of %d for coordinate %Lg", c,
              g.nc[0], cl);
      };
      for (int j = 0; j <= nc; ++j) {
        const float p = lo[0] + (float)j * g.cell;
        at(p);
        at(std::nextafter(p, -kInf));
        at(std::nextafter(p, kInf));
      }
      at(lo[0]);
      at(hi[0]);
      at(std::nextafter(hi[0], -kInf));
      check(worst < 1e-3L, "rounding: box %g + %g, %d cells: a cell coordinate is off by %Lg cells", box[0], box[1], nc, worst);
    }
}

}  // namespace

int main() {
  sanity();
  for (const Cloud &c : clouds()) {
    if (c.dim == 1) covering_and_ring<1>(c);
    else if (c.dim == 2) covering_and_ring<2>(c);
    else covering_and_ring<3>(c);
  }
  rounding();
  // the sweep reached what it is for
  check(n_ordinary > 0 && n_capped > 0 && n_coarsened > 0 && n_one_cell > 0, "regimes: %ld ordinary, %ld capped, %ld coarsened, %ld one-cell",
        n_ordinary, n_capped, n_coarsened, n_one_cell);
  check(n_accepted > 100000 && n_ring_pairs > 100000, "vacuous: %ld accepted pairs, %ld ring pairs", n_accepted, n_ring_pairs);
  std::printf("grids: %ld ordinary, %ld capped, %ld coarsened, %ld one-cell; %ld accepted pairs, %ld ring pairs\n", n_ordinary, n_capped,
              n_coarsened, n_one_cell, n_accepted, n_ring_pairs);
  std::printf("%ld checks, %ld failed\n", checks, failures);
  return failures ? 1 : 0;
}
