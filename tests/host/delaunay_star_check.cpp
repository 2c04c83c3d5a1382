// delaunay_star_check.cpp -- csrc/delaunay_star.h, the geometry of the Delaunay builder, as a stand-alone host program: the star
// of every point of small clouds, built by the header's clip steps, against the rule restated by brute force.  The clouds have
// integer coordinates, so the brute force is exact (64-bit integers, fractions compared by cross-multiplication) and knows the
// ties: cocircular points, lattices, collinear points, unbounded cells.  Built with ASan + UBSan and -ffp-contract=off by
// tests/test_mesh_host.py.  Prints "<n> checks, <f> failed".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "delaunay_star.h"

using namespace ngpde::star;

static long long checks = 0, failed = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    ++checks;                            \
    if (!(cond)) {                       \
      if (++failed <= 20) {              \
        std::printf("FAILED: " __VA_ARGS__); \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

struct Pt {
  long long x, y;
};

// the rule: the part of the bisector of (i, j) that is no nearer to any other point is not empty.  The bisector is
// q / 2 + t * perp(q); point k allows t * c <= b with c = perp(q) . q_k and b = (|q_k|^2 - q . q_k) / 2.
static bool rule(const std::vector<Pt> &p, int i, int j) {
  const long long qx = p[j].x - p[i].x, qy = p[j].y - p[i].y;
  bool has_lo = false, has_hi = false;
  long long lo_n = 0, lo_d = 1, hi_n = 0, hi_d = 1;   // fractions with positive denominators
  for (int k = 0; k < (int)p.size(); ++k) {
    if (k == i || k == j) continue;
    const long long kx = p[k].x - p[i].x, ky = p[k].y - p[i].y;
    const long long c = -qy * kx + qx * ky, b2 = kx * kx + ky * ky - (qx * kx + qy * ky);
    if (c == 0) {
      if (b2 < 0) return false;
    } else if (c > 0) {   // t <= b2 / (2c)
      if (!has_hi || (__int128)b2 * hi_d < (__int128)hi_n * c) hi_n = b2, hi_d = c;
      has_hi = true;
    } else {              // t >= b2 / (2c) = (-b2) / (-2c)
      if (!has_lo || (__int128)(-b2) * lo_d > (__int128)lo_n * (-c)) lo_n = -b2, lo_d = -c;
      has_lo = true;
    }
  }
  if (!has_lo || !has_hi) return true;
  return (__int128)lo_n * hi_d <= (__int128)hi_n * lo_d;
}

struct Cell {
  std::vector<Vertex> v;
  Vertex get(int k) const { return v.at(k); }
  void set(int k, const Vertex &x) { v.at(k) = x; }
};

struct Stats {
  int max_cell = 0, max_degree = 0;
  long long unbounded = 0, stops = 0;
};

// the star of point i with the candidates in `order`; -1 when the cell overflows `cap`
static int star_of(const std::vector<Pt> &p, int i, const std::vector<int> &order, int cap, std::vector<char> *nbr, Stats *st,
                   bool check_stop) {
  Cell P;
  P.v.resize(cap);
  int m = 4;
  for (int k = 0; k < 4; ++k) P.set(k, plane_corner(k));
  auto line_of = [&](int tag) { return line_to((float)p[i].x, (float)p[i].y, (float)p[tag].x, (float)p[tag].y, tag); };
  for (size_t pos = 0; pos < order.size(); ++pos) {
    const int j = order[pos];
    if (j == i) continue;
    if (check_stop) {   // candidates come nearest first: once the cell is certified against this distance, nothing further touches it
      double r2 = 0;
      for (int k = 0; k < m; ++k) r2 = std::max(r2, rho2(P.get(k)));
      const double dx = (double)(p[j].x - p[i].x), dy = (double)(p[j].y - p[i].y);
      if (certified(r2, (float)(dx * dx + dy * dy))) {
        ++st->stops;
        for (size_t rest = pos; rest < order.size(); ++rest)
          if (order[rest] != i) CHECK(!rule(p, i, order[rest]), "stop at %d cut off neighbour %d of %d", j, order[rest], i);
        break;
      }
    }
    const Line l = line_of(j);
    CHECK(!coincident(l), "coincident %d %d", i, j);
    const ClipResult r = clip(P, &m, cap, l, line_of);
    if (r == kOverflow) return -1;
    st->max_cell = std::max(st->max_cell, m);
    for (int k = 0; k < m; ++k) CHECK(P.get(k).w >= 0.0, "w < 0 in the cell of %d", i);
  }
  bool open = false;
  for (int k = 0; k < m; ++k) open |= P.get(k).w == 0.0;
  st->unbounded += open;
  nbr->assign(p.size(), 0);
  int deg = 0;
  for (int j = 0; j < (int)p.size(); ++j) {
    if (j == i) continue;
    const Line l = line_of(j);
    bool hit = false;
    for (int k = 0; k < m && !hit; ++k) hit = touches(P.get(k), P.get(k + 1 == m ? 0 : k + 1), l);
    (*nbr)[j] = hit;
    deg += hit;
  }
  st->max_degree = std::max(st->max_degree, deg);
  return deg;
}

static void run_cloud(const char *name, const std::vector<Pt> &p, long long want_edges, unsigned seed) {
  const int n = (int)p.size();
  Stats st;
  std::vector<char> nbr;
  long long directed = 0;
  for (int pass = 0; pass < 3; ++pass)   // index order, a shuffled order, nearest first with the stop
    for (int i = 0; i < n; ++i) {
      std::vector<int> order(n);
      for (int k = 0; k < n; ++k) order[k] = (i + 1 + k) % n;
      if (pass == 1) {
        for (int k = n - 1; k > 0; --k) {
          seed = seed * 1664525u + 1013904223u;
          std::swap(order[k], order[(seed >> 8) % (unsigned)(k + 1)]);
        }
      } else if (pass == 2) {
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
          const long long ax = p[a].x - p[i].x, ay = p[a].y - p[i].y, bx = p[b].x - p[i].x, by = p[b].y - p[i].y;
          return ax * ax + ay * ay < bx * bx + by * by;
        });
      }
      const int deg = star_of(p, i, order, 2048, &nbr, &st, pass == 2);
      CHECK(deg >= 0, "%s: overflow at cap 2048", name);
      for (int j = 0; j < n; ++j) {
        if (j == i) continue;
        const bool want = rule(p, i, j);
        CHECK((bool)nbr[j] == want, "%s pass %d: star of %d %s %d", name, pass, i, want ? "misses" : "holds", j);
        if (pass == 0) directed += want;
      }
    }
  if (want_edges >= 0) CHECK(directed == 2 * want_edges, "%s: %lld edges, expected %lld", name, directed / 2, want_edges);
  std::printf("%s: %d points, %lld edges, largest cell %d, largest degree %d, %lld unbounded cells, %lld stops\n", name, n, directed / 2,
              st.max_cell, st.max_degree, st.unbounded, st.stops);
}

int main() {
  unsigned seed = 12345u;
  auto rnd = [&](int mod) {
    seed = seed * 1664525u + 1013904223u;
    return (long long)((seed >> 8) % (unsigned)mod);
  };
  {   // random, distinct points
    std::vector<Pt> p;
    while (p.size() < 120) {
      const Pt c{rnd(4096), rnd(4096)};
      bool dup = false;
      for (const Pt &o : p) dup |= o.x == c.x && o.y == c.y;
      if (!dup) p.push_back(c);
    }
    run_cloud("random", p, -1, 1u);
  }
  {   // 5 x 4 lattice: the 8-neighbour stencil, 55 edges
    std::vector<Pt> p;
    for (int x = 0; x < 5; ++x)
      for (int y = 0; y < 4; ++y) p.push_back({x, y});
    run_cloud("lattice", p, 55, 2u);
  }
  {   // collinear: the path
    std::vector<Pt> p;
    for (int k = 0; k < 9; ++k) p.push_back({3 * k * k - 40, 2 * (3 * k * k - 40) + 7});
    run_cloud("collinear", p, 8, 3u);
  }
  const long long circ[5][2] = {{65, 0}, {16, 63}, {25, 60}, {33, 56}, {39, 52}};
  std::vector<Pt> circle;
  for (const auto &c : circ)
    for (int sx = -1; sx <= 1; sx += 2)
      for (int sy = -1; sy <= 1; sy += 2)
        for (int sw = 0; sw < 2; ++sw) {
          const Pt q{sx * (sw ? c[1] : c[0]), sy * (sw ? c[0] : c[1])};
          bool dup = false;
          for (const Pt &o : circle) dup |= o.x == q.x && o.y == q.y;
          if (!dup) circle.push_back(q);
        }
  {   // every pair of cocircular points is tied: the complete graph
    const long long n = (long long)circle.size();
    run_cloud("circle", circle, n * (n - 1) / 2, 4u);
  }
  {
    run_cloud("three", {{0, 0}, {7, 1}, {2, 9}}, 3, 5u);
    run_cloud("two", {{0, 0}, {7, 1}}, 1, 5u);
  }
  {   // a hub: the circle and its centre; the circle's points keep only their two neighbours and the centre
    std::vector<Pt> p = circle;
    p.push_back({0, 0});
    const long long n = (long long)circle.size();
    run_cloud("hub", p, 2 * n, 6u);
    // a budget below the hub's degree is reported, not overrun
    Stats st;
    std::vector<char> nbr;
    std::vector<int> order(p.size());
    for (size_t k = 0; k < p.size(); ++k) order[k] = (int)k;
    CHECK(star_of(p, (int)p.size() - 1, order, 24, &nbr, &st, false) == -1, "hub: no overflow at cap 24");
    CHECK(star_of(p, 0, order, 24, &nbr, &st, false) == 3, "hub: a rim point's degree");
  }
  std::printf("%lld checks, %lld failed\n", checks, failed);
  return failed ? 1 : 0;
}
