// coarsen_rule_check.cpp -- csrc/coarsen_rule.h against a plain brute force, as a stand-alone host program (built by
// tests/test_coarsen_host.py with -fsanitize=address,undefined -ffp-contract=off): the selection comparator and the reductions built
// on it, farthest-point sampling run through the header's pieces the way each kernel runs them (per-thread strided sets, 64-lane
// butterflies, 16 wave slots / per-slice partials) against the rule written out as two loops, the plan's work layout, and the
// cell / key rule.  Prints "<n> checks, <m> failed" and one line per input family.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "coarsen_rule.h"

using namespace ngpde::coarsen;

static long checks = 0, failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) {                                                    \
      if (++failed <= 20) std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
    }                                                                 \
  } while (0)

static bool same_bits(float a, float b) {
  uint32_t x, y;
  std::memcpy(&x, &a, 4);
  std::memcpy(&y, &b, 4);
  return x == y;
}

// ---- the rule, as the header's words say it ------------------------------------------------------------------------------------
static void fps_words(const std::vector<float> &p, int dim, int n, int k, int start, std::vector<int> *idx, std::vector<float> *d2, long *tied_rounds) {
  std::vector<float> key(n, INFINITY);
  idx->assign(k, 0);
  d2->assign(k, 0.f);
  for (int r = 0; r < k; ++r) {
    int s = start;
    if (r > 0) {
      s = -1;
      int ties = 0;
      for (int i = 0; i < n; ++i)
        if (key[i] != -1.f && (s < 0 || key[i] > key[s])) s = i;   // the first of the largest
      for (int i = 0; i < n; ++i) ties += key[i] != -1.f && key[i] == key[s];
      if (ties > 1) ++*tied_rounds;
    }
    (*idx)[r] = s;
    (*d2)[r] = key[s];
    key[s] = -1.f;
    for (int i = 0; i < n; ++i) {
      if (key[i] == -1.f) continue;
      volatile float acc = 0.f;   // every operation rounded to float, in coordinate order
      for (int c = 0; c < dim; ++c) {
        volatile float dx = p[(size_t)i * dim + c] - p[(size_t)s * dim + c];
        volatile float sq = dx * dx;
        acc = c == 0 ? (float)sq : acc + sq;
      }
      key[i] = std::min(key[i], (float)acc);
    }
  }
}

// ---- the tile kernel's data flow on the host: threads with strided points, wave butterflies, 16 slots ---------------------------
static Cand butterfly(std::vector<Cand> lanes) {   // 64 lanes, xor offsets 1 .. 32: every lane ends with the same candidate
  for (int o = 1; o < 64; o <<= 1) {
    std::vector<Cand> next(64);
    for (int l = 0; l < 64; ++l) next[l] = pick(lanes[l], lanes[l ^ o]);
    lanes = next;
  }
  for (int l = 1; l < 64; ++l) CHECK(lanes[l].idx == lanes[0].idx && same_bits(lanes[l].key, lanes[0].key));
  return lanes[0];
}

static void fps_tile_flow(const std::vector<float> &p, int dim, int n, int k, int start, int W, std::vector<int> *idx, std::vector<float> *d2) {
  const int ppt = (n + W - 1) / W;
  std::vector<float> key((size_t)W * ppt);
  for (int t = 0; t < W; ++t)
    for (int j = 0; j < ppt; ++j) key[(size_t)t * ppt + j] = t + j * W < n ? INFINITY : kKeyNone;
  idx->assign(k, 0);
  d2->assign(k, 0.f);
  int s = std::min(std::max(start, 0), n - 1);
  float skey = INFINITY;
  for (int r = 0;; ++r) {
    (*idx)[r] = s;
    (*d2)[r] = skey;
    if (r == k - 1) break;
    std::vector<Cand> mine(W, Cand{kKeyNone, kIdxNone});
    for (int t = 0; t < W; ++t)
      for (int j = 0; j < ppt; ++j) {
        const int i = t + j * W;
        float kj = key[(size_t)t * ppt + j];
        if (kj >= 0.f) {
          kj = i == s ? kKeySelected : updated_key(kj, dist2(dim, &p[(size_t)i * dim], &p[(size_t)s * dim]));
          key[(size_t)t * ppt + j] = kj;
        }
        if (kj >= 0.f && better(kj, i, mine[t].key, mine[t].idx)) mine[t] = Cand{kj, i};
      }
    Cand best = {kKeyNone, kIdxNone};
    for (int w = 0; w < W / 64; ++w) {
      const Cand wb = butterfly(std::vector<Cand>(mine.begin() + w * 64, mine.begin() + (w + 1) * 64));
      if (better(wb.key, wb.idx, best.key, best.idx)) best = wb;
    }
    s = std::min(std::max(best.idx, 0), n - 1);
    skey = best.key;
  }
}

// ---- the round kernel's data flow: slices of kFpsSlice points, one partial each, reduced again by every slice ------------------
static void fps_round_flow(const std::vector<float> &p, int dim, const FpsGraph &G, int start, std::vector<int> *idx, std::vector<float> *d2) {
  const int n = G.n, k = G.k;
  std::vector<float> key(n, 0.f);
  std::vector<Cand> part[2] = {std::vector<Cand>(G.n_parts), std::vector<Cand>(G.n_parts)};
  idx->assign(k, 0);
  d2->assign(k, 0.f);
  for (int r = 0; r < k; ++r) {
    Cand sel = {INFINITY, std::min(std::max(start, 0), n - 1)};
    if (r > 0) {
      sel = Cand{kKeyNone, kIdxNone};
      for (int q = G.n_parts - 1; q >= 0; --q) sel = pick(sel, part[(r - 1) & 1][q]);   // (any order: the comparison is a total order)
    }
    const int s = std::min(std::max(sel.idx, 0), n - 1);
    (*idx)[r] = s;
    (*d2)[r] = sel.key;
    if (r == k - 1) break;
    for (int slice = 0; slice < G.n_parts; ++slice) {
      Cand mine = {kKeyNone, kIdxNone};
      for (int i = slice * kFpsSlice; i < std::min(n, (slice + 1) * kFpsSlice); ++i) {
        float kj = r == 0 ? INFINITY : key[i];
        if (kj >= 0.f) {
          kj = i == s ? kKeySelected : updated_key(kj, dist2(dim, &p[(size_t)i * dim], &p[(size_t)s * dim]));
          key[i] = kj;
          if (kj >= 0.f && better(kj, i, mine.key, mine.idx)) mine = Cand{kj, i};
        }
      }
      part[r & 1][slice] = mine;
    }
  }
}

static void run_family(const char *name, const std::vector<float> &p, int dim, int n, int k, int start) {
  std::vector<int> want_i, got_i;
  std::vector<float> want_d, got_d;
  long tied = 0;
  fps_words(p, dim, n, k, start, &want_i, &want_d, &tied);
  long bad = failed;
  for (int W : {64, 128, 1024}) {
    if ((n + W - 1) / W > 64) continue;
    fps_tile_flow(p, dim, n, k, start, W, &got_i, &got_d);
    for (int r = 0; r < k; ++r) CHECK(got_i[r] == want_i[r] && same_bits(got_d[r], want_d[r]));
  }
  FpsGraph G = {0, n, k, 0, 0, 0, (n + kFpsSlice - 1) / kFpsSlice, 0};
  fps_round_flow(p, dim, G, start, &got_i, &got_d);
  for (int r = 0; r < k; ++r) CHECK(got_i[r] == want_i[r] && same_bits(got_d[r], want_d[r]));
  std::vector<int> seen(n, 0);
  for (int r = 0; r < k; ++r) CHECK(++seen[want_i[r]] == 1);   // a selected point is never selected twice
  std::printf("%s: %d points, dim %d, %d samples, %ld tied rounds, %ld mismatches\n", name, n, dim, k, tied, failed - bad);
}

static void check_comparator(std::mt19937 &rng) {
  const float keys[] = {-2.f, -1.f, 0.f, 1e-45f, 1e-38f, 1.f, 2.f, 3e38f, INFINITY};
  std::vector<Cand> all;
  int next = 0;
  for (float k : keys)
    for (int rep = 0; rep < 3; ++rep) all.push_back(Cand{k, next++});
  for (const Cand &a : all)
    for (const Cand &b : all) {
      const bool ab = better(a.key, a.idx, b.key, b.idx), ba = better(b.key, b.idx, a.key, a.idx);
      CHECK(a.idx == b.idx ? (!ab && !ba) : (ab != ba));   // total and antisymmetric on distinct indices
      CHECK(ab == (a.key > b.key || (a.key == b.key && a.idx < b.idx)));
      const Cand w = pick(a, b);
      CHECK(w.idx == (ba ? b.idx : a.idx));
      for (const Cand &c : all) {
        if (ab && better(b.key, b.idx, c.key, c.idx)) CHECK(better(a.key, a.idx, c.key, c.idx));   // transitive
      }
    }
  for (int trial = 0; trial < 200; ++trial) {   // the maximum does not depend on the order of the reduction
    std::vector<Cand> v(all);
    std::shuffle(v.begin(), v.end(), rng);
    Cand m = {kKeyNone, kIdxNone};
    for (const Cand &c : v) m = pick(m, c);
    CHECK(m.key == INFINITY && m.idx == 24);
  }
  CHECK(updated_key(4.f, 2.f) == 2.f && updated_key(2.f, 4.f) == 2.f && updated_key(INFINITY, INFINITY) == INFINITY);
  CHECK(updated_key(3.f, std::numeric_limits<float>::quiet_NaN()) == 3.f);
}

static void check_layout(std::mt19937 &rng) {
  const int64_t sizes[] = {0, 1, 2, 63, 1023, 1024, 1025, 4096, 4097, kFpsTileMaxPoints, kFpsTileMaxPoints + 1, 3 * kFpsSlice, 3 * kFpsSlice + 1, 50000};
  long tile_graphs = 0, round_graphs = 0;
  for (int trial = 0; trial < 300; ++trial) {
    const int G = 1 + (int)(rng() % 7), path = (int)(rng() % 3);
    std::vector<int64_t> gp(G + 1, 0), sp(G + 1, 0);
    for (int g = 0; g < G; ++g) {
      int64_t n = sizes[rng() % (sizeof(sizes) / sizeof(sizes[0]))];
      if (path == 1) n = std::min<int64_t>(n, kFpsTileMaxPoints);
      const int64_t k = n == 0 ? 0 : (rng() % 4 == 0 ? 0 : 1 + (int64_t)(rng() % n));
      gp[g + 1] = gp[g] + n;
      sp[g + 1] = sp[g] + k;
    }
    FpsLayout L;
    int32_t where = -1;
    CHECK(fps_layout(G, gp.data(), sp.data(), path, &L, &where) == kFpsOk);
    CHECK(L.n_points == gp[G] && L.n_samples == sp[G]);
    // brute force: which graph goes where, in graph order
    size_t at[3] = {0, 0, 0}, at_round = 0;
    int64_t parts = 0, keys = 0;
    int32_t launches = 0;
    for (int g = 0; g < G; ++g) {
      const int64_t n = gp[g + 1] - gp[g], k = sp[g + 1] - sp[g];
      if (k == 0) continue;
      const bool tile = path == 1 || (path == 0 && n <= kFpsTileMaxPoints);
      if (tile) {
        const int c = n <= 1024 ? 0 : n <= 4096 ? 1 : 2;
        CHECK(tile_class(n) == c && tile_per_thread(n) * (int64_t)kFpsTileThreads >= n && tile_per_thread(n) == (c == 0 ? 1 : c == 1 ? 4 : 16));
        CHECK(at[c] < L.tile[c].size());
        if (at[c] < L.tile[c].size()) {
          const FpsGraph &f = L.tile[c][at[c]++];
          CHECK(f.lo == gp[g] && f.n == n && f.k == k && f.out == sp[g] && f.g == g && f.n_parts == 0);
        }
        ++tile_graphs;
      } else {
        CHECK(at_round < L.round.size());
        if (at_round < L.round.size()) {
          const FpsGraph &f = L.round[at_round];
          const int64_t np = (n + kFpsSlice - 1) / kFpsSlice;
          CHECK(f.lo == gp[g] && f.n == n && f.k == k && f.out == sp[g] && f.g == g);
          CHECK(f.first_part == parts && f.n_parts == np && f.key_off == keys);
          for (int64_t q = 0; q < np; ++q) CHECK((size_t)(parts + q) < L.wg_graph.size() && L.wg_graph[parts + q] == (int32_t)at_round);
          CHECK((int64_t)(np - 1) * kFpsSlice < n && np * kFpsSlice >= n);   // every slice holds a point, the slices cover the graph
          parts += np;
          keys += n;
          launches = std::max<int32_t>(launches, (int32_t)k);
        }
        ++at_round;
        ++round_graphs;
      }
    }
    CHECK(at[0] == L.tile[0].size() && at[1] == L.tile[1].size() && at[2] == L.tile[2].size() && at_round == L.round.size());
    CHECK((int64_t)L.wg_graph.size() == parts && L.round_points == keys && L.round_launches == launches);
  }
  // the refusals, each naming its graph
  FpsLayout L;
  int32_t where = -1;
  {
    const int64_t gp[] = {0, 5, 3}, sp[] = {0, 1, 2};
    CHECK(fps_layout(2, gp, sp, 0, &L, &where) == kFpsDecreasing && where == 1);
  }
  {
    const int64_t gp[] = {0, 5, 9}, sp[] = {0, 2, 1};
    CHECK(fps_layout(2, gp, sp, 0, &L, &where) == kFpsSamplesDecreasing && where == 1);
  }
  {
    const int64_t gp[] = {0, 5, 9}, sp[] = {0, 2, 7};
    CHECK(fps_layout(2, gp, sp, 0, &L, &where) == kFpsTooMany && where == 1);
  }
  {
    const int64_t gp[] = {1, 5}, sp[] = {0, 2};
    CHECK(fps_layout(1, gp, sp, 0, &L, &where) == kFpsBadStart);
  }
  {
    const int64_t gp[] = {0, 4, 4 + kFpsTileMaxPoints + 1}, sp[] = {0, 2, 4};
    CHECK(fps_layout(2, gp, sp, 1, &L, &where) == kFpsOverCap && where == 1);
    CHECK(fps_layout(2, gp, sp, 0, &L, &where) == kFpsOk && L.n_tile_graphs() == 1 && L.round.size() == 1);
    CHECK(fps_layout(2, gp, sp, 2, &L, &where) == kFpsOk && L.n_tile_graphs() == 0 && L.round.size() == 2);
  }
  {
    const int64_t gp[] = {0, 0x80000000LL}, sp[] = {0, 1};
    CHECK(fps_layout(1, gp, sp, 2, &L, &where) == kFpsTooLarge && where == 0);
  }
  std::printf("layout: %ld graphs on the tile path, %ld on the round path\n", tile_graphs, round_graphs);
}

static void check_cells(std::mt19937 &rng) {
  // the quotient is one float subtraction and one float division; which quotients are cells
  CHECK(cell_quotient(4.f, 0.f, 2.f) == 2.f && cell_quotient(3.9999998f, 0.f, 2.f) == 1.f);   // a point on a cell edge belongs to the upper cell
  CHECK(cell_quotient(-0.5f, 0.f, 2.f) == -1.f && !cell_fits(-1.f));
  CHECK(cell_fits(0.f) && cell_fits(2147483520.f) && !cell_fits(2147483648.f) && !cell_fits(INFINITY) && !cell_fits(NAN));
  CHECK(bits_holding(0) == 0 && bits_holding(1) == 1 && bits_holding(2) == 2 && bits_holding(255) == 8 && bits_holding(256) == 9);
  CHECK(bits_holding(0x7fffffffu) == 31);
  std::uniform_real_distribution<float> U(-50.f, 50.f);
  for (int trial = 0; trial < 2000; ++trial) {
    const float p = U(rng), o = U(rng) - 50.f, h = 0.01f + std::fabs(U(rng));
    volatile float diff = p - o;
    volatile float quo = diff / h;
    CHECK(same_bits(cell_quotient(p, o, h), std::floor((float)quo)));
  }
  // the key orders (graph, c_z, c_y, c_x), x fastest, and is injective inside its fields
  long keys_checked = 0;
  for (int dim = 1; dim <= 3; ++dim)
    for (int trial = 0; trial < 40; ++trial) {
      const int G = 1 + (int)(rng() % 5);
      int64_t top[3] = {0, 0, 0};
      for (int d = 0; d < dim; ++d) top[d] = (int64_t)(rng() % (trial % 2 ? 6 : 70000));
      const KeyBits kb = key_bits(dim, top, G);
      for (int d = 0; d < 3; ++d) CHECK(kb.c[d] == (d < dim ? bits_holding((uint64_t)top[d]) : 0u));
      CHECK(kb.g == bits_holding((uint64_t)(G - 1)) && kb.total() <= 63);
      std::vector<std::tuple<int, int, int, int>> tup;
      std::vector<uint64_t> key;
      for (int q = 0; q < 60; ++q) {
        int32_t c[3] = {0, 0, 0};
        for (int d = 0; d < dim; ++d) c[d] = (int32_t)(rng() % (uint64_t)(top[d] + 1));
        const int g = (int)(rng() % G);
        tup.emplace_back(g, c[2], c[1], c[0]);
        key.push_back(cell_key(dim, c, g, kb.c[0], kb.c[1], kb.c[2]));
        CHECK((key.back() >> (kb.c[0] + kb.c[1] + kb.c[2])) == (uint64_t)g && (key.back() >> kb.total()) == 0);
      }
      for (size_t a = 0; a < key.size(); ++a)
        for (size_t b = 0; b < key.size(); ++b) {
          CHECK((key[a] < key[b]) == (tup[a] < tup[b]) && (key[a] == key[b]) == (tup[a] == tup[b]));
          ++keys_checked;
        }
    }
  {
    const int64_t top[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};
    CHECK(key_bits(3, top, 1).total() == 93 && key_bits(2, top, 4).total() == 64 && key_bits(2, top, 2).total() == 63);
  }
  std::printf("cells: %ld key pairs ordered\n", keys_checked);
}

int main() {
  std::mt19937 rng(20240607);
  check_comparator(rng);
  check_layout(rng);
  check_cells(rng);
  std::uniform_real_distribution<float> U(0.f, 1.f);
  for (int dim = 1; dim <= 3; ++dim)
    for (int n : {1, 2, 63, 64, 65, 127, 129, 700}) {
      std::vector<float> p((size_t)n * dim);
      for (float &v : p) v = U(rng);
      for (int k : {1, 2, n}) run_family("random", p, dim, n, std::min(k, n), (int)(rng() % n));
    }
  {   // more than one slice on the round path, more than one point per thread on the tile flow
    const int n = 2 * kFpsSlice + 77;
    std::vector<float> p((size_t)n * 2);
    for (float &v : p) v = U(rng);
    run_family("slices", p, 2, n, 40, 5);
  }
  {   // a shuffled 9 x 9 lattice from a corner: ties from round 2 on
    std::vector<int> perm(81);
    for (int i = 0; i < 81; ++i) perm[i] = i;
    std::shuffle(perm.begin() + 1, perm.end(), rng);
    std::vector<float> p(162);
    for (int i = 0; i < 81; ++i) {
      p[2 * i] = (float)(perm[i] % 9);
      p[2 * i + 1] = (float)(perm[i] / 9);
    }
    run_family("lattice", p, 2, 81, 81, 0);
  }
  {   // ten coincident copies among distinct points
    std::vector<float> p;
    for (int i = 0; i < 30; ++i) {
      const bool copy = i % 3 == 0;
      p.push_back(copy ? 0.25f : U(rng));
      p.push_back(copy ? 0.75f : U(rng));
      p.push_back(copy ? 0.5f : U(rng));
    }
    run_family("coincident", p, 3, 30, 30, 1);
  }
  for (float scale : {1e-24f, 1e-20f, 1e20f}) {   // squares that round to 0, to denormals, to inf
    std::vector<float> p(200);
    for (float &v : p) v = U(rng) * scale;
    run_family(scale < 1e-22f ? "underflow" : scale < 1.f ? "denormal" : "overflow", p, 2, 100, 100, 3);
  }
  std::printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
