// persistent_plan.hip -- what the three device-resident solvers (GCN: node_persistent.hip, GAT: gat_fused.hip, VMH: node_vmh.hip) share
// on the host: the wait lists and node_wait_lists_fit, the hub geometry's tile partition and lists (ngpde_hub_partition_host),
// node_persistent_setup / _free, the abort word, and the bracket of every persistent launch (the per-device turnstile, PersistentTurn and
// its two one-thread kernels).  The solver kernels, their residency queries and their launchers are in the three files above.
#include <algorithm>
#include <cstring>
#include <mutex>

#include "common.h"
#include "persistent_gcn_tile.h"
#include "switches.h"

namespace ngpde {

bool capturing(hipStream_t stream) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) cs = hipStreamCaptureStatusNone;
  return cs != hipStreamCaptureStatusNone;
}

// Wait lists from each tile's foreign tiles (foreign[t]: the tiles that own a row tile t stages, either direction, repeats allowed):
// tile T waits for every tile that owns a row of T's halo, and for every tile whose halo holds a row of T (they read what T is about
// to overwrite) -- the symmetric closure.  out: [n_tiles][stride], ascending, -1 padded; skip63: position 63 stays free (hub geometry:
// that lane watches the abort word).  Returns false when a list overflows its stride - 1 entries.
static bool wait_lists_from(int nt, int stride, bool skip63, const std::vector<std::vector<int>> &foreign, std::vector<int> &out) {
  std::vector<std::vector<int>> nb(nt);
  for (int t = 0; t < nt; ++t)
    for (int u : foreign[t]) {
      if (u == t) continue;
      nb[t].push_back(u);
      nb[u].push_back(t);
    }
  out.assign((size_t)nt * stride, -1);
  for (int t = 0; t < nt; ++t) {
    std::sort(nb[t].begin(), nb[t].end());
    nb[t].erase(std::unique(nb[t].begin(), nb[t].end()), nb[t].end());
    if ((int)nb[t].size() > stride - 1) return false;
    for (size_t k = 0; k < nb[t].size(); ++k) out[(size_t)t * stride + (skip63 && k >= 63 ? k + 1 : k)] = nb[t][k];
  }
  return true;
}
// tile of every node under the schedule order
static std::vector<int32_t> tiles_of(const std::vector<int32_t> &order) {
  std::vector<int32_t> tile_of(order.size(), 0);
  for (size_t pos = 0; pos < order.size(); ++pos) tile_of[order[pos]] = (int32_t)(pos / kTileRows);
  return tile_of;
}

// The handle's wait lists (96-row geometry), from its halo lists: [n_tiles][kNbrStride].  Returns false when a list overflows.
static bool build_wait_lists(const ngpde_graph *g, std::vector<int> &out) {
  const int nt = g->n_sched / kTileRows;
  std::vector<int32_t> order((size_t)g->n_nodes);
  if (!g->h_order.empty()) order = g->h_order;
  else if (hipMemcpy(order.data(), g->order, order.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  const std::vector<int32_t> tile_of = tiles_of(order);
  std::vector<std::vector<int>> foreign(nt);
  for (const Csr *c : {&g->by_t, &g->by_s}) {
    std::vector<int2> halo((size_t)nt * kHaloCap), info(nt);
    if (hipMemcpy(halo.data(), c->halo, halo.size() * sizeof(int2), hipMemcpyDeviceToHost) != hipSuccess) return false;
    if (hipMemcpy(info.data(), c->tile_info, info.size() * sizeof(int2), hipMemcpyDeviceToHost) != hipSuccess) return false;
    for (int t = 0; t < nt; ++t)
      for (int k = kTileRows; k < info[t].x; ++k) foreign[t].push_back(tile_of[halo[(size_t)t * kHaloCap + k].x]);
  }
  return wait_lists_from(nt, kNbrStride, false, foreign, out);
}

bool node_wait_lists_fit(const ngpde_graph *g) {
  if (!g) return false;
  std::lock_guard<std::mutex> lock(g->lazy_mu);
  if (g->wait_lists_fit < 0) {
    std::vector<int> lists;
    g->wait_lists_fit = build_wait_lists(g, lists) ? 1 : 0;
  }
  return g->wait_lists_fit == 1;
}

// The hub geometry's own tile partition.  The handle's locality order grows clusters breadth-first, which puts a hub and the hubs
// next to it into ONE tile (Cora-shaped graphs: > 256 distinct rows).  Here the nodes are dealt out worst first, in order of
// descending degree: the n_tiles highest-degree nodes one per tile, every further node to the tile whose set of referenced rows H_t
// (members and all their neighbours, both directions) grows least by it, among the tiles with a free slot that stay within the cap
// with one row reserved per slot still free; a node with more than kSlotWidth entries (a long row: summed by the whole workgroup, two
// barriers each) prefers the tiles with the fewest long rows.  Leaves end up with the hub they hang on (growth 0), hubs apart from each
// other: at BASELINE config 1's shape one long row per tile at most, 94 referenced rows per tile on average, 131 at most (the first form
// of this deal -- least growth only -- put the hubs next to each other: the tile with most of them took 17 k cycles per phase and every
// other tile waited for it; the second -- hubs apart, least growth -- filled the largest hub's tile to the cap of 255 rows).  Returns the positions -> node order (tile t = positions 32 t ..), or an empty vector when some node fits nowhere.
static std::vector<int32_t> hub_partition(int64_t n, const std::vector<int32_t> rp[2], const std::vector<int32_t> cl[2], bool balance) {
  const int nt = (int)((n + kTileRows - 1) / kTileRows);
  std::vector<std::vector<int32_t>> nb((size_t)n);
  for (int64_t v = 0; v < n; ++v) {
    std::vector<int32_t> &a = nb[(size_t)v];
    for (int dir = 0; dir < 2; ++dir)
      for (int32_t p = rp[dir][v]; p < rp[dir][v + 1]; ++p)
        if (cl[dir][p] != v) a.push_back(cl[dir][p]);
    std::sort(a.begin(), a.end());
    a.erase(std::unique(a.begin(), a.end()), a.end());
  }
  std::vector<int32_t> by_degree((size_t)n);
  for (int64_t v = 0; v < n; ++v) by_degree[(size_t)v] = (int32_t)v;
  std::stable_sort(by_degree.begin(), by_degree.end(), [&](int32_t a, int32_t b) { return nb[a].size() > nb[b].size(); });
  std::vector<uint8_t> in_h((size_t)nt * n, 0);
  std::vector<int> h_size(nt, 0), cap(nt, kTileRows);
  std::vector<int> n_long(nt, 0);
  std::vector<std::vector<int32_t>> members(nt);
  cap[nt - 1] = (int)(n - (int64_t)kTileRows * (nt - 1));
  int64_t dealt = 0;
  for (int32_t v : by_degree) {
    const bool is_long = (int)nb[v].size() > kSlotWidth;
    int best_t = -1, best_score = 1 << 30, best_l = 1 << 30;
    if (dealt < nt) best_t = (int)dealt;   // the n_tiles highest-degree nodes: one per tile
    ++dealt;
    for (int t = 0; t < nt && dealt > nt; ++t) {
      if ((int)members[t].size() >= cap[t]) continue;
      const uint8_t *h = in_h.data() + (size_t)t * n;
      int inc = h[v] ? 0 : 1;
      for (int32_t w : nb[v]) inc += h[w] ? 0 : 1;
      if (h_size[t] + inc + (cap[t] - (int)members[t].size() - 1) > kHubHalo) continue;
      const int l = is_long ? n_long[t] : 0;
      // growth, plus a sixteenth of what the tile already references: every tile waits for the slowest one each phase, so a node that
      // would add one row to a tile of 200 goes to a tile of 60 even if it adds three there (largest tile at config 1's shape: 255 -> 131
      // rows, the average unchanged at 94)
      const int score = balance ? 16 * inc + h_size[t] : 512 * inc + h_size[t];   // (not balanced: least growth, then the smaller tile)
      if (l < best_l || (l == best_l && score < best_score)) { best_t = t; best_score = score; best_l = l; }
    }
    if (best_t < 0) return {};
    uint8_t *h = in_h.data() + (size_t)best_t * n;
    if (!h[v]) { h[v] = 1; ++h_size[best_t]; }
    for (int32_t w : nb[v])
      if (!h[w]) { h[w] = 1; ++h_size[best_t]; }
    if (h_size[best_t] + (cap[best_t] - (int)members[best_t].size() - 1) > kHubHalo) return {};   // (a seed beyond the cap: a hub of > ~224 neighbours)
    members[best_t].push_back(v);
    n_long[best_t] += is_long ? 1 : 0;
  }
  std::vector<int32_t> order;
  order.reserve((size_t)n);
  for (int t = 0; t < nt; ++t) order.insert(order.end(), members[t].begin(), members[t].end());
  return order;
}

struct HubHost {
  std::vector<int32_t> halo;
  std::vector<float> w;   // beside `slots` (weighted graphs), else empty
  std::vector<uint8_t> slots, longs;
  std::vector<int2> rows;
  std::vector<int4> info;
};
static bool host_csr(const ngpde_graph *g, const Csr &c, std::vector<int32_t> &rowptr, std::vector<int32_t> &col) {
  const int64_t n = g->n_nodes, m = g->n_edges;
  if (!c.h_rowptr.empty()) { rowptr = c.h_rowptr; col = c.h_col; return true; }
  rowptr.resize((size_t)n + 1); col.resize((size_t)std::max<int64_t>(m, 1));
  if (hipMemcpy(rowptr.data(), c.rowptr, rowptr.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  if (m > 0 && hipMemcpy(col.data(), c.col, (size_t)m * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
  return true;
}
// The hub geometry's lists of one direction, from the CSR lists and the schedule order (host copies, or downloaded from a
// device-built handle).  Slot numbering: own rows first (slot k = k-th row of the tile), every other row in order of first reference
// (rows of the tile in order, entries in CSR order).  false: some tile exceeds a cap.
// w_csr: the entries' edge weights in the list's own order, or NULL
static bool build_hub_lists(int64_t n, int nt, const std::vector<int32_t> &rowptr, const std::vector<int32_t> &col,
                            const std::vector<int32_t> &order, HubHost &o, const float *w_csr = nullptr) {
  o.halo.assign((size_t)nt * kHubHalo, 0);
  o.slots.assign((size_t)nt * kHubList, 0);
  if (w_csr) o.w.assign((size_t)nt * kHubList, 0.f);
  o.longs.assign((size_t)nt * kTileRows, 0);
  o.rows.assign((size_t)nt * kTileRows, make_int2(0, 0));
  o.info.assign((size_t)nt, make_int4(0, 0, 0, 0));
  std::vector<int32_t> slot_of((size_t)n, -1), stamp((size_t)n, -1);
  for (int t = 0; t < nt; ++t) {
    int count = kTileRows, bytes = 0, n_long = 0;
    for (int k = 0; k < kTileRows; ++k) {
      const int64_t pos = (int64_t)t * kTileRows + k;
      if (pos >= n) continue;
      const int32_t v = order[pos];
      stamp[v] = t; slot_of[v] = k;
      o.halo[(size_t)t * kHubHalo + k] = v;
    }
    for (int k = 0; k < kTileRows; ++k) {
      const int64_t pos = (int64_t)t * kTileRows + k;
      if (pos >= n) break;
      const int32_t v = order[pos];
      const int32_t rs = rowptr[v], deg = rowptr[v + 1] - rs;
      if (bytes + deg > kHubList) return false;
      o.rows[(size_t)pos] = make_int2(bytes, deg);
      if (deg > kSlotWidth) o.longs[(size_t)t * kTileRows + n_long++] = (uint8_t)k;
      for (int j = 0; j < deg; ++j) {
        const int32_t u = col[rs + j];
        if (stamp[u] != t) {
          if (count >= kHubHalo) return false;
          stamp[u] = t; slot_of[u] = count;
          o.halo[(size_t)t * kHubHalo + count++] = u;
        }
        o.slots[(size_t)t * kHubList + bytes + j] = (uint8_t)slot_of[u];
        if (w_csr) o.w[(size_t)t * kHubList + bytes + j] = w_csr[rs + j];
      }
      bytes = (bytes + deg + 3) & ~3;
      if (bytes > kHubList) return false;
    }
    o.info[t] = make_int4(count, (bytes + 15) & ~15, n_long, 0);
  }
  return true;
}
// The partition (balanced; the balanced deal can strand the last nodes when a hub's tile is near the cap and only its own leaves would
// fit it: then least growth alone) and both directions' lists.  w_csr[dir]: as for build_hub_lists.
static int32_t hub_plan_host(int64_t n, int nt, const std::vector<int32_t> rp[2], const std::vector<int32_t> cl[2], const float *const w_csr[2],
                             std::vector<int32_t> &order, HubHost hh[2]) {
  order = hub_partition(n, rp, cl, true);
  if ((int64_t)order.size() != n) order = hub_partition(n, rp, cl, false);
  NGPDE_REQUIRE((int64_t)order.size() == n, NGPDE_ERR_UNSUPPORTED,
                "persistent solver, hub geometry: no partition into 32-row tiles of at most %d referenced rows each (a node of more than %d distinct in+out neighbours, or tiles that do not close)",
                kHubHalo, kHubHalo - kTileRows);
  NGPDE_REQUIRE(build_hub_lists(n, nt, rp[0], cl[0], order, hh[0], w_csr[0]) && build_hub_lists(n, nt, rp[1], cl[1], order, hh[1], w_csr[1]),
                NGPDE_ERR_UNSUPPORTED,
                "persistent solver, hub geometry: a tile references more than %d distinct rows or holds more than %d entries", kHubHalo, kHubList);
  return NGPDE_OK;
}

// Host only (no device call): the hub geometry's tile partition of a graph given as its two CSR lists -- what node_persistent_setup
// would use -- so that a caller (and the CPU tests, tests/test_hub_partition.py) can ask whether a graph with hubs fits the persistent
// solver.  order[32 t + k] = the node in row k of tile t; tile_rows[2 t + dir] = the distinct rows tile t references in direction
// dir (0: lists by target, 1: by source; members included).
}  // namespace ngpde
extern "C" int32_t ngpde_hub_partition_host(int64_t n_nodes, const int32_t *rowptr_by_target, const int32_t *col_by_target,
                                            const int32_t *rowptr_by_source, const int32_t *col_by_source, int32_t *order,
                                            int32_t *tile_rows) {
  using namespace ngpde;
  NGPDE_REQUIRE(n_nodes > 0 && rowptr_by_target && rowptr_by_source && order, NGPDE_ERR_INVALID_ARGUMENT,
                "ngpde_hub_partition_host: n_nodes > 0, both row pointer arrays and `order` are required");
  const int nt = (int)((n_nodes + kTileRows - 1) / kTileRows);
  NGPDE_REQUIRE(nt <= kHubNbr, NGPDE_ERR_UNSUPPORTED, "persistent solver, hub geometry: at most %d tiles, one per workgroup", kHubNbr);
  std::vector<int32_t> rp[2], cl[2];
  const int32_t *rps[2] = {rowptr_by_target, rowptr_by_source}, *cls[2] = {col_by_target, col_by_source};
  for (int dir = 0; dir < 2; ++dir) {
    rp[dir].assign(rps[dir], rps[dir] + n_nodes + 1);
    const int64_t m = rp[dir][(size_t)n_nodes];
    NGPDE_REQUIRE(rp[dir][0] == 0 && m >= 0 && (m == 0 || cls[dir]), NGPDE_ERR_INVALID_ARGUMENT, "ngpde_hub_partition_host: CSR list %d is malformed", dir);
    for (int64_t v = 0; v < n_nodes; ++v)
      NGPDE_REQUIRE(rp[dir][v] <= rp[dir][v + 1], NGPDE_ERR_INVALID_ARGUMENT, "ngpde_hub_partition_host: row pointers of list %d decrease at row %lld", dir, (long long)v);
    cl[dir].assign(cls[dir], cls[dir] + m);
    for (int64_t e = 0; e < m; ++e)
      NGPDE_REQUIRE(cl[dir][e] >= 0 && cl[dir][e] < n_nodes, NGPDE_ERR_INVALID_ARGUMENT, "ngpde_hub_partition_host: list %d names node %d of %lld", dir, cl[dir][e], (long long)n_nodes);
  }
  std::vector<int32_t> ord;
  HubHost hh[2];
  const float *const no_w[2] = {nullptr, nullptr};
  if (int32_t st = hub_plan_host(n_nodes, nt, rp, cl, no_w, ord, hh)) return st;
  std::copy(ord.begin(), ord.end(), order);
  if (tile_rows)
    for (int t = 0; t < nt; ++t)
      for (int dir = 0; dir < 2; ++dir) tile_rows[2 * t + dir] = hh[dir].info[(size_t)t].x;
  return NGPDE_OK;
}
namespace ngpde {

int32_t node_persistent_setup(const ngpde_graph *g, const float *coef_host, NodePersist *ps, bool pair, bool hub) {
  std::vector<int> lists;
  const int nt = g->n_sched / kTileRows;
  ps->hub = false;
  if (hub) {
    NGPDE_REQUIRE(!pair && nt <= kHubNbr, NGPDE_ERR_UNSUPPORTED, "persistent solver, hub geometry: at most %d tiles, one per workgroup", kHubNbr);
    std::vector<int32_t> rp[2], cl[2];
    NGPDE_REQUIRE(host_csr(g, g->by_t, rp[0], cl[0]) && host_csr(g, g->by_s, rp[1], cl[1]), NGPDE_ERR_HIP, "download of the CSR lists failed");
    // edge weights: the handle's COO copy through each list's entry -> COO position map
    std::vector<float> wcsr[2];
    if (g->w_coo && g->n_edges > 0) {
      std::vector<float> wc((size_t)g->n_edges);
      NGPDE_HIP_CHECK(hipMemcpy(wc.data(), g->w_coo, wc.size() * sizeof(float), hipMemcpyDeviceToHost));
      const Csr *cs[2] = {&g->by_t, &g->by_s};
      for (int dir = 0; dir < 2; ++dir) {
        std::vector<int32_t> eid = cs[dir]->h_eid;
        if (eid.empty()) {
          eid.resize((size_t)g->n_edges);
          NGPDE_HIP_CHECK(hipMemcpy(eid.data(), cs[dir]->eid, eid.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
        wcsr[dir].resize((size_t)g->n_edges);
        for (int64_t e = 0; e < g->n_edges; ++e) wcsr[dir][(size_t)e] = wc[(size_t)eid[(size_t)e]];
      }
    }
    std::vector<int32_t> order;
    HubHost hh[2];
    const float *const w_csr[2] = {wcsr[0].empty() ? nullptr : wcsr[0].data(), wcsr[1].empty() ? nullptr : wcsr[1].data()};
    if (int32_t st = hub_plan_host(g->n_nodes, nt, rp, cl, w_csr, order, hh)) return st;
    // the partition's schedule: {node, 0, 0, bits of c[node]} per position, -1 padded
    std::vector<float> cnode((size_t)g->n_nodes);
    NGPDE_HIP_CHECK(hipMemcpy(cnode.data(), g->c, cnode.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<int4> hsched((size_t)nt * kTileRows, make_int4(-1, 0, 0, 0));
    for (int64_t pos = 0; pos < g->n_nodes; ++pos) {
      int4 e = make_int4(order[pos], 0, 0, 0);
      std::memcpy(&e.w, &cnode[order[pos]], 4);
      hsched[(size_t)pos] = e;
    }
    // wait lists: symmetric closure over both directions, up to 255 tiles, position 63 left free (that lane watches the abort word)
    const std::vector<int32_t> tile_of = tiles_of(order);
    std::vector<std::vector<int>> foreign(nt);
    for (const HubHost &h : hh)
      for (int t = 0; t < nt; ++t)
        for (int k = kTileRows; k < h.info[t].x; ++k) foreign[t].push_back(tile_of[h.halo[(size_t)t * kHubHalo + k]]);
    NGPDE_REQUIRE(wait_lists_from(nt, kHubNbr, true, foreign, lists), NGPDE_ERR_UNSUPPORTED,
                  "persistent solver, hub geometry: a wait list exceeds %d tiles", kHubNbr - 1);
    for (int dir = 0; dir < 2; ++dir) {
      NodePersist::HubLists &L = ps->hub_lists[dir];
      const HubHost &h = hh[dir];
      auto up = [&](auto **dst, const auto &v) -> int32_t {
        NGPDE_HIP_CHECK(hipMalloc((void **)dst, std::max<size_t>(v.size(), 1) * sizeof(v[0])));
        NGPDE_HIP_CHECK(hipMemcpy(*dst, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice));
        return NGPDE_OK;
      };
      int32_t st;
      if ((st = up(&L.halo, h.halo)) || (st = up(&L.slots, h.slots)) || (st = up(&L.rows, h.rows)) || (st = up(&L.info, h.info)) ||
          (st = up(&L.longs, h.longs)) || (st = up(&L.sched, hsched)))
        return st;
      if (!h.w.empty() && (st = up(&L.w, h.w))) return st;
    }
    ps->hub = true;
  } else {
    NGPDE_REQUIRE(build_wait_lists(g, lists), NGPDE_ERR_UNSUPPORTED, "persistent solver: a tile's wait list exceeds %d tiles", kNbrStride);
  }
  ps->n_tiles = nt;
  ps->pair_wgs = 0;
  if (pair) {
    // workgroup b holds tiles t = xcd_tile(b, W) and t + W (W = ceil(nt / 2)): half a schedule apart, so never neighbours on a
    // graph with any locality -- but it is checked: a tile waiting for its own workgroup's other tile would wait for a flag that is
    // published only after the wait
    const int W = (nt + 1) / 2;
    for (int t = 0; t + W < nt; ++t)
      for (int k = 0; k < kNbrStride; ++k)
        NGPDE_REQUIRE(lists[(size_t)t * kNbrStride + k] != t + W, NGPDE_ERR_UNSUPPORTED,
                      "persistent solver: tiles %d and %d of one workgroup are neighbours", t, t + W);
    ps->pair_wgs = W;
  }
  NGPDE_HIP_CHECK(hipMalloc((void **)&ps->nbr, lists.size() * sizeof(int)));
  NGPDE_HIP_CHECK(hipMemcpy(ps->nbr, lists.data(), lists.size() * sizeof(int), hipMemcpyHostToDevice));
  // flag words: one 128-byte line per tile and slot (two slots: the interleaved kernels), + one line for the abort word; zeroed
  // (by a kernel) before every launch
  ps->sync_bytes = (size_t)(2 * nt + 1) * 128;
  NGPDE_HIP_CHECK(hipMalloc((void **)&ps->sync, ps->sync_bytes));
  NGPDE_HIP_CHECK(hipMemset(ps->sync, 0, ps->sync_bytes));
  NGPDE_HIP_CHECK(hipMalloc((void **)&ps->coef, 90 * sizeof(float)));
  NGPDE_HIP_CHECK(hipMemcpy(ps->coef, coef_host, 90 * sizeof(float), hipMemcpyHostToDevice));
  // the sticky fault word lives in pinned, device-mapped HOST memory: the latch kernel writes it through the device pointer, and
  // every later entry of the plan can look at it without a synchronisation (ngpde_node_gcn2_forward / _backward refuse to go on)
  NGPDE_HIP_CHECK(hipHostMalloc((void **)&ps->fault_host, 128, hipHostMallocMapped));
  *ps->fault_host = 0u;
  NGPDE_HIP_CHECK(hipHostGetDevicePointer((void **)&ps->fault, const_cast<unsigned *>(ps->fault_host), 0));
  NGPDE_HIP_CHECK(hipMalloc((void **)&ps->stats, (size_t)nt * 2 * sizeof(int)));
  NGPDE_HIP_CHECK(hipMemset(ps->stats, 0, (size_t)nt * 2 * sizeof(int)));
  return NGPDE_OK;
}

void node_persistent_free(NodePersist *ps) {
  if (ps->nbr) (void)hipFree(ps->nbr);
  if (ps->sync) (void)hipFree(ps->sync);
  if (ps->fault_host) (void)hipHostFree(const_cast<unsigned *>(ps->fault_host));
  ps->fault_host = nullptr;
  if (ps->coef) (void)hipFree(ps->coef);
  if (ps->stats) (void)hipFree(ps->stats);
  ps->stats = nullptr;
  for (NodePersist::HubLists &L : ps->hub_lists) {
    if (L.halo) (void)hipFree(L.halo);
    if (L.slots) (void)hipFree(L.slots);
    if (L.rows) (void)hipFree(L.rows);
    if (L.info) (void)hipFree(L.info);
    if (L.longs) (void)hipFree(L.longs);
    if (L.sched) (void)hipFree(L.sched);
    if (L.w) (void)hipFree(L.w);
    L = NodePersist::HubLists();
  }
  ps->hub = false;
  ps->nbr = nullptr; ps->sync = nullptr; ps->fault = nullptr; ps->coef = nullptr;
}

namespace {
// NGPDE_DEBUG_FORCE_ABORT=1 (tests only): the launch starts with its abort word set, i.e. every workgroup gives up at its first wait
__global__ void set_word_kernel(unsigned *w, unsigned v) {
  if (threadIdx.x == 0) *w = v;
}
// fault |= abort word of the launch that just ran (sticky, read by ngpde_node_fault)
__global__ void latch_fault_kernel(const unsigned *abort_word, unsigned *fault) {
  if (threadIdx.x == 0 && *abort_word != 0) *fault = 1u;
}
}  // namespace
const unsigned *node_persistent_abort_word(const NodePersist *ps) { return ps->sync ? sync_abort_word(ps->sync, ps->n_tiles) : nullptr; }
// A persistent launch needs ALL its workgroups resident, and two of them in flight on one device (two plans on two streams) can
// starve each other of residency until both time out.  Inside one process they are therefore made to take turns: every persistent
// launch first makes its stream wait for the event recorded behind the previous persistent launch on that device, whatever stream
// that one ran on.  (Nothing can be done about another PROCESS on the same device: one rank per GPU, include/ngpde.h.)
namespace {
struct Turnstile {
  std::mutex mu;
  hipEvent_t last[16] = {};
  bool used[16] = {};
};
Turnstile &turnstile() {
  static Turnstile t;
  return t;
}
}  // namespace

int32_t PersistentTurn::enter(const NodePersist &p, hipStream_t s) {
  ps = &p;
  stream = s;
  NGPDE_HIP_CHECK(hipGetDevice(&dev));
  if (dev >= 0 && dev < 16) {
    Turnstile &t = turnstile();
    t.mu.lock();
    held = true;
    if (!capturing(stream) && t.used[dev]) NGPDE_HIP_CHECK(hipStreamWaitEvent(stream, t.last[dev], 0));
  }
  int32_t st;
  if ((st = launch_zero(p.sync, p.sync_bytes, stream))) return st;
  if (switch_on(Switch::DebugForceAbort)) hipLaunchKernelGGL(set_word_kernel, dim3(1), dim3(64), 0, stream, sync_abort_word(p.sync, p.n_tiles), 1u);
  return NGPDE_OK;
}
int32_t PersistentTurn::latch() {
  hipLaunchKernelGGL(latch_fault_kernel, dim3(1), dim3(64), 0, stream, sync_abort_word(ps->sync, ps->n_tiles), ps->fault);
  NGPDE_LAUNCH_CHECK("latch_fault_kernel");
  return NGPDE_OK;
}
int32_t PersistentTurn::leave() {
  if (!held) return NGPDE_OK;
  Turnstile &t = turnstile();
  int32_t st = NGPDE_OK;
  if (!capturing(stream)) {
    if (!t.last[dev] && hipEventCreateWithFlags(&t.last[dev], hipEventDisableTiming) != hipSuccess) st = fail(NGPDE_ERR_HIP, "hipEventCreate failed");
    if (st == NGPDE_OK && hipEventRecord(t.last[dev], stream) != hipSuccess) st = fail(NGPDE_ERR_HIP, "hipEventRecord failed");
    if (st == NGPDE_OK) t.used[dev] = true;
  }
  held = false;
  t.mu.unlock();
  return st;
}
PersistentTurn::~PersistentTurn() {
  if (held) {
    held = false;
    turnstile().mu.unlock();
  }
}

}  // namespace ngpde
