// edge_mlp_forms.h -- which kernels every one-launch message-MLP call runs, decided in one place (host only, plain C++17: no HIP).
//
// The family behind ngpde_edge_mlp_* and ngpde_edge_layer_* (ExplicitEdgeConv, VMHConv, MPPDEConv) picks its kernels from the
// graph's tile geometry (TileGeom: all any choice reads of a handle), the message MLP and what the caller passes (EdgeMlpDesc:
// widths, activations, aggregation and presence bits for what are pointers in a call).  Every choice is a pure function here that
// returns a small plain struct -- the decision -- and the launchers (edge_mlp_fused.hip, edge_mlp64.hip, edge_mlp_deep_bwd.hip) and
// entries (api_mp.hip, api_layers.hip) execute a decision without judging the shape again.  A decision names the kernels it stands
// for, in launch order (names()), and tests/host/edge_mlp_forms_check.cpp prints decisions for tests/test_edge_mlp_forms_host.py to
// compare, line by line, with the restatement the float64 tests take their thresholds from (tests/edge_mlp_forms_spec.py).  No
// function here touches the device or dereferences a data pointer.
//
// Every form needs the tile schedule (a graph with its normalisation set whose tiles fit: <= kHaloCap distinct rows, degrees
// <= kSlotWidth) and widths that are multiples of 4 in 4 .. 64.  All grids are persistent: 8 x min(cap, ceil(tiles / 8))
// workgroups, cap = 64 per XCD (two workgroups per CU) where the LDS request + the form's slack fits kLdsBudget, else 32.
//
// ngpde_edge_mlp_forward (edge_mlp_fwd_plan), n_tail 0 .. 3, in this order:
//   edge64   edge_mlp64_fwd_kernel<A1, A2>      P and Q given, no per-edge term, 64 => 64 with one tail layer, + / mean, A1 in
//                                               swish / relu / tanh, A2 = A1 or identity, nothing saved per edge, NGPDE_NO_EDGE64
//                                               unset; 256 threads, (halo + 225) rows of LDS, slack 4096
//   general  edge_mlp_fused_fwd_kernel<n_tail>  everything else; 512 threads, (halo + 161 + 64 n_tail) rows, slack 2048
// ngpde_edge_mlp_backward (edge_mlp_bwd_plan), in this order:
//   deep     edge_mlp_deep_bwd_kernel<n_tail>   n_tail 2 or 3, + / mean; 256 threads, (halo + 97 + 128 n_tail) rows, cap 32
//   edge64   edge_mlp64_bwd_kernel<A1, A2, DQ>  n_tail 0 or 1 and the forward's edge64 conditions (save_z aside); 256 threads, (halo
//                                               + 225) rows, slack 4096.  DQ -- the by-source sum inside the launch, no [E][64]
//                                               buffer -- iff dQ is wanted, every halo is within kDqStride rows and
//                                               NGPDE_EDGE64_NO_DQ is unset
//   general  edge_mlp_fused_bwd_kernel<n_tail>  n_tail 0 or 1, all five aggregations; 512 threads, (halo + 193 + 128 n_tail
//                                               (+ 32 for max / min / *)) rows, cap 32
//   then dense_weight_reduce_kernel per tail layer, then edge64_dq_combine_kernel (DQ; skipped at launch time when no tile's halo
//   holds a foreign row) or, where dQ is wanted, edge_sum_by_source_kernel.
// The pullback's workspace (edge_mlp_bwd_layout, edge_mlp_bwd_workspace_bytes): one weight slab per workgroup and tail layer; at
// 64 => 64 the larger of the general and the edge64 layouts whatever the switches say, so that one buffer serves both.
// A layer's message path (edge_layer_msg_path): the fused forward unless NGPDE_NO_FUSED_EDGE, no edges, or max / min / * in training
// without a fused pullback; the fused pullback unless NGPDE_NO_FUSED_EDGE_BWD, and for n_tail >= 2 from kDeepBwdNodes nodes
// (NGPDE_DEEP_EDGE_BWD=1 forces, =0 forbids).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "switches.h"
#include "tile_geom.h"
#include "workspace.h"

namespace ngpde {

// ---- what the message-MLP family measures in (short names: the three kernel files and edge_mlp_tile.h say `using namespace`) ---------
namespace edge_mlp {
constexpr int kW = 64, kTS = kW + 4, kRows = kTileRows;   // widest layer, LDS row stride (floats), rows of a tile
constexpr int kT = 512, kChunk = 128, kGroups = 32;       // general kernels: threads, edges per chunk (8 waves x 16), 16-lane groups
constexpr int kT4 = 256, kChunk4 = 64;                    // edge64 and deep kernels: threads, edges per chunk (4 waves x 16)
constexpr int kDqSlots = 3;                               // halo slots per 16-lane group whose sums stay in registers (DQ)
constexpr int kDqStride = 16 * kDqSlots;                  // = the largest halo the in-launch by-source sum takes (48 rows)
constexpr int kMaxTail = 3;                               // Dense layers after the first
constexpr int kPerXcd1 = 32, kPerXcd2 = 64;               // persistent workgroups per XCD: one / two per CU
constexpr size_t kLdsBudget = 80 * 1024;                  // two workgroups per CU where request + slack fits this
constexpr size_t kFwdLdsSlack = 2048, kEdge64LdsSlack = 4096;   // static LDS beside the request: general forward / edge64 pair
constexpr int64_t kDeepBwdNodes = 32768;                  // the deep pullback pays from here (one 4-wave workgroup per CU, long chain)
}  // namespace edge_mlp

using EdgeKernelNames = std::vector<std::string>;

// ---- the tile schedule as this family reads it (TileGeom, tile_geom.h: the by-target side) ------------------------------------------------
inline bool edge_tiles_ok(const TileGeom &g) { return g.graph && g.has_norm && g.halo_ok; }
// LDS rows of the halo region = the largest halo of this graph's tiles
inline int edge_halo_rows(const TileGeom &g) { return std::max<int>(kTileRows, std::min<int>(kHaloCap, g.max_halo)); }
// Persistent workgroups, at most per_xcd_cap per XCD.  EdgeTileRange splits the tiles into 8 per-XCD ranges and lets gridDim.x / 8
// workgroups walk each: the grid has to be a multiple of 8, or the workgroups beyond the last multiple walk tiles of their XCD a
// second time (and add their weight gradients twice).
inline int edge_persistent_grid(const TileGeom &g, int per_xcd_cap) { return 8 * std::max(1, std::min(per_xcd_cap, (g.n_tiles + 7) / 8)); }
// the dynamic LDS of a form: the halo region, its zero row and the form's other rows, kTS floats each
inline size_t edge_lds_bytes(const TileGeom &g, int other_rows) {
  return (size_t)(edge_halo_rows(g) + 1 + other_rows) * edge_mlp::kTS * sizeof(float);
}
inline int edge_per_xcd(size_t lds, size_t slack) { return lds + slack <= edge_mlp::kLdsBudget ? edge_mlp::kPerXcd2 : edge_mlp::kPerXcd1; }

// ---- a call: the message MLP and what the caller passes ------------------------------------------------------------------------------
struct EdgeMlpDesc {
  int h1 = 0, act1 = 0, n_tail = 0, aggr = 0;
  int dout[edge_mlp::kMaxTail] = {0, 0, 0}, act[edge_mlp::kMaxTail] = {0, 0, 0};
  bool tails = true;   // the tail layers' tables are given (a query may pass NULL)
  bool P = false, Q = false, Eterm = false, save_z = false;   // forward and pullback: the arrays given (save_z: any of them)
  bool dQ = false, dE = false;                                // pullback: the source gradient is wanted, the [E][h1] buffer is given
  int din(int l) const { return l == 0 ? h1 : dout[l - 1]; }
};
// widths, activations and aggregation from a call's tables (nullable; n_tail is kept as passed, at most kMaxTail layers are read)
inline EdgeMlpDesc edge_mlp_desc(int h1, int act1, int n_tail, const int32_t *tail_dout, const int32_t *tail_act, int aggr) {
  EdgeMlpDesc d;
  d.h1 = h1; d.act1 = act1; d.n_tail = n_tail; d.aggr = aggr;
  d.tails = n_tail <= 0 || tail_dout != nullptr;
  for (int l = 0; l < std::min(n_tail, edge_mlp::kMaxTail); ++l) {
    if (tail_dout) d.dout[l] = tail_dout[l];
    if (tail_act) d.act[l] = tail_act[l];
  }
  return d;
}

inline bool edge_width_ok(int w) { return w > 0 && w <= edge_mlp::kW && w % 4 == 0; }
inline bool edge_chain_ok(const EdgeMlpDesc &d, int min_tail, int max_tail) {
  if (!edge_width_ok(d.h1) || d.n_tail < min_tail || d.n_tail > max_tail || !d.tails) return false;
  for (int l = 0; l < d.n_tail; ++l)
    if (!edge_width_ok(d.dout[l])) return false;
  return true;
}
inline bool edge_sum_or_mean(int aggr) { return aggr == NGPDE_AGGR_SUM || aggr == NGPDE_AGGR_MEAN; }

// The 64-wide pipelined pair applies to: P and Q present, no per-edge term, h1 = 64, one further Dense 64 => 64, + / mean, and an
// activation pair that is instantiated (edge64_pair in edge_mlp64.hip).  NGPDE_NO_EDGE64=1 keeps the general kernels.
inline bool edge64_shape(const EdgeMlpDesc &d) {
  if (switch_on(Switch::NoEdge64)) return false;
  if (!d.P || !d.Q || d.Eterm || d.h1 != edge_mlp::kW || d.n_tail != 1 || !d.tails || d.dout[0] != edge_mlp::kW) return false;
  if (!edge_sum_or_mean(d.aggr)) return false;
  const bool a1 = d.act1 == NGPDE_ACT_SWISH || d.act1 == NGPDE_ACT_RELU || d.act1 == NGPDE_ACT_TANH;
  return a1 && (d.act[0] == d.act1 || d.act[0] == NGPDE_ACT_IDENTITY);
}
// its pullback sums by source inside the launch (no [E][64] array): dQ wanted, every halo within kDqStride rows
inline bool edge64_dq_halo(const TileGeom &g, const EdgeMlpDesc &d) {
  return !switch_on(Switch::Edge64NoDq) && d.dQ && g.halo_ok && g.max_halo <= edge_mlp::kDqStride;
}
inline const char *edge_act_name(int act) {
  return act == NGPDE_ACT_SWISH ? "swish" : act == NGPDE_ACT_RELU ? "relu" : act == NGPDE_ACT_TANH ? "tanh" : "identity";
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
enum class EdgeFwdForm { None, Edge64, General };
struct EdgeFwd {
  bool supported = false;
  EdgeFwdForm form = EdgeFwdForm::None;   // None: unsupported, or no nodes (nothing to launch)
  int act1 = 0, act2 = 0, n_tail = 0;     // the template arguments
  int threads = 0, per_xcd = 0, grid = 0;
  size_t lds = 0;
  EdgeKernelNames names() const {
    if (form == EdgeFwdForm::None) return {};
    if (form == EdgeFwdForm::Edge64) return {std::string("edge_mlp64_fwd_kernel<") + edge_act_name(act1) + "," + edge_act_name(act2) + ">"};
    return {"edge_mlp_fused_fwd_kernel<" + std::to_string(n_tail) + ">"};
  }
};
inline bool edge_mlp_fwd_supported(const TileGeom &g, const EdgeMlpDesc &d) { return edge_tiles_ok(g) && edge_chain_ok(d, 0, edge_mlp::kMaxTail); }
inline EdgeFwd edge_mlp_fwd_plan(const TileGeom &g, const EdgeMlpDesc &d) {
  using namespace edge_mlp;
  EdgeFwd p;
  p.supported = edge_mlp_fwd_supported(g, d);
  if (!p.supported || g.n_nodes == 0) return p;
  p.act1 = d.act1; p.act2 = d.act[0]; p.n_tail = d.n_tail;
  if (edge64_shape(d) && !d.save_z) {
    p.form = EdgeFwdForm::Edge64;
    p.threads = kT4;
    p.lds = edge_lds_bytes(g, kRows + kW + 2 * kChunk4);   // P rows, W2^T, two message chunks
    p.per_xcd = edge_per_xcd(p.lds, kEdge64LdsSlack);
  } else {
    p.form = EdgeFwdForm::General;
    p.threads = kT;
    p.lds = edge_lds_bytes(g, kGroups + d.n_tail * kW + kChunk);   // P rows, the tail's W^T, one message chunk
    p.per_xcd = edge_per_xcd(p.lds, kFwdLdsSlack);
  }
  p.grid = edge_persistent_grid(g, p.per_xcd);
  return p;
}

// ---- the pullback's workspace --------------------------------------------------------------------------------------------------------
enum class EdgeBwdForm { General, Edge64, Deep };
// partial[l]: the weight slabs of tail layer l, one [(din + 1)][dout] per workgroup (row din = bias gradient), nullptr from n_tail
// on; dqpart: the edge64 pullback's per-tile sums by foreign halo slot, on a graph whose halos allow the by-source sum in the launch
struct EdgeBwdWs {
  float *partial[edge_mlp::kMaxTail] = {nullptr, nullptr, nullptr};
  float *dqpart = nullptr;
};
inline size_t edge_slab_bytes(int grid, int din, int dw) { return (size_t)grid * (din + 1) * dw * sizeof(float); }
inline int edge_general_dw(const EdgeMlpDesc &d) { return (d.n_tail == 1 && d.tails) ? d.dout[0] : 0; }   // the general pullback's tail width
inline void edge_mlp_bwd_layout(Workspace &w, const TileGeom &g, const EdgeMlpDesc &d, EdgeBwdForm form, EdgeBwdWs &p) {
  using namespace edge_mlp;
  p = EdgeBwdWs();
  if (form == EdgeBwdForm::Edge64) {   // slabs of the larger grid (two workgroups per CU), then the partials
    p.partial[0] = reinterpret_cast<float *>(w.take<char>(edge_slab_bytes(edge_persistent_grid(g, kPerXcd2), kW, kW)));
    if (g.halo_ok && g.max_halo <= kDqStride) p.dqpart = w.take<float>((size_t)g.n_tiles * kDqStride * kW);
    return;
  }
  const int grid = edge_persistent_grid(g, kPerXcd1);
  if (form == EdgeBwdForm::General) {   // (no tail layer: no bytes, the base)
    p.partial[0] = reinterpret_cast<float *>(w.take<char>(edge_slab_bytes(grid, d.h1, edge_general_dw(d))));
    return;
  }
  for (int l = 0; l < std::min(d.n_tail, kMaxTail); ++l) p.partial[l] = reinterpret_cast<float *>(w.take<char>(edge_slab_bytes(grid, d.din(l), d.dout[l])));
}
// what ngpde_edge_mlp_backward_workspace_bytes answers.  n_tail <= 1: the general kernel's slabs start at the base and end unrounded;
// at 64 => 64 the edge64 layout counts too (whatever the switches and activations: the query knows neither)
inline size_t edge_mlp_bwd_workspace_bytes(const TileGeom &g, const EdgeMlpDesc &d) {
  using namespace edge_mlp;
  if (!g.graph) return 0;
  EdgeBwdWs p;
  if (d.n_tail >= 2) return (d.n_tail <= kMaxTail && d.tails) ? measure(edge_mlp_bwd_layout, g, d, EdgeBwdForm::Deep, p) + kWsSlack : 0;
  const int dw = edge_general_dw(d);
  const size_t general = edge_slab_bytes(edge_persistent_grid(g, kPerXcd1), d.h1, dw);
  const size_t edge64 = (d.h1 == kW && dw == kW) ? measure(edge_mlp_bwd_layout, g, d, EdgeBwdForm::Edge64, p) : 0;
  return std::max(general, edge64) + kWsSlack;
}

// ---- pullback -----------------------------------------------------------------------------------------------------------------------
struct EdgeBwd {
  bool supported = false;
  EdgeBwdForm form = EdgeBwdForm::General;   // by shape, also where unsupported (the entry's message names the form)
  bool launch = false;                       // supported and the graph has nodes
  bool dq = false;                           // Edge64: the by-source sum inside the launch
  bool edge_buffer = true;                   // the [E][h1] buffer is required ...
  bool dE_missing = false;                   // ... and it is not given though the graph has edges
  bool by_source = false;                    // dQ by edge_sum_by_source_kernel
  int act1 = 0, act2 = 0, n_tail = 0;        // the template arguments
  int threads = 0, grid = 0;
  size_t lds = 0, workspace_bytes = 0;
  EdgeKernelNames names() const {
    if (!launch) return {};
    EdgeKernelNames k;
    if (form == EdgeBwdForm::Edge64)
      k.push_back(std::string("edge_mlp64_bwd_kernel<") + edge_act_name(act1) + "," + edge_act_name(act2) + (dq ? ",true>" : ",false>"));
    else
      k.push_back((form == EdgeBwdForm::Deep ? "edge_mlp_deep_bwd_kernel<" : "edge_mlp_fused_bwd_kernel<") + std::to_string(n_tail) + ">");
    for (int l = 0; l < n_tail; ++l) k.push_back("dense_weight_reduce_kernel");
    if (dq) k.push_back("edge64_dq_combine_kernel");
    if (by_source) k.push_back("edge_sum_by_source_kernel");
    return k;
  }
};
inline EdgeBwd edge_mlp_bwd_plan(const TileGeom &g, const EdgeMlpDesc &d) {
  using namespace edge_mlp;
  EdgeBwd p;
  p.act1 = d.act1; p.act2 = d.act[0]; p.n_tail = d.n_tail;
  if (d.n_tail >= 2) {   // message MLPs of three / four layers
    p.form = EdgeBwdForm::Deep;
    p.supported = edge_tiles_ok(g) && edge_chain_ok(d, 2, kMaxTail) && edge_sum_or_mean(d.aggr);
    p.threads = kT4;
    p.lds = edge_lds_bytes(g, kRows + kChunk4 + 2 * d.n_tail * kW);   // P rows, a chunk, W^T and W of every tail layer
    p.grid = edge_persistent_grid(g, kPerXcd1);
  } else {
    // (max / min / * on the general kernel only: the 64-wide and deep ones take + / mean)
    p.supported = edge_tiles_ok(g) && edge_chain_ok(d, 0, 1) && d.aggr >= NGPDE_AGGR_SUM && d.aggr <= NGPDE_AGGR_MUL;
    if (edge64_shape(d)) {
      p.form = EdgeBwdForm::Edge64;
      p.dq = edge64_dq_halo(g, d);
      p.threads = kT4;
      p.lds = edge_lds_bytes(g, kRows + kChunk4 + 2 * kW);   // P rows, a chunk, W2^T and W2
      p.grid = edge_persistent_grid(g, edge_per_xcd(p.lds, kEdge64LdsSlack));   // (the workspace holds slabs for the larger grid)
    } else {
      p.threads = kT;
      // P and gradient rows, a chunk, W2^T and W2, and for max / min / * the targets' extremum or zero count
      p.lds = edge_lds_bytes(g, 2 * kGroups + kChunk + (d.n_tail ? 2 * kW : 0) + (d.aggr >= NGPDE_AGGR_MAX ? kGroups : 0));
      p.grid = edge_persistent_grid(g, kPerXcd1);
    }
  }
  p.launch = p.supported && g.n_nodes != 0;
  p.edge_buffer = !p.dq;
  p.dE_missing = p.edge_buffer && !d.dE && g.n_edges != 0;
  p.by_source = d.dQ && !p.dq;
  p.workspace_bytes = edge_mlp_bwd_workspace_bytes(g, d);
  return p;
}

// ---- the message path of a layer (make_plan in api_layers.hip): d describes the call the layer would make (P, Q, dQ set; Eterm iff
// the layer has edge features) -----------------------------------------------------------------------------------------------------
struct EdgeMsgPath {
  bool fused_msg = false, fused_bwd = false, need_dE = false;
  size_t bwd_workspace_bytes = 0;   // fused_bwd: what the fused pullback asks for
};
inline EdgeMsgPath edge_layer_msg_path(const TileGeom &g, const EdgeMlpDesc &d, bool training) {
  EdgeMsgPath m;
  // max / min / *: with gradients only where the one-launch pullback takes it -- the primitives' pullbacks of those need the per-edge
  // messages, which the fused forward does not keep
  const EdgeBwd bwd = edge_mlp_bwd_plan(g, d);
  const bool bwd_ok = !switch_on(Switch::NoFusedEdgeBwd) && bwd.supported;
  m.fused_msg = !switch_on(Switch::NoFusedEdge) && g.n_edges > 0 && (edge_sum_or_mean(d.aggr) || !training || bwd_ok) && edge_mlp_fwd_supported(g, d);
  if (!m.fused_msg || !training) return m;
  m.fused_bwd = bwd_ok;
  if (m.fused_bwd && d.n_tail >= 2) {
    const char *deep = switch_text(Switch::DeepEdgeBwd);
    const char d0 = deep ? deep[0] : '\0';
    m.fused_bwd = d0 == '1' || (d0 != '0' && g.n_nodes >= edge_mlp::kDeepBwdNodes);
  }
  if (m.fused_bwd) {
    m.need_dE = bwd.edge_buffer;
    m.bwd_workspace_bytes = bwd.workspace_bytes;
  }
  return m;
}

}  // namespace ngpde
