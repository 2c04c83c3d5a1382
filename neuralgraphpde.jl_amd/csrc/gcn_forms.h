// gcn_forms.h -- which kernels every GCNConv call runs, decided in one place (host only, plain C++17: no HIP).
//
// The family behind ngpde_gcn_forward / _backward / _backward_ew picks its kernels from the widths, the activation, the graph's tile
// geometry (TileGeom, tile_geom.h: all a choice reads of a handle) and one switch.  Every choice is a pure function here that returns
// a small plain struct -- the decision -- and the launchers (gcn_fused.hip, gcn_generic.hip) and the entries (api_gcn.hip) execute a
// decision without judging the shape again.  A decision names the kernels it stands for, in launch order (names()), and
// tests/host/gcn_gat_forms_check.cpp prints decisions for tests/test_gcn_gat_forms_host.py to compare, line by line, with the
// restatement the float64 tests take their thresholds from (tests/gcn_gat_forms_spec.py).  No function here touches the device or
// dereferences a data pointer.  The solvers' own plans (node.hip, node_persistent.hip) call the fused_* functions by name.
//
// A layer (gcn_layer_form), in the order the kinds are tried:
//   fused            din == dout in {16, 32, 64, 128}: one launch forward, gcn_fused_fwd_kernel<D, ACT, HALO, PRE> (gcn_fused_fwd_form);
//                    the pullback is zero_bytes_kernel over the slabs, gcn_fused_bwd_kernel<D, AGG = false, ACT, false, PAIR, PRE> (dz,
//                    the dW / db slabs, G = dz W^T), <D, AGG = true, ..> when dx is asked for (dx = A^T G), reduce_slabs_kernel for dW
//                    and for db (gcn_fused_bwd_form).  Needs saved_agg.  No forward workspace.
//   aggregate first  dout >= din: spmm_generic_kernel<DP> on din columns, then the Dense forward; the pullback is act_bwd_kernel, the
//                    Dense weight pullback (its bias row is db), and for dx the Dense input pullback and spmm_generic_kernel<DP> by
//                    source.  Needs saved_agg.
//   multiply first   dout < din: the Dense forward split dense_fwd_splits() ways over the input features (dense_forms.h), its
//                    dense_fwd_split_count() partial products summed by sum_partials_kernel, then spmm_generic_kernel<DP> on dout
//                    columns with bias and activation in its tail; the pullback is act_bwd_kernel, the bias column sum
//                    (colsum_kernel, in two stages -- colsum_partial_kernel first -- above 4 * kColsumChunks rows),
//                    spmm_generic_kernel<DP> by source and the two Dense pullbacks.  Needs x, leaves save_agg alone.
//   DP = 8 / 16 / 32 / 64 for at most 8 / 16 / 32 / more columns (gcn_spmm_dp).
// The fused launches: ACT is instantiated for relu and identity and read at run time (-1) otherwise.  HALO -- the tile's distinct rows
// staged in LDS -- iff every tile of the launch's direction fits (forward: by target, dx launch: by source; the dense launch never
// gathers) and NGPDE_NO_HALO is not 1; the switch is latched ONCE per process.  PRE -- the solvers' pre-scaled rows -- needs self
// loops and both directions' tiles to fit (fused_prescaled_supported) and implies HALO wherever the launch gathers.  PAIR -- two tiles
// per 1024-thread workgroup, one slab per pair -- iff D <= 64.  Feature rows are fetched with 32-bit byte offsets: n_nodes * d * 4
// must stay below 2^32 (rows_fit_32bit: the one place that says so, for the GAT kernels too).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/ngpde.h"
#include "dense_forms.h"
#include "switches.h"
#include "tile_geom.h"
#include "workspace.h"

namespace ngpde {

// ---- the family's constants ---------------------------------------------------------------------------------------------------------
constexpr int kFusedThreads = 512;        // threads of a tile's workgroup (gcn_tile.h: kThreads)
constexpr int kFusedPairMaxD = 64;        // pullback: two tiles per workgroup up to this width (two 60 KB regions fit the CU's LDS)
constexpr uint64_t kRowBytesLimit = 1ull << 32;
constexpr int kColsumChunks = 128;        // row chunks of a two-stage column sum
constexpr size_t kGcnSlack = 256;         // what the queries add behind the pullback's own pieces; the ew pieces start after it

using GcnKernelNames = std::vector<std::string>;

constexpr bool rows_fit_32bit(int64_t n_nodes, int d) { return (uint64_t)n_nodes * (uint64_t)d * 4u < kRowBytesLimit; }
constexpr bool fused_supported(int din, int dout) { return din == dout && (din == 16 || din == 32 || din == 64 || din == 128); }
constexpr int fused_num_blocks(int64_t n_nodes) { return (int)((n_nodes + kTileRows - 1) / kTileRows); }
constexpr bool fused_bwd_pairs(int d) { return d <= kFusedPairMaxD; }
// slabs the backward launches write (paired workgroups share one)
constexpr int fused_num_slabs(int64_t n_nodes, int d) { return fused_bwd_pairs(d) ? (fused_num_blocks(n_nodes) + 1) / 2 : fused_num_blocks(n_nodes); }
// bytes of one sign-bit mask (FusedFwdArgs::save_mask): 4 sign bits of z per thread and row of its group (Geo<d>::R rows)
constexpr size_t fused_mask_bytes(int64_t n_nodes, int d) {
  const int groups = kFusedThreads / (d / 4);
  return (size_t)fused_num_blocks(n_nodes) * ((kTileRows + groups - 1) / groups) * kFusedThreads;
}
// the pre-scaled pipeline (rows stored as c .* x, gathered raw by LDS-DMA): every tile staged from LDS in both directions, and c
// finite and positive (self loops: degree >= 1)
inline bool fused_prescaled_supported(const TileGeom &g, int d) {
  return g.graph && g.has_norm && g.self_loops && fused_supported(d, d) && g.halo_ok && g.halo_ok_s && !switch_on(Switch::NoHalo);
}

enum class GcnAct { Relu, Identity, RunTime };   // the ACT a fused kernel is instantiated for
inline GcnAct gcn_act_class(int act) { return act == NGPDE_ACT_RELU ? GcnAct::Relu : act == NGPDE_ACT_IDENTITY ? GcnAct::Identity : GcnAct::RunTime; }
inline int gcn_act_template(GcnAct a) { return a == GcnAct::Relu ? NGPDE_ACT_RELU : a == GcnAct::Identity ? NGPDE_ACT_IDENTITY : -1; }
inline const char *gcn_act_name(GcnAct a) { return a == GcnAct::Relu ? "relu" : a == GcnAct::Identity ? "identity" : "runtime"; }
inline const char *gcn_tf(bool b) { return b ? "true" : "false"; }

// ---- the fused launches --------------------------------------------------------------------------------------------------------------
struct GcnFusedFwd {
  bool supported = false;   // the width is one of the fused ones
  bool rows_ok = false;     // rows within kRowBytesLimit
  bool pre_ok = false;      // PRE is not asked for, or the graph allows it
  bool launch = false;      // all of these on a graph with its normalisation and nodes
  int d = 0;
  GcnAct act = GcnAct::RunTime;
  bool halo = false, pre = false;   // the template arguments
  bool own_first = false;           // a solver plan's own-first slot tables replace the handle's (LDS-staged aggregation only)
  int grid = 0, block = kFusedThreads;
  GcnKernelNames names() const {
    if (!launch) return {};
    return {"gcn_fused_fwd_kernel<" + std::to_string(d) + "," + gcn_act_name(act) + "," + gcn_tf(halo) + "," + gcn_tf(pre) + ">"};
  }
};
inline GcnFusedFwd gcn_fused_fwd_form(const TileGeom &g, int d, int act, bool pre, bool own_first) {
  GcnFusedFwd f;
  f.supported = fused_supported(d, d);
  f.rows_ok = rows_fit_32bit(g.n_nodes, d);
  f.pre_ok = !pre || fused_prescaled_supported(g, d);
  f.d = d; f.act = gcn_act_class(act); f.pre = pre;
  const bool staged = g.halo_ok && !switch_on(Switch::NoHalo);
  f.halo = pre || staged;
  f.own_first = own_first && staged;
  f.launch = g.graph && g.has_norm && f.supported && g.n_nodes > 0 && f.rows_ok && f.pre_ok;
  f.grid = fused_num_blocks(g.n_nodes);
  return f;
}

struct GcnFusedBwd {
  bool supported = false, rows_ok = false, pre_ok = false, launch = false;   // as in the forward
  int d = 0;
  GcnAct act = GcnAct::RunTime;
  bool aggregate = false, halo = false, pre = false, pair = false;           // the template arguments <D, AGG, ACT, HALO, PAIR, PRE>
  int grid = 0, block = kFusedThreads, slabs = 0;
  GcnKernelNames names() const {
    if (!launch) return {};
    return {"gcn_fused_bwd_kernel<" + std::to_string(d) + "," + gcn_tf(aggregate) + "," + gcn_act_name(act) + "," + gcn_tf(halo) + "," + gcn_tf(pair) + "," +
            gcn_tf(pre) + ">"};
  }
};
inline GcnFusedBwd gcn_fused_bwd_form(const TileGeom &g, int d, int act, bool aggregate, bool pre) {
  GcnFusedBwd f;
  f.supported = fused_supported(d, d);
  f.rows_ok = rows_fit_32bit(g.n_nodes, d);
  f.pre_ok = !pre || fused_prescaled_supported(g, d);
  f.d = d; f.act = gcn_act_class(act); f.aggregate = aggregate; f.pre = pre;
  f.halo = aggregate && (pre || (g.halo_ok_s && !switch_on(Switch::NoHalo)));   // (the dense launch never gathers)
  f.pair = fused_bwd_pairs(d);
  f.launch = g.graph && g.has_norm && f.supported && g.n_nodes > 0 && f.rows_ok && f.pre_ok;
  const int nb = fused_num_blocks(g.n_nodes);
  f.grid = f.pair ? (nb + 1) / 2 : nb;
  f.block = f.pair ? 2 * kFusedThreads : kFusedThreads;
  f.slabs = fused_num_slabs(g.n_nodes, d);
  return f;
}

// ---- a layer ---------------------------------------------------------------------------------------------------------------------------
constexpr int gcn_spmm_dp(int d) { return d <= 8 ? 8 : d <= 16 ? 16 : d <= 32 ? 32 : 64; }   // spmm_generic_kernel<DP>
constexpr bool colsum_two_stage(int64_t n) { return n > 4 * kColsumChunks; }

enum class GcnKind { Fused, AggregateFirst, MultiplyFirst };
struct GcnLayerForm {
  GcnKind kind = GcnKind::AggregateFirst;
  int din = 0, dout = 0;
  int64_t n = 0;
  int dp = 0;                      // any width: the spmm instantiation (on min(din, dout) columns)
  int nsplit = 1, parts = 1;       // multiply first: the Dense forward's split and the partial products it writes
  bool colsum_two = false;         // multiply first: the bias gradient's column sum in two stages
  bool needs_saved_agg = false, needs_x = false;   // what the pullback reads of the forward's arrays
  bool fused() const { return kind == GcnKind::Fused; }
  bool aggregate_first() const { return kind == GcnKind::AggregateFirst; }
  // the forward's one region in floats (fused: none)
  size_t fwd_floats() const { return fused() ? 0 : (size_t)n * (aggregate_first() ? (size_t)std::max(din, dout) : (size_t)dout * parts); }
  GcnKernelNames fwd_names(const TileGeom &g, int act) const {
    if (fused()) return gcn_fused_fwd_form(g, din, act, false, false).names();
    if (n == 0) return {};
    const std::string spmm = "spmm_generic_kernel<" + std::to_string(dp) + ">";
    if (aggregate_first()) return {spmm, "ngpde_dense_forward"};
    GcnKernelNames k = {"dense_forward_split"};
    if (parts > 1) k.push_back("sum_partials_kernel");
    k.push_back(spmm);
    return k;
  }
  // the pullback with dx and dbias asked for or not (the edge-weight gradient's two kernels follow either)
  GcnKernelNames bwd_names(const TileGeom &g, int act, bool dx, bool dbias) const {
    if (n == 0) return {};
    GcnKernelNames k;
    auto add = [&k](const GcnKernelNames &more) { k.insert(k.end(), more.begin(), more.end()); };
    if (fused()) {
      k.push_back("zero_bytes_kernel");
      add(gcn_fused_bwd_form(g, din, act, false, false).names());
      if (dx) add(gcn_fused_bwd_form(g, din, act, true, false).names());
      k.insert(k.end(), dbias ? 2 : 1, "reduce_slabs_kernel");
      return k;
    }
    const std::string spmm = "spmm_generic_kernel<" + std::to_string(dp) + ">";
    k.push_back("act_bwd_kernel");
    if (aggregate_first()) {
      k.push_back("dense_backward_weight");
      if (dx) add({"dense_backward_input", spmm});
      return k;
    }
    if (dbias) add(colsum_two ? GcnKernelNames{"colsum_partial_kernel", "colsum_kernel"} : GcnKernelNames{"colsum_kernel"});
    add({spmm, "dense_backward_weight"});
    if (dx) k.push_back("dense_backward_input");
    return k;
  }
};
inline GcnLayerForm gcn_layer_form(int64_t n_nodes, int din, int dout) {
  GcnLayerForm f;
  f.din = din; f.dout = dout; f.n = n_nodes;
  f.kind = fused_supported(din, dout) ? GcnKind::Fused : dout >= din ? GcnKind::AggregateFirst : GcnKind::MultiplyFirst;
  f.needs_saved_agg = dout >= din;
  f.needs_x = dout < din;
  if (f.fused()) return f;
  f.dp = gcn_spmm_dp(std::min(din, dout));
  if (f.aggregate_first()) return f;
  f.nsplit = dense_fwd_splits(n_nodes, din, dout);
  f.parts = dense_fwd_split_count(din, f.nsplit);
  f.colsum_two = colsum_two_stage(n_nodes);
  return f;
}

// ---- the workspaces (ngpde_gcn_workspace_bytes, ngpde_gcn_backward_ew_workspace_bytes and the entries carve with these) -----------------
inline float *gcn_fwd_layout(Workspace &w, const GcnLayerForm &f) { return f.fused() ? nullptr : w.take<float>(f.fwd_floats()); }

struct GcnBwdWs {
  float *slab_dw, *slab_db, *gbuf;   // fused: the weight and bias slabs of the blocks (zeroed as one span), dz W^T
  float *dz, *tmp, *partial;         // any width: dz, one [N][max] buffer, the weight pullback's slabs
  float *ew_dx, *ew_xw, *ew_nd;      // behind those when dedge_weight is asked for
};
inline void gcn_bwd_layout(Workspace &w, const GcnLayerForm &f, bool ew, GcnBwdWs &p) {
  const size_t n = (size_t)f.n;
  p = GcnBwdWs{};
  if (f.fused()) {
    const size_t nb = (size_t)fused_num_blocks(f.n);
    p.slab_dw = w.take<float>(nb * (size_t)f.din * f.dout);
    p.slab_db = w.take<float>(nb * (size_t)f.dout);
    p.gbuf = w.take<float>(n * f.din);
  } else {
    const size_t dmax = (size_t)std::max(f.din, f.dout);
    p.dz = w.take<float>(n * dmax);
    p.tmp = w.take<float>(n * dmax);
    // this region serves two users: the weight pullback's slabs (chunks x (din + 1) x dout) and, when dout < din, the two-stage
    // column sums of the bias gradient (kColsumChunks x dout) -- with narrow layers the second is the larger one
    const size_t slabs = (size_t)dense_weight_chunks(f.n, f.din, f.dout) * (f.din + 1) * f.dout;
    p.partial = w.take<float>(std::max(slabs, (size_t)kColsumChunks * f.dout));
  }
  w.take<char>(kGcnSlack);
  if (!ew) return;
  // dx (the caller may pass none), x W (dout < din: the array that entered the propagation), the per-node degree terms
  p.ew_dx = w.take<float>(n * f.din);
  p.ew_xw = w.take<float>(n * (size_t)std::min(f.din, f.dout));
  p.ew_nd = w.take<float>(n);
}
inline size_t gcn_workspace_bytes(const GcnLayerForm &f, bool backward, bool ew) {
  GcnBwdWs p;
  return backward ? measure(gcn_bwd_layout, f, ew, p) : measure(gcn_fwd_layout, f) + kGcnSlack;
}

}  // namespace ngpde
