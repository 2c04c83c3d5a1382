// gat_forms.h -- which kernels every GATConv call runs, decided in one place (host only, plain C++17: no HIP).
//
// The family behind ngpde_gat_forward / _backward, ngpde_gat_layer_* and the host half of ngpde_node_gat_supported picks its kernels
// from heads, c = channels per head, the graph's tile geometry (TileGeom, tile_geom.h) and three switches.  As in gcn_forms.h every
// choice is a pure function that returns a small plain struct, the launchers (mp_kernels.hip, gcn_fused.hip, gat_fused.hip) and
// entries (api_mp.hip) execute it, and tests/host/gcn_gat_forms_check.cpp prints it for tests/test_gcn_gat_forms_host.py to compare
// with tests/gcn_gat_forms_spec.py.  No function here touches the device or dereferences a data pointer.
//
// The aggregation primitive's forward (gat_fwd_form), in this order:
//   tiled     gat_fused_fwd_kernel            heads * c == 64, heads in {1, 2, 4}, the normalisation set (the handle has its tile
//                                             schedule), every by-target tile fits, rows within 2^32 bytes; NGPDE_NO_FUSED_GAT unset
//   blocked   gat_fwd_blocked_kernel<H>       heads in {1, 2, 4, 8, 16}, heads * c <= 256
//   row       gat_fwd_kernel                  everything else (a wave per row)
// Its pullback (gat_bwd_form):
//   blocked   gat_bwd_target_blocked_kernel<H>, gat_bwd_source_blocked_kernel<H>   the blocked shape, c % 4 == 0, wx and dout on
//                                             16-byte boundaries (one presence bit here, not the pointers)
//   row       gat_bwd_target_kernel, gat_bwd_source_kernel
//   then gat_scores_bwd_dwx_kernel and gat_scores_bwd_da_kernel.
// The one-launch layer (gat_layer_form): gat_layer_fwd_kernel<H>; gat_layer_bwd_target_kernel<H> on one workgroup per tile,
// gat_layer_bwd_source_kernel<H> on one per kGatSrcTiles tiles, gat_layer_reduce_kernel.  din == heads * c == 64, heads in {1, 2, 4},
// the normalisation set, at least one edge, every tile fits in BOTH directions, rows within 2^32 bytes; NGPDE_NO_FUSED_GAT_LAYER not 1.
// The resident solver (gat_node_host_supported): the layer's conditions and NGPDE_NO_PERSISTENT not 1; what it asks of the device
// after that (residency, wait lists, equal schedules) stays in gat_fused.hip.
// Asymmetries, kept: the tiled primitive needs has_norm though it normalises nothing; it does NOT need an edge, the layer does; the
// primitive reads only NGPDE_NO_FUSED_GAT (on when set at all) and the layer only NGPDE_NO_FUSED_GAT_LAYER (on when 1); neither
// reads NGPDE_NO_HALO.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "gcn_forms.h"

namespace ngpde {

// ---- the family's constants ---------------------------------------------------------------------------------------------------------
constexpr int kGatWidth = 64;           // tiled forward and layer: heads * c (gat_fused.hip: GD)
constexpr int kGatSrcTiles = 2;         // tiles per workgroup of the layer's by-source pullback launch (dW accumulators stay in registers)
constexpr int kGatBlockedMax = 256;     // blocked<H>: heads * c at most

using GatKernelNames = std::vector<std::string>;

constexpr bool gat_tile_heads(int heads) { return heads == 1 || heads == 2 || heads == 4; }
constexpr bool gat_blocked_shape(int heads, int c) {
  return heads * c <= kGatBlockedMax && (heads == 1 || heads == 2 || heads == 4 || heads == 8 || heads == 16);
}

// ---- the aggregation primitives -------------------------------------------------------------------------------------------------------
inline bool gat_tiled_supported(const TileGeom &g, int heads, int c) {
  return g.graph && g.has_norm && g.halo_ok && heads * c == kGatWidth && gat_tile_heads(heads) && rows_fit_32bit(g.n_nodes, kGatWidth);
}
enum class GatForm { Tiled, Blocked, Row };
struct GatFwd {
  GatForm form = GatForm::Row;
  int heads = 0;          // Blocked: <H>
  bool launch = false;    // the graph has nodes
  GatKernelNames names() const {
    if (!launch) return {};
    if (form == GatForm::Tiled) return {"gat_fused_fwd_kernel"};
    if (form == GatForm::Blocked) return {"gat_fwd_blocked_kernel<" + std::to_string(heads) + ">"};
    return {"gat_fwd_kernel"};
  }
};
inline GatFwd gat_fwd_form(const TileGeom &g, int heads, int c) {
  GatFwd f;
  f.heads = heads;
  f.launch = g.n_nodes > 0;
  f.form = (!switch_on(Switch::NoFusedGat) && gat_tiled_supported(g, heads, c)) ? GatForm::Tiled : gat_blocked_shape(heads, c) ? GatForm::Blocked : GatForm::Row;
  return f;
}
struct GatBwd {
  GatForm form = GatForm::Row;   // Blocked or Row
  int heads = 0;
  bool launch = false;
  GatKernelNames names() const {
    if (!launch) return {};
    const std::string h = "<" + std::to_string(heads) + ">";
    GatKernelNames k = form == GatForm::Blocked ? GatKernelNames{"gat_bwd_target_blocked_kernel" + h, "gat_bwd_source_blocked_kernel" + h}
                                               : GatKernelNames{"gat_bwd_target_kernel", "gat_bwd_source_kernel"};
    k.insert(k.end(), {"gat_scores_bwd_dwx_kernel", "gat_scores_bwd_da_kernel"});
    return k;
  }
};
// aligned: wx and dout both on 16-byte boundaries
inline GatBwd gat_bwd_form(const TileGeom &g, int heads, int c, bool aligned) {
  GatBwd f;
  f.heads = heads;
  f.launch = g.n_nodes > 0;
  f.form = (gat_blocked_shape(heads, c) && c % 4 == 0 && aligned) ? GatForm::Blocked : GatForm::Row;
  return f;
}
// the primitives' pullback workspace: the edges' score gradients, the two per-node score gradients
struct GatBwdWs {
  float *dscore, *dal, *dar;
};
inline void gat_bwd_layout(Workspace &w, const TileGeom &g, int heads, GatBwdWs &p) {
  p.dscore = w.take<float>((size_t)std::max<int64_t>(g.n_edges, 1) * heads);
  p.dal = w.take<float>((size_t)std::max<int64_t>(g.n_nodes, 1) * heads);
  p.dar = w.take<float>((size_t)std::max<int64_t>(g.n_nodes, 1) * heads);
}

// ---- the one-launch layer -------------------------------------------------------------------------------------------------------------
struct GatLayer {
  bool supported = false;
  int h = 4;                        // the <H> instantiation: 1, 2, else 4
  int n_tiles = 0, src_wgs = 0;     // grids: forward and by-target pullback; by-source pullback
  int64_t n = 0;
  GatKernelNames fwd_names() const {
    if (!supported || n == 0) return {};
    return {"gat_layer_fwd_kernel<" + std::to_string(h) + ">"};
  }
  GatKernelNames bwd_names() const {
    if (!supported) return {};
    const std::string hh = "<" + std::to_string(h) + ">";
    if (n == 0) return {"gat_layer_reduce_kernel"};
    return {"gat_layer_bwd_target_kernel" + hh, "gat_layer_bwd_source_kernel" + hh, "gat_layer_reduce_kernel"};
  }
};
inline bool gat_layer_fused_supported(const TileGeom &g, int din, int heads, int c) {
  return g.graph && g.has_norm && g.n_edges > 0 && g.halo_ok && g.halo_ok_s && din == kGatWidth && heads * c == kGatWidth && gat_tile_heads(heads) &&
         rows_fit_32bit(g.n_nodes, kGatWidth) && !switch_on(Switch::NoFusedGatLayer);
}
inline GatLayer gat_layer_form(const TileGeom &g, int din, int heads, int c) {
  GatLayer f;
  f.supported = gat_layer_fused_supported(g, din, heads, c);
  f.h = heads == 1 || heads == 2 ? heads : 4;
  f.n = g.n_nodes;
  f.n_tiles = fused_num_blocks(g.n_nodes);
  f.src_wgs = (f.n_tiles + kGatSrcTiles - 1) / kGatSrcTiles;
  return f;
}
inline bool gat_node_host_supported(const TileGeom &g, int heads, int c) {
  return !switch_on(Switch::NoPersistent) && gat_layer_fused_supported(g, kGatWidth, heads, c);
}
struct GatLayerBwdWs {   // the pieces of the caller's pullback workspace
  float *dz, *dscore, *dal, *slab_db, *slab_dw, *slab_u;
};
inline void gat_layer_bwd_layout(Workspace &w, const TileGeom &g, int heads, GatLayerBwdWs &p) {
  const GatLayer f = gat_layer_form(g, kGatWidth, heads, 0);   // (the grids depend on the graph alone)
  p.dz = w.take<float>((size_t)g.n_nodes * kGatWidth);
  p.dscore = w.take<float>((size_t)std::max<int64_t>(g.n_edges, 1) * heads);
  p.dal = w.take<float>((size_t)g.n_nodes * heads);
  p.slab_db = w.take<float>((size_t)f.n_tiles * kGatWidth);
  p.slab_dw = w.take<float>((size_t)f.src_wgs * kGatWidth * kGatWidth);
  p.slab_u = w.take<float>((size_t)f.src_wgs * 2 * kGatWidth);
}
inline size_t gat_layer_workspace_bytes(const TileGeom &g, int heads) {
  GatLayerBwdWs p;
  return g.graph ? measure(gat_layer_bwd_layout, g, heads, p) : 0;
}

}  // namespace ngpde
