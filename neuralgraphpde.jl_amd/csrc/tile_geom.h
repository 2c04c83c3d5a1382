// tile_geom.h -- the tile schedule's constants and all that a choice of kernels reads of a graph handle (host only, plain C++17: no
// HIP).  Every tiled kernel of the library counts in these; the forms headers (edge_mlp_forms.h, gcn_forms.h, gat_forms.h) decide
// on a TileGeom, never on the handle, so that their stand-alone check programs can state a graph in a line of integers.
#pragma once

#include <cstdint>

namespace ngpde {

constexpr int kTileRows = 32;   // node rows per workgroup of the fused kernels
constexpr int kHaloCap = 96;    // unique rows a tile may stage in LDS (24 KB at D = 64), plus one zero row
constexpr int kSlotWidth = 32;  // slot bytes per row of the LDS-staged aggregation (rows with more: global gather)
constexpr int kEllWidth = 16;   // entries per row held in the fixed-width block (rows with more spill to the CSR list)

// tile_geom(g) in common.h fills it; a NULL handle gives the default
struct TileGeom {
  bool graph = false, has_norm = false;
  bool halo_ok = false;     // every by-target tile fits: <= kHaloCap distinct rows, degrees <= kSlotWidth
  bool halo_ok_s = false;   // ... every by-source tile
  bool self_loops = false;  // the normalisation adds them
  int max_halo = 0, n_tiles = 0;   // by target: the largest halo; tiles of the schedule
  int64_t n_nodes = 0, n_edges = 0;
};

}  // namespace ngpde
