// neighbor_cells.h -- the neighbour search's sorted cell grid (neighbors.hip) for another translation unit of the library:
// delaunay.hip walks the same (graph, cell)-sorted points ring by ring.  The one definition of the box, the grid sizing and the sort
// stays in neighbors.hip; this is its declaration.
#pragma once
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "neighbor_grid.h"

namespace ngpde {

struct PointCells {
  unsigned *key = nullptr;    // [n] sorted (graph, cell) keys: graph * g.cells + cell
  int32_t *idx = nullptr;     // [n] original index per sorted position
  float *pts = nullptr;       // [n][2] points in sorted order
  int32_t *start = nullptr;   // [n_graphs * g.cells + 1] first sorted position of every cell
};

// Boxes the 2-D points (refusing a bad graph id, a non-finite coordinate and a non-finite span by name), sizes the grid for
// about k / 2 points per cell as the k-NN search does, and sorts the points into it.  The device arrays are appended to `owned`,
// which the caller frees with hipFree.  Synchronises `stream` once (the box is read back).
int32_t point_cells_2d(int64_t n, const float *pts, const int32_t *gid, int n_graphs, int id_base, int k, hipStream_t stream,
                       std::vector<void *> &owned, Grid *g, PointCells *out);

}  // namespace ngpde
