/*
 * ngpde_interp.h -- C ABI of libngpde_hip.so, second block: relating TWO point sets.  Search of the k nearest / all within r
 * DATA points of every QUERY point, and k-nearest-neighbour interpolation of node features from the data points onto the
 * queries, with its pullback.  Types, status codes and conventions are those of ngpde.h, which this header includes; the
 * functions here are bound by the table _lib.INTERP_SIGNATURES.
 *
 * What it replaces.  The models of the reference live on scattered clouds that change from sample to sample (the VMH
 * tutorial's 24 simulations are "observed on different 2D grids with 3000 points", docs/src/tutorials/VMH.md:53), and a graph
 * kernel network is evaluated at discretisations it was not trained on.  Comparing a solution with data on other points,
 * putting a field on a regular grid, initialising a fine cloud from a coarse solve and carrying features across add_nodes /
 * remove_nodes all need "the k nearest data points of every query point", which upstream users write with the trees
 * GNNGraphs.knn_graph / radius_graph are built on ([UPSTREAM] NearestNeighbors.jl: knn(tree, queries, k),
 * inrange(tree, queries, r); the graph builders are re-exported at src/NeuralGraphPDE.jl:4).
 */
#ifndef NGPDE_INTERP_H
#define NGPDE_INTERP_H

#include "ngpde.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Two-set neighbour search on the device: NearestNeighbors.knn(tree, queries, k) and inrange(tree, queries, r) over the
 * tree of `points`.
 *   points          device float [n][dim] (a (dim x n) column-major matrix), dim = 1, 2 or 3: the data, which the cell grid is
 *                   built over
 *   queries         device float [m][dim]; they may lie anywhere, also far outside the data's bounding box
 *   point_graph_id, query_graph_id   device int32[n] / int32[m] or NULL (both NULL when n_graphs == 1): a query is searched among
 *                   the points of its own graph only (ids id_base .. id_base + n_graphs - 1)
 *   index_base      added to every point index written
 * The decision rule is the float rule of ngpde_radius_graph / ngpde_knn_graph, unchanged: d2 is the sum over the coordinates, in
 * order, of (q - p)^2 with every operation rounded to float and no fused multiply-add; comparisons are in float; equal
 * distances are ordered by point index.  A call with finite coordinates returns the brute-force list of that rule bit for
 * bit at every magnitude (r*r = inf connects everything, squares that round to 0 or to denormals connect what the float
 * comparison connects, distances that are all inf are ordered by index) or is refused by name: a non-finite coordinate,
 * and two sets whose union spans more than the largest finite float in a coordinate, are NGPDE_ERR_INVALID_ARGUMENT.
 * ngpde_knn_query: idx int32 [m][k] and d2 float [m][k] (nullable) receive, for every query, the k smallest (d2, index) pairs,
 *   nearest first; 0 <= k <= NGPDE_KNN_MAX_K.  A query whose graph holds fewer than k points (none included) is refused
 *   with NGPDE_ERR_INVALID_ARGUMENT and a message that names the graph; a graph with points and no queries is fine.
 * ngpde_radius_query: the count / fill protocol of ngpde_radius_graph.  With nbr == NULL the call counts: *n_found (host)
 *   receives the number of (query, point) pairs with d2 <= r*r and nothing else is written.  Otherwise ptr int32 [m + 1]
 *   receives the row bounds (0-based positions into nbr) and nbr int32 [capacity] the point indices, rows by query, the
 *   neighbours of a query ascending by index; a list longer than `capacity` is refused before ptr or nbr is written.  A query
 *   whose graph has no points, or none within r, has an empty row.
 * Both synchronise `stream`.  The neighbour positions are not differentiable and nothing here has a pullback: upstream's
 * knn / inrange give none either.
 * ---------------------------------------------------------------------------------------------- */
int32_t ngpde_knn_query(int64_t n, int64_t m, int32_t dim, const float *points, const float *queries, int32_t k,
                        const int32_t *point_graph_id, const int32_t *query_graph_id, int32_t n_graphs, int32_t id_base,
                        int32_t index_base, int32_t *idx, float *d2, ngpde_stream_t stream);
int32_t ngpde_radius_query(int64_t n, int64_t m, int32_t dim, const float *points, const float *queries, float r,
                           const int32_t *point_graph_id, const int32_t *query_graph_id, int32_t n_graphs, int32_t id_base,
                           int32_t index_base, int64_t capacity, int32_t *ptr, int32_t *nbr, int64_t *n_found,
                           ngpde_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * k-nearest-neighbour interpolation of node features: y_q = sum_j w_qj x_{idx_qj} / sum_j w_qj over the k nearest data points
 * of every query.  This is Shepard's inverse-squared-distance interpolation, the knn_interpolate of PyTorch Geometric
 * ([UPSTREAM] torch_geometric.nn.unpool.knn_interpolate: w = 1 / clamp(d2, min = 1e-16)), with one deliberate difference:
 * the weights are normalised by the NEAREST distance instead of clamped at a constant.
 *   For a query with neighbour ranks j = 0 .. k-1 (nearest first, as ngpde_knn_query writes them):
 *     c_j = max(d2_j, FLT_MIN),   w_j = c_0 / c_j,   W = sum_j w_j,   y = (sum_j w_j x_{idx_j}) / W,
 *   and every w_j = 1 where c_0 is inf.  Hence w_0 = 1, the weights do not change when all coordinates are scaled, and
 *   1 <= W <= k: nothing overflows or underflows at any coordinate scale (1 / d2 is inf below 1e-19 and 0 above 1e19, and a
 *   clamp at 1e-16 makes every point of a cloud in nanometres coincident).  Data points that coincide with the query (d2 = 0)
 *   share the value equally, and the others then weigh FLT_MIN / d2.
 *   Both sums run in ascending j from 0.f without fused multiply-add.  ngpde_knn_interp_weights writes the NORMALISED weights
 *   w_j / W, [m][k]; the forward is the plain weighted sum with them, y_q = sum_j w[q][j] * x[idx[q][j]] in ascending j from 0.f,
 *   and the backward is exactly its transpose.
 * There is no gradient to the positions (points, queries): idx is piecewise constant, and the weights are taken as constants
 * of the interpolation operator, as upstream's knn gives no gradient either.
 *   d2      device float [m][k], ascending per query           w     device float [m][k]
 *   idx     device int32 [m][k], 0-based point indices (ngpde_knn_query with index_base 0); an entry outside 0 : n-1
 *           contributes nothing
 *   x       device float [n][d] (a (d x n) column-major matrix)  y     device float [m][d]
 *   ybar    device float [m][d]                                  xbar  device float [n][d], overwritten
 * Forward: lanes run over the features of a row, so a neighbour's row is one coalesced read; idx and w of a query are read once
 * by the lanes of that query and handed round; 64 / (d rounded up to a power of two) queries share a wave when d < 64; any d >= 1.
 * Transpose: the by-point rows of idx -- ptr int32 [n + 1], slot int32 [m * k]: slot[ptr[i] : ptr[i+1]] are the positions
 * q * k + j with idx[q][j] == i, ascending -- built with one stable sort of the positions by point.  `workspace` is device memory
 * of ngpde_knn_interp_transpose_workspace_bytes(n, m, k) bytes (0 when a size is negative or m * k exceeds int32); the call
 * allocates the sort's own temporary and synchronises `stream`, so it is made once per search, not per step.
 * Backward: xbar_i = sum over the slots of point i of w[slot] * ybar[slot / k], without atomics: one wave per point, the lanes
 * laid out (slot, feature) as the library's other row reductions are (64 / d' slots at once for d' = d rounded up to a power of
 * two, so a point that hundreds of queries name is not walked by single lanes when d is small); every slot lane sums its slots in
 * ascending order and the partial sums are combined by a fixed butterfly, so the result is bitwise reproducible from run to run; with
 * one slot lane (d > 32) it is the plain sum in ascending slot order.  A point no query names gets an explicit 0.
 * ngpde_knn_interp_weights, _forward and _backward only enqueue work on `stream`: they allocate nothing and read nothing back,
 * so they replay from a HIP graph.
 * ---------------------------------------------------------------------------------------------- */
int32_t ngpde_knn_interp_weights(int64_t m, int32_t k, const float *d2, float *w, ngpde_stream_t stream);
int32_t ngpde_knn_interp_forward(int64_t n, int64_t m, int32_t k, int32_t d, const int32_t *idx, const float *w, const float *x,
                                 float *y, ngpde_stream_t stream);
size_t ngpde_knn_interp_transpose_workspace_bytes(int64_t n, int64_t m, int32_t k);
int32_t ngpde_knn_interp_transpose(int64_t n, int64_t m, int32_t k, const int32_t *idx, int32_t *ptr, int32_t *slot, void *workspace,
                                   size_t workspace_bytes, ngpde_stream_t stream);
int32_t ngpde_knn_interp_backward(int64_t n, int64_t m, int32_t k, int32_t d, const int32_t *ptr, const int32_t *slot, const float *w,
                                  const float *ybar, float *xbar, ngpde_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NGPDE_INTERP_H */
