/*
 * ngpde_coarsen.h -- C ABI of libngpde_hip.so, fourth block: choosing the COARSE cloud.  Farthest-point sampling, grid clusters and
 * pooling of node features over clusters, with its pullback.  Types, status codes and conventions are those of ngpde.h, which this
 * header includes; the functions here are bound by the table _lib.COARSEN_SIGNATURES.
 *
 * What it completes.  The library makes a graph from points (ngpde_radius_graph, ngpde_knn_graph, ngpde_delaunay_graph), cuts one
 * (remove_nodes, induced_subgraph) and carries a field from one cloud to another (ngpde_interp.h: "initialising a fine cloud from a
 * coarse solve").  These entries choose the coarse cloud on the device: the operations PyTorch Geometric users know as fps,
 * voxel_grid and avg_pool / max_pool, of which knn_interpolate (ngpde_interp.h) is the "unpool".
 */
#ifndef NGPDE_COARSEN_H
#define NGPDE_COARSEN_H

#include "ngpde.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------------
 * Farthest-point sampling of every graph of a batch.
 *
 * THE RULE, a pure function of its arguments that treats every graph by itself.  For a graph with the points lo .. hi-1 and k
 * samples every point has a key: +inf at first, -1.f once the point has been selected.  Round r = 0 .. k-1
 *   1. selects s_r: for r = 0 the graph's start point, otherwise the point with the LARGEST KEY, equal keys going to the SMALLEST
 *      INDEX;
 *   2. writes idx[r] = s_r and d2[r] = the key s_r had when it was selected, i.e. its squared distance to the set chosen so far
 *      (d2[0] = +inf; d2[k-1] bounds the covering radius of the sample);
 *   3. sets key[s_r] = -1 and key[i] = min(key[i], d2(p_i, p_{s_r})) for every unselected i.
 * d2 is the neighbour search's float rule, unchanged: the sum over the coordinates, in order, of (p - q)^2, every operation rounded
 * to float, no fused multiply-add.  Hence a selected point is never selected twice, coincident points are taken in index order
 * once all keys are 0, and squares that round to 0, to denormals or to inf select what the float comparison selects.  Selection
 * order makes the results nested: the first a samples of a call with k = b > a are the call with k = a at the same start.
 *
 * The plan.  The host must know the sizes to lay the work out, so the call is split as ngpde_readout_create is:
 *   graph_ptr, sample_ptr   HOST int64 [n_graphs + 1]: graph g holds the points graph_ptr[g] : graph_ptr[g+1]-1 and receives
 *                           sample_ptr[g+1] - sample_ptr[g] samples at idx[sample_ptr[g] ...].  Both start at 0 and are
 *                           non-decreasing; more samples than points, a graph_ptr beyond 2^31 - 1, dim outside 1:3 and a path
 *                           outside 0:2 are NGPDE_ERR_INVALID_ARGUMENT with a message that names the graph (0-based) -- all
 *                           found BEFORE any device call.  Empty graphs and graphs without samples are fine.
 *   path                    0 auto, 1 the tile path for every graph, 2 the round path for every graph.  A plan created with 1
 *                           for a graph of more than NGPDE_FPS_TILE_MAX_POINTS points is refused by name.  Auto sends a graph
 *                           to the tile path iff it fits; a batch may use both paths in one call.
 * ngpde_fps_plan_create builds the plan's device tables (it allocates and synchronises `stream`); ngpde_fps_plan_info writes
 * info[0..5] = points, samples, graphs on the tile path, graphs on the round path (graphs with work: k > 0), launches of the round
 * path in one ngpde_fps call (the largest k of its graphs), launches of the tile path (one per occupied size class).
 *
 * TWO KERNELS, BITWISE EQUAL to each other and to the rule.
 *   Tile path: one workgroup of NGPDE_FPS_TILE_THREADS threads per graph, the whole graph resident in registers (thread t owns the
 *   points t, t + W, t + 2W ...: 1, 4 or 16 per thread by the graph's size), all k rounds inside one launch.  A thread updates its
 *   keys and keeps its best (key, index) under "larger key, then smaller index"; a wave reduces by shuffles; the waves' results
 *   cross through a double-buffered LDS slot, so a round costs one workgroup barrier.  Nothing waits on another workgroup.
 *   Round path: one launch per round over all its graphs, max k_g launches enqueued back to back.  A graph is cut into slices of
 *   2 048 points, one workgroup each; a workgroup first reduces the previous round's per-slice partials of its graph (redundantly;
 *   the comparison is a total order, so the shape of the reduction does not matter) to learn s_r, the graph's first workgroup
 *   writes idx[r] and d2[r], then each updates the keys of its slice in the workspace and writes its partial into the other half
 *   of a double buffer.  No atomics; no launch depends on the host.
 *
 * ngpde_fps
 *   points   device float [n][dim] (a (dim x n) column-major matrix), finite
 *   start    device int32 [n_graphs] or NULL: the start position of every graph (a global position, index_base added); NULL is
 *            every graph's first point.  PRECONDITION: a start inside its graph.  An entry outside is clamped into its graph by
 *            the kernel: the call stays memory-safe and samples from the clamped point.
 *   idx      device int32 [samples]: global positions + index_base, graphs concatenated, each graph's in selection order
 *   d2       device float [samples] or NULL
 *   workspace  device memory of ngpde_fps_workspace_bytes(plan) bytes (0 when no graph takes the round path; then NULL is fine)
 * It only enqueues on `stream`: it allocates nothing, reads nothing back, and replays from a HIP graph.
 * ---------------------------------------------------------------------------------------------- */
#define NGPDE_FPS_TILE_THREADS 1024
#define NGPDE_FPS_TILE_MAX_POINTS 16384

typedef struct ngpde_fps_plan ngpde_fps_plan_t;

int32_t ngpde_fps_plan_create(int32_t n_graphs, const int64_t *graph_ptr, const int64_t *sample_ptr, int32_t dim, int32_t path,
                              ngpde_stream_t stream, ngpde_fps_plan_t **plan);
int32_t ngpde_fps_plan_destroy(ngpde_fps_plan_t *plan);
int32_t ngpde_fps_plan_info(const ngpde_fps_plan_t *plan, int64_t *info);
size_t ngpde_fps_workspace_bytes(const ngpde_fps_plan_t *plan);
int32_t ngpde_fps(const ngpde_fps_plan_t *plan, const float *points, const int32_t *start, int32_t index_base, int32_t *idx, float *d2,
                  void *workspace, size_t workspace_bytes, ngpde_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Grid clusters: two points share a cluster iff they share graph and cell.
 *
 * THE RULE.  The cell of a point is c_d = (int32) floorf((p_d - o_d) / size_d) per coordinate: one float subtraction and one
 * correctly rounded float division.  o is `origin` (HOST float [dim]) for all graphs, or with origin == NULL the minimum of the
 * graph's OWN points per coordinate, so that a graph clusters the same way alone or inside a batch.  Clusters are numbered by
 * ascending key (graph, c_z, c_y, c_x), x fastest: labels are non-decreasing in the graph, and the coarse set is again a batch.
 * The key packs the cells into bit fields as wide as the cloud's largest cell of each coordinate needs, under the graph's; a key
 * that does not fit 63 bits (and a cell beyond int32) is refused by name: "cell size too small for the cloud's extent".  A
 * non-finite coordinate and a point below an explicit origin are refused with the position of the first such point.
 *   points         device float [n][dim], dim 1:3          graph_ptr   HOST int64 [n_graphs + 1], from 0 to n, non-decreasing
 *   size           HOST float [dim], finite and > 0
 *   labels         device int32 [n]: the cluster of every point, 0-based
 *   ptr            device int32 [n + 1]: the first *n_clusters + 1 entries are the row bounds of `order`
 *   order          device int32 [n]: the members of every cluster, ascending by node
 *   cluster_graph  device int32 [n]: the first *n_clusters entries are the clusters' graphs, 1-BASED
 *   n_clusters     HOST int64
 * One launch finds the cells' extents and the refusals (one read-back), one writes the keys, then one stable radix sort and a
 * head-flag scan.  What a call allocates it frees before it returns; it synchronises `stream`.
 * ---------------------------------------------------------------------------------------------- */
int32_t ngpde_grid_cluster(int64_t n, int32_t dim, const float *points, int32_t n_graphs, const int64_t *graph_ptr, const float *size,
                           const float *origin, int32_t *labels, int32_t *ptr, int32_t *order, int32_t *cluster_graph,
                           int64_t *n_clusters, ngpde_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Pooling over clusters: out_c = aggr over the members i of cluster c of x_i, aggr = NGPDE_AGGR_SUM / MEAN / MAX / MIN.
 *   ptr, order   device int32 [c + 1] / [n]: the by-cluster rows (ngpde_grid_cluster, or ngpde_knn_interp_transpose with k = 1 of
 *                user labels); an entry of order outside 0 : n-1 contributes nothing
 *   labels       device int32 [n]                x, dx   device float [n][d] (a (d x n) column-major matrix), any d >= 1
 *   out, dout    device float [c][d]
 * ORDER CONTRACT.  One wave per cluster, its lanes laid out (slot, column) as the library's other row reductions are (64 / d' slot
 * lanes for d' = d rounded up to a power of two, at most 64): every slot lane adds its members in ascending node order from 0.f
 * and the partials combine by the fixed xor butterfly; MEAN divides that sum by (float)count.  With one slot lane (d > 32) it is
 * the plain ascending sum.  No atomics: the same bits every run.  An empty cluster gives 0 (SUM, MEAN), -inf (MAX), +inf (MIN).
 * The pullback is one gather launch: dx_i = dout[label_i]; for MEAN dout[label_i] / (float)count; for MAX / MIN the gradient goes
 * where x_i == out[label_i] -- to EVERY tied entry, the convention of ngpde_readout_reduce_backward.  A label outside 0 : c-1
 * gives 0.  Both only enqueue on `stream`: they allocate nothing, read nothing back, and replay from a HIP graph.
 * ---------------------------------------------------------------------------------------------- */
int32_t ngpde_cluster_pool_forward(int64_t n, int64_t c, int32_t d, int32_t aggr, const int32_t *ptr, const int32_t *order, const float *x,
                                   float *out, ngpde_stream_t stream);
int32_t ngpde_cluster_pool_backward(int64_t n, int64_t c, int32_t d, int32_t aggr, const int32_t *labels, const int32_t *ptr,
                                    const float *x, const float *out, const float *dout, float *dx, ngpde_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* NGPDE_COARSEN_H */
