/*
 * ngpde_mesh.h -- C ABI of libngpde_hip.so, third block: meshes from points.  The Delaunay neighbour graph of 2-D point clouds and
 * its triangles, built on the device.  Types, status codes and conventions are those of ngpde.h, which this header includes; the
 * functions here are bound by the table _lib.MESH_SIGNATURES.
 *
 * What it replaces.  The graphs of the reference's VMH tutorial are Delaunay graphs: "Neighbors for each node were selected by
 * applying Delaunay triangulation to the measurement positions. Two nodes were considered to be neighbors if they lie on the same
 * edge of at least one triangle." (docs/src/tutorials/VMH.md:53-55).  The tutorial reads the triangles from a file; a new cloud, or
 * one refined or cut with add_nodes / remove_nodes, gets its graph here without a host triangulation.
 */
#ifndef NGPDE_MESH_H
#define NGPDE_MESH_H

#include "ngpde.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the largest star: a point's Voronoi cell may have this many vertices while it is built, and a point this many neighbours */
#define NGPDE_DELAUNAY_MAX_DEGREE 2048
/* 12 * 2^-53: a decision |D| <= NGPDE_DELAUNAY_TIE_BOUND * |a||b||j| (|a| + |b| + |j|) is a tie (see Arithmetic) */
#define NGPDE_DELAUNAY_TIE_BOUND 1.3322676295501878e-15

/* ------------------------------------------------------------------------------------------------
 * The object.  points: device float [n][2] (a (2 x n) column-major matrix); graph_id: device int32 [n] or NULL (n_graphs == 1), ids
 * id_base .. id_base + n_graphs - 1.  Every graph of a batch is handled by itself; nothing crosses graphs.
 * Edges.  i and j (i != j) are joined iff some closed disk has p_i and p_j on its boundary and no other point of the graph strictly
 *   inside.  In general position this is the edge set of the Delaunay triangulation.  Where four or more points are cocircular every
 *   tied diagonal is kept: an integer lattice gives the 8-neighbour stencil.  The rule is a pure function of the points and breaks
 *   no symmetry of the cloud.  A half-plane is no disk: of three collinear points the outer two are not joined.
 * Arithmetic.  Decisions are made in double on the float coordinates, translated to the star's own point (q = p - p_i, one rounding
 *   each), without fused multiply-add.  The decision that j touches the corner of i's Voronoi cell between its neighbours a and b is
 *   the sign of the in-circle determinant
 *     D = |j|^2 (a x b) + |a|^2 (b x j) + |b|^2 (j x a),         a x b = a_x b_y - a_y b_x,
 *   evaluated as |j|^2 / 2 * w - j_x * x - j_y * y on the corner (x, y, w) = (h_a b_y - h_b a_y, h_b a_x - h_a b_x, a x b), h = |.|^2 / 2,
 *   which is computed from the two bisectors and never from earlier corners.  Each monomial of D passes at most 11 roundings, so
 *     |computed D - D| < 12 * 2^-53 * |a||b||j| (|a| + |b| + |j|)                      (derivation: csrc/delaunay_star.h).
 *   A computed margin inside that bound is a tie, and ties keep the edge: keep when in doubt.  A decision that exact arithmetic
 *   makes by more than the bound comes out right.  In a star that holds a tie, other margins within a few bounds may also be kept.
 * Symmetry.  An edge is listed iff at least one endpoint's star holds it, and both directions are always written.
 * Order.  That of ngpde_radius_graph: by point, the neighbours of a point ascending by index.  dir_out = 0 writes the neighbour
 *   to s and the point to t, dir_out = 1 the reverse.  index_base is added to every index written.
 * Triangles.  Read off the final symmetric rows WITHOUT max_edge_length.  Around each point i the neighbours are ordered
 *   counter-clockwise by an exact comparator (the half-plane of the first, then the sign of the orientation determinant in double);
 *   a neighbour j and the next one k with orient(i, j, k) > 0 and k in j's row form a triangle.  It is written once, by its smallest
 *   index, as (i, j, k) counter-clockwise, and the list is sorted lexicographically.  In general position this is the triangulation,
 *   T = 2N - 2 - h for h hull points.  TIED TRIANGLES OVERLAP: four cocircular points give all four triangles of their two diagonals.
 * max_edge_length.  +inf (or any r whose float square is inf) is no limit.  Otherwise every edge with d2 > r * r under the neighbour
 *   search's float rule (ngpde.h: sum of float squares in coordinate order, float product r * r) is dropped, and every triangle that
 *   has such an edge.  NaN and negative values are refused.
 * Refused by name with NGPDE_ERR_INVALID_ARGUMENT: a non-finite coordinate or span (the rule of ngpde_radius_graph); two coincident
 *   points of one graph (the message names the smallest such pair; found by the launch that builds the stars); a star over
 *   NGPDE_DELAUNAY_MAX_DEGREE (the message names the point).  There is no `dim`: the points are 2-D.
 * Valid: n = 0 gives nothing; a graph of 1 point no edge, of 2 points one edge; collinear points the path through them in order;
 *   none of these has a triangle.
 * Protocol.  That of ngpde_radius_graph: with s == t == NULL (tri == NULL) the call counts, *n_edges (*n_triangles; host) receives
 *   the number of directed edges (of triangles) and nothing else is written.  Otherwise the count is written, then compared with
 *   `capacity` BEFORE anything is written to s, t or tri.  Both calls synchronise `stream`; every launch, copy and sort runs on it.
 * What a call allocates.  Each call computes the stars itself: a counting call and a filling call do the work twice, and
 *   ngpde_delaunay_triangles builds the edge list again.  No handle keeps the stars in between (measured: 7 ms for
 *   16 384 points on an MI355X): a caller who passes a capacity of 6 n + 64 directed edges or 2 n triangles fills in one call
 *   whenever the cloud has no ties.  Per call: the sorted grid of the neighbour search (24 bytes a point), 12 bytes a point of row
 *   bounds and flags, 16 bytes per star entry for the keys of the symmetrising sort and its output, the sort's own temporary, and
 *   for triangles 12 bytes per directed edge; all freed before the call returns.
 * Method.  Each point computes its own star: its Voronoi cell, held as homogeneous vertices (an unbounded cell needs no bounding
 *   box), clipped by the bisector of every candidate, ring by ring around the point's cell of the neighbour search's grid, until
 *   reach(ring) / 2 exceeds the farthest vertex or the grid is exhausted.  First pass: one lane per point, 24 vertices, 6 rings.
 *   Second pass, for the points that overflow either (hull points, near-hull points, hubs): one wave per point, the cell in LDS,
 *   8 rings and then the rest of the point's graph in one sweep.
 *   The stars are symmetrised by one sort of 64-bit (point, neighbour) keys with duplicates removed.  No float atomics; the integer
 *   atomics are minima, maxima and one counter, so the bits are the same on every run.
 * There is no gradient to the positions, as with every other builder of the library.
 * ngpde_delaunay_last_passes: how many points of the calling thread's last ngpde_delaunay_graph / _triangles call finished in
 *   the first pass and how many took the second (either pointer may be NULL).  Host only; no device work.
 * ---------------------------------------------------------------------------------------------- */
int32_t ngpde_delaunay_graph(int64_t n, const float *points, const int32_t *graph_id, int32_t n_graphs, int32_t id_base,
                             float max_edge_length, int32_t dir_out, int32_t index_base, int64_t capacity, int32_t *s, int32_t *t,
                             int64_t *n_edges, ngpde_stream_t stream);
int32_t ngpde_delaunay_triangles(int64_t n, const float *points, const int32_t *graph_id, int32_t n_graphs, int32_t id_base,
                                 float max_edge_length, int32_t index_base, int64_t capacity, int32_t *tri, int64_t *n_triangles,
                                 ngpde_stream_t stream);
int32_t ngpde_delaunay_last_passes(int64_t *lane_points, int64_t *wave_points);

#ifdef __cplusplus
}
#endif

#endif /* NGPDE_MESH_H */
