/*
 * ngpde.h -- C ABI of libngpde_hip.so: the MI355X (gfx950) implementation of the message-passing
 * hot path of NeuralGraphPDE.jl (edge gather -> per-edge function -> node scatter-reduce, plus the
 * dense node-feature x weight contraction), i.e. what a Julia `ccall` shim replacing the bodies of
 * /root/reference/src/layers.jl would bind.  See INTEGRATION.md for the reference-side binding.
 *
 * Conventions
 *   - Every function returns an int32 status (0 = NGPDE_OK, < 0 = error); the message of the last
 *     error on the calling thread is returned by ngpde_last_error().  No C++ exception or abort()
 *     crosses this boundary.  The reference raises AssertionError / DimensionMismatch at the same
 *     places (src/layers.jl:204,207,216 and GNNGraph's check_num_nodes/edges).
 *   - All tensor arguments are raw DEVICE pointers to float32 unless a parameter is documented as
 *     "host".  A Julia (D x N) column-major matrix is passed as-is: it is the row-major [N][D]
 *     array the kernels use (node n = D contiguous floats).  A weight (out x in) column-major is
 *     the row-major [in][out] array.
 *   - `stream` is a hipStream_t (NULL = the default stream).  Forward/backward calls only enqueue
 *     work; they never allocate, free or synchronise (graph-capture safe).  Handle creation is
 *     synchronous.
 *   - Creates.  A create call that has no stream parameter (ngpde_node_gcn2_create*, ngpde_node_gat_create*,
 *     ngpde_node_vmh_create, ngpde_ode_create) does its device work on the NULL stream, which is NOT ordered with
 *     streams created hipStreamNonBlocking (torch's, AMDGPU.jl's).  Device arrays passed to such a call (`pos`) must
 *     therefore be complete when it is called -- synchronise the stream that produces them first -- and the call
 *     returns with its own device work complete: the plan may be used on any stream at once.
 *   - The library keeps no hidden parameter state: parameters and inputs are passed on every call,
 *     as in Lux's `y, st = layer(x, ps, st)` (src/layers.jl:200, :94, :312, :390, :509).  The only
 *     cached object is the derived-graph handle, whose life is tied to the GNNGraph in `st.graph`.
 */
#ifndef NGPDE_H
#define NGPDE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGPDE_VERSION_STRING "0.1.0"

typedef struct ngpde_graph ngpde_graph_t;     /* derived graph: CSR by target + CSR by source  */
typedef struct ngpde_node ngpde_node_t;       /* fixed-step neural-ODE plan over 2 x GCNConv   */
typedef struct ngpde_node_gat ngpde_node_gat_t; /* fixed-step neural-ODE plan over one GAT-style layer */
typedef struct ngpde_node_vmh ngpde_node_vmh_t; /* fixed-step neural-ODE plan over VMHConv(phi, gamma) */
typedef void *ngpde_stream_t;                 /* hipStream_t                                   */

typedef enum {
  NGPDE_OK = 0,
  NGPDE_ERR_INVALID_ARGUMENT = -1,   /* Julia: ArgumentError / AssertionError */
  NGPDE_ERR_DIMENSION_MISMATCH = -2, /* Julia: DimensionMismatch              */
  NGPDE_ERR_HIP = -3,                /* a HIP runtime call failed             */
  NGPDE_ERR_UNSUPPORTED = -4,        /* shape/option outside what is built    */
  NGPDE_ERR_WORKSPACE = -5,          /* caller workspace too small            */
  NGPDE_ERR_STATE = -6               /* call order violated (e.g. norm not set, backward before forward) */
} ngpde_status_t;

/* NNlib activation names used by the reference's layers (src/layers.jl:180, Lux Dense).  exp / log / reciprocal are the
 * hardware v_exp_f32 / v_log_f32 / v_rcp_f32 (1 ulp): tanh, sigmoid, swish, gelu (tanh form, as NNlib 0.8), elu and softplus
 * are within ~2e-7 absolute of the libm forms, two orders below the parity tolerance of 1e-4. */
typedef enum {
  NGPDE_ACT_IDENTITY = 0, NGPDE_ACT_RELU = 1, NGPDE_ACT_TANH = 2, NGPDE_ACT_SIGMOID = 3,
  NGPDE_ACT_SWISH = 4, NGPDE_ACT_GELU = 5, NGPDE_ACT_LEAKYRELU = 6, NGPDE_ACT_ELU = 7,
  NGPDE_ACT_SOFTPLUS = 8
} ngpde_act_t;

/* `aggr` of propagate(...): +, mean, max, min, * (src/layers.jl:49,257,348,441; fields :90,303,384,496; default mean).
 * The product of an empty neighbourhood is 1 (NNlib scatter(*) starts from the neutral element); its pullback gives every
 * entry the product of the others.  The fused message kernel (ngpde_edge_mlp_forward) takes the first four. */
typedef enum { NGPDE_AGGR_SUM = 0, NGPDE_AGGR_MEAN = 1, NGPDE_AGGR_MAX = 2, NGPDE_AGGR_MIN = 3, NGPDE_AGGR_MUL = 4 } ngpde_aggr_t;

typedef enum { NGPDE_TABLEAU_EULER = 0, NGPDE_TABLEAU_TSIT5 = 1 } ngpde_tableau_t;

const char *ngpde_version(void);
const char *ngpde_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Derived-graph handle.  Replaces what the reference recomputes on EVERY layer call:
 * add_self_loops (src/layers.jl:211), degree (:224) and, inside propagate [GraphNeuralNetworks.jl],
 * the COO -> sparse-matrix build / gather+scatter index walk (:228-232, :111, :326, :416, :534).
 *   s, t        host, int64, length n_edges, the COO vectors of the GNNGraph (edge e: s[e] -> t[e])
 *   index_base  1 for the vectors a Julia GNNGraph holds, 0 for 0-based callers
 *   n_graphs    number of graphs of a batched (block-diagonal) GNNGraph (test/runtests.jl:89-102)
 * The handle is immutable after ngpde_graph_set_gcn_norm and may be shared across streams.
 * ---------------------------------------------------------------------------------------------- */
int32_t ngpde_graph_create(int64_t n_nodes, int64_t n_edges, const int64_t *s, const int64_t *t,
                           int32_t index_base, int32_t n_graphs, ngpde_graph_t **out);
/* The same handle built ON THE DEVICE from a COO list already in HBM (the reference moves the graph with `g |> gpu`
 * and swaps it every minibatch, docs/src/tutorials/VMH.md:132-134 + src/utils.jl:24-31): s, t are DEVICE arrays of
 * int32 or int64 (index_bits) with the given index_base.  `order` (device, n_nodes int32, nullable) is a node
 * permutation to use as the locality schedule -- e.g. the concatenated cached orders of a batch's member graphs,
 * see ngpde_graph_node_order; when NULL the lists are downloaded once and the order is computed on the host.
 * Every derived array is bit-identical to ngpde_graph_create's for the same edge list and order. Synchronises `stream`. */
int32_t ngpde_graph_create_device(int64_t n_nodes, int64_t n_edges, const void *s, const void *t, int32_t index_bits,
                                  int32_t index_base, int32_t n_graphs, const int32_t *order, ngpde_stream_t stream,
                                  ngpde_graph_t **out);
/* the handle's locality order (host buffer of n_nodes int32): cache it per graph, offset + concatenate it for batches */
int32_t ngpde_graph_node_order(const ngpde_graph_t *g, int32_t *order_out);
/* ngpde_graph_set_gcn_norm with DEVICE edge weights, built on the device (any handle) */
int32_t ngpde_graph_set_gcn_norm_device(ngpde_graph_t *g, int32_t add_self_loops, const float *edge_weight,
                                        int32_t weighted_degree, ngpde_stream_t stream);
/* Introspection of the derived arrays (device pointers; tests compare the host and device builders with it).
 * direction 0 = lists by target, 1 = by source. For NGPDE_GRAPH_HALO_OK *bytes is 1/0 and *ptr NULL. */
enum {
  NGPDE_GRAPH_ROWPTR = 0, NGPDE_GRAPH_COL = 1, NGPDE_GRAPH_EID = 2, NGPDE_GRAPH_XPOS = 3, NGPDE_GRAPH_ENT = 4,
  NGPDE_GRAPH_SCHED = 5, NGPDE_GRAPH_ELL = 6, NGPDE_GRAPH_HALO = 7, NGPDE_GRAPH_TILE_INFO = 8, NGPDE_GRAPH_SLOTS = 9,
  NGPDE_GRAPH_SLOT_W = 10, NGPDE_GRAPH_C = 11, NGPDE_GRAPH_ORDER = 12, NGPDE_GRAPH_HALO_OK = 13
};
int32_t ngpde_graph_array(const ngpde_graph_t *g, int32_t direction, int32_t which, const void **ptr, size_t *bytes);
int32_t ngpde_graph_destroy(ngpde_graph_t *g);
int32_t ngpde_graph_info(const ngpde_graph_t *g, int64_t *n_nodes, int64_t *n_edges, int32_t *n_graphs);
/* ------------------------------------------------------------------------------------------------
 * Neighbour search on the device: the COO lists that GNNGraphs.radius_graph(points, r; graph_indicator, self_loops, dir)
 * and knn_graph(points, k; ...) build on the host with NearestNeighbors.jl trees ([UPSTREAM] GraphNeuralNetworks.jl,
 * re-exported at src/NeuralGraphPDE.jl:4); the BASELINE workloads C2 and C5 are such graphs.
 *   points     device float, (dim x n) column-major = [n][dim], dim = 1, 2 or 3
 *   graph_id   device int32[n] or NULL: only points of the same graph are connected (ids id_base .. id_base+n_graphs-1)
 *   dir_out    0 = dir :in (neighbours are the sources, the point is the target; the default), 1 = :out
 *   s, t       device int32 outputs with index_base added, ordered by point; the neighbours of a point ascending by index
 *              (radius graph) or by (distance, index) (k-NN).  The reference's edge order is the tree's traversal order;
 *              the edge SET is the same.
 * Distances are sums of float squares in coordinate order without fused multiply-add; a pair is connected iff
 * d2 <= r*r (float).  ngpde_radius_graph with s == t == NULL only counts; otherwise `capacity` entries are available and
 * *n_edges (host) receives the number written.  k-NN writes exactly n*k entries; coincident points are ordered by index
 * (the reference keeps a point's own entry only while it is among the k+1 nearest).  Both synchronise `stream`.
 * The float rule holds at every magnitude: a call with finite coordinates and a valid r or k returns the brute-force list
 * of that rule or is refused by name.  Where r*r is inf (r = inf, or a finite r above 1.8e19) every pair of a graph is
 * connected; where r*r and the squares round to 0 or to denormals (below ~1e-19) d2 <= r*r connects pairs further apart
 * than r, all of them once both sides are 0; k-NN orders distances that are all 0 or all inf by index.  Points whose
 * span max - min is not finite in some coordinate (e.g. -3e38 .. 3e38) are refused with NGPDE_ERR_INVALID_ARGUMENT, like a
 * non-finite coordinate, by all three entries.
 * ngpde_spatial_order: a node permutation (device int32[n]) along a space-filling curve through the points -- Hilbert in
 * 2-D, Morton in 3-D, the coordinate in 1-D, graph by graph -- usable as `order` of ngpde_graph_create_device, so that a
 * structure never seen before gets its locality schedule without a host traversal.  A coordinate whose extent is below
 * 2^-69 (1.7e-21) does not take part in the curve: it quantises as extent 0.
 * ---------------------------------------------------------------------------------------------- */
#define NGPDE_KNN_MAX_K 128
int32_t ngpde_radius_graph(int64_t n, int32_t dim, const float *points, float r, const int32_t *graph_id, int32_t n_graphs,
                           int32_t id_base, int32_t self_loops, int32_t dir_out, int32_t index_base, int64_t capacity, int32_t *s,
                           int32_t *t, int64_t *n_edges, ngpde_stream_t stream);
int32_t ngpde_knn_graph(int64_t n, int32_t dim, const float *points, int32_t k, const int32_t *graph_id, int32_t n_graphs,
                        int32_t id_base, int32_t self_loops, int32_t dir_out, int32_t index_base, int32_t *s, int32_t *t,
                        ngpde_stream_t stream);
int32_t ngpde_spatial_order(int64_t n, int32_t dim, const float *points, const int32_t *graph_id, int32_t n_graphs, int32_t id_base,
                            int32_t *order, ngpde_stream_t stream);

/* Device arrays of the derived graph (for callers that batch / inspect): CSR by target.
 * rowptr: int32[n_nodes+1]; col: int32[n_edges] source node of each entry; eid: int32[n_edges]
 * position of the entry in the caller's COO list. */
int32_t ngpde_graph_csr_by_target(const ngpde_graph_t *g, const int32_t **rowptr, const int32_t **col,
                                  const int32_t **eid);
int32_t ngpde_graph_csr_by_source(const ngpde_graph_t *g, const int32_t **rowptr, const int32_t **col,
                                  const int32_t **eid);

/* GCN normalisation of src/layers.jl:210-226: c = 1/sqrt(in-degree (+1 with self loops)).
 *   edge_weight       host float[n_edges] or NULL: the per-edge factor of e_mul_xj / w_mul_xj (:228,:230)
 *   weighted_degree   non-zero: degree = sum of incoming weights (explicit `edge_weight` argument,
 *                     :224 with edge_weight != nothing); zero: unweighted count (the
 *                     `use_edge_weight=true` path of the reference normalises with unweighted degrees)
 */
int32_t ngpde_graph_set_gcn_norm(ngpde_graph_t *g, int32_t add_self_loops, const float *edge_weight,
                                 int32_t weighted_degree);

/* ------------------------------------------------------------------------------------------------
 * GCNConv  -- replaces (l::GCNConv)(x, ps, st[, edge_weight]), src/layers.jl:200-239.
 *   y = act.( W * (x C (A+I) C) .+ b )     (W applied before the aggregation iff dout < din, :220)
 *   x [N][din], weight (dout x din) column-major, bias [dout] or NULL (bias=false), y [N][dout]
 *   save_agg  [N][din] or NULL: the aggregated input X C (A+I) C kept for backward (only written when dout >= din)
 *   save_z    [N][dout] or NULL: pre-activation, kept for backward
 * ---------------------------------------------------------------------------------------------- */
size_t ngpde_gcn_workspace_bytes(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t backward);
int32_t ngpde_gcn_forward(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act,
                          const float *x, const float *weight, const float *bias, float *y,
                          float *save_agg, float *save_z, void *workspace, size_t workspace_bytes,
                          ngpde_stream_t stream);
/* Pullback of the above (what a ChainRulesCore.rrule for the shim returns; the reference gets it
 * from Zygote through gather / scatter / mul).  z: pre-activation saved by forward (for relu/identity the
 * output y may be passed instead).  saved_agg: as written by forward (ignored when dout < din).
 * dx [N][din] or NULL; dweight (dout x din) column-major; dbias [dout] or NULL.  Results overwrite. */
int32_t ngpde_gcn_backward(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act,
                           const float *x, const float *weight, const float *z, const float *saved_agg,
                           const float *dy, float *dx, float *dweight, float *dbias, void *workspace,
                           size_t workspace_bytes, ngpde_stream_t stream);
/* ngpde_gcn_backward plus the gradient w.r.t. the `edge_weight` ARGUMENT of the call, which the reference differentiates through
 * e_mul_xj and through the weighted degree (src/layers.jl:206-231): dedge_weight[n_edges] in the caller's COO order (the ones
 * appended for the self loops are constants).  The handle must carry that call's normalisation (ngpde_graph_set_gcn_norm with
 * the weights and weighted_degree = 1).  x is always needed; bias only when dout < din (may be NULL for a layer without bias);
 * dx may be NULL.  Workspace: ngpde_gcn_backward_ew_workspace_bytes. */
size_t ngpde_gcn_backward_ew_workspace_bytes(const ngpde_graph_t *g, int32_t din, int32_t dout);
int32_t ngpde_gcn_backward_ew(const ngpde_graph_t *g, int32_t din, int32_t dout, int32_t act, const float *x, const float *weight,
                              const float *bias, const float *z, const float *saved_agg, const float *dy, float *dx, float *dweight,
                              float *dbias, float *dedge_weight, void *workspace, size_t workspace_bytes, ngpde_stream_t stream);

/* Generic aggregation  out[:, i] = sum_{e: t_e = i} w_e * x[:, s_e]  (propagate(copy_xj / w_mul_xj, g, +),
 * src/layers.jl:228-232) and its transpose (by_source != 0), any feature width d.
 * edge_weight: device float[n_edges] in COO order or NULL. aggr: NGPDE_AGGR_SUM or NGPDE_AGGR_MEAN. */
int32_t ngpde_propagate_copy_xj(const ngpde_graph_t *g, int32_t d, int32_t aggr, int32_t by_source,
                                const float *x, const float *edge_weight, float *out, ngpde_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Message-passing primitives -- the pieces `propagate(message, g, aggr; xi, xj, e)` [GraphNeuralNetworks.jl]
 * is made of, as used by ExplicitEdgeConv (src/layers.jl:94-112), VMHConv (:308-332), MPPDEConv (:390-422),
 * GNOConv (:509-547), SpectralConv (:652-657) and the GAT-style aggregation (softmax_edge_neighbors,
 * src/NeuralGraphPDE.jl:7).  Per-edge arrays are in "p order": CSR by target (ngpde_graph_csr_by_target),
 * the incoming edges of one node contiguous; ngpde_edge_permute converts from / to the COO order of
 * g.edata.  Each *_backward is the pullback Zygote would derive for the corresponding forward.
 * ---------------------------------------------------------------------------------------------- */

/* Lux Dense on a virtual vcat of up to 4 blocks:  y = act.(W * vcat(X1, X2, ...) .+ b)  (src/layers.jl:106,
 * :316, :328, :409, :418, :523 build the vcat explicitly).  Block i is [n / row_div[i]][width[i]] row-major;
 * row_div > 1 = a per-graph feature repeated over that graph's rows (repeat(theta; inner=...), :410,:418).
 * weight: (dout x sum width) column-major; save_z nullable. */
int32_t ngpde_dense_forward(int64_t n, int32_t n_seg, const float *const *seg_ptr, const int32_t *seg_width,
                            const int32_t *seg_row_div, int32_t dout, int32_t act, const float *weight,
                            const float *bias, float *y, float *save_z, ngpde_stream_t stream);
/* Up to four INDEPENDENT Dense layers (ngpde_dense_forward's arguments as tables; the segment tables of the problems follow
 * each other in seg_ptr / seg_width / seg_row_div) in ONE launch: GNOConv's node-level terms P, Q, B2 h, W h
 * (src/layers.jl:523,536) are latency-bound launches of a few dozen workgroups each. */
int32_t ngpde_dense_multi_forward(int32_t count, const int64_t *n, const int32_t *n_seg, const float *const *seg_ptr,
                                  const int32_t *seg_width, const int32_t *seg_row_div, const int32_t *dout, const int32_t *act,
                                  const float *const *weight, const float *const *bias, float *const *y, float *const *save_z,
                                  ngpde_stream_t stream);
/* Two Dense layers that share their leading input block, y_a = Dense_a(vcat(X, ...)), y_b = Dense_b(vcat(X, ...)), in one pass
 * over X: the two node-level halves of a message MLP's first layer (the `vcat(xi..., xj..., ...)` of src/layers.jl:106, :316,
 * :409-410 split into a target term and a source term).  Exactly two ngpde_dense_forward calls in effect; one launch when X
 * is 64 wide, both outputs <= 64 wide and the other blocks narrow. */
int32_t ngpde_dense_pair_forward(int64_t n, int32_t n_seg_a, const float *const *seg_ptr_a, const int32_t *seg_width_a,
                                 const int32_t *seg_row_div_a, int32_t dout_a, int32_t act_a, const float *weight_a, const float *bias_a,
                                 float *y_a, float *save_z_a, int32_t n_seg_b, const float *const *seg_ptr_b,
                                 const int32_t *seg_width_b, const int32_t *seg_row_div_b, int32_t dout_b, int32_t act_b,
                                 const float *weight_b, const float *bias_b, float *y_b, float *save_z_b, ngpde_stream_t stream);
/* Pullback of such a pair when neither layer has an activation of its own (the first-layer halves of a message MLP: the
 * activation is applied per edge) and dout = 64: dx = dy_a Wa^T + dy_b Wb^T [+ dx_addend] for the shared leading block (one
 * array, already summed; dx_addend nullable, may alias dx), both weight / bias gradients; other blocks get no gradient.
 * ngpde_dense_pair_backward_workspace_bytes returns 0 for shapes that need two ngpde_dense_backward calls instead. */
size_t ngpde_dense_pair_backward_workspace_bytes(int64_t n, int32_t n_seg_a, const float *const *seg_ptr_a, const int32_t *seg_width_a,
                                                 const int32_t *seg_row_div_a, int32_t n_seg_b, const float *const *seg_ptr_b,
                                                 const int32_t *seg_width_b, const int32_t *seg_row_div_b, int32_t dout);
int32_t ngpde_dense_pair_backward(int64_t n, int32_t n_seg_a, const float *const *seg_ptr_a, const int32_t *seg_width_a,
                                  const int32_t *seg_row_div_a, const float *weight_a, const float *dy_a, float *dweight_a,
                                  float *dbias_a, int32_t n_seg_b, const float *const *seg_ptr_b, const int32_t *seg_width_b,
                                  const int32_t *seg_row_div_b, const float *weight_b, const float *dy_b, float *dweight_b,
                                  float *dbias_b, int32_t dout, float *dx, const float *dx_addend, void *workspace,
                                  size_t workspace_bytes, ngpde_stream_t stream);
/* Chain(Dense(. => dmid, act1), Dense(dmid => dout, act2)) on a virtual vcat -- the node update psi / gamma of MPPDEConv /
 * VMHConv (src/layers.jl:418, :328).  a1 (the first layer's activations, [n][dmid]) and the save_* arrays are nullable when
 * ngpde_dense_chain2_fused(...) == 1: the intermediate then stays on chip (one launch); otherwise a1 is required. */
int32_t ngpde_dense_chain2_fused(int64_t n, int32_t n_seg, const float *const *seg_ptr, const int32_t *seg_width,
                                 const int32_t *seg_row_div, int32_t dmid, int32_t dout);
int32_t ngpde_dense_chain2_forward(int64_t n, int32_t n_seg, const float *const *seg_ptr, const int32_t *seg_width,
                                   const int32_t *seg_row_div, int32_t dmid, int32_t act1, const float *weight1, const float *bias1,
                                   float *a1, float *save_z1, int32_t dout, int32_t act2, const float *weight2, const float *bias2,
                                   float *y, float *save_z2, ngpde_stream_t stream);
size_t ngpde_dense_workspace_bytes(int64_t n, int32_t din_total, int32_t dout);
/* dseg_ptr[i] nullable: gradient block for X_i (never written for row_div > 1 blocks: graph-level features
 * are @ignore_derivatives in the reference, :397,:418).  dweight (dout x sum width) column-major, dbias nullable. */
int32_t ngpde_dense_backward(int64_t n, int32_t n_seg, const float *const *seg_ptr, const int32_t *seg_width,
                             const int32_t *seg_row_div, int32_t dout, int32_t act, const float *weight, const float *z,
                             const float *dy, float *const *dseg_ptr, float *dweight, float *dbias, void *workspace,
                             size_t workspace_bytes, ngpde_stream_t stream);

/* dst[p] = src[eid[p]] (COO order -> p order; inverse != 0: the opposite scatter), rows of d floats */
int32_t ngpde_edge_permute(const ngpde_graph_t *g, int32_t d, int32_t inverse, const float *src, float *dst,
                           ngpde_stream_t stream);

/* apply_edges for a first layer that is linear in its blocks:  z_p = P[t_p] + Q[s_p] + E_p,  a_p = act(z_p).
 * P, Q: [N][h] node-level terms (gathered at the target / source: xi = gather(., t), xj = gather(., s));
 * e_term: [E][h] in p order or NULL; outputs a_out, z_out (nullable) [E][h] in p order. */
int32_t ngpde_edge_combine_forward(const ngpde_graph_t *g, int32_t h, int32_t act, const float *p_target,
                                   const float *q_source, const float *e_term, float *a_out, float *z_out,
                                   ngpde_stream_t stream);
/* dz_p = da_p * act'(z_p) (also the gradient of e_term); dP[i] = sum over incoming edges; dQ[j] = sum over
 * outgoing edges (pullback of gather = scatter(+)).  z NULL = identity activation.  dp/dq nullable. */
int32_t ngpde_edge_combine_backward(const ngpde_graph_t *g, int32_t h, int32_t act, const float *da, const float *z,
                                    float *dz, float *dp_target, float *dq_source, ngpde_stream_t stream);

/* aggregate_neighbors(g, aggr, m): out[:, i] = aggr over the incoming edges of i of m[:, e]; mean of an empty
 * neighbourhood is 0; max/min pullback routes to every extremal entry (NNlib). */
int32_t ngpde_segment_reduce_forward(const ngpde_graph_t *g, int32_t d, int32_t aggr, const float *m, float *out,
                                     ngpde_stream_t stream);
int32_t ngpde_segment_reduce_backward(const ngpde_graph_t *g, int32_t d, int32_t aggr, const float *m, const float *out,
                                      const float *dout, float *dm, ngpde_stream_t stream);

/* ---- the public message-passing API (src/NeuralGraphPDE.jl:5-11 re-exports propagate, apply_edges, aggregate_neighbors,
 * softmax_edge_neighbors, copy_xj, copy_xi, xi_dot_xj, e_mul_xj, w_mul_xj; docs/src/devdoc.md:47-52 builds user layers on
 * propagate(message, g, aggr; xi, xj, e)).  Atomic-free, bitwise reproducible, no workspace.  Checked before any device call, in
 * this order: a negative width (NGPDE_ERR_DIMENSION_MISMATCH), an aggregation the entry does not take (NGPDE_ERR_INVALID_ARGUMENT),
 * a NULL graph (NGPDE_ERR_INVALID_ARGUMENT). */

/* The gather half of propagate (src/NeuralGraphPDE.jl:5-11, docs/src/devdoc.md:47-52): for the n <= 4 node arrays x[k] ([N][width[k]])
 * xi[k][p] = x[k][t_p] and xj[k][p] = x[k][s_p], [E][width[k]] in p order, in ONE launch; xi / xj (the tables or their entries)
 * nullable.  The pullback, one launch: dx[k][i] = sum over the incoming p of dxi[k][p] + sum over the outgoing p of dxj[k][p]
 * (dxi / dxj nullable: that side contributes nothing). */
int32_t ngpde_gather_forward(const ngpde_graph_t *g, int32_t n, const float *const *x, const int32_t *width, float *const *xi,
                             float *const *xj, ngpde_stream_t stream);
int32_t ngpde_gather_backward(const ngpde_graph_t *g, int32_t n, const int32_t *width, const float *const *dxi, const float *const *dxj,
                              float *const *dx, ngpde_stream_t stream);

/* propagate(e_mul_xj | w_mul_xj | copy_xj, g, + | mean; xj = x, e) fused (src/NeuralGraphPDE.jl:5-11, docs/src/devdoc.md:47-52; the
 * weighted form of src/layers.jl:228-232): out[i] = aggr over the incoming e of e_e .* x[s_e], no [E][d] message array.  e: [E][e_width]
 * in COO order with e_width 1 (a scalar per edge: w_mul_xj's edge weights) or d, or e_width 0 and e NULL (copy_xj).  aggr
 * NGPDE_AGGR_SUM or NGPDE_AGGR_MEAN (an empty neighbourhood gives 0).  The pullback: dx [N][d] (nullable) summed over each source's
 * outgoing edges; de [E][e_width] in COO order (nullable): the elementwise dout[t_e] .* x[s_e] for e_width d, the dot product
 * <dout[t_e], x[s_e]> for e_width 1 (/ deg t_e under mean).  ngpde_propagate_copy_xj is unchanged. */
int32_t ngpde_propagate_emul_forward(const ngpde_graph_t *g, int32_t d, int32_t e_width, int32_t aggr, const float *x, const float *e,
                                     float *out, ngpde_stream_t stream);
int32_t ngpde_propagate_emul_backward(const ngpde_graph_t *g, int32_t d, int32_t e_width, int32_t aggr, const float *x, const float *e,
                                      const float *dout, float *dx, float *de, ngpde_stream_t stream);

/* apply_edges(xi_dot_xj, g; xi, xj) (src/NeuralGraphPDE.jl:5-11, docs/src/devdoc.md:47-52): out[e] = <xi[t_e], xj[s_e]>, [E] in COO
 * order; xi, xj [N][d] (may be different arrays).  The pullback: dxi[i] = sum over the incoming e of dout_e xj[s_e], dxj[j] = sum
 * over the outgoing e of dout_e xi[t_e] (each nullable). */
int32_t ngpde_apply_edges_dot_forward(const ngpde_graph_t *g, int32_t d, const float *xi, const float *xj, float *out,
                                      ngpde_stream_t stream);
int32_t ngpde_apply_edges_dot_backward(const ngpde_graph_t *g, int32_t d, const float *xi, const float *xj, const float *dout, float *dxi,
                                       float *dxj, ngpde_stream_t stream);

/* softmax_edge_neighbors(g, e) (src/NeuralGraphPDE.jl:5-11, docs/src/devdoc.md:47-52): per target, a softmax over its incoming edges
 * with the row maximum subtracted; e, y [E][h] in COO order, any h >= 1.  The pullback de = y .* (dy - sum over the row of y .* dy).
 * One launch each. */
int32_t ngpde_softmax_edge_neighbors_forward(const ngpde_graph_t *g, int32_t h, const float *e, float *y, ngpde_stream_t stream);
int32_t ngpde_softmax_edge_neighbors_backward(const ngpde_graph_t *g, int32_t h, const float *y, const float *dy, float *de,
                                              ngpde_stream_t stream);

/* ---- the per-graph readouts (src/NeuralGraphPDE.jl:5-7 re-exports reduce_nodes, reduce_edges, softmax_nodes, softmax_edges,
 * broadcast_nodes, broadcast_edges): one row per graph of a block-diagonal batch out of its nodes' or edges' rows, and back.
 * A readout is 1 to a few hundred segments of 10^3 to 10^5 rows each -- the opposite shape of a neighbourhood -- so it has kernels
 * of its own: a PLAN cuts every segment into chunks of at most chunk_rows rows, one workgroup reduces a chunk, and one wave per
 * segment folds the chunks' partial rows in chunk order.  Atomic-free; the chunking is the plan's alone, so every result is bitwise
 * equal from run to run.  Nothing is allocated after create: the caller provides the workspace, and every entry can be captured
 * into a HIP graph.  Checked before any device call, in this order: a negative width (NGPDE_ERR_DIMENSION_MISMATCH), an aggregation
 * other than NGPDE_AGGR_SUM / MEAN / MAX / MIN (NGPDE_ERR_INVALID_ARGUMENT), a NULL plan (NGPDE_ERR_INVALID_ARGUMENT), a workspace
 * smaller than ngpde_readout_workspace_bytes (NGPDE_ERR_WORKSPACE). */
typedef struct ngpde_readout ngpde_readout_t;

/* The plan depends on the map from items to segments alone: segment of item i = id[index ? index[i] : i] - id_base; id NULL: one
 * segment.  id, index: device int32; index entries address id.  Nodes: (N, indicator, NULL); edges: (E, indicator, the sources in COO
 * order).  n_items <= 2^31 - 1, n_segments >= 1 (n_segments > 1 needs id: both refused without touching the device); an id outside
 * id_base : id_base + n_segments - 1 is NGPDE_ERR_INVALID_ARGUMENT.  Non-decreasing ids (every batch) make the plan `contiguous`:
 * rows are addressed directly; otherwise through a stable permutation of the items by segment.  Synchronises the stream.
 * PRECONDITION, NOT CHECKED: every index[i] lies inside id.  The entry is not told id's length, so an index entry outside it is an
 * out-of-bounds device read, not an error status; pass the sources of a graph whose edges were validated (ngpde_graph_create). */
int32_t ngpde_readout_create(int64_t n_items, const int32_t *id, const int32_t *index, int32_t id_base, int32_t n_segments,
                             ngpde_stream_t stream, ngpde_readout_t **out);
int32_t ngpde_readout_destroy(ngpde_readout_t *r);
/* every output nullable */
int32_t ngpde_readout_info(const ngpde_readout_t *r, int64_t *n_items, int32_t *n_segments, int32_t *contiguous, int64_t *n_chunks,
                           int32_t *chunk_rows);
/* bytes that cover every entry below at width d (0 for a NULL plan or d <= 0) */
size_t ngpde_readout_workspace_bytes(const ngpde_readout_t *r, int32_t d);

/* reduce_nodes / reduce_edges(aggr, g, x): out[s] = aggr over the items of segment s of x[i]; x [n][d], out [S][d].  An empty
 * segment gives 0 for sum and mean, -inf / +inf for max / min (the conventions of ngpde_segment_reduce_forward).  One launch when
 * every segment is a single chunk, two otherwise.  The pullback (one launch, no workspace): dx[i] = dout[s_i], / count for mean, and
 * where x[i] == out[s_i] for max / min (every tied entry, as NNlib's); x and out are read for max / min only. */
int32_t ngpde_readout_reduce_forward(const ngpde_readout_t *r, int32_t d, int32_t aggr, const float *x, float *out, void *workspace,
                                     size_t workspace_bytes, ngpde_stream_t stream);
int32_t ngpde_readout_reduce_backward(const ngpde_readout_t *r, int32_t d, int32_t aggr, const float *x, const float *out,
                                      const float *dout, float *dx, ngpde_stream_t stream);

/* softmax_nodes / softmax_edges(g, x): per segment and column, the softmax over the segment's items with the maximum subtracted;
 * x, y [n][d].  The maximum and the sum of exponentials are found in ONE pass over x (two launches when every segment is a single
 * chunk, three otherwise).  The pullback dx = y .* (dy - sum over the segment of y .* dy), the same launch counts. */
int32_t ngpde_readout_softmax_forward(const ngpde_readout_t *r, int32_t d, const float *x, float *y, void *workspace,
                                      size_t workspace_bytes, ngpde_stream_t stream);
int32_t ngpde_readout_softmax_backward(const ngpde_readout_t *r, int32_t d, const float *y, const float *dy, float *dx, void *workspace,
                                       size_t workspace_bytes, ngpde_stream_t stream);

/* broadcast_nodes / broadcast_edges(g, u): out[i] = u[s_i]; u [S][d], out [n][d].  The pullback du[s] = the sum of dout over the
 * segment (the reduce with NGPDE_AGGR_SUM). */
int32_t ngpde_readout_broadcast_forward(const ngpde_readout_t *r, int32_t d, const float *u, float *out, ngpde_stream_t stream);
int32_t ngpde_readout_broadcast_backward(const ngpde_readout_t *r, int32_t d, const float *dout, float *du, void *workspace,
                                         size_t workspace_bytes, ngpde_stream_t stream);

/* ---- graph queries and transforms on a device COO list (src/NeuralGraphPDE.jl:4 re-exports GNNGraphs: degree, has_self_loops,
 * has_multi_edges, is_bidirected, add_self_loops, remove_self_loops, remove_multi_edges, to_bidirected, getgraph, unbatch): what a
 * user does to a graph between making it (ngpde_radius_graph / ngpde_knn_graph write such lists) and ngpde_graph_create_device.
 *   s, t         device int32[n_edges] with `index_base` added, as the neighbour search writes them; outputs carry the same base
 *   n_nodes      <= 2^31 - 1; n_edges (2 * n_edges when symmetrising) <= 2^31 - 1, refused beyond (NGPDE_ERR_INVALID_ARGUMENT)
 * Checked before any device call: NULL and negative arguments (NGPDE_ERR_INVALID_ARGUMENT).  An edge end outside the node range is
 * NGPDE_ERR_DIMENSION_MISMATCH from the entries that index by node or build a sort key; no kernel reads or writes through such an end.
 * MEMORY: temporary storage (sort buffers, flags, scans: a few arrays of n_edges or n_nodes words) is allocated with hipMalloc inside
 * the call and freed before it returns, as ngpde_graph_create_device does; these entries are therefore not capturable into a HIP graph.
 * The group reduce below allocates nothing and is.
 * SYNCHRONISATION: ngpde_coo_flags, ngpde_coo_compact and ngpde_coo_coalesce return a data-dependent count or flags through HOST
 * pointers and synchronise `stream` before they return, as ngpde_radius_graph does; their device outputs are sized by the caller to
 * the upper bound given with each.  Nothing here uses float atomics: every result is bitwise equal from run to run. */
enum { NGPDE_DIR_OUT = 0, NGPDE_DIR_IN = 1, NGPDE_DIR_BOTH = 2 };

/* degree(g, dir; edge_weight): exactly one of out_counts / out_sums is given (the other NULL) and selects the form.  out_counts
 * int32[n_nodes] = the number of edges leaving (OUT) / entering (IN) a node, BOTH = the sum of the two; w is not read.  out_sums
 * float[n_nodes] = the sum of w (device float[n_edges], required unless n_edges == 0) over those edges, added in COO order from 0.0f
 * (a stable sort of the COO positions by node, then one thread per node: the order of norm_kernel in graph_device.hip); BOTH = the OUT
 * sum + the IN sum. */
int32_t ngpde_coo_degree(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                         const float *w, int32_t *out_counts, float *out_sums, ngpde_stream_t stream);

/* The three predicates from one call (host outputs, each nullable): has_self_loops = some s == t; has_multi_edges = some (s, t) pair
 * occurs twice; is_bidirected = for every pair the multiplicity of (s, t) equals that of (t, s) (the sorted 64-bit keys s*n + t and
 * t*n + s are the same sequence).  Synchronises. */
int32_t ngpde_coo_flags(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t *has_self_loops,
                        int32_t *has_multi_edges, int32_t *is_bidirected, ngpde_stream_t stream);

/* Stable compaction.  An edge is kept iff (drop_self_loops == 0 or s != t) and, with `nodes`, both ends are listed.
 *   nodes        device int64[n_keep], 0-based, or NULL: the induced subgraph -- node nodes[k] becomes node k, every other node is
 *                dropped (a relabel table, -1 = dropped, is built in front of the compaction).  An entry outside 0 : n_nodes - 1 or a
 *                repeated one is NGPDE_ERR_INVALID_ARGUMENT, detected on the device and read back with the count.
 *   s_out, t_out device int32[n_edges] (upper bound): the kept edges in COO order, renumbered under `nodes`
 *   kept         device int64[n_edges] (upper bound): the COO position (0-based) of every kept edge, ascending -- the index list
 *                ngpde_rows_index takes to move the edge features
 *   n_out        host: the number of kept edges.  Synchronises. */
int32_t ngpde_coo_compact(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_keep,
                          const int64_t *nodes, int32_t drop_self_loops, int32_t *s_out, int32_t *t_out, int64_t *kept, int64_t *n_out,
                          ngpde_stream_t stream);

/* Coalesce: one edge per distinct (s, t), ORDERED BY SOURCE, THEN TARGET.  M = n_edges copies, or with symmetrize != 0 the M = 2 * n_edges
 * copies of [s; t], [t; s] (copy e < n_edges is edge e, copy e >= n_edges is edge e - n_edges reversed; the 2E list is never written).
 * The copies are sorted stably by the 64-BIT key s*n_nodes + t (rocPRIM radix sort; a 32-bit key overflows from n = 65 536 on); a copy
 * whose key differs from its predecessor's heads a group.  Outputs, all device int32, sized by the caller to M (group_ptr: M + 1):
 *   s_out, t_out   [n_out]      the distinct pairs
 *   group_ptr      [n_out + 1]  group g holds the sorted copies group_ptr[g] .. group_ptr[g + 1] - 1
 *   member         [M]          the source-edge ROW of every sorted copy (copy e >= n_edges names row e - n_edges), ascending by copy
 *                               -- hence by COO position -- inside a group
 *   group_of       [M]          the inverse: the group that copy e fell into (what the pullback of the group reduce reads)
 *   n_out          host: the number of groups.  Synchronises. */
int32_t ngpde_coo_coalesce(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t symmetrize,
                           int32_t *s_out, int32_t *t_out, int32_t *group_ptr, int32_t *member, int32_t *group_of, int64_t *n_out,
                           ngpde_stream_t stream);

/* The features of coalesced edges: out[g][:] = aggr over the members of group g of src[member][:], rows of d floats, src [n_rows][d],
 * out [n_groups][d]; aggr NGPDE_AGGR_SUM (a plain float sum in member order from the first member), MEAN (that sum divided by the
 * member count), MAX / MIN (exact).  One launch, a lane per (group, 4 columns) with float4 rows where d % 4 == 0 and the arrays are
 * 16-byte aligned, a lane per (group, column) otherwise; a group of any length is walked by its lane.
 * Pullback, one launch, atomic-free: source row r occurs in exactly `copies` groups (1, or 2 after symmetrize: group_of[r] and
 * group_of[r + n_rows]); dsrc[r] = the sum in copy order of dout[g] (SUM), dout[g] / count(g) (MEAN), dout[g] where src[r] == out[g]
 * else 0 (MAX / MIN: every extremal member, as ngpde_segment_reduce_backward); src and out are read for MAX / MIN only.
 * PRECONDITION, NOT CHECKED: group_ptr, member and group_of are those ngpde_coo_coalesce wrote for n_rows edges. */
int32_t ngpde_group_reduce_forward(int64_t n_groups, int64_t n_rows, int32_t d, int32_t aggr, const int32_t *group_ptr,
                                   const int32_t *member, const float *src, float *out, ngpde_stream_t stream);
int32_t ngpde_group_reduce_backward(int64_t n_groups, int64_t n_rows, int32_t copies, int32_t d, int32_t aggr, const int32_t *group_ptr,
                                    const int32_t *group_of, const float *src, const float *out, const float *dout, float *dsrc,
                                    ngpde_stream_t stream);

/* add_self_loops: s_out, t_out int32[n_edges + n_nodes] = the old edges in order, then (i, i) for i = 0 .. n_nodes - 1; w_out (nullable,
 * with w) float[n_edges + n_nodes] = w, then n_nodes ones.  Concatenation and iota in one launch; existing loops are not looked for. */
int32_t ngpde_coo_add_self_loops(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, const float *w,
                                 int32_t *s_out, int32_t *t_out, float *w_out, ngpde_stream_t stream);

/* ---- random graph sampling on a device COO list (src/NeuralGraphPDE.jl:4 re-exports GNNGraphs: sample_neighbors, rand_edge_split):
 * a fresh sub-sample of every neighbourhood, or a random hold-out of the edges, per epoch, without the lists leaving the device.  The
 * conventions are those of the block above: int32 lists with `index_base`, outputs sized by the caller to the upper bound given with
 * each, n_nodes, n_edges and the number of draws <= 2^31 - 1 (refused beyond), NULL and negative arguments refused before any device
 * call (NGPDE_ERR_INVALID_ARGUMENT), an edge end outside the node range NGPDE_ERR_DIMENSION_MISMATCH without a read or write through
 * it, temporaries from hipMalloc inside the call (not capturable), the data-dependent count through a HOST pointer after one
 * synchronisation of `stream`.  No float arithmetic and no racing writes: every result is bitwise equal from run to run.
 * RANDOMNESS: Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), stateless: a value is a
 * pure function of (seed, stream, counter) -- key (lo32(seed), hi32(seed)), counter (c0, c1, stream, 0), the 64-bit draw
 * out[0] | out[1] << 32 -- never of the thread, the launch geometry or the call order.  Streams: 1 = the neighbour keys, 2 = the draws
 * with replacement, 3 = the split keys, 4 = the negative-sampling candidates (graph editing, below), 5 = the Lanczos start
 * vector (graph matrices, below), so one seed gives the five operations independent values. */

/* out[i] (device uint64[n]) = the draw at counter (lo32(first + i), c1, stream_id, 0): the generator's bits through the ABI, for tests.
 * The samplers below evaluate the same device function in their kernels and write no keys they do not need. */
int32_t ngpde_random_keys(uint64_t seed, uint32_t stream_id, uint32_t c1, uint64_t first, int64_t n, uint64_t *out, ngpde_stream_t stream);

/* Rows longer than this are selected by a segmented sort instead of in LDS (below): 2048 keys of 8 bytes are the 16 KB of LDS a
 * 256-thread workgroup stages, 9 workgroups per CU; rank counting is quadratic in the row, ~2 * 10^4 comparisons per thread here. */
#define NGPDE_SAMPLE_LDS_ROW_MAX 2048

/* sample_neighbors(g, nodes, K; dir, replace).  The ROW of a node is the list of COO positions of its inbound (dir NGPDE_DIR_IN) or
 * outbound (NGPDE_DIR_OUT) edges in COO order (the stable grouping ngpde_coo_degree makes).  Only the rows of listed nodes take part.
 *   nodes        device int64[n_listed], 0-based, distinct, or NULL (with n_listed 0): every node.  An entry outside 0 : n_nodes - 1
 *                or a repeated one is NGPDE_ERR_INVALID_ARGUMENT, detected on the device and read back with the count.
 *   k            -1: every edge of a listed row; 0: none; k < -1 refused
 *   replace == 0 the edge at COO position e has the key draw(stream 1, counter (lo32(e), hi32(e))); a listed row keeps its min(k, deg)
 *                edges with the smallest (key, e) -- a uniform k-subset, and since the key belongs to the edge, what a node gets does
 *                not depend on which other nodes are listed.  A row with deg <= k is copied through without drawing; a longer one of
 *                at most NGPDE_SAMPLE_LDS_ROW_MAX edges is selected in ONE launch for all rows by exact rank counting on keys drawn
 *                in the kernel and staged in LDS (an edge is kept iff fewer than k edges of its row have a smaller (key, e)): a wave
 *                per row of up to NGPDE_SAMPLE_LDS_ROW_MAX / 4 edges, the 256-thread workgroup per longer row; rows beyond the bound
 *                go through rocprim::segmented_radix_sort_pairs of the keys, stable, so ties break by position there too (that sort
 *                is enqueued whenever n_edges exceeds the bound, over empty segments if no row does: only the device knows).  The
 *                kept edges are compacted in COO order.  Outputs hold up to n_edges entries.
 *   replace != 0 (k >= 0): a listed node v with deg > 0 gets exactly k edges, draw j being entry (draw(stream 2, counter (v, j)) * deg)
 *                >> 64 of its row; a node without edges gets none.  Output order: listed-node order (node order with nodes NULL),
 *                then j.  Outputs hold up to n_listed * k (n_nodes * k with nodes NULL) entries.
 *   s_out, t_out device int32: the sampled edges, with `index_base`;  eid_out device int64: their COO positions (0-based) in the input
 *   n_out        host: the number of sampled edges.  Synchronises. */
int32_t ngpde_coo_sample_neighbors(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                                   int64_t n_listed, const int64_t *nodes, int32_t k, int32_t replace, uint64_t seed, int32_t *s_out,
                                   int32_t *t_out, int64_t *eid_out, int64_t *n_out, ngpde_stream_t stream);

/* rand_edge_split(g, frac): a random partition of the edges into a first and a second part, n_first = round(frac * ...) made by the
 * caller.  side_out device int32[n_edges]: 0 = first part, 1 = second; kept0 / kept1 device int64[n_edges] (upper bound each): the COO
 * positions of the two parts, ascending; n0_out host: the size of the first part (the second has n_edges - n0).  Synchronises.
 *   by_pair == 0 the key of edge e is draw(stream 3, counter (lo32(e), hi32(e))); the n_first edges with the smallest (key, e) -- one
 *                stable 64-bit radix sort -- are the first part.  n_first <= n_edges.
 *   by_pair != 0 for bidirected lists: the key is draw(stream 3, counter (min(s, t), max(s, t))), shared by both directions of a pair
 *                and by parallel copies.  The RANKED edges are those with s <= t; n_first counts them (more than there are:
 *                NGPDE_ERR_INVALID_ARGUMENT, read back with the count).  tau = the key of the ranked edge of rank n_first - 1; every
 *                edge with key <= tau goes to the first part, so a pair is never torn (with parallel copies the first part may hold
 *                more than n_first ranked edges); n_first == 0 sends everything to the second part.  The sort runs over all n_edges
 *                keys and an inclusive scan of the ranked flags in sorted order finds the rank: the number of ranked edges never has
 *                to reach the host. */
int32_t ngpde_coo_rand_split(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_first,
                             int32_t by_pair, uint64_t seed, int32_t *side_out, int64_t *kept0, int64_t *kept1, int64_t *n0_out,
                             ngpde_stream_t stream);

/* ---- graph editing on a device COO list (src/NeuralGraphPDE.jl:4 re-exports GNNGraphs: add_edges, remove_edges, remove_nodes,
 * to_unidirected, negative_sample): the transforms that CHANGE a graph -- a cloud refined, coarsened or cut between two updategraph
 * calls, the non-edges an edge predictor trains against.  The conventions are those of the two blocks above: int32 lists with
 * `index_base`, outputs sized by the caller to the upper bound given with each, n_nodes, n_edges and every count <= 2^31 - 1 (refused
 * beyond), NULL and negative arguments refused before any device call (NGPDE_ERR_INVALID_ARGUMENT), an edge end outside the node range
 * NGPDE_ERR_DIMENSION_MISMATCH from the entries that build a sort key, without a read or write through it, temporaries from hipMalloc
 * inside the call (not capturable), data-dependent counts and errors through the status / HOST pointers after one synchronisation of
 * `stream` (ngpde_coo_negative_sample: one per round).  No float arithmetic and no racing writes of different values: every result is
 * bitwise equal from run to run. */

/* add_edges: s_out, t_out int32[n_edges + n_new] = the old edges in order, then the new ones (s_new, t_new: device int32[n_new], with
 * `index_base`) in the order given.  Concatenation and checks in ONE launch: a new end outside the node range is
 * NGPDE_ERR_DIMENSION_MISMATCH; with graph_of (device int32[n_nodes], the graph of every node; nullable) a new edge whose ends lie in
 * different graphs is NGPDE_ERR_INVALID_ARGUMENT.  Both are detected on the device and read back once.  Synchronises. */
int32_t ngpde_coo_append(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_new,
                         const int32_t *s_new, const int32_t *t_new, const int32_t *graph_of, int32_t *s_out, int32_t *t_out,
                         ngpde_stream_t stream);

/* remove_edges, one of two forms per call (the other form's pointers NULL):
 *   positions    device int64[n_listed], 0-based COO positions; repeats allowed; an entry outside 0 : n_edges - 1 is
 *                NGPDE_ERR_INVALID_ARGUMENT.  A flag array.
 *   ls, lt       device int32[n_listed], with `index_base`: every edge whose (s, t) equals a listed pair goes, all its parallel copies
 *                included; a listed pair the list does not hold is ignored; a listed end outside the node range is
 *                NGPDE_ERR_INVALID_ARGUMENT.  The listed 64-BIT keys s*n_nodes + t are radix-sorted and one thread per edge does a binary
 *                search.
 * Then the stable compaction of ngpde_coo_compact (one definition: csrc/coo_compact.h) with the same outputs: s_out, t_out
 * int32[n_edges], kept int64[n_edges] (upper bounds), n_out host.  The kept edges stay in COO order.  Synchronises. */
int32_t ngpde_coo_remove_edges(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_listed,
                               const int64_t *positions, const int32_t *ls, const int32_t *lt, int32_t *s_out, int32_t *t_out, int64_t *kept,
                               int64_t *n_out, ngpde_stream_t stream);

/* remove_nodes, first half: out device int64[n_nodes] (upper bound) = the nodes NOT listed (nodes: device int64[n_listed], 0-based,
 * repeats allowed, an entry out of range NGPDE_ERR_INVALID_ARGUMENT), ascending; n_out host: how many.  What ngpde_coo_compact then
 * takes as `nodes`.  Synchronises. */
int32_t ngpde_coo_complement_nodes(int64_t n_nodes, int64_t n_listed, const int64_t *nodes, int64_t *out, int64_t *n_out,
                                   ngpde_stream_t stream);

/* to_unidirected, first half: (s_out, t_out)[e] = (min(s, t), max(s, t)), int32[n_edges]; ngpde_coo_coalesce then merges the copies
 * and checks the ends.  One launch, no synchronisation. */
int32_t ngpde_coo_orient(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t *s_out, int32_t *t_out,
                         ngpde_stream_t stream);

/* negative_sample: n_target pairs of distinct nodes that are not edges of the list; never a self loop.  A pure function of (list,
 * arguments, seed).  With U = n_nodes * (n_nodes - 1), candidate j = 0, 1, 2, ... has the code
 *   c_j = (draw(stream 4, counter (lo32(j), hi32(j))) * U) >> 64      (64-bit multiply-high; its bias is at most U / 2^64, U < 2^62)
 * which decodes as a = c / (n_nodes - 1), b' = c % (n_nodes - 1), b = b' + (b' >= a); with bidirected != 0 the pair is then made
 * (min, max).  A candidate is a NEGATIVE if (a, b) is not an edge -- with bidirected, nor (b, a).  The result is THE FIRST n_target
 * DISTINCT NEGATIVES OF THE SEQUENCE, IN SEQUENCE ORDER: s_out, t_out device int32[n_target] = the pairs; with bidirected
 * int32[2 * n_target] = [a; b], [b; a].  n_out host: the number of edges written.
 *   K            the number of distinct non-loop pairs of the list (unordered with bidirected), counted on the device; with U_eff = U
 *                (U / 2 with bidirected), n_target > U_eff - K is NGPDE_ERR_INVALID_ARGUMENT
 *   chunk        candidates per round, <= 2^24; 0: the library's choice (the expected number for n_target negatives and a quarter more,
 *                at least 256).  THE RESULT DOES NOT DEPEND ON IT.  Setup, once: the list's keys a*n_nodes + b (64 bits; canonical with
 *                bidirected, so one search answers both orientations) radix-sorted, K counted.  A round: draw and decode in the
 *                kernel, binary-search the list's keys and the keys accepted so far, stable-sort the survivors by key with j as the
 *                payload, the heads of the key groups are the new negatives, merge them into the accepted set, read back the count.
 *                At the end the accepted set is sorted by j and cut at n_target.
 *   cap          the walk stops with NGPDE_ERR_STATE once 64 * ceil(U_eff / (U_eff - K)) * (n_target + 16) candidates are behind it
 *                without n_target negatives (coupon collecting needs about U_eff * ln(U_eff - K): never reached in practice; nothing
 *                spins).  It never truncates.
 * Synchronises (once per round). */
int32_t ngpde_coo_negative_sample(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int64_t n_target,
                                  int32_t bidirected, uint64_t seed, int64_t chunk, int32_t *s_out, int32_t *t_out, int64_t *n_out,
                                  ngpde_stream_t stream);

/* ---- graph matrices on a device COO list (src/NeuralGraphPDE.jl:4 re-exports GNNGraphs: adjacency_matrix, laplacian_matrix,
 * normalized_laplacian, scaled_laplacian, laplacian_lambda_max, khop_adj): the graph as a sparse float32 matrix -- the discrete
 * diffusion operator, the step bound 2 / lambda_max of the explicit solvers, the operator of Chebyshev filters, the k-hop graph.
 * A MATRIX is coalesced COO with a row pointer, all on the device: rows, cols int32[nnz] (0-BASED POSITIONS, whatever `index_base` the
 * edge list carries), vals float[nnz], sorted by row, then column, each (row, col) at most once; row_ptr int32[n + 1].
 * The conventions are those of the blocks above: int32 lists with `index_base`, outputs sized by the caller to the upper bound given
 * with each, sizes <= 2^31 - 1 (refused beyond), NULL and negative arguments refused before any device call
 * (NGPDE_ERR_INVALID_ARGUMENT), an edge end or a column outside the node range NGPDE_ERR_DIMENSION_MISMATCH without a read or write
 * through it, temporaries from hipMalloc inside the call (not capturable), data-dependent counts and errors through the status / HOST
 * pointers after one synchronisation of `stream`.  No float atomics: every result is bitwise equal from run to run. */
enum { NGPDE_MATRIX_ADJ = 0, NGPDE_MATRIX_LAPLACIAN = 1, NGPDE_MATRIX_NORM_LAPLACIAN = 2 };

/* The assembly (src/NeuralGraphPDE.jl:4).  With dir NGPDE_DIR_OUT an edge s -> t is position (s, t), with NGPDE_DIR_IN (t, s): the ends
 * are swapped where the sort key is made, no second list is written.  The M copies -- the n_edges edges, then for LAPLACIAN and
 * NORM_LAPLACIAN the n_nodes diagonal positions -- are sorted stably by the 64-BIT key row*n_nodes + col; a copy whose key differs from
 * its predecessor's heads an entry.  a[i][j] = the sum of w (device float[n_edges], or NULL: ones) over the entry's edges in COO order
 * from 0.0f, plus 1.0f last on the diagonal with add_self_loops (NORM_LAPLACIAN only); d[i] = the sum of a over row i, front to back.
 *   ADJ             vals = a; only existing pairs are entries
 *   LAPLACIAN       vals[i][j] = -a[i][j], vals[i][i] = d[i] - a[i][i]; every diagonal position is an entry
 *   NORM_LAPLACIAN  vals[i][j] = (i == j) - ((1 / sqrt(d[i])) * a[i][j]) * (1 / sqrt(d[j])); every diagonal position is an entry.  A row
 *                   sum that is not positive is NGPDE_ERR_INVALID_ARGUMENT (the smallest such node is named), found by the launch that
 *                   adds the rows; no value is written through it.  With scale (device float[n_graphs], > 0, NOT CHECKED; graph_of
 *                   device int32[n_nodes], 0-based, NULL for one graph) vals = (2 / scale[graph_of[i]]) * that - (i == j): the scaled
 *                   Laplacian, every graph of a batch by its own lambda_max.
 * Outputs, sized by the caller to M (group_ptr M + 1, row_ptr n_nodes + 1, deg n_nodes):
 *   rows, cols, vals, row_ptr   the matrix
 *   group_ptr, member           entry g holds the sorted copies group_ptr[g] .. group_ptr[g + 1] - 1; member[p] = the copy number (c <
 *                               n_edges: edge c; else the diagonal position of node c - n_edges, always last in its entry)
 *   group_of        [M]         the entry that copy c fell into: what a pullback to w reads
 *   adj, deg, sym_tol           nullable: a per entry, d per node (not for ADJ), and per entry (m - 1) * 2^-23 * sum |w| over its m edges
 *                               (0 for m <= 1): the rounding bound ngpde_csr_check_symmetric takes
 *   nnz_out         host: the number of entries.  Synchronises. */
int32_t ngpde_coo_matrix(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t kind, int32_t dir,
                         int32_t add_self_loops, const float *w, int32_t n_graphs, const int32_t *graph_of, const float *scale, int32_t *rows,
                         int32_t *cols, float *vals, int32_t *row_ptr, int32_t *group_ptr, int32_t *member, int32_t *group_of, float *adj,
                         float *deg, float *sym_tol, int64_t *nnz_out, ngpde_stream_t stream);

/* Is the matrix symmetric (src/NeuralGraphPDE.jl:4: what laplacian_lambda_max requires)?  A lane per off-diagonal entry (i, j) looks (j, i)
 * up in row j by bisection; the entry fails if the partner is missing or |vals[i][j] - vals[j][i]| > tol[i][j] + tol[j][i] (tol device
 * float[nnz] or NULL: exact; with the sym_tol of ngpde_coo_matrix two entries of one edge each must be equal).  NGPDE_ERR_INVALID_ARGUMENT
 * names the failing pair with the smallest (i, j).  Synchronises. */
int32_t ngpde_csr_check_symmetric(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *rows, const int32_t *cols, const float *vals,
                                  const float *tol, ngpde_stream_t stream);

/* laplacian_lambda_max (src/NeuralGraphPDE.jl:4): the largest eigenvalue of a SYMMETRIC matrix (NOT CHECKED here) that is block-diagonal
 * over n_graphs graphs, per graph, by a Lanczos iteration that stays on the device; one sparse product per step serves every graph.
 *   graph_of     device int32[n], 0-based, NON-DECREASING (checked on the device: NGPDE_ERR_INVALID_ARGUMENT), or NULL with n_graphs 1
 *   start        v_0[i] = 0.5 + (draw(stream 5, counter (lo32(p), hi32(p))) >> 41) * 2^-23 with p the node's position INSIDE its graph
 *                (uniform in [0.5, 1.5); a member of a batch starts as it would alone), normalised per graph
 *   step j       w = M v_j (8 lanes per row, lane-strided, a fixed xor butterfly); twice: h = [v_0 .. v_j]' w, w -= sum_k h_k v_k (full
 *                reorthogonalisation by two classical Gram-Schmidt passes; alpha_j = the two h_j); beta_j = |w|; v_(j+1) = w / beta_j.
 *                Every inner product is per graph: a 256-thread workgroup per chunk of 1024 nodes of one graph, then one lane per (graph,
 *                vector) adds the graph's partials in chunk order.  The basis (max_iter x n floats) lives in the workspace.
 *   stops        a graph stops after min(max_iter, its node count) steps, or when beta_j <= 8 * 2^-23 * max_k(|alpha_k| + beta_k +
 *                beta_(k-1)) (its Krylov space is exhausted: the value is exact), both decided on the device; alpha and beta are read
 *                back once every 8 steps, the tridiagonal eigenproblem is solved on the host (implicit QL, double) and a graph with
 *                |beta_j * s_last| <= tol * theta stops too.  A stopped graph is frozen: no kernel reads or writes its rows again.
 *   outputs      device: lambda_out float[n_graphs] = theta; residual_out float[n_graphs] (nullable) = |M y - theta y| of the unit Ritz
 *                vector y, by one more product; iterations_out int32[n_graphs] (nullable); vector_out float[n] (nullable) = y.  A graph
 *                without nodes gets 0.
 * max_iter <= 4096; tol finite, >= 0.  Synchronises (setup, every 8 steps, end). */
size_t ngpde_csr_lambda_max_workspace_bytes(int64_t n, int32_t n_graphs, int32_t max_iter);
int32_t ngpde_csr_lambda_max(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *cols, const float *vals, int32_t n_graphs,
                             const int32_t *graph_of, int32_t max_iter, float tol, uint64_t seed, float *lambda_out, float *residual_out,
                             int32_t *iterations_out, float *vector_out, void *workspace, size_t workspace_bytes, ngpde_stream_t stream);

/* khop_adj (src/NeuralGraphPDE.jl:4): C = P A for two n x n matrices by expand, sort, combine.  Entry q of P at (i, j) expands to one term
 * P[i][j] * A[j][c] per entry of row j of A; the terms are written row by row in ascending j (a lane per term, which finds its entry of P
 * by bisection in the scanned counts: a hub row is spread over as many lanes as it has terms), sorted stably by the 64-bit key i*n + c and
 * each entry's terms are added in that order -- ascending middle index -- from the first.  The structure is that of the boolean product:
 * an entry whose terms cancel to 0.0 stays.
 *   ngpde_csr_spgemm_count   total_out host = the number of terms (64-bit count and scan); above `limit` (<= 2^31 - 1)
 *                            NGPDE_ERR_INVALID_ARGUMENT, "the product is too dense".  offsets_out device int64[nnz_p + 1] (nullable) =
 *                            the scanned counts, offsets_out[nnz_p] = the total: what the product takes, so that it counts nothing
 *                            again.  Synchronises.
 *   ngpde_csr_spgemm         offsets, total = what the count wrote for the same matrices; rows_out, cols_out, vals_out sized to total,
 *                            row_ptr_out to n + 1; nnz_out host.  Offsets that do not fit the matrices (a term without a place in its
 *                            row of A, a last offset that is not total) are NGPDE_ERR_INVALID_ARGUMENT, found by the expanding launch,
 *                            which reads nothing through them.  Synchronises once. */
int32_t ngpde_csr_spgemm_count(int64_t n, int64_t nnz_p, const int32_t *p_cols, int64_t nnz_a, const int32_t *a_row_ptr, int64_t limit,
                               int64_t *offsets_out, int64_t *total_out, ngpde_stream_t stream);
int32_t ngpde_csr_spgemm(int64_t n, int64_t nnz_p, const int32_t *p_rows, const int32_t *p_cols, const float *p_vals, int64_t nnz_a,
                         const int32_t *a_row_ptr, const int32_t *a_cols, const float *a_vals, const int64_t *offsets, int64_t total,
                         int32_t *rows_out, int32_t *cols_out, float *vals_out, int32_t *row_ptr_out, int64_t *nnz_out,
                         ngpde_stream_t stream);

/* ---- graph solves (csrc/graph_solve.hip): the inverse side of a graph matrix, what upstream writes as `A \ b` or IterativeSolvers.cg on
 * the SparseMatrixCSC -- an implicit Euler step (I + dt L) u+ = u, a screened Poisson solve, Laplacian smoothing.
 * ngpde_csr_cg solves (shift I + scale M) x_d = b_d for every one of the n_rhs feature rows of B by the conjugate-gradient iteration.
 * shift I + scale M must be SYMMETRIC (NOT CHECKED here: ngpde_csr_check_symmetric) and positive definite (found out by the iteration).
 * M is block-diagonal over n_graphs graphs; every (graph, column) PAIR is its own CG with its own scalars, stop and iteration count.
 *   graph_of     device int32[n], 0-based, NON-DECREASING (checked on the device), or NULL with n_graphs 1
 *   B, x0, X     device float, (n_rhs x n) row-major: column d of the system is the contiguous row d, as GraphMatrix.matmul takes it;
 *                x0 nullable (start at 0).  X may not alias B or x0.
 *   precondition NGPDE_CG_NONE: z = r.  NGPDE_CG_JACOBI: z = r * (1 / (shift + scale * M[i][i])) (M[i][i] = 0 where the diagonal is no
 *                entry); a diagonal that is not > 0 is NGPDE_ERR_INVALID_ARGUMENT naming the smallest such node, found by the launch
 *                that builds the diagonal
 *   iteration    r = b - A x0 (r = b without x0), z, p = z, rho = r . z; step: q = A p, alpha = rho / (p . q), x = x + alpha * p,
 *                r = r - alpha * q, z, rho' = r . z, beta = rho' / rho, p = z + beta * p.  A pair stops with status 0 when
 *                sqrt(r . r) <= max(rtol * sqrt(b . b), atol) (r: the recurrence residual; checked before the first step too, so a start
 *                that solves the system takes 0 iterations), with status 1 after max_iter steps, with status 2 (breakdown: not positive
 *                definite) at a step with p . q <= 0 or a non-finite alpha, beta, rho or r . r; the breaking step changes nothing.  A
 *                stopped pair is frozen: no later launch reads or writes its columns.
 *   sum orders   (the contract: a pair's bits depend on neither n_rhs, the column's place in B, the other graphs of the batch nor
 *                check_every)
 *                product: (A p)[i] = shift * p[i] + scale * s, s = the row's entries in ascending column from 0.0f, one multiply and one
 *                add each.  Inner product: per chunk of 256 rows -- a graph's chunks start at its first node -- the balanced binary tree
 *                over the chunk's rows (row 2 j with 2 j + 1, then pairs of pairs; rows past the graph's end count 0.0f); a graph's chunk
 *                sums are then added in chunk order from 0.0f by every workgroup that needs the scalar.
 *   launches     three per step, every dependency between steps a launch boundary (no cooperative launch, no spin-wait, no float
 *                atomics): q = A p with the chunk sums of p . q | alpha, x, r, z with the chunk sums of r . z and r . r | beta, the
 *                stops, p.  The state is node-major ([n][n_rhs padded]); B is transposed where it is loaded, X where a pair stops.
 *   check_every  0: no read-back at all -- exactly max_iter steps are enqueued, stopped pairs freeze on the device, the call may be
 *                captured into a HIP graph; input the device refuses (graph_of, a CSR list, the diagonal) then leaves every status 2
 *                and X unwritten.  k > 0: the refusals are read once after the setup (named errors) and every k steps ONE word, the
 *                number of pairs still running; the loop ends when it is 0.
 *   outputs      device, [n_graphs][n_rhs]: status_out int32 (0 converged, 1 max_iter reached, 2 breakdown), iterations_out int32,
 *                residual_out float = sqrt(r . r) at the stop.  A graph without nodes: 0, 0, 0.
 * The call allocates nothing: everything lives in `workspace` (ngpde_csr_cg_workspace_bytes; 0 = sizes it refuses), device memory. */
enum { NGPDE_CG_NONE = 0, NGPDE_CG_JACOBI = 1 };
size_t ngpde_csr_cg_workspace_bytes(int64_t n, int32_t n_graphs, int32_t n_rhs);
int32_t ngpde_csr_cg(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *cols, const float *vals, int32_t n_graphs,
                     const int32_t *graph_of, float shift, float scale, int32_t n_rhs, const float *B, const float *x0, float *X,
                     int32_t precondition, float rtol, float atol, int32_t max_iter, int32_t check_every, int32_t *status_out,
                     int32_t *iterations_out, float *residual_out, void *workspace, size_t workspace_bytes, ngpde_stream_t stream);

/* ---- graph queries by node and by pair on a device COO list (src/NeuralGraphPDE.jl:4 re-exports GNNGraphs and with it the Graphs.jl
 * queries a GNNGraph answers: has_edge, neighbors / inneighbors / outneighbors, adjacency_list, intersect, random_walk_pe): "is (s, t)
 * an edge?", "who are node i's neighbours?", "which edges do two graphs share?", and the random-walk positional encoding.  The
 * conventions are those of the blocks above: int32 lists with `index_base`, outputs sized by the caller to the upper bound given with
 * each, sizes <= 2^31 - 1 (refused beyond), NULL and negative arguments refused before any device call (NGPDE_ERR_INVALID_ARGUMENT), a
 * node id outside the node range NGPDE_ERR_DIMENSION_MISMATCH, found on the device by the launch that does the work without a read or
 * write through it, the SMALLEST offending id named; data-dependent counts and errors through the status / HOST pointers after one
 * synchronisation of `stream`.  No float atomics: every result is bitwise equal from run to run and independent of the launch
 * geometry.  Only ngpde_coo_has_edge and ngpde_csr_random_walk_pe allocate nothing and can be captured into a HIP graph. */

/* The sorted-key plan of a list (src/NeuralGraphPDE.jl:4: what has_edge and intersect read): keys_out device uint64[n_edges] = the 64-BIT
 * keys s*n_nodes + t (0-based ends) ascending, positions_out device int32[n_edges] = the COO position of every sorted key.  ONE stable
 * radix sort (the sort of ngpde_coo_coalesce and ngpde_coo_matrix), so equal keys ascend by COO position: the first sorted copy of a
 * pair is its smallest position.  Temporaries from hipMalloc inside the call (not capturable).  Synchronises. */
int32_t ngpde_coo_sort_keys(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, uint64_t *keys_out,
                            int32_t *positions_out, ngpde_stream_t stream);

/* has_edge (src/NeuralGraphPDE.jl:4): one lane per query bisects the plan (keys, positions: what ngpde_coo_sort_keys wrote; NULL with
 * n_edges 0) for the first key >= qs*n_nodes + qt.  qs, qt device int64[n_queries] with `index_base`; found_out device uint8[n_queries]
 * (nullable) = 1 / 0; eid_out device int32[n_queries] (nullable) = the SMALLEST COO position of an edge qs -> qt, or -1; at least one
 * of the two.  status: device uint64[1], the caller's -- the entry zeroes it and the launch leaves 0 there or, if a query end lies
 * outside the node range, a word that is not 0 (such a query gets 0 / -1).  Allocates nothing.  Outside a capture the word is read
 * back after one synchronisation and a bad end is NGPDE_ERR_DIMENSION_MISMATCH naming the smallest; on a stream that is being captured
 * nothing is read back and the word stays with the caller.  Zero queries and zero edges are valid. */
int32_t ngpde_coo_has_edge(int64_t n_nodes, int64_t n_edges, const uint64_t *keys, const int32_t *positions, int64_t n_queries,
                           const int64_t *qs, const int64_t *qt, int32_t index_base, uint8_t *found_out, int32_t *eid_out, uint64_t *status,
                           ngpde_stream_t stream);

/* adjacency_list / neighbors (src/NeuralGraphPDE.jl:4), in two entries like ngpde_csr_spgemm_count / ngpde_csr_spgemm.  The ROW of a node
 * is that of ngpde_coo_sample_neighbors -- the COO positions of its outbound (NGPDE_DIR_OUT) or inbound (NGPDE_DIR_IN) edges in COO order,
 * built by the same code (csrc/coo_rows.h) -- so parallel edges repeat and self loops are included.  nodes: device int64[n_listed],
 * 0-based, in any order, repeats allowed (a node listed twice gets two rows), or NULL (with n_listed 0): every node.
 *   ngpde_coo_adjacency_count   row_ptr_out int32[n_nodes + 1], row_eid_out int32[n_edges]: the rows of ALL nodes (what the fill reads);
 *                               ptr_out int32[R + 1] (R = n_listed, or n_nodes with nodes NULL) = the exclusive scan of the listed rows'
 *                               lengths (counted and scanned in 64 bits); total_out host = ptr_out[R], above 2^31 - 1
 *                               NGPDE_ERR_INVALID_ARGUMENT.  A listed id outside the node range is NGPDE_ERR_DIMENSION_MISMATCH.
 *                               Temporaries from hipMalloc.  Synchronises.
 *   ngpde_coo_adjacency_fill    neighbors_out, eid_out int32[total]: row i of the result is neighbors_out[ptr[i] .. ptr[i + 1] - 1] = the
 *                               other ends (as stored: with the list's index base) and eid_out = their COO positions.  One lane per
 *                               OUTPUT ELEMENT, which finds its row by bisection in ptr: a hub's row is spread over as many lanes as it
 *                               has neighbours.  Lists that are not what the count wrote (an element without a place in its row, a last
 *                               offset that is not total) are NGPDE_ERR_INVALID_ARGUMENT, found by the launch, which reads nothing
 *                               through them.  Synchronises once. */
int32_t ngpde_coo_adjacency_count(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                                  int64_t n_listed, const int64_t *nodes, int32_t *row_ptr_out, int32_t *row_eid_out, int32_t *ptr_out,
                                  int64_t *total_out, ngpde_stream_t stream);
int32_t ngpde_coo_adjacency_fill(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t dir, int64_t n_listed,
                                 const int64_t *nodes, const int32_t *row_ptr, const int32_t *row_eid, const int32_t *ptr, int64_t total,
                                 int32_t *neighbors_out, int32_t *eid_out, ngpde_stream_t stream);

/* intersect (src/NeuralGraphPDE.jl:4): the DISTINCT pairs (s, t) that are edges of both lists, in the order of their first appearance
 * in the first list.  (s, t): the first list; keys, positions: its plan; keys2 uint64[n_edges2]: the sorted keys of the second list's
 * plan (same n_nodes).  One lane per edge of the first list: it is kept iff its position is the one its own plan lists first for
 * its key and the key occurs in keys2 (two bisections); then the stable compaction of ngpde_coo_compact (csrc/coo_compact.h): s_out,
 * t_out int32[n_edges], kept int64[n_edges] (upper bounds) = the kept edges' positions in the first list, n_out host.  Temporaries
 * from hipMalloc.  Synchronises. */
int32_t ngpde_coo_intersect(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, const uint64_t *keys,
                            const int32_t *positions, int64_t n_edges2, const uint64_t *keys2, int32_t *s_out, int32_t *t_out, int64_t *kept,
                            int64_t *n_out, ngpde_stream_t stream);

/* random_walk_pe (src/NeuralGraphPDE.jl:4): pe float[walk_length][n], pe[k - 1][i] = (RW^k)[i][i].  No gradient, as upstream.
 *   A            (row_ptr, cols, vals) = adjacency_matrix(g, dir = out, weighted) exactly as ngpde_coo_matrix(NGPDE_MATRIX_ADJ) assembles
 *                it: coalesced, weights summed in COO order, entries ordered by row, then column
 *   d[j]         the sum of row j's entries, front to back, from 0.0f;  inv[j] = d[j] == 0 ? 0 : 1.0f / d[j]
 *   RW[i][j]     = A[i][j] * inv[j], rounded once.  A node without outgoing weight has an all-zero column: its pe is 0, never inf / nan
 *   Y = RW X     per row i and column c: Y[i][c] = the sum over the entries of row i IN ASCENDING COLUMN ORDER, from 0.0f, of
 *                RW[i][j] * X[j][c], every term one multiply and one add, each rounded (the library is built with -ffp-contract=off)
 * Seeds are taken in blocks of `block` consecutive nodes [b0, b0 + block): the state X [n][block] holds in column c the walk started
 * at node b0 + c (X_0 = those rows of the identity), one step is X <- RW X, ping-ponged between two buffers of the workspace, and the
 * step's launch stores the diagonal itself: the wave that finishes row i in [b0, b0 + block) writes Y[i][i - b0] to pe[k - 1][i].  A wave
 * per (row, 64 or 256 columns), the lanes over the columns, so an entry's row of X is one contiguous read.  ceil(n / block) *
 * walk_length step launches and one init launch per block.
 *   block        a multiple of 64 (anything else NGPDE_ERR_INVALID_ARGUMENT); 0: the library's choice (256, fewer for fewer nodes or where
 *                the state would pass 256 MiB).  Columns are independent and every sum has a fixed order: THE RESULT DOES NOT DEPEND ON
 *                IT, nor on the grid, nor on whether a graph is solved alone or as a member of a batch.
 *   graph_of     device int32[n], 0-based, or NULL with n_graphs 1: the matrix is block-diagonal over the graphs (NOT CHECKED).  Where
 *                graph_of is non-decreasing (checked on the device) a block's launches cover only the rows of the graphs its seeds lie
 *                in -- a batch costs the sum of N_g^2, not N^2 --, otherwise all rows.  An id outside 0 : n_graphs - 1 is
 *                NGPDE_ERR_INVALID_ARGUMENT.
 *   workspace    ngpde_csr_random_walk_pe_workspace_bytes(n, block) = 2 * n * block * 4 (the two states) plus a part that does not depend
 *                on block: n * 4 rounded up to a multiple of 256 (inv) + 256 (flag words); 0 for invalid arguments.  16-byte aligned.
 * Allocates nothing.  Outside a capture it synchronises once before the first step (the flags and the row ranges are read back; a
 * column or row pointer outside the matrix is NGPDE_ERR_DIMENSION_MISMATCH); on a stream that is being captured nothing is read back,
 * every launch covers all rows -- the same bits -- and a column outside the matrix contributes nothing. */
size_t ngpde_csr_random_walk_pe_workspace_bytes(int64_t n, int32_t block);
int32_t ngpde_csr_random_walk_pe(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *cols, const float *vals, int32_t n_graphs,
                                 const int32_t *graph_of, int32_t walk_length, int32_t block, float *pe, void *workspace, size_t workspace_bytes,
                                 ngpde_stream_t stream);

/* ---- graph traversal on a device COO list (csrc/graph_traverse.hip; src/NeuralGraphPDE.jl:4 re-exports GNNGraphs, whose GNNGraph is a
 * Graphs.AbstractGraph -- `using Graphs`, src/NeuralGraphPDE.jl:16 -- so that connected_components, is_connected, gdistances and
 * neighborhood work on it): "which nodes hang together?" and "how many edges from the nearest source?".  The conventions are those of
 * the block above: int32 lists with `index_base`, sizes <= 2^31 - 1 (refused beyond), NULL and negative arguments refused before any
 * device call (NGPDE_ERR_INVALID_ARGUMENT), an edge end or a listed node outside the node range NGPDE_ERR_DIMENSION_MISMATCH, found on
 * the device by the launch that does the work without a read or write through it, the SMALLEST offending id named.  Every result but
 * the shortest paths is an integer and the only atomics are integer min / or / add, which commute: the bits depend neither on the COO
 * order, the launch geometry nor the run (the float32 shortest paths use no atomic in their rounds and are as reproducible: their
 * comment).  Kernel boundaries are the only synchronisation (no spin-wait, no grid barrier).
 *   check_every  as in ngpde_csr_cg.  k > 0: rounds / levels are enqueued in groups of k; every launch exits at once when the round /
 *                level before it found nothing, and the host reads the 64-byte control block once per group (the named errors with
 *                the first).  0: nothing is read back, exactly max_rounds rounds / max_hops levels are enqueued, the call allocates
 *                nothing and may be captured into a HIP graph; input the device refuses is skipped and not raised. */

/* connected_components, the labelling (src/NeuralGraphPDE.jl:4, :16): weak connectivity, the edges seen as undirected; self loops,
 * parallel edges, isolated nodes and n_edges 0 are valid.  labels_out device int32[n_nodes]: the SMALLEST MEMBER (0-based) of every
 * node's component -- a function of the edge set alone.  Root hooking with compression on labels_out itself (parent[i] = i to start):
 *   round        hook: one lane per edge reads the roots of its two ends and, where they differ, runs an agent-scope int32 atomicMin
 *                on parent[larger root] with the smaller.  compress: every parent[i] is brought to its root by path halving --
 *                parent[i] <- its ancestor 8 links up, in place -- in ceil(ceil(log2 n) / 3) launches, each of which exits at once when
 *                the one before found every node at its root: a chain of depth n (a sequentially numbered path after its first hook)
 *                costs log launches, not n loads in one lane.  1 + ceil(ceil(log2 n) / 3) launches per round, 4 bytes per node.
 *   stale reads  parent[x] <= x always, so there is no cycle.  Within a launch a lane may read a value of parent[x] that another
 *                compute unit has since lowered; every value it can read is a start-of-round root of x's true component (hook) or an
 *                ancestor of x (compress), and the kernels are correct for each (csrc/graph_traverse.hip, the file comment).
 *   stop         the first round that hooks nothing.  max_rounds 0: the library's choice, 2 * ceil(log2(max(n, 2))) + 8 rounded up to
 *                whole groups.  Still hooking after max_rounds rounds: NGPDE_ERR_STATE (check_every > 0), never a silent partial answer.
 *   rounds_out   device int32[2], nullable: [0] the rounds run, the confirming one included; [1] 1 if the last enqueued round still
 *                hooked (what a caller with check_every 0 reads instead of the status).
 *   workspace    ngpde_coo_components_workspace_bytes(n_nodes) = 256 (the control block); 0 for sizes it refuses.  8-byte aligned. */
size_t ngpde_coo_components_workspace_bytes(int64_t n_nodes);
int32_t ngpde_coo_components(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t max_rounds,
                             int32_t check_every, int32_t *labels_out, int32_t *rounds_out, void *workspace, size_t workspace_bytes,
                             ngpde_stream_t stream);

/* connected_components, the ranking (src/NeuralGraphPDE.jl:4, :16): from labels (what ngpde_coo_components wrote; anything else is
 * NGPDE_ERR_INVALID_ARGUMENT, found on the device) the components ranked by their smallest member.  A root flag and an exclusive scan
 * (rocPRIM) give rank_out int32[n_nodes]; ONE stable radix sort of the ranks with the node ids gives order_out int32[n_nodes], the nodes
 * grouped by component and ascending inside it; ptr_out int32[n_nodes + 1] (upper bound; count + 1 written) by bisection, component k =
 * order_out[ptr_out[k] .. ptr_out[k + 1] - 1]; sizes_out int32[n_nodes] (upper bound; count written); count_out HOST.  per_graph_out
 * device int32[n_graphs], nullable: the components of every graph of a batch (graph_of device int32[n_nodes], 0-based, any order, or
 * NULL with n_graphs 1; an id outside 0 : n_graphs - 1 is NGPDE_ERR_INVALID_ARGUMENT).  Temporaries from hipMalloc.  Synchronises. */
int32_t ngpde_components_rank(int64_t n_nodes, const int32_t *labels, int32_t n_graphs, const int32_t *graph_of, int32_t *rank_out,
                              int32_t *sizes_out, int32_t *order_out, int32_t *ptr_out, int64_t *count_out, int32_t *per_graph_out,
                              ngpde_stream_t stream);

/* The rows plan of a list (src/NeuralGraphPDE.jl:4, :16: what the level loop below walks): the by-node rows of csrc/coo_rows.h -- the one
 * definition ngpde_coo_sample_neighbors and ngpde_coo_adjacency_count use -- grouped by source (NGPDE_DIR_OUT) or target (NGPDE_DIR_IN),
 * COO order inside a row.  row_ptr_out int32[n_nodes + 1]; row_other_out int32[n_edges] = the 0-BASED other end of every row entry.
 * Temporaries from hipMalloc.  Synchronises. */
int32_t ngpde_coo_rows(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                       int32_t *row_ptr_out, int32_t *row_other_out, ngpde_stream_t stream);

/* gdistances (src/NeuralGraphPDE.jl:4, :16): breadth-first levels by a level-synchronous PULL on 64-bit source masks.  (row_ptr_a,
 * other_a, nnz_a) and, for both directions, a second set b (NULL, NULL, 0 otherwise) are rows plans: node v is reached at a level from
 * the other ends of its rows that were reached at the level before.  Following edges s -> t needs the rows grouped by TARGET
 * (NGPDE_DIR_IN), against them the rows grouped by source, either way both.
 *   sources      device int64[n_sources] with `index_base`, any order, repeats allowed
 *   separate 0   dist_out int32[n]: the edges on a shortest path from the NEAREST source (all sources share mask bit 0; one pass)
 *   separate 1   dist_out int32[n_sources][n]: row i from source i alone; 64 sources per pass (bit b = source b of the pass),
 *                ceil(n_sources / 64) passes
 *   max_hops     nodes further than max_hops edges, and unreachable ones, get -1; negative: no bound (needs check_every > 0)
 *   level        ONE launch, a lane per node: it ORs the frontier words of the other ends of its rows, masks with ~seen[v], stores the
 *                level for every new bit, writes seen[v] and next[v] -- a lane writes its own node only: no atomics, no race, the same
 *                bits whatever the geometry.  A row of NGPDE_HOP_WAVE_ROW entries or more is walked by the whole wave with an OR
 *                across its lanes: a hub row does not serialise on one lane.  A node that has seen every source reads no row.
 *   workspace    ngpde_csr_hop_distance_workspace_bytes(n) = 3 * (8 n rounded up to 256) + 256: seen and the double-buffered frontier,
 *                24 bytes per node, and the control block; 0 for sizes it refuses.  8-byte aligned.
 * A row pointer or entry outside the lists is NGPDE_ERR_DIMENSION_MISMATCH (nothing is read through it). */
#define NGPDE_HOP_WAVE_ROW 64
size_t ngpde_csr_hop_distance_workspace_bytes(int64_t n);
int32_t ngpde_csr_hop_distance(int64_t n, int64_t nnz_a, const int32_t *row_ptr_a, const int32_t *other_a, int64_t nnz_b,
                               const int32_t *row_ptr_b, const int32_t *other_b, int64_t n_sources, const int64_t *sources, int32_t index_base,
                               int32_t separate, int64_t max_hops, int32_t check_every, int32_t *dist_out, void *workspace,
                               size_t workspace_bytes, ngpde_stream_t stream);

/* neighborhood (src/NeuralGraphPDE.jl:4, :16): nodes_out int64[n] (upper bound) = the nodes with dist[i] >= 0, ascending, with
 * `index_base`; n_out HOST.  The flags -> exclusive scan -> scatter of csrc/coo_compact.h.  Temporaries from hipMalloc.  Synchronises. */
int32_t ngpde_hop_reached_nodes(int64_t n, const int32_t *dist, int32_t index_base, int64_t *nodes_out, int64_t *n_out, ngpde_stream_t stream);

/* The rows plan with its COO positions (src/NeuralGraphPDE.jl:4, :16: what the relaxation rounds below walk): ngpde_coo_rows, and
 * row_eid_out int32[n_edges] = the 0-BASED COO position of every row entry (the `eid` of csrc/coo_rows.h, which ngpde_coo_rows drops):
 * the weight of an entry is weights[eid], and a tree edge is named by it.  Temporaries from hipMalloc.  Synchronises. */
int32_t ngpde_coo_rows_eid(int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int32_t index_base, int32_t dir,
                           int32_t *row_ptr_out, int32_t *row_other_out, int32_t *row_eid_out, ngpde_stream_t stream);

/* dijkstra_shortest_paths / bellman_ford_shortest_paths (src/NeuralGraphPDE.jl:4, :16): weighted shortest paths by synchronous
 * relaxation rounds (csrc/graph_paths.hip).  The rows plans a and b (NULL, NULL, NULL, 0 otherwise) are those of ngpde_coo_rows_eid for ONE
 * list, so nnz_b, where given, equals nnz_a = E; the directions are ngpde_csr_hop_distance's (following s -> t: the rows grouped by TARGET).
 *   weights      device float[nnz_a] in COO order, or NULL: 1 per edge.  +inf and 0 are valid; a NEGATIVE or NaN weight is
 *                NGPDE_ERR_INVALID_ARGUMENT, found on the device by the launch that gathers the weights into row order (so that a
 *                round's loads are contiguous), the SMALLEST offending 0-based COO position named; nothing is relaxed through it.
 *   sources      device int64[n_sources] with `index_base`, any order, repeats allowed; one outside the node range is
 *                NGPDE_ERR_DIMENSION_MISMATCH, the smallest named
 *   separate 0   dist_out float[n]: the distance from the NEAREST source.  separate 1: dist_out float[n_sources][n], row i from
 *                source i alone; NGPDE_SSSP_PASS sources per pass, ceil(n_sources / NGPDE_SSSP_PASS) passes, ONE launch per round
 *                covers every source of a pass (grid y: groups of NGPDE_SSSP_LANE_SOURCES sources, which a lane relaxes from one read
 *                of its row; a lane's stores into row i of the [n_sources][n] outputs are contiguous across the wave)
 *   the result   d = the FIXED POINT of d[v] = min(d[v], min over row entries p of fl32(d[other[p]] + w[p])) that the rounds descend to
 *                from d0 = 0 at the sources, +inf elsewhere: the greatest one below d0, every value the fp32 length of a walk from
 *                a source.  fp32 addition is monotone, so d is a pure function of graph, weights and sources, bitwise what a
 *                float32 heap Dijkstra returns; +inf where unreachable or farther than max_dist (candidates above max_dist are
 *                dropped: exact, because distances do not decrease along a path; +inf: no bound; negative or NaN refused)
 *   round        DOUBLE-BUFFERED: round r reads only the values of round r - 1 (two buffers of the workspace alternate; a lane that
 *                lowers a distance also stores it, and the tree edge, into the caller's arrays, which so hold the last value of
 *                every cell).  ONE launch, __launch_bounds__(256), a lane per (node, source group): it writes its own cells only
 *                -- no atomics, no race, the same bits whatever the geometry; the only flag writes are the plain "changed"
 *                stores into three rotating control words (csrc/traverse_rounds.h).  A launch exits at once when the round before changed nothing.
 *                The round buffers are one slab [n][NGPDE_SSSP_LANE_SOURCES] per group of sources (the last group padded): what a
 *                round gathers, the distances of a row entry's other end for the lane's sources, is one aligned 16-byte load,
 *                and a wave's own cells are contiguous.
 *                A row of NGPDE_SSSP_WAVE_ROW entries or more is walked by the whole wave, which reduces (distance, row position)
 *                lexicographically.  Kernel boundaries are the only synchronisation.
 *   parents      parent_eid_out / parent_out int32, shaped like dist_out, each nullable: the COO position of the tree edge into
 *                every node and the 0-based node at its other end; -1 at sources and unreached nodes.  Written only when the node's
 *                distance STRICTLY decreases; among the equal candidates of one round the first in row order wins (COO order inside
 *                a row, set a before set b).  Rounds are defined, so parents and rounds_out are pure functions too, every parent
 *                edge is tight -- fl32(d[parent] + w) == d[v] -- and the parents form a tree also with zero or absorbed weights.
 *   max_rounds   0: the library's choice, n (a shortest path has fewer than n edges, so n rounds suffice, the confirming one
 *                included).  Still changing after max_rounds rounds: NGPDE_ERR_STATE (check_every > 0), never a silent partial answer.
 *   check_every  as above; 0 needs max_rounds > 0 and replays from a HIP graph
 *   rounds_out   device int32[2], nullable: [0] the rounds run, the confirming one included (the largest over the passes); [1] 1 if
 *                the last enqueued round of a pass still changed a distance (what a caller with check_every 0 reads)
 *   workspace    ngpde_csr_shortest_paths_workspace_bytes(n, nnz_a, nnz_b, n_sources, separate) = (2 x 4 n width + 4 nnz_a +
 *                4 nnz_b, each term rounded up to 256) + 256: the two round buffers of a pass, the weights in row order and the
 *                control block; width = 1 for one row of dist_out, else min(n_sources, NGPDE_SSSP_PASS) rounded up to a multiple
 *                of NGPDE_SSSP_LANE_SOURCES; 0 for sizes it refuses.  16-byte aligned.
 * A row pointer, entry or COO position outside the lists is NGPDE_ERR_DIMENSION_MISMATCH (nothing is read through it). */
#define NGPDE_SSSP_WAVE_ROW 64
#define NGPDE_SSSP_PASS 64
#define NGPDE_SSSP_LANE_SOURCES 4
size_t ngpde_csr_shortest_paths_workspace_bytes(int64_t n, int64_t nnz_a, int64_t nnz_b, int64_t n_sources, int32_t separate);
int32_t ngpde_csr_shortest_paths(int64_t n, int64_t nnz_a, const int32_t *row_ptr_a, const int32_t *other_a, const int32_t *eid_a,
                                 int64_t nnz_b, const int32_t *row_ptr_b, const int32_t *other_b, const int32_t *eid_b, int64_t n_sources,
                                 const int64_t *sources, int32_t index_base, int32_t separate, const float *weights, float max_dist,
                                 int32_t max_rounds, int32_t check_every, float *dist_out, int32_t *parent_eid_out, int32_t *parent_out,
                                 int32_t *rounds_out, void *workspace, size_t workspace_bytes, ngpde_stream_t stream);

/* GNOConv message (src/layers.jl:527-530): K_e = reshape(phi_out[:, e], cout, cin) column-major,
 * m_e = K_e * h[:, s_e].  k: [E][cin*cout] p order (element o + cout*i), h: [N][cin], m: [E][cout]. */
int32_t ngpde_gno_contract_forward(const ngpde_graph_t *g, int32_t cin, int32_t cout, const float *k, const float *h,
                                   float *m, ngpde_stream_t stream);
/* dk [E][cin*cout] nullable, dh [N][cin] nullable (needs workspace of n_edges*cin*4 bytes) */
int32_t ngpde_gno_contract_backward(const ngpde_graph_t *g, int32_t cin, int32_t cout, const float *k, const float *h,
                                    const float *dm, float *dk, float *dh, void *workspace, size_t workspace_bytes,
                                    ngpde_stream_t stream);

/* GNOConv message in reassociated form: when the last layer of phi is Dense(k => in*out) with identity activation,
 *   m_e = reshape(W2 z_e + b2, out, in) h_j = T_j z_e + Bh_j,   T_j[o][kk] = sum_i W2[o + out*i][kk] h_j[i]  (node level),
 * so the in*out x E kernel tensor of src/layers.jl:527 is never formed.  t: [N][cout*kdim] (element o*kdim + kk),
 * bh: [N][cout] or NULL, z: [E][kdim] last hidden activation of phi (p order), m: [E][cout] (p order).
 * Backward: dt [N][cout*kdim], dbh [N][cout], dz [E][kdim], each nullable. */
int32_t ngpde_gno_apply_supported(int32_t cout, int32_t kdim);
int32_t ngpde_gno_apply_forward(const ngpde_graph_t *g, int32_t cout, int32_t kdim, const float *t, const float *bh,
                                const float *z, float *m, ngpde_stream_t stream);
int32_t ngpde_gno_apply_backward(const ngpde_graph_t *g, int32_t cout, int32_t kdim, const float *t, const float *z,
                                 const float *dm, float *dt, float *dbh, float *dz, ngpde_stream_t stream);

/* The reassociated message with its per-edge input formed in the same launch:  z_e = act1(P[t_e] + Q[s_e] + E_e)  (the first Dense
 * of phi split into node-level terms, as ngpde_edge_combine_forward),  m_e = T_{s_e} z_e + Bh_{s_e}; the message is a per-source
 * GEMM on the matrix pipe (out a multiple of 16, k in {16, 32, 64}: ngpde_gno_message_supported).  z_out [E][k] (p order,
 * nullable) keeps the ACTIVATED input for the pullback, which is ngpde_gno_apply_backward followed by
 * ngpde_edge_combine_backward (for identity / relu the activated value serves as `z` there). */
int32_t ngpde_gno_message_supported(int32_t cout, int32_t kdim);
int32_t ngpde_gno_message_forward(const ngpde_graph_t *g, int32_t cout, int32_t kdim, int32_t act1, const float *p_target,
                                  const float *q_source, const float *e_term, const float *t, const float *bh, float *z_out, float *m,
                                  ngpde_stream_t stream);

/* Pullback of ngpde_gno_message_forward FOLLOWED BY the sum / mean aggregation over targets (aggregate_neighbors(g, aggr, m),
 * /root/reference/src/layers.jl:527-534), from the node-level gradient dagg [N][out]: dm_e = dagg[t_e] (sum) or dagg[t_e] /
 * deg(t_e) (mean) is formed while the per-source launch stages its rows, so the [E][out] array ngpde_segment_reduce_backward
 * would write (231 MB at BASELINE config 5, r = 0.1) is neither written nor read.  z [E][k] = z_out of the forward (the
 * ACTIVATED per-edge input), act1 identity or relu.  Outputs: dt [N][out][k], dbh [N][out] (nullable) as
 * ngpde_gno_apply_backward; dz [E][k] (p order, nullable) is the gradient of the PRE-activation, T_s^T dm_e . act1'(z_e) -- so
 * dE = dz, dP = its sums by target (ngpde_segment_reduce_forward with NGPDE_AGGR_SUM) --; dq [N][k] (nullable, needs dz) = its
 * sums by source, formed in the launch (every edge of a workgroup has the same source).  NGPDE_ERR_UNSUPPORTED for max / min /
 * mul, other activations, and shapes outside ngpde_gno_message_supported. */
int32_t ngpde_gno_message_backward_from_nodes(const ngpde_graph_t *g, int32_t cout, int32_t kdim, int32_t aggr, int32_t act1,
                                              const float *t, const float *z, const float *dagg, float *dt, float *dbh, float *dz,
                                              float *dq, ngpde_stream_t stream);

/* GNOConv's aggregated message with the EDGE index contracted first, per target over its CSR row (/root/reference/src/layers.jl:523-534;
 * the other reassociation of m_i = aggr_{e -> i} reshape(W2 z_e + b2, out, in) h_{s_e}):
 *   ngpde_gno_gform_aggregate:  z_e = act1(P[t_e] + Q[s_e] + E_e) as in ngpde_gno_message_forward;  gout [N][k][in]:
 *     G_i[k][i'] = sum_{e -> i} z_e[k] h_{s_e}[i']  (Z_i^T H_i on the matrix pipe);  hsum [N][in] (nullable) = sum_{e -> i} h_{s_e};
 *     both divided by deg(i) when `mean`;  z_out [E][k] (p order, nullable) keeps the activated input for the pullback.
 *     k = 64 and in in {32, 64, 128} (ngpde_gno_gform_supported); every array 16-byte aligned.
 *   ngpde_gno_gform_transform:  y [N][out] = act.(G W2' + hsum B2 + h W + bias)  with W2' = phi's last weight (k x in*out, Julia
 *     (in*out x k)) read as the [k*in][out] matrix it is in memory (row k*in + i', column o  <->  K_e[o, i'] = phi_out[o + out*i'],
 *     :525), the contraction split into `nsplit` slabs (ngpde_gno_gform_splits); the b2 term (hsum [N][in] with b2 read as
 *     B2[i'][o] = b2[o + out*i']; both or neither NULL) and the layer's own linear map (h [N][in], w [in][out]; both or neither NULL) are
 *     two more slabs of the SAME launch; slabs [nsplit + 2][N][out] is scratch; bias nullable; zt (nullable) keeps the pre-activation
 *     (:536).  in a multiple of 16, out of 4.
 * No [E][out] message array, no scatter, no atomics; the pullback is the by-source form's (ngpde_gno_message_backward_from_nodes). */
int32_t ngpde_gno_gform_supported(int32_t in_chs, int32_t kdim);
/* does ngpde_gno_layer_* take this form for the shape?  (inference: whenever supported; training: from about 64 edges per node, where
 * it wins back the T = W2 (x) h that the by-source pullback needs and only the by-source forward leaves behind) */
int32_t ngpde_gno_gform_preferred(int64_t n_nodes, int64_t n_edges, int32_t in_chs, int32_t kdim, int32_t cout, int32_t training);
int32_t ngpde_gno_gform_splits(int64_t n_nodes, int32_t in_chs, int32_t kdim, int32_t cout);
int32_t ngpde_gno_gform_aggregate(const ngpde_graph_t *g, int32_t in_chs, int32_t kdim, int32_t act1, int32_t mean, const float *p_target,
                                  const float *q_source, const float *e_term, const float *h, float *gout, float *hsum, float *z_out,
                                  ngpde_stream_t stream);
int32_t ngpde_gno_gform_transform(int64_t n_nodes, int32_t in_chs, int32_t kdim, int32_t cout, int32_t act, const float *gin, const float *w2,
                                  const float *hsum, const float *b2, const float *h, const float *w, const float *bias, float *y, float *zt,
                                  float *slabs, int32_t nsplit, ngpde_stream_t stream);

/* GAT-style aggregation [GraphNeuralNetworks.jl GATConv]: wx [N][heads*c] (= reshape(W x, c, heads, N)),
 * a (2c x heads) column-major; logit_e = leakyrelu(a[1:c,k].Wx[:,k,t_e] + a[c+1:2c,k].Wx[:,k,s_e]);
 * alpha = softmax over the incoming edges of each node; out[N][heads*c] = sum_e alpha_e Wx[s_e].
 * Saved for backward: alpha [E][heads] (p order), al, ar [N][heads]. */
int32_t ngpde_gat_forward(const ngpde_graph_t *g, int32_t heads, int32_t c, float negative_slope, const float *wx,
                          const float *a, float *out, float *alpha, float *al, float *ar, ngpde_stream_t stream);
size_t ngpde_gat_workspace_bytes(const ngpde_graph_t *g, int32_t heads);
int32_t ngpde_gat_backward(const ngpde_graph_t *g, int32_t heads, int32_t c, float negative_slope, const float *wx,
                           const float *a, const float *al, const float *ar, const float *alpha, const float *dout,
                           float *dwx, float *da, void *workspace, size_t workspace_bytes, ngpde_stream_t stream);

/* The whole GAT-style layer  y = act.(GAT(x) .+ b)  with W (heads*c x din), a (2c x heads), heads concatenated, in ONE launch
 * (pullback: two launches + one reduction) when din == heads * c == 64, heads in {1, 2, 4} and the graph's tiles fit the LDS halo
 * in both directions (ngpde_gat_layer_supported; BASELINE config 3 = 64 => 4 x 16): W x of the rows a tile stages (its own and its
 * halo) is formed on the matrix pipe inside the launch, logits and messages work on it per head; no W x array exists in memory.  Self loops are edges of g (the caller appends them, as GATConv's add_self_loops does).
 *   save_alpha [E][heads] nullable: attention coefficients in p order, the sign bit carrying leakyrelu's branch (pullback only)
 *   save_z     [N][64] nullable: pre-activation (the pullback of activations other than identity / relu needs it)
 * backward: y_or_z = y for relu, z otherwise (ignored for identity); dx nullable; dweight (64 x 64) column-major, da (2c x heads),
 * dbias [64] nullable.  workspace: ngpde_gat_layer_workspace_bytes. */
int32_t ngpde_gat_layer_supported(const ngpde_graph_t *g, int32_t din, int32_t heads, int32_t c);
size_t ngpde_gat_layer_workspace_bytes(const ngpde_graph_t *g, int32_t heads, int32_t c);
int32_t ngpde_gat_layer_forward(const ngpde_graph_t *g, int32_t din, int32_t heads, int32_t c, float negative_slope, int32_t act,
                                const float *x, const float *weight, const float *a, const float *bias, float *y,
                                float *save_alpha, float *save_z, ngpde_stream_t stream);
int32_t ngpde_gat_layer_backward(const ngpde_graph_t *g, int32_t din, int32_t heads, int32_t c, float negative_slope, int32_t act,
                                 const float *x, const float *weight, const float *a, const float *y_or_z, const float *save_alpha,
                                 const float *dy, float *dx, float *dweight, float *da, float *dbias, void *workspace,
                                 size_t workspace_bytes, ngpde_stream_t stream);

/* y = act.(a .+ addend .+ b): the tail of a layer whose linear part was computed elsewhere -- GNOConv's
 * sigma(W x + m + b) (src/layers.jl:536-547) with a = aggregated messages, addend = W x; the GAT-style layer's bias + activation.
 * a, y [n][d]; addend [n][d] nullable; bias [d] nullable; save_z nullable.  Backward: dz = dy .* act'(z) (the gradient of a AND
 * of addend; for the identity dz may alias dy and the pass is skipped), dbias = column sums of dz (nullable; needs the workspace). */
int32_t ngpde_bias_act_forward(int64_t n, int32_t d, int32_t act, const float *a, const float *addend, const float *bias, float *y,
                               float *save_z, ngpde_stream_t stream);
size_t ngpde_bias_act_workspace_bytes(int32_t d);
int32_t ngpde_bias_act_backward(int64_t n, int32_t d, int32_t act, const float *dy, const float *z, float *dz, float *dbias,
                                void *workspace, size_t workspace_bytes, ngpde_stream_t stream);

/* Fused message path  m_i = aggr_{e: t_e = i} phi(...)  for a message MLP whose first layer has been split into
 * node-level terms (ngpde_edge_combine_forward) and whose remaining layers are Dense, all widths <= 64 and
 * multiples of 4, at most 3 layers after the first (e.g. MPPDEConv 132 => 64 => 64, src/layers.jl:402-416; the VMH
 * tutorial's 4 => 60 => 60 => 60 => 40, docs/src/tutorials/VMH.md:75-79): gather through LDS, MFMA layers with
 * LDS-resident weights, in-tile segmented reduction; no per-edge array is written unless save_z[l] is non-NULL
 * (save_z[0]: z1 [E][h1]; save_z[l]: pre-activation of layer l [E][tail_dout[l-1]], p order) for the pullback.
 * Needs ngpde_graph_set_gcn_norm to have been called (it builds the tile schedule) and a graph whose tiles fit
 * the LDS halo; ngpde_edge_mlp_supported returns 1 when this entry can be used, otherwise compose the
 * primitives above.  aggr: + / mean / max / min / * (NGPDE_AGGR_MUL: an empty neighbourhood gives 1, like scatter(*)).
 * out: [N][last width]. */
int32_t ngpde_edge_mlp_supported(const ngpde_graph_t *g, int32_t h1, int32_t n_tail, const int32_t *tail_dout);
int32_t ngpde_edge_mlp_forward(const ngpde_graph_t *g, int32_t h1, int32_t act1, const float *p_target,
                               const float *q_source, const float *e_term, int32_t n_tail, const int32_t *tail_dout,
                               const int32_t *tail_act, const float *const *tail_weight, const float *const *tail_bias,
                               int32_t aggr, float *out, float *const *save_z, ngpde_stream_t stream);
/* Fused pullback of the same message path for 0 or 1 Dense layer after the first and any of the five aggregations (*: a first pass over
 * a tile's edges forms each target's product of the nonzero messages and the number of zeros; every message then receives the gradient
 * times the product of the OTHERS -- the one zero message of a row the product of the rest, nothing where two are zero; max / min: the
 * first pass leaves the target's extremum and every message equal to it receives the gradient, as NNlib's scatter pullback): recomputes the
 * per-edge activations inside the tile (nothing per-edge has to be saved by the forward), accumulates the tail layer's
 * weight / bias gradient on MFMA in per-workgroup slabs, writes dz1 once ([E][h1], p order: de_term, required -- it is the
 * gradient of the per-edge first-layer term and the input of the by-source sum that gives dq_source) and sums it per target
 * into dp_target.  dout: [N][last width] gradient of the aggregated messages.
 * Without a per-edge first-layer term (e_term NULL: MPPDEConv on graphs without edge features, src/layers.jl:407-410) the
 * 64-wide two-layer specialisation sums dz1 by source inside its launch where every tile's halo has at most 48 rows (meshes):
 * de_term may then be NULL and no [E][h1] array exists at all (ngpde_edge_mlp_backward_needs_edge_buffer returns 0). */
int32_t ngpde_edge_mlp_backward_supported(const ngpde_graph_t *g, int32_t h1, int32_t n_tail, const int32_t *tail_dout, int32_t aggr);
int32_t ngpde_edge_mlp_backward_needs_edge_buffer(const ngpde_graph_t *g, int32_t h1, int32_t act1, int32_t has_e_term, int32_t n_tail,
                                                   const int32_t *tail_dout, const int32_t *tail_act, int32_t aggr);
size_t ngpde_edge_mlp_backward_workspace_bytes(const ngpde_graph_t *g, int32_t h1, int32_t n_tail, const int32_t *tail_dout);
int32_t ngpde_edge_mlp_backward(const ngpde_graph_t *g, int32_t h1, int32_t act1, const float *p_target, const float *q_source,
                                const float *e_term, int32_t n_tail, const int32_t *tail_dout, const int32_t *tail_act,
                                const float *const *tail_weight, const float *const *tail_bias, int32_t aggr, const float *dout,
                                float *dp_target, float *dq_source, float *de_term, float *const *dtail_weight,
                                float *const *dtail_bias, void *workspace, size_t workspace_bytes, ngpde_stream_t stream);
/* a = act.(z) (re-materialises an activation from a saved pre-activation in the pullback of the fused path) */
int32_t ngpde_activation_forward(int64_t count, int32_t act, const float *z, float *a, ngpde_stream_t stream);

/* SpectralConv message weights (src/layers.jl:654): w_e = cos(e n / 2) cot(e / 2) / 2; the layer is then
 * propagate(e_mul_xj, g, +) = ngpde_propagate_copy_xj with these weights. */
int32_t ngpde_spectral_weights(int64_t n_edges, int32_t n, const float *e, float *w, ngpde_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Fixed-step neural graph ODE over  Chain(GCNConv(d => d, act), GCNConv(d => d, act))  -- the caller
 * of the hot path in the reference's tutorial (docs/src/tutorials/graph_node.md:44-66, :78): the
 * right-hand side dudt(u, p, t) is evaluated once per Runge-Kutta stage.  BASELINE configs fix the
 * step count (Euler x 10, Tsit5 x 50), so the integrator is fixed-step and the backward pass is the
 * discrete adjoint (backprop through the steps), with the whole solve replayed from one HIP graph.
 * d in {16, 32, 64, 128}.  The plan owns its tape (saved activations) and scratch buffers.
 * ---------------------------------------------------------------------------------------------- */
int32_t ngpde_node_gcn2_create(const ngpde_graph_t *g, int32_t d, int32_t act, int32_t tableau,
                               int32_t n_steps, float dt, int32_t with_backward, ngpde_node_t **out);
/* The same plan for a block-diagonal batch of `members` graphs that all have the structure of `member` ("all graphs need to
 * have the same structure", src/layers.jl:359-361; MLUtils.batch, test/runtests.jl:89-102): u0 / uT / duT / du0 are
 * [members * N][d], member after member; the parameter gradients are the sums over the members.  The trajectories are solved
 * one after the other inside the persistent launches (a tile keeps a trajectory's state in registers, see ngpde_node_flags), so
 * the derived-graph handle, the wait lists and the exchanged arrays are those of ONE member.  NGPDE_ERR_UNSUPPORTED when the
 * persistent plan is not available for this graph / width / activation: batch the graphs into one handle then. */
int32_t ngpde_node_gcn2_create_batch(const ngpde_graph_t *member, int32_t members, int32_t d, int32_t act, int32_t tableau,
                                     int32_t n_steps, float dt, int32_t with_backward, ngpde_node_t **out);
int32_t ngpde_node_destroy(ngpde_node_t *plan);
size_t ngpde_node_tape_bytes(const ngpde_node_t *plan);
/* u0 [N][d]; w1,w2 (d x d) column-major; b1,b2 [d]; uT [N][d].  Enqueues the whole solve. */
int32_t ngpde_node_gcn2_forward(ngpde_node_t *plan, const float *u0, const float *w1, const float *b1,
                                const float *w2, const float *b2, float *uT, ngpde_stream_t stream);
/* duT: adjoint of u(T).  Outputs: du0 [N][d], dw1,dw2 (d x d) column-major, db1,db2 [d]. */
int32_t ngpde_node_gcn2_backward(ngpde_node_t *plan, const float *duT, float *du0, float *dw1,
                                 float *db1, float *dw2, float *db2, ngpde_stream_t stream);
/* ONE solve in flight per plan: the plan owns a single tape, u0 copy and parameter copies, so a second
 * ngpde_node_gcn2_forward overwrites what the first one's backward needs.  Every forward stamps a new generation (1, 2, ...);
 * a caller that may interleave solves (an autograd tape holding two forwards) records the generation after its forward and
 * calls ngpde_node_expect_generation right before its backward: NGPDE_ERR_STATE when another forward has run on the plan
 * since.  *backward_pending = 1 while a forward of a with_backward plan has not been followed by its backward (take another
 * plan for the next solve then).  A plan must be used from one stream at a time: its buffers are shared by whatever streams
 * the calls are given and carry no cross-stream ordering. */
int32_t ngpde_node_generation(const ngpde_node_t *plan, uint64_t *generation, int32_t *backward_pending);
int32_t ngpde_node_expect_generation(const ngpde_node_t *plan, uint64_t generation);
/* Names and average device time of the plan's kernels are visible to rocprofv3 --kernel-trace;
 * this returns the number of kernel launches one forward (+ backward) solve enqueues. */
int32_t ngpde_node_launch_count(const ngpde_node_t *plan, int32_t *forward, int32_t *backward);
/* which internal forms the plan chose: bit 0 = pre-scaled arrays (rows held as c .* x, halo rows staged by LDS-DMA),
 * bit 1 = relu sign-bit masks instead of saved layer outputs, bit 2 = reserved (never set), bits 3 / 4 = the forward solve / the
 * adjoint run as ONE persistent launch each (a plan is persistent in every direction it has or in none: bit 4 is set exactly when
 * bit 3 is and the plan has a backward), tiles synchronised inside the launch by per-tile phase flags:
 * graphs whose tiles fit the LDS halo, d = 64 (d = 16 / 32 zero-padded onto it, bit 7), any activation; up to 2 tiles per
 * co-resident workgroup in registers (bit 5), up to 8 taking turns (bit 6); graphs with edge weights on the turn-taking form with
 * the slot weights in LDS (up to 3 tiles per workgroup); graphs with hubs of at most one tile per CU in the hub geometry (bit 8).  d = 128,
 * larger graphs with hubs keep the replayed plan (edge weights and batches of same-structure graphs with hubs run in the hub geometry).  A persistent launch
 * needs all its workgroups resident at once: run one such solve at a time per device (NGPDE_NO_PERSISTENT=1 selects the
 * replayed plan otherwise).  Its waits are bounded; a launch that gives up writes NaN outputs and raises the plan's fault
 * flag, which ngpde_node_fault reads (synchronises `stream`). */
enum { NGPDE_NODE_PRESCALED = 1, NGPDE_NODE_SIGN_MASKS = 2, /* 4: reserved, never set (was NGPDE_NODE_EAGER) */ NGPDE_NODE_PERSISTENT_FWD = 8,
       NGPDE_NODE_PERSISTENT_BWD = 16, NGPDE_NODE_TILE_PAIRS = 32 /* persistent launches with two tiles per workgroup */,
       NGPDE_NODE_TILE_ROUNDS = 64 /* persistent launches with k tiles per workgroup taking turns (larger graphs) */,
       NGPDE_NODE_WIDENED = 128 /* d = 16 / 32 run zero-padded on the 64-wide persistent kernels (NGPDE_NO_WIDEN=1 turns it off) */,
       NGPDE_NODE_HUB_GEOMETRY = 256 /* persistent launches in the hub geometry: graphs of at most one 32-row tile per CU whose tiles reach
                                        beyond the 96-row halo / 32-entry rows (a Cora-shaped graph, docs/src/tutorials/graph_node.md:14-23):
                                        256-row halos, variable-length rows, hub rows summed by all lane groups of the workgroup */,
       NGPDE_NODE_OWN_FIRST = 512 /* the plan reads its own slot tables (by-target lists): each row's own-tile neighbours first, which the
                                     one-tile forward launch sums while it waits for the neighbouring tiles; every forward kernel of
                                     the plan sums in that order (graphs of at most two tiles per CU; NGPDE_NO_OWN_FIRST=1 at create keeps the handle's order) */ };
int32_t ngpde_node_flags(const ngpde_node_t *plan, int32_t *flags);
/* Host only, no device call: the node numbering of a block-diagonal batch (Flux.batch / MLUtils.batch of single graphs,
 * /root/reference/test/runtests.jl:89-102, docs/src/tutorials/VMH.md:120-134) whose members are padded to whole 32-row tiles, so
 * that a solver plan for `n_members` identical-shape members (ngpde_ode_create, members > 1) or the tile kernels can take it:
 * member k keeps its node order and is followed by isolated nodes up to the next multiple of 32.  sizes[k] = nodes of member k.
 * Out: padded_offsets[k] = first node of member k in the padded batch (n_members + 1 entries, the last = padded node count);
 * index[v] = position of node v of the unpadded batch (sum of sizes entries) -- the gather / scatter index of
 * ngpde_rows_index; if `order` (a locality order of the unpadded batch, each member's nodes contiguous) is given, order_padded
 * (padded node count entries) = the same order with every member's padding nodes behind it.  NGPDE_ERR_INVALID_ARGUMENT for a
 * negative size or an `order` that is no such permutation. */
int32_t ngpde_batch_pad_host(int32_t n_members, const int64_t *sizes, int64_t *padded_offsets, int64_t *index, const int32_t *order,
                             int32_t *order_padded);
/* Host only, no device call: would a graph with hubs run on the persistent solver's hub geometry (NGPDE_NODE_HUB_GEOMETRY)?  The
 * graph is given as its two 0-based CSR lists (by target: the in-neighbours of every node; by source: the out-neighbours).  On
 * NGPDE_OK order[32 t + k] is the node the solver would put in row k of tile t (n_nodes entries) and, if tile_rows is not NULL,
 * tile_rows[2 t + dir] the distinct rows tile t references through list dir (its own rows included; at most 256).
 * NGPDE_ERR_UNSUPPORTED (text in ngpde_last_error) when the graph has more than 256 tiles, a node of more than ~224 distinct in+out
 * neighbours, or a tile of more than 4 096 list entries: the solver then replays its per-stage launches.  [no reference counterpart:
 * the reference evaluates Cora (docs/src/tutorials/graph_node.md:14-23) with the generic gather / scatter] */
int32_t ngpde_hub_partition_host(int64_t n_nodes, const int32_t *rowptr_by_target, const int32_t *col_by_target,
                                 const int32_t *rowptr_by_source, const int32_t *col_by_source, int32_t *order, int32_t *tile_rows);
int32_t ngpde_node_fault(ngpde_node_t *plan, ngpde_stream_t stream, int32_t *fault);
/* Diagnostic of the interleaved batch solve (ngpde_node_gcn2_create_batch, two members per workgroup): of the `slot_phases`
 * (tile, member, phase) units of the last forward / adjoint launch, how many found their halo rows gathered ahead of time, i.e.
 * paid no exposed hand-off.  Zeros for plans without persistent launches.  Synchronises `stream`.  [no reference counterpart:
 * the batch is test/runtests.jl:89-102] */
int32_t ngpde_node_pipeline_stats(ngpde_node_t *plan, ngpde_stream_t stream, int64_t *ahead_forward, int64_t *ahead_backward,
                                  int64_t *slot_phases);
/* The same solve with ONE GAT-style layer (ngpde_gat_layer_*: din = heads * c = 64, heads in {1, 2, 4}, weight (64 x 64), a (2c x
 * heads), bias [64] nullable, activation `act`) as the right-hand side  du/dt = act.(GAT(u) .+ b): one persistent launch for the
 * forward solve, one for the discrete adjoint, per-tile phase flags between neighbouring tiles as in the GCN solver.  Runs the
 * one-launch layer's own per-tile code and combines the stages with the coefficients float(dt * a_ij) in the order of
 * ngpde_rk_stage_combine, so u(T) and du0 are bitwise those of the generic solver over ngpde_gat_layer_forward / _backward;
 * parameter gradients agree to rounding (summed per tile over the whole adjoint).  [BASELINE config 3 "GAT as ODE RHS";
 * /root/reference/docs/src/tutorials/VMH.md:85-89 NeuralODE(layer); softmax_edge_neighbors: src/NeuralGraphPDE.jl:7]
 *   create:   ERR_UNSUPPORTED when ngpde_node_gat_supported is 0 (other widths / head counts, tiles that do not fit the LDS halo,
 *             more tiles than the device keeps resident, NGPDE_NO_PERSISTENT=1): use the generic solver.
 *   forward:  u0, uT [N][64]; with_backward plans keep the tape (stage inputs, y / z, alpha: ngpde_node_gat_tape_bytes).
 *   backward: duT [N][64] -> du0 [N][64], dweight (64 x 64, layout of weight), da (2c x heads), dbias [64] nullable.
 *   fault:    1 when a launch gave up waiting (outputs NaN); the plan then refuses further launches (ERR_STATE).
 *   supported: compares the two directions' tile schedules on the device and SYNCHRONISES: ask once per graph handle, not per solve. */
int32_t ngpde_node_gat_supported(const ngpde_graph_t *g, int32_t din, int32_t heads, int32_t c);
int32_t ngpde_node_gat_create(const ngpde_graph_t *g, int32_t heads, int32_t c, float negative_slope, int32_t act, int32_t tableau,
                              int32_t n_steps, double dt, int32_t with_backward, ngpde_node_gat_t **out);
/* A block-diagonal batch of `members` identical structures (g is ONE member; test/runtests.jl:89-102): u0 / uT / duT / du0 are
 * [members][N][64], the parameter gradients the sum over the members; two members at a time share a workgroup, one computing while
 * the other's rows and flags travel. */
int32_t ngpde_node_gat_create_batch(const ngpde_graph_t *g, int32_t members, int32_t heads, int32_t c, float negative_slope,
                                    int32_t act, int32_t tableau, int32_t n_steps, double dt, int32_t with_backward,
                                    ngpde_node_gat_t **out);
int32_t ngpde_node_gat_destroy(ngpde_node_gat_t *plan);
size_t ngpde_node_gat_tape_bytes(const ngpde_node_gat_t *plan);
int32_t ngpde_node_gat_fault(ngpde_node_gat_t *plan, ngpde_stream_t stream, int32_t *fault);
int32_t ngpde_node_gat_forward(ngpde_node_gat_t *plan, const float *u0, const float *weight, const float *a, const float *bias,
                               float *uT, ngpde_stream_t stream);
int32_t ngpde_node_gat_backward(ngpde_node_gat_t *plan, const float *weight, const float *a, const float *duT, float *du0,
                                float *dweight, float *da, float *dbias, ngpde_stream_t stream);
/* ---- NeuralODE(VMHConv(phi, gamma)) device-resident (node_vmh.hip) -----------------------------------------------------------
 * The reference's second neural-ODE caller: docs/src/tutorials/VMH.md:75-89 -- du/dt = VMHConv(phi, gamma)(u) (src/layers.jl:308-332:
 * m_i = aggr_j phi([h_i; h_j - h_i; x_j - x_i]), h' = gamma([h_i; m_i])) under a fixed-step solver, forward + discrete adjoint as ONE
 * persistent launch each (+ one weight-pullback GEMM per Dense layer).  Shapes taken: a scalar state (hd = 1: u0, uT, duT, du0 are
 * [N]), pd = 1..3 position coordinates (pos: device [N][pd], copied at creation), MLPs of 2..4 Dense layers up to 64 wide --
 * phi: dims[0] = 2 hd + pd, gamma: dims[0] = hd + phi's output width, gamma's output width = hd --, hidden activations identity /
 * relu / tanh / sigmoid, identity output layers, + or mean aggregation, graphs of up to 64 tiles per resident workgroup (more half tiles than resident
 * workgroups: whole 32-row tiles, K per workgroup, walked in turn in every phase -- "tile rounds", NGPDE_NODE_TILE_ROUNDS in ngpde_ode_create's
 * flags) whose tiles neighbour at most 63 other tiles each.  What ngpde_node_vmh_supported accepts, ngpde_node_vmh_create builds (memory permitting).
 * ngpde_node_vmh_supported says so; the host's generic solver takes everything else.  Weights are [in][out] (Julia's (out x in)
 * column-major), passed as HOST arrays of device pointers (bias pointers / the bias arrays may be NULL).  One solve's tape per plan. */
int32_t ngpde_node_vmh_supported(const ngpde_graph_t *g, int32_t hd, int32_t pd, int32_t n_phi, const int32_t *phi_dims, const int32_t *phi_acts,
                                 int32_t n_gamma, const int32_t *gamma_dims, const int32_t *gamma_acts, int32_t aggr);
int32_t ngpde_node_vmh_create(const ngpde_graph_t *g, int32_t hd, int32_t pd, const float *pos, int32_t n_phi, const int32_t *phi_dims,
                              const int32_t *phi_acts, int32_t n_gamma, const int32_t *gamma_dims, const int32_t *gamma_acts, int32_t aggr,
                              int32_t tableau, int32_t n_steps, double dt, int32_t with_backward, ngpde_node_vmh_t **out);
int32_t ngpde_node_vmh_destroy(ngpde_node_vmh_t *plan);
size_t ngpde_node_vmh_tape_bytes(const ngpde_node_vmh_t *plan);
/* The tapes of destroyed VMH plans are parked for the next plan they fit (a training loop that re-batches its point clouds every epoch,
 * VMH.md:120-141, builds a plan per step; blocks of tens of GB cost seconds to allocate and free).  Gives them back to the device;
 * returns the bytes released.  The library does it by itself before it reports that a plan's tapes do not fit.  [no reference
 * counterpart: CUDA.reclaim() is the caller-side analogue] */
size_t ngpde_release_cached_memory(void);
int32_t ngpde_node_vmh_fault(ngpde_node_vmh_t *plan, ngpde_stream_t stream, int32_t *fault);
int32_t ngpde_node_vmh_forward(ngpde_node_vmh_t *plan, const float *u0, const float *const *phi_weight, const float *const *phi_bias,
                               const float *const *gamma_weight, const float *const *gamma_bias, float *uT, ngpde_stream_t stream);
int32_t ngpde_node_vmh_backward(ngpde_node_vmh_t *plan, const float *const *phi_weight, const float *const *gamma_weight, const float *duT,
                                float *du0, float *const *dphi_weight, float *const *dphi_bias, float *const *dgamma_weight,
                                float *const *dgamma_bias, ngpde_stream_t stream);
/* saveat (docs/src/tutorials/VMH.md:85 `NeuralODE(gnn, tspan, Tsit5(); saveat = dt_train)`, the loss of :104-108 reads every saved
 * state): usave / dusave are [T][N], T = n_steps / save_every + (save_start ? 1 : 0), slot 0 = u0 when save_start, the last slot =
 * u(T); save_every must divide the plan's steps.  The adjoint adds dusave[j] to lambda at the time of state j; du0 must not lie
 * inside dusave.  (forward / backward above are the T = 1 case.) */
int32_t ngpde_node_vmh_forward_saveat(ngpde_node_vmh_t *plan, const float *u0, const float *const *phi_weight, const float *const *phi_bias,
                                      const float *const *gamma_weight, const float *const *gamma_bias, int32_t save_every,
                                      int32_t save_start, float *usave, ngpde_stream_t stream);
int32_t ngpde_node_vmh_backward_saveat(ngpde_node_vmh_t *plan, const float *const *phi_weight, const float *const *gamma_weight,
                                       int32_t save_every, int32_t save_start, const float *dusave, float *du0, float *const *dphi_weight,
                                       float *const *dphi_bias, float *const *dgamma_weight, float *const *dgamma_bias,
                                       ngpde_stream_t stream);

/* Measurement aid (not on the product path): re-runs the last solve (forward, and backward of
 * loss = sum(u(T)) when the plan has one) launch by launch with start/stop events attached to every
 * `stride`-th dispatch and returns the mean DEVICE time per launch in microseconds -- the quantity
 * rocprofv3 --kernel-trace reports -- for the four kernel roles:
 *   out_us[0] forward layer 1, out_us[1] forward layer 2 + stage combination,
 *   out_us[2] backward layer 1, out_us[3] backward stage combination + layer 2.
 * A persistent plan has one launch per direction: out_us[0] = the forward solve, out_us[2] = the adjoint, the others 0.
 * out_count[4] (nullable) receives the number of sampled launches per role.  Synchronises `stream`. */
int32_t ngpde_node_profile(ngpde_node_t *plan, int32_t stride, float *out_us, int32_t *out_count,
                           ngpde_stream_t stream);

/* Runge-Kutta combination for right-hand sides evaluated by ARBITRARY layers (a GAT-style layer, NeuralODE(VMHConv) of
 * docs/src/tutorials/VMH.md:85-89, ...):  out = c_self * base + sum_k coefs[k] * terms[k]  over `count` floats, n_terms <= 8
 * (Tsit5 has at most six stage terms).  It is the stage input u + dt sum_j a_ij k_j, the step update u + dt sum_i b_i k_i, and in
 * the discrete adjoint K-bar_i = dt b_i lambda + dt sum_{j>i} a_ji U-bar_j, lambda += sum_j U-bar_j and the accumulation of the
 * parameter gradients over the stages.  terms / coefs are HOST arrays (of device pointers / floats); base may be NULL
 * (c_self ignored); out may alias base or a term.  One launch, no allocation: graph-capture safe. */
int32_t ngpde_rk_stage_combine(int64_t count, float c_self, const float *base, int32_t n_terms, const float *const *terms,
                               const float *coefs, float *out, ngpde_stream_t stream);

/* acc[k][i] += g[k][i], i < counts[k], for n_arrays arrays in one launch (per 24 arrays): the cotangents of ALL parameters of one
 * right-hand-side pullback added to their accumulators over the stages of the discrete adjoint (the same arithmetic as
 * ngpde_rk_stage_combine(count, 1, acc, 1, {g}, {1}, acc) per array: fma(1, g, 1 * acc)).  acc / g / counts are HOST arrays. */
int32_t ngpde_accumulate_many(int32_t n_arrays, float *const *acc, const float *const *g, const int64_t *counts, ngpde_stream_t stream);

/* ---- adaptive Tsit5 for right-hand sides evaluated by arbitrary layers ---------------------------------------------------------
 * The reference's tutorials solve with adaptive Tsit5: docs/src/tutorials/graph_node.md:80-81 `NeuralODE(node_chain; save_everystep =
 * false, reltol = 1e-3, abstol = 1e-3, save_start = false)` and VMH.md:87 `NeuralODE(gnn, tspan, Tsit5(); saveat = dt_train, reltol =
 * 1e-9, abstol = 1e-3)`.  The caller forms the stages as for a fixed step (ngpde_rk_stage_combine), evaluates f(u_new) as the seventh
 * stage (FSAL: the next step's first), gets EEst from ngpde_rk_error_norm, reads it back and asks ngpde_rk_control_step what to do.
 * The pullback is the discrete adjoint of the ACCEPTED steps with their step sizes held fixed (rejected attempts contribute nothing,
 * the step sizes are not differentiated through the controller); the reference's InterpolatingAdjoint is a continuous adjoint, the
 * two gradients differ by O(tol).
 *
 * Scaled RMS norm (OrdinaryDiffEq calculate_residuals + its default internalnorm), written to the DEVICE double *out:
 *   out = sqrt( (1/count) sum_i ( e_i / (abstol + reltol max(|u_prev_i|, |u_new_i|)) )^2 ),  e_i = sum_j coefs[j] terms[j][i]
 * e_i is formed as ngpde_rk_stage_combine forms it (base NULL: the fmaf chain in term order), the rest in double.  With the seven Tsit5
 * stages and coefs = float(dt btilde_j) (formed in double) it is Tsit5's EEst; one term with u_prev = u_new = u0 gives |u0/sk| and
 * |f0/sk| of the starting-step heuristic, two terms with coefficients +1, -1 give |(f1 - f0)/sk|.  count >= 1, 1 <= n_terms <= 8;
 * terms / coefs are HOST arrays as in ngpde_rk_stage_combine.  Two launches (per-block partials, then one block adds them in a fixed
 * order): no atomics, bitwise reproducible, no allocation or synchronisation -- graph-capture safe.  `workspace` holds
 * ngpde_rk_error_norm_workspace_bytes(count) bytes (at most 16 KiB). */
size_t ngpde_rk_error_norm_workspace_bytes(int64_t count);
int32_t ngpde_rk_error_norm(int64_t count, int32_t n_terms, const float *const *terms, const float *coefs, const float *u_prev,
                            const float *u_new, double abstol, double reltol, void *workspace, double *out /* device */,
                            ngpde_stream_t stream);

/* Step-size controller, host only (no device call), caller-owned state.  OrdinaryDiffEq's PI controller with the Tsit5 defaults
 * beta1 = 7/50, beta2 = 2/25, gamma = 9/10, qmin = 1/5, qmax = 10, qsteady = [1, 1], qoldinit = 1e-4:
 *   q11 = EEst^beta1, q = clamp(q11 / qold^beta2 / gamma, 1/qmax, 1/qmin) (q = 1/qmax when EEst == 0);
 *   accept when EEst <= 1: qold = max(EEst, qoldinit), dt_next = dt / q;  reject otherwise: dt_next = dt / min(1/qmin, q11/gamma);
 *   a non-finite EEst is a reject with dt_next = dt qmin.
 * The next attempt takes min(dt_next, dtmax), cut to land exactly on the next stop (t_end and, with saveat > 0, every save point
 * t0 + k saveat, as tstops make DiffEq land): on landing t becomes the stop itself.  A step whose proposal falls below dtmin (or is
 * NaN), and the attempt after `maxiters` attempts (rejected ones included), fail with NGPDE_ERR_STATE naming dtmin / maxiters and t;
 * the state then refuses further steps.
 *   init:        dt > 0 is the first attempt's step (capped by dtmax, cut to the first stop); dt <= 0: chosen by the two calls below.
 *                dtmax <= 0: t_end - t0; maxiters <= 0: 100 000 (DiffEq's default); saveat 0: no save points, otherwise it must
 *                divide tspan (NGPDE_ERR_INVALID_ARGUMENT).  dtmin = 1e-12 (t_end - t0); the caller may change it after init.
 *   trial_dt:    Hairer-Norsett-Wanner's starting step as ode_determine_initdt applies it (order 5), first half: with d0 = |u0/sk|,
 *                d1 = |f0/sk|, sk = abstol + reltol |u0|: dt0 = 1e-6 if d0 < 1e-5 or d1 < 1e-5, else 0.01 d0 / d1; capped by dtmax.
 *                The caller evaluates f1 = f(u0 + dt0 f0).
 *   initial_dt:  second half, with norm_df = |(f1 - f0)/sk|: d2 = norm_df / dt0; dt1 = max(1e-6, 1e-3 dt0) if max(d1, d2) <= 1e-15,
 *                else (0.01 / max(d1, d2))^(1/5); the first step is min(100 dt0, dt1, dtmax), cut to the first stop.  Non-finite
 *                norms: NGPDE_ERR_STATE.
 *   step:        EEst of the attempt just made -> *action: NGPDE_RK_REJECT (retry from t with the new dt), NGPDE_RK_ACCEPT (t
 *                advanced; `saved` says the step ended on a save point), NGPDE_RK_DONE (accepted, t = t_end). */
typedef enum { NGPDE_RK_REJECT = 0, NGPDE_RK_ACCEPT = 1, NGPDE_RK_DONE = 2 } ngpde_rk_action_t;
typedef struct ngpde_rk_control {
  double t0, t, t_end;
  double dt;                   /* step of the next attempt */
  double dtmax, dtmin;
  double saveat;               /* 0: no save points */
  double qold, q11, eest;      /* PI controller memory; eest: the last attempt's EEst */
  int64_t maxiters, naccept, nreject, nattempt;
  int64_t n_save, next_save;   /* save points t0 + k saveat, k = 1 .. n_save (the last is t_end); the next one's k */
  int32_t lands;               /* dt reaches the next stop */
  int32_t saved;               /* the last accepted step ended on a save point */
  int32_t done;                /* 1: t_end reached; -1: failed */
  int32_t reserved;
} ngpde_rk_control_t;
int32_t ngpde_rk_control_init(ngpde_rk_control_t *state, double t0, double t_end, double dt, double dtmax, double saveat, int64_t maxiters);
int32_t ngpde_rk_control_trial_dt(const ngpde_rk_control_t *state, double d0, double d1, double *dt0);
int32_t ngpde_rk_control_initial_dt(ngpde_rk_control_t *state, double d0, double d1, double norm_df);
int32_t ngpde_rk_control_step(ngpde_rk_control_t *state, double eest, int32_t *action);

/* Dense output (DiffEq's `saveat` semantics: the save points do not change the steps taken).  Tsit5's free 4th-order interpolant
 * (Tsitouras 2011, as OrdinaryDiffEq's Tsit5 evaluates it) over an accepted step [t_n, t_n + dt]:
 *   u(t_n + theta dt) = u_n + dt sum_{i=1..7} b_i(theta) k_i,   b_i(theta) = r_i1 theta + r_i2 theta^2 + r_i3 theta^3 + r_i4 theta^4,
 * k_7 = f(u_{n+1}) (the seventh stage of the attempt, FSAL).  b_i(0) = 0 and b_i(1) = Tsit5's b_i (b_7 = 0).
 *   tsit5_interp_coefs:  host only; coefs[i] = dt b_i(theta) in double, i < 7.  0 <= theta <= 1 and a finite dt, else
 *                        NGPDE_ERR_INVALID_ARGUMENT.
 *   dense_output:        out_j = u_prev + sum_i coefs[j n_stages + i] k_i for j < n_out in one pass over u_prev and the stages (one
 *                        launch per 16 outputs).  out_j is BITWISE ngpde_rk_stage_combine(count, 1, u_prev, n_stages, k, coefs + j
 *                        n_stages, out_j): 1 * u_prev, then the fmaf chain in stage order.  1 <= n_stages <= 8; k / coefs / outs are
 *                        HOST arrays (of device pointers / floats [n_out][n_stages] / device pointers); the outputs must not alias the
 *                        inputs.
 *   dense_output_pullback: its adjoint.  kbar_i = sum_j coefs[j n_stages + i] douts[j] (written) and, when ubar is not NULL,
 *                        ubar += sum_j douts[j].  BITWISE the fmaf chain in j order that ngpde_rk_stage_combine forms (kbar_i: base
 *                        NULL, coefficients coefs[.][i]; ubar: c_self = 1, coefficients 1), chained through calls with the previous
 *                        partial as base (c_self 1) beyond 8 terms -- 1 * v is exact, so the split does not change the bits.  Each
 *                        cotangent is read once per launch of up to 16; n_out >= 1.
 * Both: element-wise, float4 when count % 4 == 0 and every pointer is 16-byte aligned; no atomics, no allocation, graph-capture safe. */
int32_t ngpde_rk_tsit5_interp_coefs(double theta, double dt, double *coefs /* [7] */);
int32_t ngpde_rk_dense_output(int64_t count, const float *u_prev, int32_t n_stages, const float *const *k, int32_t n_out,
                              const float *coefs, float *const *outs, ngpde_stream_t stream);
int32_t ngpde_rk_dense_output_pullback(int64_t count, int32_t n_out, const float *const *douts, int32_t n_stages, const float *coefs,
                                       float *ubar, float *const *kbar, ngpde_stream_t stream);

/* Optimiser step on the flat parameter vector, one launch behind the gradient all-reduce on the same stream
 * [UPSTREAM Optimisers.jl Adam / Rprop; reference call sites docs/src/tutorials/graph_node.md:90,122-129, VMH.md:97].
 * grad_scale multiplies the (reduced) gradient first: 1/world_size for a mean over data-parallel ranks.
 * Adam: step counts from 1.  Rprop: grad_prev starts at 0, step_size at eta. */
int32_t ngpde_adam_step(int64_t n, float *x, const float *grad, float *m, float *v, float eta, float beta1, float beta2,
                        float eps, int64_t step, float grad_scale, ngpde_stream_t stream);
int32_t ngpde_rprop_step(int64_t n, float *x, const float *grad, float *grad_prev, float *step_size, float shrink, float grow,
                         float step_min, float step_max, float grad_scale, ngpde_stream_t stream);

/* ---- data-parallel collective (comm.hip) -----------------------------------------------------------------------------------
 * New functionality (the reference has no multi-GPU code): whole trajectories / graphs of a batch shard across one process per
 * GPU (test/runtests.jl:89-102, src/layers.jl:359-361), parameters are replicated, and the flat parameter-gradient vector is
 * summed over the ranks once per backward pass -- ncclAllReduce(sum, fp32) over RCCL / xGMI on the caller's stream, in place --
 * optionally with the fused Adam step (1 / world folded in) as the next launch on that stream (graph_node.md:122-129).
 *   ngpde_comm_unique_id: rank 0 makes the id (NGPDE_COMM_ID_BYTES bytes); the HOST ships it to the other ranks.
 *   ngpde_comm_create:    every rank, on its current device; collective (returns when all ranks have joined).
 * RCCL is looked up at the first call: NGPDE_ERR_UNSUPPORTED when librccl.so is absent.  One rank per device (RCCL refuses two). */
typedef struct ngpde_comm ngpde_comm_t;
#define NGPDE_COMM_ID_BYTES 128
int32_t ngpde_comm_unique_id(void *id_out, size_t id_bytes);
int32_t ngpde_comm_create(const void *unique_id, int32_t rank, int32_t world, ngpde_comm_t **out);
int32_t ngpde_comm_destroy(ngpde_comm_t *comm);
int32_t ngpde_comm_info(const ngpde_comm_t *comm, int32_t *rank, int32_t *world);
/* what RCCL reports about the communicator (ncclCommCount, ncclCommUserRank): evidence in a run's record that `count` ranks met */
int32_t ngpde_comm_rccl_info(const ngpde_comm_t *comm, int32_t *count, int32_t *user_rank);
int32_t ngpde_grad_allreduce(ngpde_comm_t *comm, float *flat, int64_t count, ngpde_stream_t stream);
int32_t ngpde_grad_allreduce_adam(ngpde_comm_t *comm, int64_t n, float *x, float *grad, float *m, float *v, float eta, float beta1,
                                  float beta2, float eps, int64_t step, ngpde_stream_t stream);

/* ---- weight-sized rearrangements around the edge-function layers (row_blocks.hip) ------------------------------------------
 * The first Dense layer of phi is split by ROW BLOCKS of its [in][out] weight and the blocks are recombined with signs
 * (src/layers.jl:106 ExplicitEdgeConv, :316 VMHConv, :409-410 MPPDEConv, :523 GNOConv).  ngpde_row_blocks_gather builds up to
 * four recombined matrices in ONE launch: output o, rows dst_row0[s] .. + n_rows[s], += sign[s] * src rows src_row0[s] .. (rows no
 * segment covers are zero; overlapping segments add, e.g. VMHConv's wa - wb).  ngpde_row_blocks_scatter is its pullback: the
 * gradient of the source from the gradients of the outputs (a NULL entry of `douts` counts as zero), every source row written. */
int32_t ngpde_row_blocks_gather(int32_t width, int32_t src_rows, const float *src, int32_t n_seg, const int32_t *out_index,
                                const int32_t *dst_row0, const int32_t *src_row0, const int32_t *n_rows, const float *sign,
                                int32_t n_out, float *const *outs, const int32_t *out_rows, ngpde_stream_t stream);
int32_t ngpde_row_blocks_scatter(int32_t width, int32_t src_rows, float *dsrc, int32_t n_seg, const int32_t *out_index,
                                 const int32_t *dst_row0, const int32_t *src_row0, const int32_t *n_rows, const float *sign,
                                 int32_t n_out, float *const *douts, const int32_t *out_rows, ngpde_stream_t stream);
/* dst [cols][rows] = transpose of src [rows][cols] (GNOConv's reassociated form reads phi's last weight transposed,
 * src/layers.jl:527-530; its pullback transposes the gradient back) */
int32_t ngpde_transpose(int32_t rows, int32_t cols, const float *src, float *dst, ngpde_stream_t stream);
/* Rows by an index list (int64, device, 0-based; entries distinct and in [0, n_rows) -- an entry outside that range names no row: the
 * gather writes a zero row for it, the scatter skips it): gather  dst[o][i][:] = src[o][index[i]][:]  (src [outer][n_rows][d],
 * dst [outer][n_index][d]) or, scatter != 0, dst[o][index[i]][:] = src[o][i][:] with every other row of dst zero (each is the other's
 * pullback).  The state of a batch of point clouds whose members were padded to whole tiles goes in and out of the device-resident
 * NeuralODE(VMHConv) plan through it (docs/src/tutorials/VMH.md:120-134: the batch is one block-diagonal graph). */
int32_t ngpde_rows_index(int64_t outer, int64_t n_rows, int64_t n_index, int32_t d, const int64_t *index, const float *src, float *dst,
                         int32_t scatter, ngpde_stream_t stream);
/* out[i][:] = x[i][:] * scale[i]  (mean aggregation's 1 / degree applied once per node to a cotangent, :534) */
int32_t ngpde_rows_scale(int64_t n, int32_t d, const float *x, const float *scale, float *out, ngpde_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Layer-level entries: ONE call evaluates an edge-function layer of the reference, one call its pullback.
 *   ExplicitEdgeConv  h'_i = aggr_j phi([h_i; h_j; x_j - x_i])                                    /root/reference/src/layers.jl:94-112
 *   VMHConv           m_i = aggr_j phi([h_i; h_j - h_i; x_j - x_i]),  h'_i = gamma([h_i; m_i])     :308-332
 *   MPPDEConv         m_i = aggr_j phi([h_i; h_j; d_i - d_j; e_ij; theta]),  h'_i = psi([h_i; m_i; theta])   :390-422
 * The caller describes the layer -- the blocks the reference vcats and the Dense stacks phi / update (gamma, psi) -- and the
 * library does what the host side had to orchestrate before: the split of phi's first weight into a target-side and a
 * source-side matrix (the signed row blocks of :106, :316, :409-410), the node-level terms P, Q (one pass over h when the shape
 * allows) and the per-edge term of the edge features, the message path (one fused launch where the message MLP fits the fused
 * kernels, the gather / Dense / segmented-reduce primitives otherwise), the node update as a chained launch, and in the pullback
 * the same steps in reverse with every temporary and saved activation laid out in ONE caller-provided workspace.
 *
 * Blocks are row-major device arrays (= the reference's column-major matrices):
 *   state[k] [N][state_width[k]]   the values of `x` (an array = one block; a NamedTuple = its values in order, :94-96, :308-310);
 *                                  MPPDEConv takes exactly one (h)
 *   node_feat [N][node_feat_width] EdgeConv / VMH: vcat of g.ndata WITHOUT :x (constants, concatenated behind the state on both
 *                                  sides of the message, :104, :315, :324); MPPDE: vcat(values(g.ndata)...) = d (:403-405)
 *   pos [N][pos_width]             EdgeConv / VMH: g.ndata.x (x_j - x_i);  MPPDE: unused
 *   edge_feat [E][edge_feat_width] MPPDE: vcat(values(g.edata)...) in p order (ngpde_edge_permute), nullable (:407)
 *   theta [G][theta_width]         MPPDE: vcat(values(g.gdata)...) per graph of the batch, repeated over each graph's nodes / edges
 *                                  (:397, :410, :418); the batch's graphs share one structure (:359-361)
 * Only `state` carries a gradient (graph features are closed-over constants, theta is @ignore_derivatives).
 * A Dense stack: n_layers in 1..NGPDE_MLP_MAX_LAYERS, layer l maps dims[l] => dims[l + 1] with activation act[l], weight[l]
 * (dims[l + 1] x dims[l]) column-major, bias[l] nullable.  update.n_layers = 0 for ExplicitEdgeConv.
 *
 * forward:  y [N][out]; `training` != 0 keeps what the pullback needs in the workspace (ngpde_edge_layer_workspace_bytes with the
 *           same flag); the workspace must be left untouched until ngpde_edge_layer_backward has run with the SAME descriptor.
 * backward: dy [N][out]; d_state[k] nullable (NULL array: no state gradient); gradients of every weight and bias of phi / update
 *           are written (dbias[l] may be NULL where bias[l] is).
 * Errors: NGPDE_ERR_DIMENSION_MISMATCH when the stacks do not chain or phi's / update's input width is not the message's / the
 * node update's vcat (the reference fails in its matrix product), NGPDE_ERR_WORKSPACE, NGPDE_ERR_UNSUPPORTED for more than four
 * blocks on one side of the message. */
#define NGPDE_MLP_MAX_LAYERS 8
typedef struct ngpde_mlp {
  int32_t n_layers;
  int32_t dims[NGPDE_MLP_MAX_LAYERS + 1];
  int32_t act[NGPDE_MLP_MAX_LAYERS];
  const float *weight[NGPDE_MLP_MAX_LAYERS];
  const float *bias[NGPDE_MLP_MAX_LAYERS];
} ngpde_mlp_t;
typedef struct ngpde_mlp_grad {
  float *dweight[NGPDE_MLP_MAX_LAYERS];
  float *dbias[NGPDE_MLP_MAX_LAYERS];
} ngpde_mlp_grad_t;
typedef enum { NGPDE_LAYER_EDGECONV = 0, NGPDE_LAYER_VMH = 1, NGPDE_LAYER_MPPDE = 2 } ngpde_edge_layer_kind_t;
typedef struct ngpde_edge_layer {
  int32_t kind;                 /* ngpde_edge_layer_kind_t */
  int32_t aggr;                 /* ngpde_aggr_t */
  int32_t n_state;
  const float *state[4];
  int32_t state_width[4];
  const float *node_feat;
  int32_t node_feat_width;
  const float *pos;
  int32_t pos_width;
  const float *edge_feat;
  int32_t edge_feat_width;
  const float *theta;
  int32_t theta_width;
  ngpde_mlp_t phi, update;
} ngpde_edge_layer_t;
size_t ngpde_edge_layer_workspace_bytes(const ngpde_graph_t *g, const ngpde_edge_layer_t *layer, int32_t training);
int32_t ngpde_edge_layer_forward(const ngpde_graph_t *g, const ngpde_edge_layer_t *layer, int32_t training, float *y, void *workspace,
                                 size_t workspace_bytes, ngpde_stream_t stream);
int32_t ngpde_edge_layer_backward(const ngpde_graph_t *g, const ngpde_edge_layer_t *layer, const float *dy, float *const *d_state,
                                  const ngpde_mlp_grad_t *dphi, const ngpde_mlp_grad_t *dupdate, void *workspace,
                                  size_t workspace_bytes, ngpde_stream_t stream);

/* GNOConv (/root/reference/src/layers.jl:509-547) in one call, its pullback in one:
 *   K_e = reshape(phi([s_i; s_j; e_ij]), out, in),  m_i = aggr_j K_e h_j,  y = act.(W h + m + b)
 * h [N][in]; node_feat = vcat(values(g.ndata)...) [N][ds] (:517-519); edge_feat = vcat(values(g.edata)...) [E][de] in p order (:521);
 * phi: dims[0] = 2 ds + de, dims[n_layers] = in * out (column-major reshape: element o + out * i, :527); weight (out x in), bias [out]
 * nullable.  The library picks the form: reassociated (the last Dense of phi without activation: T_j = W2 (x) h_j at node level, the
 * in*out x E tensor is never formed), with the per-edge input formed inside the message launch for a two-layer phi, or the literal
 * batched_mul (NGPDE_GNO_MATERIALIZE=1 forces it).  Workspace / training / pullback conventions as ngpde_edge_layer_*; dh nullable. */
typedef struct ngpde_gno_layer {
  int32_t in_chs, out_chs;
  int32_t aggr;                 /* ngpde_aggr_t */
  int32_t act;                  /* ngpde_act_t of the layer's tail */
  const float *h;
  const float *node_feat;
  int32_t node_feat_width;
  const float *edge_feat;
  int32_t edge_feat_width;
  ngpde_mlp_t phi;
  const float *weight, *bias;
} ngpde_gno_layer_t;
size_t ngpde_gno_layer_workspace_bytes(const ngpde_graph_t *g, const ngpde_gno_layer_t *layer, int32_t training);
int32_t ngpde_gno_layer_forward(const ngpde_graph_t *g, const ngpde_gno_layer_t *layer, int32_t training, float *y, void *workspace,
                                size_t workspace_bytes, ngpde_stream_t stream);
int32_t ngpde_gno_layer_backward(const ngpde_graph_t *g, const ngpde_gno_layer_t *layer, const float *dy, float *dh,
                                 const ngpde_mlp_grad_t *dphi, float *dweight, float *dbias, void *workspace, size_t workspace_bytes,
                                 ngpde_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------------------------
 * Solver level, ONE create call: the device-resident fixed-step neural-ODE plan for a right-hand side, chosen and checked by the library.
 * What a Lux / DiffEqFlux host binds where the tutorials write  NeuralODE(model, tspan, Tsit5(); saveat = ...)  and differentiate through
 * the solve (/root/reference/docs/src/tutorials/graph_node.md:44-66, :78; docs/src/tutorials/VMH.md:85-89, :104-108, :132-141):
 *   rhs = NGPDE_RHS_GCN2: Chain(GCNConv(d => d, act), GCNConv(d => d, act)), width = d in {16, 32, 64, 128}; `members` > 1: a block-diagonal
 *         batch of identical structures on the MEMBER's handle (test/runtests.jl:89-102; ERR_UNSUPPORTED when the persistent plan does not
 *         take it: create again on the batch's own handle with members = 1)            -> ngpde_node_gcn2_create[_batch]
 *   rhs = NGPDE_RHS_GAT:  one GAT-style layer, width = 64 = heads * head_width          -> ngpde_node_gat_create[_batch]
 *   rhs = NGPDE_RHS_VMH:  VMHConv(phi, gamma) on a state of `width` rows per node (1), pos [N][pos_width] (copied), phi / gamma given by
 *         their layer widths and activations; the entry checks that the stacks chain as src/layers.jl:316, :328 feed them
 *         (phi_dims[0] = 2 width + pos_width, gamma_dims[0] = width + phi's output, gamma's output = width: DimensionMismatch otherwise)
 *                                                                                       -> ngpde_node_vmh_create
 * NGPDE_ERR_UNSUPPORTED (text in ngpde_last_error) = no device-resident plan takes this right-hand side on this graph: the host steps the
 * layer itself, every Runge-Kutta combination one ngpde_rk_stage_combine launch (any other right-hand side does that too).
 * *flags (nullable): the NGPDE_NODE_* bits of the plan chosen.  Parameters travel per call (no hidden parameter state):
 *   GCN2: first.weight[0..1], first.bias[0..1] (nullable);  GAT: first.weight[0], attention (2c x heads), first.bias[0] (nullable);
 *   VMH: first = phi's layers, second = gamma's.  Gradients come back in the same places of ngpde_ode_grads_t.
 * forward: out = u(T) [N * members][width], or with save_every > 0 (VMH only) the saved states [T][N] of ngpde_node_vmh_forward_saveat;
 * backward: dout in the same shape, du0 [N * members][width].  One solve in flight per plan (ngpde_node_generation's rule). */
typedef struct ngpde_ode ngpde_ode_t;
typedef enum { NGPDE_RHS_GCN2 = 1, NGPDE_RHS_GAT = 2, NGPDE_RHS_VMH = 3 } ngpde_rhs_t;
typedef struct ngpde_ode_desc {
  int32_t rhs;                 /* ngpde_rhs_t */
  int32_t tableau;             /* ngpde_tableau_t */
  int32_t n_steps, with_backward, members;
  double dt;
  int32_t width;               /* GCN2: d; GAT: 64; VMH: rows of the state per node */
  int32_t act;                 /* GCN2 / GAT: the layers' activation */
  int32_t heads, head_width;   /* GAT */
  float negative_slope;        /* GAT */
  int32_t pos_width, aggr;     /* VMH */
  const float *pos;            /* VMH: device [N][pos_width] */
  int32_t n_phi, phi_dims[NGPDE_MLP_MAX_LAYERS + 1], phi_acts[NGPDE_MLP_MAX_LAYERS];
  int32_t n_gamma, gamma_dims[NGPDE_MLP_MAX_LAYERS + 1], gamma_acts[NGPDE_MLP_MAX_LAYERS];
} ngpde_ode_desc_t;
typedef struct ngpde_ode_wb {
  const float *weight[NGPDE_MLP_MAX_LAYERS];
  const float *bias[NGPDE_MLP_MAX_LAYERS];
} ngpde_ode_wb_t;
typedef struct ngpde_ode_params {
  ngpde_ode_wb_t first, second;
  const float *attention;
} ngpde_ode_params_t;
typedef struct ngpde_ode_grads {
  ngpde_mlp_grad_t first, second;
  float *dattention;
} ngpde_ode_grads_t;
int32_t ngpde_ode_create(const ngpde_graph_t *g, const ngpde_ode_desc_t *desc, ngpde_ode_t **out, int32_t *flags);
int32_t ngpde_ode_destroy(ngpde_ode_t *plan);
size_t ngpde_ode_tape_bytes(const ngpde_ode_t *plan);
int32_t ngpde_ode_fault(ngpde_ode_t *plan, ngpde_stream_t stream, int32_t *fault);
int32_t ngpde_ode_forward(ngpde_ode_t *plan, const float *u0, const ngpde_ode_params_t *params, int32_t save_every, int32_t save_start,
                          float *out, ngpde_stream_t stream);
int32_t ngpde_ode_backward(ngpde_ode_t *plan, const ngpde_ode_params_t *params, int32_t save_every, int32_t save_start, const float *dout,
                           float *du0, const ngpde_ode_grads_t *grads, ngpde_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* NGPDE_H */
