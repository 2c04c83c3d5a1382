"""Which kernels a GCNConv or GATConv call runs, restated in Python line for line from csrc/gcn_forms.h and csrc/gat_forms.h:
tests/test_gcn_gat_forms_host.py compares this with the headers' own functions, and the float64 tests (tests/test_gcn_forms_gpu.py,
tests/test_gat_forms_gpu.py) take their thresholds and the form a case must show from here.  A graph enters as `geom`, a dict with the
fields of csrc/tile_geom.h (TileGeom): graph, has_norm, halo_ok (by target), halo_ok_s (by source), self_loops, n_nodes, n_edges.
NGPDE_NO_HALO is latched by the library at its first use in a process; here, as every other switch, it is read at every call."""
import os

from dense_forms_spec import align256, cdiv, weight_chunks

# ---- the families' constants --------------------------------------------------------------------------------------------------------
TILE_ROWS, HALO_CAP, SLOT_WIDTH, ELL_WIDTH = 32, 96, 32, 16                    # csrc/tile_geom.h
FUSED = (16, 32, 64, 128)                                                      # GCNConv: the fused layer's widths (din == dout)
THREADS = 512                                                                  # threads of a tile's workgroup
PAIR_MAX_D = 64                                                                # the pullback runs two tiles per workgroup up to here
ROW_BYTES_LIMIT = 1 << 32                                                      # feature rows are fetched with 32-bit byte offsets
COLSUM_CHUNKS = 128
COLSUM_TWO_STAGE = 4 * COLSUM_CHUNKS                                           # the bias column sum takes two stages above this many rows
GCN_SLACK = 256
GAT_WIDTH, GAT_HEADS, GAT_SRC_TILES = 64, (1, 2, 4), 2                         # the tiled forward and the one-launch layer
GAT_BLOCKED_HEADS, GAT_BLOCKED_MAX = (1, 2, 4, 8, 16), 256                     # blocked<H>

ACT = {"identity": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "swish": 4, "gelu": 5, "leakyrelu": 6, "elu": 7, "softplus": 8}

NO_HALO, NO_FUSED_GAT, NO_FUSED_GAT_LAYER, NO_PERSISTENT = "NGPDE_NO_HALO", "NGPDE_NO_FUSED_GAT", "NGPDE_NO_FUSED_GAT_LAYER", "NGPDE_NO_PERSISTENT"
SWITCHES = (NO_HALO, NO_FUSED_GAT, NO_FUSED_GAT_LAYER, NO_PERSISTENT)
LATCHED = (NO_HALO,)                                                           # read once per process by the library

# ---- the boundary values of every condition (the host test's and the golden's grids) ------------------------------------------------
WIDTHS = (0, 1, 8, 9, 15, 16, 17, 32, 33, 63, 64, 65, 128, 129, 256)
HEADS = (0, 1, 2, 3, 4, 8, 16, 32)
PRODUCTS = (63, 64, 65, 256, 260)                                              # heads * c


def head_widths(heads):
    """the c of the grid at a head count: heads * c on the PRODUCTS it can hit and one step to either side, c % 4 == 0 and not"""
    if heads <= 0:
        return (0, 3, 4, 64)
    cs = {3, 4}
    for p in PRODUCTS:
        cs |= {p // heads, cdiv(p, heads)}
    return tuple(sorted(c for c in cs if c > 0))


def on(name):
    """a switch of the `One` kind: on when the value starts with 1"""
    return os.environ.get(name, "")[:1] == "1"


def is_set(name):
    """a switch of the `Any` kind: on when set at all"""
    return os.environ.get(name) is not None


def geom(n_nodes, n_edges=1, halo_ok=True, halo_ok_s=True, has_norm=True, self_loops=True, graph=True):
    return dict(graph=graph, has_norm=has_norm, halo_ok=halo_ok, halo_ok_s=halo_ok_s, self_loops=self_loops, n_nodes=n_nodes, n_edges=n_edges)


def rows_ok(n_nodes, d):
    return n_nodes * d * 4 < ROW_BYTES_LIMIT


def act_class(act):
    return {ACT["relu"]: "relu", ACT["identity"]: "identity"}.get(act, "runtime")


def tf(b):
    return "true" if b else "false"


# ---- GCNConv: the fused launches ----------------------------------------------------------------------------------------------------
def fused_supported(din, dout):
    return din == dout and din in FUSED


def fused_num_blocks(n_nodes):
    return cdiv(n_nodes, TILE_ROWS)


def fused_bwd_pairs(d):
    return d <= PAIR_MAX_D


def n_slabs(n_nodes, d):
    nb = fused_num_blocks(n_nodes)
    return (nb + 1) // 2 if fused_bwd_pairs(d) else nb


def fused_mask_bytes(n_nodes, d):
    groups = THREADS // (d // 4)
    return fused_num_blocks(n_nodes) * cdiv(TILE_ROWS, groups) * THREADS


def fused_prescaled_supported(g, d):
    return (g["graph"] and g["has_norm"] and g["self_loops"] and d <= 128 and fused_supported(d, d) and g["halo_ok"] and g["halo_ok_s"]
            and not on(NO_HALO))


def fused_fwd_form(g, d, act, pre, own_first):
    f = dict(supported=fused_supported(d, d), rows_ok=rows_ok(g["n_nodes"], d),
             pre_ok=not pre or fused_prescaled_supported(g, d), d=d, act=act_class(act), pre=bool(pre))
    staged = g["halo_ok"] and not on(NO_HALO)
    f["halo"] = bool(pre or staged)
    f["own_first"] = bool(own_first and staged)
    f["launch"] = g["graph"] and g["has_norm"] and f["supported"] and g["n_nodes"] > 0 and f["rows_ok"] and f["pre_ok"]
    f["grid"], f["block"] = fused_num_blocks(g["n_nodes"]), THREADS
    return f


def fused_fwd_names(f):
    return [f"gcn_fused_fwd_kernel<{f['d']},{f['act']},{tf(f['halo'])},{tf(f['pre'])}>"] if f["launch"] else []


def fused_bwd_form(g, d, act, aggregate, pre):
    f = dict(supported=fused_supported(d, d), rows_ok=rows_ok(g["n_nodes"], d),
             pre_ok=not pre or fused_prescaled_supported(g, d), d=d, act=act_class(act), aggregate=bool(aggregate), pre=bool(pre))
    staged = g["halo_ok_s"] and not on(NO_HALO)
    f["halo"] = bool(aggregate and (pre or staged))                            # the dense launch never gathers
    f["pair"] = fused_bwd_pairs(d)
    f["launch"] = g["graph"] and g["has_norm"] and f["supported"] and g["n_nodes"] > 0 and f["rows_ok"] and f["pre_ok"]
    nb = fused_num_blocks(g["n_nodes"])
    f["grid"], f["block"] = ((nb + 1) // 2, 2 * THREADS) if f["pair"] else (nb, THREADS)
    f["slabs"] = n_slabs(g["n_nodes"], d)
    return f


def fused_bwd_names(f):
    if not f["launch"]:
        return []
    return [f"gcn_fused_bwd_kernel<{f['d']},{tf(f['aggregate'])},{f['act']},{tf(f['halo'])},{tf(f['pair'])},{tf(f['pre'])}>"]


# ---- GCNConv: the layer ---------------------------------------------------------------------------------------------------------------
def spmm_dp(d):
    return 8 if d <= 8 else 16 if d <= 16 else 32 if d <= 32 else 64


def fwd_splits(n, din, dout):
    """dense_forms.h: dense_fwd_splits"""
    tiles = cdiv(n, 64) * cdiv(dout, 64)
    if tiles == 0 or tiles >= 256 or din < 256:
        return 1
    return max(1, min(cdiv(512, tiles), din // 64))


def fwd_split_count(din, nsplit):
    """dense_forms.h: dense_fwd_split_count"""
    kper = cdiv(cdiv(din, nsplit), 16) * 16
    return cdiv(din, kper)


def layer_form(g, din, dout, act=1):
    """ngpde_gcn_forward / _backward / _backward_ew and their size queries"""
    n = g["n_nodes"]
    f = dict(kind="fused" if fused_supported(din, dout) else "aggregate_first" if dout >= din else "multiply_first", din=din, dout=dout, n=n)
    f["dp"] = 0 if f["kind"] == "fused" else spmm_dp(min(din, dout))
    f["nsplit"] = fwd_splits(n, din, dout) if f["kind"] == "multiply_first" else 1
    f["parts"] = fwd_split_count(din, f["nsplit"]) if f["kind"] == "multiply_first" else 1
    f["colsum_two_stage"] = f["kind"] == "multiply_first" and n > COLSUM_TWO_STAGE
    f["needs_saved_agg"], f["needs_x"] = dout >= din, dout < din
    f["fwd"] = fused_fwd_form(g, din, act, False, False) if f["kind"] == "fused" else None
    f["bwd"] = [fused_bwd_form(g, din, act, ag, False) for ag in (False, True)] if f["kind"] == "fused" else None
    return f


def layer_fwd_names(f):
    if f["kind"] == "fused":
        return fused_fwd_names(f["fwd"])
    if f["n"] == 0:
        return []
    if f["kind"] == "aggregate_first":
        return [f"spmm_generic_kernel<{f['dp']}>", "ngpde_dense_forward"]
    return ["dense_forward_split"] + (["sum_partials_kernel"] if f["parts"] > 1 else []) + [f"spmm_generic_kernel<{f['dp']}>"]


def layer_bwd_names(f, dx=True, dbias=True):
    """the pullback with dx and dbias asked for or not (the edge-weight gradient's two kernels follow either)"""
    if f["kind"] == "fused":
        k = ["zero_bytes_kernel"] + fused_bwd_names(f["bwd"][0]) + (fused_bwd_names(f["bwd"][1]) if dx else [])
        return k + ["reduce_slabs_kernel"] * (2 if dbias else 1) if f["n"] > 0 else []
    if f["n"] == 0:
        return []
    spmm = f"spmm_generic_kernel<{f['dp']}>"
    if f["kind"] == "aggregate_first":
        return ["act_bwd_kernel", "dense_backward_weight"] + (["dense_backward_input", spmm] if dx else [])
    colsum = (["colsum_partial_kernel", "colsum_kernel"] if f["colsum_two_stage"] else ["colsum_kernel"]) if dbias else []
    return ["act_bwd_kernel"] + colsum + [spmm, "dense_backward_weight"] + (["dense_backward_input"] if dx else [])


def layer_workspace_bytes(g, din, dout, backward, ew=False):
    """ngpde_gcn_workspace_bytes (both directions) and ngpde_gcn_backward_ew_workspace_bytes"""
    f, n = layer_form(g, din, dout), g["n_nodes"]
    take = lambda count: align256(count * 4)
    if not backward:
        if f["kind"] == "fused":
            return GCN_SLACK
        return take(n * (dout * f["parts"] if f["kind"] == "multiply_first" else max(din, dout))) + GCN_SLACK
    if f["kind"] == "fused":
        nb = fused_num_blocks(n)
        b = take(nb * din * dout) + take(nb * dout) + take(n * din)
    else:
        b = 2 * take(n * max(din, dout)) + take(max(weight_chunks(n, din, dout) * (din + 1) * dout, COLSUM_CHUNKS * dout))
    b += GCN_SLACK
    return b + take(n * din) + take(n * min(din, dout)) + take(n) if ew else b


# ---- GATConv: the aggregation primitives ------------------------------------------------------------------------------------------
def gat_tiled_supported(g, heads, c):
    """gat_fused_fwd_kernel: the normalisation set (the handle has its tile schedule) -- but no edge is needed, and only
    NGPDE_NO_FUSED_GAT is read, not the layer's switch"""
    return (g["graph"] and g["has_norm"] and g["halo_ok"] and heads * c == GAT_WIDTH and heads in GAT_HEADS and rows_ok(g["n_nodes"], GAT_WIDTH))


def gat_blocked_shape(heads, c):
    return heads * c <= GAT_BLOCKED_MAX and heads in GAT_BLOCKED_HEADS


def fwd_form(g, heads, c):
    """launch_gat_fwd's choice: "tiled", "blocked" or "row" """
    if not is_set(NO_FUSED_GAT) and gat_tiled_supported(g, heads, c):
        return "tiled"
    return "blocked" if gat_blocked_shape(heads, c) else "row"


def fwd_names(g, heads, c):
    if g["n_nodes"] == 0:
        return []
    form = fwd_form(g, heads, c)
    return ["gat_fused_fwd_kernel"] if form == "tiled" else [f"gat_fwd_blocked_kernel<{heads}>"] if form == "blocked" else ["gat_fwd_kernel"]


def bwd_form(heads, c, aligned):
    """launch_gat_bwd's choice: "blocked" or "row"; aligned: wx and dout both on 16-byte boundaries"""
    return "blocked" if gat_blocked_shape(heads, c) and c % 4 == 0 and aligned else "row"


def bwd_names(g, heads, c, aligned):
    if g["n_nodes"] == 0:
        return []
    first = ([f"gat_bwd_target_blocked_kernel<{heads}>", f"gat_bwd_source_blocked_kernel<{heads}>"] if bwd_form(heads, c, aligned) == "blocked"
             else ["gat_bwd_target_kernel", "gat_bwd_source_kernel"])
    return first + ["gat_scores_bwd_dwx_kernel", "gat_scores_bwd_da_kernel"]


def gat_workspace_bytes(g, heads):
    """ngpde_gat_workspace_bytes"""
    take = lambda count: align256(count * 4)
    return take(max(g["n_edges"], 1) * heads) + 2 * take(max(g["n_nodes"], 1) * heads) + 256


# ---- GATConv: the one-launch layer and the host half of the resident solver's support -------------------------------------------------
def layer_supported(g, din, heads, c):
    """ngpde_gat_layer_supported: both directions' tiles, at least one edge, and its own switch"""
    return (g["graph"] and g["has_norm"] and g["n_edges"] > 0 and g["halo_ok"] and g["halo_ok_s"] and din == GAT_WIDTH and heads * c == GAT_WIDTH
            and heads in GAT_HEADS and rows_ok(g["n_nodes"], GAT_WIDTH) and not on(NO_FUSED_GAT_LAYER))


def gat_layer_form(g, din, heads, c):
    nt = fused_num_blocks(g["n_nodes"])
    return dict(supported=layer_supported(g, din, heads, c), h=heads if heads in (1, 2) else 4, n_tiles=nt, src_wgs=cdiv(nt, GAT_SRC_TILES),
                n=g["n_nodes"])


def gat_layer_names(f):
    if not f["supported"]:
        return [], []
    h = f["h"]
    bwd = [f"gat_layer_bwd_target_kernel<{h}>", f"gat_layer_bwd_source_kernel<{h}>"] if f["n"] > 0 else []
    return ([f"gat_layer_fwd_kernel<{h}>"] if f["n"] > 0 else []), bwd + ["gat_layer_reduce_kernel"]


def gat_layer_workspace_bytes(g, heads):
    """ngpde_gat_layer_workspace_bytes (whatever the support query says)"""
    take = lambda count: align256(count * 4)
    nt = fused_num_blocks(g["n_nodes"])
    wgs = cdiv(nt, GAT_SRC_TILES)
    return (take(g["n_nodes"] * GAT_WIDTH) + take(max(g["n_edges"], 1) * heads) + take(g["n_nodes"] * heads) + take(nt * GAT_WIDTH)
            + take(wgs * GAT_WIDTH * GAT_WIDTH) + take(wgs * 2 * GAT_WIDTH))


def node_host_supported(g, heads, c):
    """what gat_node_persistent_supported decides before it asks the device (residency, wait lists, equal schedules)"""
    return not on(NO_PERSISTENT) and layer_supported(g, GAT_WIDTH, heads, c)


def layer_fits(g):
    """a graph's side of layer_supported"""
    return g["graph"] and g["has_norm"] and g["n_edges"] > 0 and g["halo_ok"] and g["halo_ok_s"]
