"""Which kernels a one-launch message-MLP call runs, restated in Python from the forms' descriptions (csrc/edge_mlp_forms.h's header
comment, the kernels' LDS maps): tests/test_edge_mlp_forms_host.py compares this with the header's own functions line by line, and
the float64 tests (tests/test_edge_mlp_forms_gpu.py) take their halo thresholds from here.  The thresholds are derived from the LDS
formulas below, not typed.

A geometry is Geom(graph, has_norm, halo_ok, max_halo, n_tiles, n_nodes, n_edges); a call is Desc(h1, act1, tail, aggr, ...) with
tail = [(dout, act), ...] or None for a NULL table (then n_tail says how many layers the caller claims)."""
import os
from collections import namedtuple

ROWS, HALO_CAP, SLOT_WIDTH = 32, 96, 32          # rows of a tile, distinct rows a tile may stage, slot bytes per row
W, TS = 64, 68                                   # widest layer, floats per LDS row
T_GENERAL, CHUNK_GENERAL, GROUPS = 512, 128, 32  # the general kernels: threads, edges per chunk, 16-lane groups
T_NARROW, CHUNK_NARROW = 256, 64                 # the edge64 pair and the deep pullback
DQ_SLOTS = 3                                     # halo slots per 16-lane group whose sums stay in registers
DQ_STRIDE = 16 * DQ_SLOTS
MAX_TAIL = 3
PER_XCD = (32, 64)                               # persistent workgroups per XCD: one / two per CU
LDS_BUDGET = 80 * 1024
FWD_SLACK, E64_SLACK = 2048, 4096
DEEP_BWD_NODES = 32768
WS_SLACK = 256

ACT = {"identity": 0, "relu": 1, "tanh": 2, "sigmoid": 3, "swish": 4, "gelu": 5, "leakyrelu": 6, "elu": 7, "softplus": 8}
ACT_NAME = {v: k for k, v in ACT.items()}
AGGR = {"+": 0, "mean": 1, "max": 2, "min": 3, "*": 4}
E64_FIRST = ("swish", "relu", "tanh")
E64_PAIRS = [(a, b) for a in E64_FIRST for b in (a, "identity")]

NO_EDGE64, EDGE64_NO_DQ = "NGPDE_NO_EDGE64", "NGPDE_EDGE64_NO_DQ"
NO_FUSED_EDGE, NO_FUSED_EDGE_BWD, DEEP_EDGE_BWD = "NGPDE_NO_FUSED_EDGE", "NGPDE_NO_FUSED_EDGE_BWD", "NGPDE_DEEP_EDGE_BWD"
SWITCHES = (NO_EDGE64, EDGE64_NO_DQ, NO_FUSED_EDGE, NO_FUSED_EDGE_BWD, DEEP_EDGE_BWD)

Geom = namedtuple("Geom", "graph has_norm halo_ok max_halo n_tiles n_nodes n_edges")
NO_GRAPH = Geom(False, False, False, 0, 0, 0, 0)


class Desc:
    def __init__(self, h1, act1, tail, aggr, n_tail=None, P=True, Q=True, Eterm=False, save_z=False, dQ=True, dE=True):
        self.h1, self.act1, self.aggr = h1, act1, aggr
        self.tail = tail                                              # None: the tables are NULL
        self.n_tail = len(tail) if n_tail is None else n_tail
        self.P, self.Q, self.Eterm, self.save_z, self.dQ, self.dE = P, Q, Eterm, save_z, dQ, dE

    @property
    def tails(self):
        return self.n_tail <= 0 or self.tail is not None

    def dout(self, l):
        return self.tail[l][0] if self.tail is not None and l < len(self.tail) else 0

    def act(self, l):
        return self.tail[l][1] if self.tail is not None and l < len(self.tail) else "identity"

    def din(self, l):
        return self.h1 if l == 0 else self.dout(l - 1)


def on(name):
    """a yes/no switch: on when the value starts with 1 (read per call)"""
    return os.environ.get(name, "")[:1] == "1"


def halo_rows(halo):
    return max(ROWS, min(HALO_CAP, halo))


def grid(n_tiles, per_xcd):
    return 8 * max(1, min(per_xcd, (n_tiles + 7) // 8))


def lds(halo, other_rows):
    """halo region + its zero row + the form's other rows, TS floats each"""
    return (halo_rows(halo) + 1 + other_rows) * TS * 4


def per_xcd(nbytes, slack):
    return PER_XCD[1] if nbytes + slack <= LDS_BUDGET else PER_XCD[0]


# the LDS maps of the kernels, in rows beside the halo region
def fwd64_rows():
    return ROWS + W + 2 * CHUNK_NARROW                    # P rows, W2^T, two message chunks


def fwd_rows(n_tail):
    return GROUPS + n_tail * W + CHUNK_GENERAL            # P rows, the tail's W^T, one message chunk


def bwd64_rows():
    return ROWS + CHUNK_NARROW + 2 * W                    # P rows, a chunk, W2^T and W2


def bwd_rows(n_tail, aggr):
    return 2 * GROUPS + CHUNK_GENERAL + (2 * W if n_tail else 0) + (GROUPS if AGGR[aggr] >= AGGR["max"] else 0)


def deep_rows(n_tail):
    return ROWS + CHUNK_NARROW + 2 * n_tail * W


def largest_halo(fits):
    """the largest halo in 32 .. 96 with fits(halo), None when none has; 96 when all have"""
    ok = [h for h in range(ROWS, HALO_CAP + 1) if fits(h)]
    return max(ok) if ok else None


def two_per_cu(nbytes, slack):
    return nbytes + slack <= LDS_BUDGET


# ---- the thresholds the float64 tests straddle ----------------------------------------------------------------------------------
DQ_MAX_HALO = DQ_STRIDE
E64_FULL_GRID_MAX_HALO = largest_halo(lambda h: two_per_cu(lds(h, fwd64_rows()), E64_SLACK) and two_per_cu(lds(h, bwd64_rows()), E64_SLACK))
FWD_TWO_PER_CU_MAX_HALO = {nt: largest_halo(lambda h, nt=nt: two_per_cu(lds(h, fwd_rows(nt)), FWD_SLACK)) for nt in range(MAX_TAIL + 1)}
FWD1_TWO_PER_CU_MAX_HALO = FWD_TWO_PER_CU_MAX_HALO[1]
assert fwd64_rows() == bwd64_rows()                                   # one bound for the pair
# every bound strictly inside 32 .. 96, each with its successor: the halos at which some form changes its grid
TWO_PER_CU_BOUNDS = sorted({b for b in [E64_FULL_GRID_MAX_HALO] + list(FWD_TWO_PER_CU_MAX_HALO.values()) if b is not None and b < HALO_CAP})


# ---- the conditions ---------------------------------------------------------------------------------------------------------------
def width_ok(w):
    return 0 < w <= W and w % 4 == 0


def tiles_ok(g):
    return g.graph and g.has_norm and g.halo_ok


def chain_ok(d, lo, hi):
    return width_ok(d.h1) and lo <= d.n_tail <= hi and d.tails and all(width_ok(d.dout(l)) for l in range(d.n_tail))


def edge64_shape(d):
    return (not on(NO_EDGE64) and d.P and d.Q and not d.Eterm and d.h1 == W and d.n_tail == 1 and d.tails and d.dout(0) == W
            and d.aggr in ("+", "mean") and d.act1 in E64_FIRST and d.act(0) in (d.act1, "identity"))


def edge64_dq(g, d):
    return edge64_shape(d) and not on(EDGE64_NO_DQ) and d.dQ and g.halo_ok and g.max_halo <= DQ_STRIDE


def fwd_supported(g, d):
    return tiles_ok(g) and chain_ok(d, 0, MAX_TAIL)


def fwd_plan(g, d):
    """None when unsupported, else dict(names, threads, lds, per_xcd, grid); no nodes: no launch"""
    if not fwd_supported(g, d):
        return None
    if g.n_nodes == 0:
        return dict(names=[])
    if edge64_shape(d) and not d.save_z:
        name, threads, nbytes, slack = f"edge_mlp64_fwd_kernel<{d.act1},{d.act(0)}>", T_NARROW, lds(g.max_halo, fwd64_rows()), E64_SLACK
    else:
        name, threads, nbytes, slack = f"edge_mlp_fused_fwd_kernel<{d.n_tail}>", T_GENERAL, lds(g.max_halo, fwd_rows(d.n_tail)), FWD_SLACK
    cap = per_xcd(nbytes, slack)
    return dict(names=[name], threads=threads, lds=nbytes, per_xcd=cap, grid=grid(g.n_tiles, cap))


def slab(n_wg, din, dw):
    return n_wg * (din + 1) * dw * 4


def up256(b):
    return (b + 255) // 256 * 256


def bwd_workspace(g, d):
    if not g.graph:
        return 0
    one = grid(g.n_tiles, PER_XCD[0])
    if d.n_tail >= 2:
        if d.n_tail > MAX_TAIL or not d.tails:
            return 0
        return sum(up256(slab(one, d.din(l), d.dout(l))) for l in range(d.n_tail)) + WS_SLACK
    dw = d.dout(0) if d.n_tail == 1 and d.tails else 0
    general = slab(one, d.h1, dw)
    edge64 = 0
    if d.h1 == W and dw == W:
        edge64 = up256(slab(grid(g.n_tiles, PER_XCD[1]), W, W))
        if g.halo_ok and g.max_halo <= DQ_STRIDE:
            edge64 += up256(g.n_tiles * DQ_STRIDE * W * 4)
    return max(general, edge64) + WS_SLACK


def bwd_supported(g, d):
    if d.n_tail >= 2:
        return tiles_ok(g) and chain_ok(d, 2, MAX_TAIL) and d.aggr in ("+", "mean")
    return tiles_ok(g) and chain_ok(d, 0, 1) and d.aggr in AGGR


def bwd_plan(g, d):
    """dict(supported, names, threads, lds, grid, edge_buffer, dE_missing, workspace); threads, lds and grid where something is launched"""
    sup = bwd_supported(g, d)
    dq = edge64_dq(g, d)
    out = dict(supported=sup, names=[], edge_buffer=not dq, dE_missing=(not dq) and not d.dE and g.n_edges != 0, workspace=bwd_workspace(g, d))
    if not sup or g.n_nodes == 0:
        return out
    if d.n_tail >= 2:
        kernel, threads, nbytes, cap = f"edge_mlp_deep_bwd_kernel<{d.n_tail}>", T_NARROW, lds(g.max_halo, deep_rows(d.n_tail)), PER_XCD[0]
    elif edge64_shape(d):
        nbytes = lds(g.max_halo, bwd64_rows())
        kernel, threads, cap = f"edge_mlp64_bwd_kernel<{d.act1},{d.act(0)},{'true' if dq else 'false'}>", T_NARROW, per_xcd(nbytes, E64_SLACK)
    else:
        kernel, threads, nbytes, cap = f"edge_mlp_fused_bwd_kernel<{d.n_tail}>", T_GENERAL, lds(g.max_halo, bwd_rows(d.n_tail, d.aggr)), PER_XCD[0]
    names = [kernel] + ["dense_weight_reduce_kernel"] * d.n_tail
    names += ["edge64_dq_combine_kernel"] if dq else ["edge_sum_by_source_kernel"] if d.dQ else []
    out.update(names=names, threads=threads, lds=nbytes, grid=grid(g.n_tiles, cap))
    return out


def msg_path(g, d, training):
    """(fused_msg, fused_bwd, need_dE, the fused pullback's workspace) of a layer whose message call is d"""
    bwd_ok = not on(NO_FUSED_EDGE_BWD) and bwd_supported(g, d)
    fused_msg = (not on(NO_FUSED_EDGE) and g.n_edges > 0 and (d.aggr in ("+", "mean") or not training or bwd_ok) and fwd_supported(g, d))
    if not fused_msg or not training:
        return fused_msg, False, False, 0
    fused_bwd = bwd_ok
    if fused_bwd and d.n_tail >= 2:
        deep = os.environ.get(DEEP_EDGE_BWD)
        d0 = deep[:1] if deep else ""
        fused_bwd = d0 == "1" or (d0 != "0" and g.n_nodes >= DEEP_BWD_NODES)
    if not fused_bwd:
        return fused_msg, False, False, 0
    return fused_msg, True, not edge64_dq(g, d), bwd_workspace(g, d)
