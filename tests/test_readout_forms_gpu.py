"""The per-graph readouts (csrc/readout.hip on the lane layout of csrc/row_lanes.h) against float64 across their forms.

Plans are built with ngpde_readout_create on raw device id / index arrays and ngpde_readout_info is held to a numpy restatement of the
plan (contiguous, n_chunks; chunk_rows is TAKEN from the call and every layout below is sized from it).  Every entry is called through
the C ABI with raw pointers, a workspace of exactly ngpde_readout_workspace_bytes between canary bytes, and outputs that start as NaN
between guard words.

Dispatch, restated below and asserted in every case (note, want_form):
  float4 columns iff d % 4 == 0 and every array the entry takes is NULL or 16-byte aligned -- reduce forward: x, out, workspace; reduce
  pullback: x, out, dout, dx (x and out count for every aggregation, read or not); softmax forward: x, y, workspace; softmax pullback:
  y, dy, dx, workspace; broadcast: u, out; broadcast pullback: dout, du, workspace.  Rows of w columns (w = d / 4 in the float4 form)
  take dpl = lanes(w) lanes per row (the next power of two, at most 64), ceil(w / dpl) column chunks with the last clamped to column
  w - 1, and 64 / dpl row slots per wave, four waves per chunk of chunk_rows rows, four rows in flight per lane.
  A segment that is exactly one chunk is finished by the chunk reduce; when every segment is, there is no finish launch and the
  workspace partials are not written.  Otherwise one wave per (segment, column chunk) folds the partials, four per slot in flight.
      d          4   8  12  16 | 20 | 36 | 68 | 132 | 260 516    1  2  3  5  7 13 21 33  65 130    64 256 with one array 4 bytes in
      dpl        1   2   4   4 |  8 | 16 | 32 |  64 |  64  64    1  2  4  8  8 16 32 64  64  64    64  64
      chunks     1                            |   2   3    1                          2   3     1   4

Segment layouts, each as a contiguous id list (base 0), a shuffled copy (base 1: the permuted plan) and the `index` form (items are the
edges of a graph whose source nodes carry the ids):
  ladder   lengths 0 | 1 2 3 4 5 15 16 17 | 0 | 63 64 65 255 256 257 511 512 513 1025 | 0
  single   every segment exactly one chunk: 1, chunk_rows, 17, chunk_rows - 1, 64, 3 rows
  one      id = NULL, one segment of 2 chunk_rows + 188 rows
  none     no items, three segments: the identities
  long     257 chunk_rows + 1 rows beside a 1-row segment, d = 1 and 4: the finish fold past 4 x 64 partials per slot pass

References are float64 numpy of the operation itself on the float32 inputs, compared element by element:
  exact     broadcast (the same bits), max / min and their pullbacks (ties included), the sum's pullback, every identity of an empty
            segment (0, -inf, +inf); non-finite entries must match exactly.
  integer   inputs from {-2 .. 2}: sums and du must equal the float64 result bit for bit (sum|term| < 2^24 asserted), the mean
            within 2 ulp of that exact sum times the float32 1 / count.  This is what no dropped, doubled or misrouted row passes.
  linear    normal draws: |out - ref| <= (k + 2) 2^-24 sum|term_i| for a segment of k rows; the mean's pullback 3 2^-24 |ref|.
  planted   a unique extremum at the first and last row, rows chunk_rows - 1, chunk_rows, chunk_rows + 1, the last row of the last
            full chunk and the first row of the ragged tail of every multi-chunk segment, one run per position: max / min must return
            it and route the gradient to it alone; the softmax (a logit 30 above the rest) must put y >= 1 - 1e-4 there.
  softmax   |y - ref| <= 1e-4 ref for every entry (logit spread below 60 in a segment: every reference entry above float32's
            smallest normal, asserted); every non-empty segment sums to 1 within (k + 2) 2^-24 + 1e-4.
  softmax pullback   as test_msgpass_forms_gpu.py derives it: on the kernel's own y = ref (1 + delta), |delta| <= 1e-4, with
            A = sum_seg |ref dy| and B_s = (k + 2) 2^-24 A (1 + 1e-4) + 1e-4 A,
            |dx - dx_ref| <= 1e-4 |dx_ref| + ref (1 + 1e-4) (B_s + 2 2^-24 (|dy| + |s_ref| + B_s));  with integer y, dy: the same bits.

Measured on the MI355X, worst err / bound over every case of this file (teardown_module prints the table under `pytest -s`):
  linear    reduce + 0.34   mean 0.51   mean pullback 0.66   broadcast du 0.38
  integer   every sum and du, the 65 793-row segment included: the same bits; the mean 0.25 of its 2 ulp
  softmax   y 0.077   segment sums 0.004   pullback 0.027;   planted: every position found by max, min and the softmax
  The mean's pullback is two roundings (1 / count, the product) under a bound that allows three: two thirds at most, and 0.66 it is.
  chunk_rows came back as 256.  Every entry came up in both column types at dpl 1 2 4 8 16 32 64 and at one, two and three
  (misaligned 256: four) column chunks; segment lengths 0 1 2 3 4 5 15 16 17 63 64 65 255 256 257 511 512 513 700 1025 65793.
"""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from test_mp_primitive_forms_gpu import DEV, EPS, TINY, In, Out, exact, lin, ok, p, rng_for, stream
from test_msgpass_forms_gpu import KINDS, aligned, draw, form_of
from test_msgpass_forms_gpu import check_mean as _check_mean
from test_msgpass_forms_gpu import check_sum as _check_sum
from test_msgpass_forms_gpu import integer_exact
from test_msgpass_forms_gpu import within as _within

gpu = pytest.mark.gpu
AGGRS = ("sum", "mean", "max", "min")
IDENTITY = dict(sum=0.0, mean=0.0, max=-np.inf, min=np.inf)
F4_WIDTHS = (4, 8, 12, 16, 20, 36, 68, 132, 260, 516)
SCALAR_WIDTHS = (1, 2, 3, 5, 7, 13, 21, 33, 65, 130)
WIDTHS = F4_WIDTHS + SCALAR_WIDTHS
MIS_WIDTHS = (64, 256)
LADDER = [0, 1, 2, 3, 4, 5, 15, 16, 17, 0, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025, 0]
FORMS = ("contiguous", "shuffled", "index")
GUARD_BYTES = 256

WORST = {}
CASES = set()
LENGTHS = set()


def within(out, ref, bound, fam, what):
    _within(out, ref, bound, fam, what, WORST)


def check_sum(out, ref, k, ab, kind, fam, what):
    _check_sum(out, ref, k, ab, kind, fam, what, WORST)


def check_mean(out, total, k, ab, kind, fam, what):
    _check_mean(out, total, k, ab, kind, fam, what, WORST)


def want_form(d, misaligned=False):
    return form_of(d, d % 4 == 0 and not misaligned)


def note(entry, d, *ptrs):
    form = form_of(d, d % 4 == 0 and aligned(*ptrs))
    CASES.add((entry,) + form)
    return form


def test_width_tables_cover_every_lane_layout():
    assert {form_of(d, True)[1] for d in F4_WIDTHS} == {form_of(d, False)[1] for d in SCALAR_WIDTHS} == {1, 2, 4, 8, 16, 32, 64}
    assert all(d % 4 == 0 for d in F4_WIDTHS + MIS_WIDTHS) and all(d % 4 for d in SCALAR_WIDTHS)
    assert want_form(260) == ("f4", 64, 2) and want_form(516) == ("f4", 64, 3) and want_form(130) == ("float", 64, 3)
    assert want_form(64, True) == ("float", 64, 1) and want_form(256, True) == ("float", 64, 4) and want_form(12) == ("f4", 4, 1)
    assert LADDER[0] == LADDER[-1] == 0 and 0 in LADDER[1:-1] and sum(LADDER) == 3584


# ---- layouts and plans -----------------------------------------------------------------------------------------------------------------

def layout_lengths(name, cr):
    """segment lengths of a layout for a plan of cr rows per chunk"""
    return dict(ladder=LADDER, single=[1, cr, 17, cr - 1, min(64, cr), 3], one=[2 * cr + 188], none=[0, 0, 0], long=[257 * cr + 1, 1])[name]


class Layout:
    """the item -> segment map of one layout in one form, and what a plan over it must be (numpy only)"""

    def __init__(self, name, form, cr):
        self.name, self.form, self.cr = name, form, cr
        lengths = np.asarray(layout_lengths(name, cr), dtype=np.int64)
        self.S, self.n = len(lengths), int(lengths.sum())
        rng = rng_for("layout", name, form)
        seg = np.repeat(np.arange(self.S), lengths)
        self.id_base, self.index = 0, None
        if form == "shuffled":
            seg, self.id_base = seg[rng.permutation(self.n)], 1
        self.seg = seg
        self.id = seg + self.id_base
        if form == "index":                                              # two nodes per segment, in shuffled node order
            node_seg = np.repeat(np.arange(self.S), 2)[rng.permutation(2 * self.S)]
            nodes_of = np.argsort(node_seg, kind="stable").reshape(self.S, 2)
            self.id, self.index = node_seg, nodes_of[seg, rng.integers(0, 2, self.n)]
            assert np.array_equal(self.id[self.index], seg)
        if name == "one":
            self.id = None
        self.counts = np.bincount(seg, minlength=self.S)
        self.segptr = np.concatenate([[0], np.cumsum(self.counts)])
        self.order = np.argsort(seg, kind="stable")                      # item at each sorted position
        self.contiguous = bool((np.diff(seg) >= 0).all())
        self.n_chunks = int((-(-self.counts // cr)).sum())
        self.single = bool((self.counts > 0).all() and (self.counts <= cr).all())
        assert list(self.counts) == list(lengths) and (form != "shuffled" or self.n < 2 or not self.contiguous or self.S == 1)

    def reduce(self, ufunc, ident, x):
        out = np.full((self.S,) + x.shape[1:], ident, dtype=np.float64)
        ne = self.counts > 0
        if ne.any():
            out[ne] = ufunc.reduceat(x[self.order], self.segptr[:-1][ne], axis=0)
        return out

    def sum(self, x):
        return self.reduce(np.add, 0.0, x)


class Plan(Layout):
    """the library's plan over a layout; ngpde_readout_info must agree with the restatement"""

    def __init__(self, name, form, cr):
        super().__init__(name, form, cr)
        lib = _lib.load()
        self.id_dev = None if self.id is None else torch.as_tensor(np.append(self.id, 0).astype(np.int32), device=DEV)
        self.index_dev = None if self.index is None else torch.as_tensor(np.append(self.index, 0).astype(np.int32), device=DEV)
        h = C.c_void_p()
        ok(lib.ngpde_readout_create(self.n, None if self.id_dev is None else self.id_dev.data_ptr(),
                                    None if self.index_dev is None else self.index_dev.data_ptr(), self.id_base, self.S, stream(), C.byref(h)))
        self.ptr = h.value
        n, S, contiguous, n_chunks, chunk_rows = C.c_int64(), C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        ok(lib.ngpde_readout_info(self.ptr, C.byref(n), C.byref(S), C.byref(contiguous), C.byref(n_chunks), C.byref(chunk_rows)))
        assert (n.value, S.value, chunk_rows.value) == (self.n, self.S, cr)
        assert bool(contiguous.value) == self.contiguous and n_chunks.value == self.n_chunks, (name, form)
        LENGTHS.update(int(c) for c in self.counts)

    def ws_bytes(self, d):
        need = _lib.load().ngpde_readout_workspace_bytes(self.ptr, d)
        assert need == 2 * (self.S + self.n_chunks) * d * 4
        return need


_PLANS = {}
_CR = []


def chunk_rows():
    """rows per chunk, asked of the library (a one-item plan)"""
    if not _CR:
        lib, h, cr = _lib.load(), C.c_void_p(), C.c_int32()
        ok(lib.ngpde_readout_create(1, None, None, 0, 1, stream(), C.byref(h)))
        ok(lib.ngpde_readout_info(h.value, None, None, None, None, C.byref(cr)))
        ok(lib.ngpde_readout_destroy(h.value))
        assert cr.value >= 64
        _CR.append(cr.value)
    return _CR[0]


def plan(name, form):
    if (name, form) not in _PLANS:
        _PLANS[name, form] = Plan(name, form, chunk_rows())
    return _PLANS[name, form]


def plans(*names):
    return [plan(name, form) for name in names for form in (FORMS if name not in ("one",) else ("contiguous",))]


def teardown_module(module):
    for pl in _PLANS.values():
        _lib.load().ngpde_readout_destroy(pl.ptr)
    _PLANS.clear()
    if WORST:
        print("\nworst err / bound per family:")
        for fam in sorted(WORST):
            print(f"  {fam:40s} {WORST[fam]:.3f}")
        print("launch forms checked (entry: column type dpl x column chunks):")
        for entry in sorted({c[0] for c in CASES}):
            print(f"  {entry:28s}", " ".join(f"{t}{d}x{n}" for _, t, d, n in sorted(c for c in CASES if c[0] == entry)))
        print("segment lengths:", " ".join(str(k) for k in sorted(LENGTHS)))


class Ws:
    """workspace of exactly `nbytes` (all-ones words: NaN) between canary bytes, optionally 4 bytes into its allocation"""

    def __init__(self, nbytes, mis=False):
        self.nbytes, self.lo = int(nbytes), GUARD_BYTES + (4 if mis else 0)
        self.full = torch.full((self.lo + self.nbytes + GUARD_BYTES,), 0xFF, dtype=torch.uint8, device=DEV)
        self.full[:self.lo] = 0xA5
        self.full[self.lo + self.nbytes:] = 0xA5
        self.ptr = self.full.data_ptr() + self.lo
        assert self.ptr % 16 == (4 if mis else 0)

    def get(self):
        torch.cuda.synchronize()
        b = self.full.cpu().numpy()
        assert (b[:self.lo] == 0xA5).all() and (b[self.lo + self.nbytes:] == 0xA5).all(), "wrote outside the workspace"
        return b[self.lo:self.lo + self.nbytes]

    def untouched(self, start=0):
        return bool((self.get()[start:] == 0xFF).all())

    def written(self, nbytes):
        b = self.get()[:nbytes]
        return not (np.frombuffer(b.tobytes(), dtype=np.uint32) == 0xFFFFFFFF).any()


# ---- the entries -------------------------------------------------------------------------------------------------------------------------

def call(fn, expect, *args):
    st = fn(*args)
    torch.cuda.synchronize()
    assert st == expect, (st, expect, _lib.load().ngpde_last_error())


def reduce_fwd(pl, d, aggr, x, mis=(), short=0, expect=_lib.OK):
    out, ws = Out(pl.S, d, mis="out" in mis), Ws(pl.ws_bytes(d) - short, "ws" in mis)
    form = note("reduce_forward", d, p(x), out.ptr, ws.ptr)
    call(_lib.load().ngpde_readout_reduce_forward, expect, pl.ptr, d, _lib.AGGR[aggr], p(x), out.ptr, ws.ptr, ws.nbytes, stream())
    assert ws.untouched() or not (pl.single or expect != _lib.OK), "partials written without a finish launch"
    return out, form


def reduce_bwd(pl, d, aggr, x, out, dout, mis=()):
    dx = Out(pl.n, d, mis="dx" in mis)
    form = note("reduce_backward", d, p(x), p(out), p(dout), dx.ptr)
    call(_lib.load().ngpde_readout_reduce_backward, _lib.OK, pl.ptr, d, _lib.AGGR[aggr], p(x), p(out), p(dout), dx.ptr, stream())
    return dx, form


def check_reduce(pl, d, aggr, kind, key, mis=(), xvals=None):
    """forward and pullback of one aggregation against float64; returns the forms the two launches took"""
    rng = rng_for("reduce", pl.name, pl.form, d, aggr, kind, key)
    xv = draw(kind, rng, pl.n, d) if xvals is None else xvals
    x, dout = In(xv, "x" in mis), In(draw(kind, rng, pl.S, d), "dout" in mis)
    what = f"{pl.name} {pl.form} d={d} {aggr} {kind} mis={mis}"
    out, f1 = reduce_fwd(pl, d, aggr, x, mis)
    k = pl.counts[:, None]
    if aggr in ("max", "min"):
        ref = pl.reduce(np.maximum if aggr == "max" else np.minimum, IDENTITY[aggr], x.r)
        exact(out, ref.astype(np.float32), what)
    elif aggr == "sum":
        ref = pl.sum(x.r)
        check_sum(out, ref, k, pl.sum(np.abs(x.r)), kind, "reduce +", what)
    else:
        ref = pl.sum(x.r) / np.maximum(k, 1)                             # (read by nothing but the misaligned `out` operand below)
        check_mean(out, pl.sum(x.r), k, pl.sum(np.abs(x.r)), kind, "reduce mean", what)
    got = out.get()[pl.counts == 0]
    assert (got == IDENTITY[aggr]).all(), f"empty segments {what}"
    with np.errstate(invalid="ignore"):
        ref_in = In(ref, "out" in mis)                                   # the float64 result rounded: exact for max / min
    ext = aggr in ("max", "min")
    dx, f2 = reduce_bwd(pl, d, aggr, x if ext or mis else None, ref_in if ext or mis else None, dout, mis)
    g = dout.r[pl.seg]
    if aggr == "sum":
        exact(dx, dout.f[pl.seg], "dx " + what, bits=True)
    elif aggr == "mean":
        r = g / pl.counts[pl.seg][:, None]
        within(dx, r, lin(1, np.abs(r)), "reduce mean pullback", "dx " + what)
    else:
        exact(dx, np.where(x.f == ref.astype(np.float32)[pl.seg], dout.f[pl.seg], np.float32(0)), "dx " + what)
    assert x.unchanged() and dout.unchanged()
    return f1, f2, out, dx


def seg_softmax(pl, x):
    z = np.exp(x - pl.reduce(np.maximum, -np.inf, x)[pl.seg])
    return z / pl.sum(z)[pl.seg]


def softmax_fwd(pl, d, x, mis=(), every=True):
    y, ws = Out(pl.n, d, mis="y" in mis), Ws(pl.ws_bytes(d), "ws" in mis)
    form = note("softmax_forward", d, p(x), y.ptr, ws.ptr)
    call(_lib.load().ngpde_readout_softmax_forward, _lib.OK, pl.ptr, d, p(x), y.ptr, ws.ptr, ws.nbytes, stream())
    ws.get()                                                             # this entry fills the workspace to its last byte: the canaries
    if pl.single:                                                        # the [S][d] (max, sum) pairs, and no partial
        assert ws.written(8 * pl.S * d) and ws.untouched(8 * pl.S * d)
    ref = seg_softmax(pl, x.r)
    rep = ref >= TINY
    assert rep.all() or not every, f"{int((~rep).sum())} reference entries below float32's smallest normal"
    got = y.get()
    what = f"{pl.name} {pl.form} d={d} mis={mis}"
    assert np.isfinite(got).all(), what
    within(got[rep], ref[rep], 1e-4 * ref[rep], "softmax y", "softmax " + what)
    ne = pl.counts > 0
    sums = pl.sum(got.astype(np.float64))[ne]
    within(sums, np.ones_like(sums), (pl.counts[ne][:, None] + 2) * EPS + 1e-4, "softmax segment sums", "sums " + what)
    return y, ref, form


def softmax_bwd(pl, d, y, dy, mis=()):
    dx, ws = Out(pl.n, d, mis="dx" in mis), Ws(pl.ws_bytes(d), "ws" in mis)
    form = note("softmax_backward", d, y.ptr, p(dy), dx.ptr, ws.ptr)
    call(_lib.load().ngpde_readout_softmax_backward, _lib.OK, pl.ptr, d, y.ptr, p(dy), dx.ptr, ws.ptr, ws.nbytes, stream())
    ws.get()                                                             # (the canaries, whatever the plan)
    if pl.single:
        assert ws.written(4 * pl.S * d) and ws.untouched(4 * pl.S * d)
    return dx, form


def softmax_logits(pl, d, key, scale=3.0):
    x = rng_for("softmax", pl.name, pl.form, d, key).normal(size=(pl.n, d)) * scale
    spread = pl.reduce(np.maximum, -np.inf, x) - pl.reduce(np.minimum, np.inf, x)
    assert spread[pl.counts > 0].max(initial=0.0) < 60.0
    return x


def check_softmax(pl, d, key, mis=(), xvals=None):
    x = In(softmax_logits(pl, d, key) if xvals is None else xvals, "x" in mis)
    y, ref, f1 = softmax_fwd(pl, d, x, mis)
    what = f"{pl.name} {pl.form} d={d} mis={mis}"
    dy = In(rng_for("softmax dy", pl.name, pl.form, d, key).normal(size=(pl.n, d)), "dy" in mis)
    dx, f2 = softmax_bwd(pl, d, y, dy, mis)
    k = pl.counts[:, None]
    A, s_ref = pl.sum(np.abs(ref * dy.r)), pl.sum(ref * dy.r)
    Bs = (lin(k, A * (1 + 1e-4)) + 1e-4 * A)[pl.seg]
    dx_ref = ref * (dy.r - s_ref[pl.seg])
    bound = 1e-4 * np.abs(dx_ref) + ref * (1 + 1e-4) * (Bs + 2 * EPS * (np.abs(dy.r) + np.abs(s_ref[pl.seg]) + Bs))
    within(dx, dx_ref, bound, "softmax pullback", "dx " + what)
    assert x.unchanged() and dy.unchanged()
    return f1, f2, y


def check_softmax_pullback_integers(pl, d, key):
    rng = rng_for("softmax int", pl.name, pl.form, d, key)
    y, dy = In(draw("int", rng, pl.n, d)), In(draw("int", rng, pl.n, d))
    s = pl.sum(y.r * dy.r)
    dx, _ = softmax_bwd(pl, d, y, dy)
    integer_exact(dx, y.r * (dy.r - s[pl.seg]), 2 * (2 + pl.sum(np.abs(y.r * dy.r))), f"int softmax pullback {pl.name} {pl.form} d={d}")


def check_broadcast(pl, d, kind, key, mis=()):
    rng = rng_for("broadcast", pl.name, pl.form, d, kind, key)
    u, dout = In(draw(kind, rng, pl.S, d), "u" in mis), In(draw(kind, rng, pl.n, d), "dout" in mis)
    what = f"{pl.name} {pl.form} d={d} {kind} mis={mis}"
    out = Out(pl.n, d, mis="out" in mis)
    f1 = note("broadcast_forward", d, u.ptr, out.ptr)
    call(_lib.load().ngpde_readout_broadcast_forward, _lib.OK, pl.ptr, d, u.ptr, out.ptr, stream())
    exact(out, u.f[pl.seg], "broadcast " + what, bits=True)
    du, ws = Out(pl.S, d, mis="du" in mis), Ws(pl.ws_bytes(d), "ws" in mis)
    f2 = note("broadcast_backward", d, p(dout), du.ptr, ws.ptr)
    call(_lib.load().ngpde_readout_broadcast_backward, _lib.OK, pl.ptr, d, p(dout), du.ptr, ws.ptr, ws.nbytes, stream())
    assert ws.untouched() or not pl.single
    check_sum(du, pl.sum(dout.r), pl.counts[:, None], pl.sum(np.abs(dout.r)), kind, "broadcast du", "du " + what)
    assert not du.get()[pl.counts == 0].any() and u.unchanged() and dout.unchanged()
    return f1, f2


# ---- conditions the references must meet, and the checkers' own test (no GPU) -------------------------------------------------------------

@pytest.mark.parametrize("cr", [64, 256, 1024])
def test_reference_conditions_hold_for_every_layout(cr):
    # whatever the plan's chunk size: integer sums stay below 2^24, and softmax references above float32's smallest normal
    for name, form in itertools.product(("ladder", "single", "one", "none", "long"), FORMS):
        lay = Layout(name, form, cr)
        d = 1 if name == "long" else 3
        x = draw("int", rng_for("conditions", name, form), lay.n, d)
        assert lay.sum(np.abs(x)).max(initial=0.0) <= 2.0 * lay.counts.max(initial=0) < 2.0 ** 24
        assert (2 * (2 + lay.sum(np.abs(x * x)))).max(initial=0.0) < 2.0 ** 24          # the integer softmax pullback
        assert np.array_equal(lay.sum(x), np.stack([x[lay.seg == s].sum(0) for s in range(lay.S)]))
        if name != "long":
            assert (seg_softmax(lay, softmax_logits(lay, d, "conditions")) >= TINY).all()
        planted = np.random.default_rng(1).uniform(-1, 1, size=(lay.n, 1))
        for j in range(7):
            xs, items = plant(lay, planted, j, 31.0)
            ys = seg_softmax(lay, xs)
            assert (ys >= TINY).all() and (ys[items] >= 1 - 1e-4).all()
    assert 516 * 4 * 1025 < 2 ** 24                                          # the widest row times the largest product of two draws


def planted_positions(count, cr):
    """sorted positions inside a segment of `count` > cr rows: one run of the planted tests per entry"""
    full = count // cr
    cand = [0, count - 1, cr - 1, cr, cr + 1, full * cr - 1, full * cr if count % cr else (full - 1) * cr]
    return [min(c, count - 1) for c in cand]


def plant(lay, x, j, value):
    """a copy of x with `value` in every column at the j-th planted position of every multi-chunk segment; the items planted"""
    x = x.copy()
    items = [lay.order[lay.segptr[s] + planted_positions(lay.counts[s], lay.cr)[j]] for s in np.flatnonzero(lay.counts > lay.cr)]
    x[items] = value
    return x, np.asarray(items, dtype=np.int64)


def found(out, lay, value):
    got = out.get() if isinstance(out, Out) else out
    assert (got[lay.counts > lay.cr] == np.float32(value)).all(), "the planted extremum was not found"


def test_planted_positions():
    assert planted_positions(1025, 256) == [0, 1024, 255, 256, 257, 1023, 1024] and planted_positions(257, 256) == [0, 256, 255, 256, 256, 255, 256]
    assert planted_positions(512, 256) == [0, 511, 255, 256, 257, 511, 256] and planted_positions(513, 256)[-2:] == [511, 512]


def test_the_checkers_reject_a_dropped_row():
    # no kernel: each family's checker is given what a reduce that lost one row of a 64-row segment would return, and must refuse it
    lay, d, scratch = Layout("ladder", "shuffled", 256), 8, {}
    s = LADDER.index(64)
    gone = lay.order[lay.segptr[s] + 5]
    for kind in KINDS:
        x = draw(kind, rng_for("mutation", kind), lay.n, d).astype(np.float32).astype(np.float64)
        x[x == 0] = 1.0
        ref, ab = lay.sum(x), lay.sum(np.abs(x))
        xb = x.copy()
        xb[gone] = 0.0
        bad = lay.sum(xb).astype(np.float32)
        _check_sum(ref.astype(np.float32), ref, lay.counts[:, None], ab, kind, "mutation", kind, scratch)
        with pytest.raises(AssertionError):
            _check_sum(bad, ref, lay.counts[:, None], ab, kind, "mutation", kind, scratch)
        with pytest.raises(AssertionError):
            _check_mean(bad / np.maximum(lay.counts, 1)[:, None].astype(np.float32), ref, lay.counts[:, None], ab, kind, "mutation", kind, scratch)
    # exact: a maximum that never saw the row holding it; a broadcast that wrote the neighbouring segment's row
    x = rng_for("mutation max").normal(size=(lay.n, d))
    x[gone] = 9.0
    xb = x.copy()
    xb[gone] = -np.inf
    ref = lay.reduce(np.maximum, -np.inf, x).astype(np.float32)
    exact(ref, ref, "max")
    with pytest.raises(AssertionError):
        exact(lay.reduce(np.maximum, -np.inf, xb).astype(np.float32), ref, "max")
    u = rng_for("mutation u").normal(size=(lay.S, d)).astype(np.float32)
    bad = u[lay.seg].copy()
    bad[gone] = u[s + 1]
    with pytest.raises(AssertionError):
        exact(bad, u[lay.seg], "broadcast", bits=True)
    # planted: the extremum of the 1025-row segment at the first row of its ragged tail, missed
    xp, items = plant(lay, x, 6, 50.0)
    found(lay.reduce(np.maximum, -np.inf, xp).astype(np.float32), lay, 50.0)
    xb = xp.copy()
    xb[items[-1]] = -np.inf
    with pytest.raises(AssertionError):
        found(lay.reduce(np.maximum, -np.inf, xb).astype(np.float32), lay, 50.0)
    assert "mutation" in scratch and not any("mutation" in k for k in WORST)


# ---- 1. plans ----------------------------------------------------------------------------------------------------------------------------

@gpu
def test_plans_match_their_restatement():
    # (Plan.__init__ holds ngpde_readout_info to the numpy restatement; here: that the layouts are what the cases need)
    cr = chunk_rows()
    for pl in plans("ladder", "single", "one", "none", "long"):
        assert pl.ws_bytes(3) == 24 * (pl.S + pl.n_chunks) and _lib.load().ngpde_readout_workspace_bytes(pl.ptr, 0) == 0
        assert pl.contiguous == (pl.form != "shuffled" or pl.name in ("one", "none")), (pl.name, pl.form)
    assert plan("single", "shuffled").single and plan("single", "index").n_chunks == 6 and not plan("ladder", "contiguous").single
    assert plan("long", "contiguous").n_chunks == 259 and plan("long", "contiguous").n == 257 * cr + 2 and 258 > 4 * 64
    assert plan("none", "index").n_chunks == 0 and plan("one", "contiguous").id is None and plan("one", "contiguous").n_chunks == 3
    assert plan("ladder", "index").index is not None and plan("ladder", "shuffled").id_base == 1
    assert _lib.load().ngpde_readout_workspace_bytes(None, 4) == 0


# ---- 2. reduce, softmax, broadcast across the widths ----------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_reduce(d):
    for pl, aggr, kind in itertools.product(plans("ladder", "single", "one", "none"), AGGRS, KINDS):
        f1, f2, _, _ = check_reduce(pl, d, aggr, kind, "widths")
        assert f1 == f2 == want_form(d), (pl.name, pl.form, aggr)


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_softmax(d):
    for pl in plans("ladder", "single", "one", "none"):
        f1, f2, _ = check_softmax(pl, d, "widths")
        assert f1 == f2 == want_form(d), (pl.name, pl.form)
        check_softmax_pullback_integers(pl, d, "widths")


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_broadcast(d):
    for pl, kind in itertools.product(plans("ladder", "single", "one", "none"), KINDS):
        assert check_broadcast(pl, d, kind, "widths") == (want_form(d), want_form(d)), (pl.name, pl.form)


@gpu
@pytest.mark.parametrize("name", ["ladder", "one"])
def test_softmax_large_logits(name):
    # +-40 and +-80 about the segment's centre: finite, and within the bound wherever float32 can hold the reference at all
    for pl, d, half in itertools.product(plans(name), (1, 4, 65), (40.0, 80.0)):
        rng = rng_for("large", pl.name, pl.form, d, half)
        x = In(rng.choice([-half, half], size=(pl.n, d)) + rng.normal(size=(pl.n, d)))
        y, _, _ = softmax_fwd(pl, d, x, every=False)
        dx, _ = softmax_bwd(pl, d, y, In(np.ones((pl.n, d))))
        assert np.isfinite(dx.get()).all()


# ---- 3. the long segment --------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("d", [1, 4])
def test_long_segment(d):
    # 259 chunks: the finish fold runs past its first 4 x slots partials at every dpl (d = 1 and d = 4 aligned: 64 slots)
    for pl in plans("long"):
        for aggr, kind in itertools.product(AGGRS, KINDS):
            f1, f2, _, _ = check_reduce(pl, d, aggr, kind, "long")
            assert f1 == f2 == want_form(d)
        for kind in KINDS:
            assert check_broadcast(pl, d, kind, "long") == (want_form(d), want_form(d))
        check_softmax(pl, d, "long")
        check_softmax_pullback_integers(pl, d, "long")
    if d == 4:                                                           # the same rows through the float form: 16 slots, dpl 4
        pl = plan("long", "shuffled")
        for aggr in AGGRS:
            assert check_reduce(pl, d, aggr, "int", "long mis", mis=("x",))[0] == want_form(d, True)


# ---- 4. planted extrema ---------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,d", [("ladder", 1), ("ladder", 4), ("ladder", 5), ("ladder", 132), ("long", 1), ("long", 4)])
def test_planted_extrema(name, d):
    for pl, j in itertools.product(plans(name), range(7)):
        base = rng_for("planted", name, pl.form, d).uniform(-1, 1, size=(pl.n, d))
        for aggr, value in (("max", 50.0), ("min", -50.0)):
            xv, items = plant(pl, base, j, value)
            _, _, out, dx = check_reduce(pl, d, aggr, "normal", ("planted", j), xvals=xv)
            found(out, pl, value)
            multi = pl.counts[pl.seg] > pl.cr
            hit = np.zeros(pl.n, dtype=bool)
            hit[items] = True
            assert not dx.get()[multi & ~hit].any(), "gradient routed past the planted row"
        xv, items = plant(pl, base, j, 31.0)                             # 30 above the rest: the others weigh < n e^-30 together
        _, _, y = check_softmax(pl, d, ("planted", j), xvals=xv)
        assert (y.get()[items] >= 1 - 1e-4).all(), "the softmax missed the planted logit"


# ---- 5. misaligned pointers -----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("d", MIS_WIDTHS)
def test_misaligned_pointers(d):
    # each array in turn 4 bytes in, the workspace included: the float form (dpl 64, one and four column chunks), the same bounds
    for pl in (plan("ladder", "shuffled"), plan("single", "contiguous")):
        for m in ("", "x", "out", "ws", "dout", "dx"):
            mis = (m,) if m else ()
            for aggr in AGGRS:
                f1, f2, _, _ = check_reduce(pl, d, aggr, "int", "mis", mis)
                assert f1 == want_form(d, m in ("x", "out", "ws")) and f2 == want_form(d, m in ("x", "out", "dout", "dx")), (m, aggr)
        for m in ("", "x", "y", "ws", "dy", "dx"):
            f1, f2, _ = check_softmax(pl, d, "mis", (m,) if m else ())
            assert f1 == want_form(d, m in ("x", "y", "ws")) and f2 == want_form(d, m in ("y", "dy", "dx", "ws")), m
        for m in ("", "u", "out", "dout", "du", "ws"):
            f1, f2 = check_broadcast(pl, d, "int", "mis", (m,) if m else ())
            assert f1 == want_form(d, m in ("u", "out")) and f2 == want_form(d, m in ("dout", "du", "ws")), m


# ---- 6. the workspace and the refusals ------------------------------------------------------------------------------------------------------

@gpu
def test_workspace_and_refusals():
    lib, d = _lib.load(), 8
    pl = plan("ladder", "shuffled")
    x, seg_rows = In(np.ones((pl.n, d))), In(np.ones((pl.S, d)))
    out_seg, out_item = Out(pl.S, d), Out(pl.n, d)

    def refused(code, word, fn, *args):
        st = fn(*args)
        torch.cuda.synchronize()
        msg = lib.ngpde_last_error().decode()
        assert st == code and word in msg, (st, code, msg)
        assert out_seg.untouched() and out_item.untouched()

    need = pl.ws_bytes(d)
    for short in (1, need):                                              # one byte short, and none at all
        ws = Ws(need - short)
        wp = ws.ptr if ws.nbytes else None
        refused(_lib.ERR_WORKSPACE, "workspace", lib.ngpde_readout_reduce_forward, pl.ptr, d, 0, x.ptr, out_seg.ptr, wp, ws.nbytes, stream())
        refused(_lib.ERR_WORKSPACE, "workspace", lib.ngpde_readout_softmax_forward, pl.ptr, d, x.ptr, out_item.ptr, wp, ws.nbytes, stream())
        refused(_lib.ERR_WORKSPACE, "workspace", lib.ngpde_readout_softmax_backward, pl.ptr, d, x.ptr, x.ptr, out_item.ptr, wp, ws.nbytes, stream())
        refused(_lib.ERR_WORKSPACE, "workspace", lib.ngpde_readout_broadcast_backward, pl.ptr, d, x.ptr, out_seg.ptr, wp, ws.nbytes, stream())
        assert ws.untouched()
    refused(_lib.ERR_WORKSPACE, "workspace", lib.ngpde_readout_reduce_forward, pl.ptr, d, 0, x.ptr, out_seg.ptr, None, need, stream())
    # (exactly enough succeeds with its canaries intact: reduce_fwd, softmax_fwd, softmax_bwd and check_broadcast read them after
    # every launch of every other test; the softmax forward is the entry that writes up to the last byte)
    ws = Ws(need)
    MUL = _lib.AGGR["mul"]
    # the documented order: a negative width, a refused aggregation, a NULL plan, the workspace
    refused(_lib.ERR_DIMENSION_MISMATCH, "negative width", lib.ngpde_readout_reduce_forward, None, -1, MUL, x.ptr, out_seg.ptr, ws.ptr, 0, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "aggregation", lib.ngpde_readout_reduce_forward, None, d, MUL, x.ptr, out_seg.ptr, ws.ptr, 0, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "readout is NULL", lib.ngpde_readout_reduce_forward, None, d, 0, x.ptr, out_seg.ptr, ws.ptr, 0, stream())
    refused(_lib.ERR_DIMENSION_MISMATCH, "negative width", lib.ngpde_readout_reduce_backward, None, -1, MUL, x.ptr, seg_rows.ptr, seg_rows.ptr,
            out_item.ptr, stream())
    for bad in (MUL, 9, -1):
        refused(_lib.ERR_INVALID_ARGUMENT, "aggregation", lib.ngpde_readout_reduce_forward, pl.ptr, d, bad, x.ptr, out_seg.ptr, ws.ptr, need, stream())
        refused(_lib.ERR_INVALID_ARGUMENT, "aggregation", lib.ngpde_readout_reduce_backward, pl.ptr, d, bad, x.ptr, seg_rows.ptr, seg_rows.ptr,
                out_item.ptr, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "readout is NULL", lib.ngpde_readout_reduce_backward, None, d, 0, x.ptr, seg_rows.ptr, seg_rows.ptr,
            out_item.ptr, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "readout is NULL", lib.ngpde_readout_softmax_forward, None, d, x.ptr, out_item.ptr, ws.ptr, need, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "readout is NULL", lib.ngpde_readout_softmax_backward, None, d, x.ptr, x.ptr, out_item.ptr, ws.ptr, need, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "readout is NULL", lib.ngpde_readout_broadcast_forward, None, d, seg_rows.ptr, out_item.ptr, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "readout is NULL", lib.ngpde_readout_broadcast_backward, None, d, x.ptr, out_seg.ptr, ws.ptr, need, stream())
    refused(_lib.ERR_DIMENSION_MISMATCH, "negative width", lib.ngpde_readout_broadcast_forward, None, -1, seg_rows.ptr, out_item.ptr, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "readout is NULL", lib.ngpde_readout_info, None, None, None, None, None, None)
    # NULL operands an entry needs
    refused(_lib.ERR_INVALID_ARGUMENT, "NULL argument", lib.ngpde_readout_reduce_forward, pl.ptr, d, 0, None, out_seg.ptr, ws.ptr, need, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "NULL argument", lib.ngpde_readout_reduce_backward, pl.ptr, d, _lib.AGGR["max"], None, seg_rows.ptr,
            seg_rows.ptr, out_item.ptr, stream())
    refused(_lib.ERR_INVALID_ARGUMENT, "NULL argument", lib.ngpde_readout_broadcast_forward, pl.ptr, d, None, out_item.ptr, stream())
    assert ws.untouched()
    # d = 0: nothing to do, nothing needed
    ok(lib.ngpde_readout_reduce_forward(pl.ptr, 0, 0, None, None, None, 0, stream()))
    ok(lib.ngpde_readout_softmax_forward(pl.ptr, 0, None, None, None, 0, stream()))
    # create: an id outside its range, either side, in every form; more than one segment without ids
    for form, (where, bad) in itertools.product(FORMS, ((0, -1), (-1, len(LADDER)))):
        lay = Layout("ladder", form, pl.cr)
        ids = lay.id.copy()
        ids[where if lay.index is None else lay.index[where]] = bad + lay.id_base     # (index form: a node that has an edge)
        id_dev = torch.as_tensor(ids.astype(np.int32), device=DEV)
        idx_dev = None if lay.index is None else torch.as_tensor(lay.index.astype(np.int32), device=DEV)
        h = C.c_void_p(1)
        st = lib.ngpde_readout_create(lay.n, id_dev.data_ptr(), None if idx_dev is None else idx_dev.data_ptr(), lay.id_base, lay.S, stream(),
                                      C.byref(h))
        assert st == _lib.ERR_INVALID_ARGUMENT and "outside" in lib.ngpde_last_error().decode() and not h.value, (form, where)
    h = C.c_void_p(1)
    assert lib.ngpde_readout_create(5, None, None, 0, 2, stream(), C.byref(h)) == _lib.ERR_INVALID_ARGUMENT and not h.value
    assert lib.ngpde_readout_create(5, None, None, 0, 0, stream(), C.byref(h)) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_readout_create(-1, None, None, 0, 1, stream(), C.byref(h)) == _lib.ERR_INVALID_ARGUMENT


# ---- 7. what the launches above covered ------------------------------------------------------------------------------------------------

@gpu
def test_every_lane_layout_and_segment_length_was_launched():
    # the last test of the file, over what the tests before it recorded (run the file as a whole): every entry in both column types at
    # every dpl and at one, two and three column chunks, the misaligned four; every ladder length, the long segment
    every = {1, 2, 4, 8, 16, 32, 64}
    for entry in ("reduce_forward", "reduce_backward", "softmax_forward", "softmax_backward", "broadcast_forward", "broadcast_backward"):
        for typ in ("f4", "float"):
            got = {(dpl, chunks) for e, t, dpl, chunks in CASES if e == entry and t == typ}
            assert {dpl for dpl, _ in got} >= every and {chunks for _, chunks in got} >= {1, 2, 3}, (entry, typ, sorted(got))
        assert (entry, "float", 64, 4) in CASES, entry
    assert set(LADDER) | {257 * chunk_rows() + 1, 2 * chunk_rows() + 188} <= LENGTHS
