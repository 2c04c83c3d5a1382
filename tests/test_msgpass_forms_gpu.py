"""The user-layer message passing (csrc/msgpass.hip on the lane layout of csrc/row_lanes.h) against float64 across its forms.

Every entry is called through the C ABI with raw pointers, so that NULL operands, NULL tables and misaligned pointers reach it.  The
library's by-target lists (rowptr / col / eid) and by-source lists are compared with np.argsort(., kind="stable") restatements before
any kernel runs (Gr.attach).  Node arrays are [N][d], per-edge inputs and outputs of propagate / apply_edges / softmax are [E][.] in
COO order, the gather's xi / xj are [E][w] in p order (by target).

Dispatch, restated below and asserted in every case (gather_vec, emul_form, dot_form, lanes):
  lanes(w)   row_lanes.h's lanes_per_entry: the next power of two >= w, at most 64.  A row of w columns (float4 columns in the f4
             form: w = d / 4) takes ceil(w / dpl) column chunks, the last one clamped to column w - 1; 64 / dpl entry slots.
  ngpde_gather_forward    per array k: float4 rows iff width[k] % 4 == 0 and x[k], xi[k], xj[k] are each NULL or 16-byte aligned;
                          an array with width 0 or neither output takes no part.  One flat walk of (entry, column) pairs, 256 a step.
  ngpde_gather_backward   per array k: float4 iff width[k] % 4 == 0 and dxi[k], dxj[k], dx[k] are each NULL or aligned.
  ngpde_propagate_emul_forward   EW = 0 for e_width 0, 1 for e_width 1 and d != 1, else 2 (so e_width == d == 1 is EW 2).  float4 iff
                          d % 4 == 0, x and out aligned, and e aligned when EW == 2 (a scalar per edge is read as floats in any case).
  ngpde_propagate_emul_backward  the by-source walk (when dx, or de at EW 2): float4 iff d % 4 == 0 and dout, dx, and at EW 2 x, de
                          and e, are NULL or aligned.  de at EW 1 is the dot kernel over (dout, x): float4 iff d % 4 == 0 and
                          dout, x aligned.  Neither dx nor de: no launch.
  ngpde_apply_edges_dot_forward  float4 iff d % 4 == 0 and xi, xj aligned (out is a float per edge).  d = 0 zeroes out.
  ngpde_apply_edges_dot_backward dxi: the by-target walk with EW = 1 (2 for d = 1) over (xj, dout, dxi); dxj: by source over
                          (xi, dout, dxj); float4 iff d % 4 == 0 and the node array and the output are aligned.
  ngpde_softmax_edge_neighbors_* one (float) form, lanes (slot, head) with dpl = lanes(h).
      d          4   8  12  16 | 20  32 | 36  64 | 68 128 | 132 256 | 260 516    1  2  3  5  7 13 21 33 63  65 130   64 256 4 bytes in
      columns    1   2   3   4 |  5   8 |  9  16 | 17  32 |  33  64 |  65 129    1  2  3  5  7 13 21 33 63  65 130   64 256
      dpl        1   2   4   4 |  8   8 | 16  16 | 32  32 |  64  64 |  64  64    1  2  4  8  8 16 32 64 64  64  64   64  64
      chunks     1                                                  |   2   3    1                          2   3    1   4
  (13 and 21 are there for the float form at dpl 16 and 32, which none of 1 2 3 5 7 33 63 65 130 reaches.)

Graphs: A has in-degrees 0 1 2 3 4 5 7 8 9 15 16 17 31 32 33 63 64 65 127 128 129 255 256 257 300 (slots, 4 slots and +-1 for every
dpl) on 33 nodes, sources drawn with replacement from nodes 0 .. 29, COO list shuffled, self loops and repeated edges among them; B is
A reversed (the same ladder by source); an edgeless graph of 5 nodes; one node without edges.

References are float64 numpy of the operation itself on the float32 inputs, compared element by element:
  exact     the gathers (the same bits), every zero of an empty row, arrays a call must not touch (NaN between guard words).
  integer   inputs drawn from {-2 .. 2}: every float32 product and partial sum is an integer below 2^24 (asserted on sum|term|), so
            sums, dot products, dx, de must equal the float64 result bit for bit in any order; the mean must be within 2 ulp of that
            exact sum times the float32 1 / count.  No dropped, doubled or misrouted entry passes this.
  linear    normal draws, sums of k float32 terms: |out - ref| <= (k + 2) 2^-24 sum|term_i|  (k - 1 roundings of partial sums, the
            term's own product, the mean's 1 / deg and scaling).  Dot products of width d over k entries: (d + k + 4) 2^-24 sum|terms|.
  softmax   |y - ref| <= 1e-4 ref for every entry (logit spread below 60 inside a row: every reference entry is above float32's
            smallest normal, asserted); with logits +-40 about the row's centre the bound applies to the entries float32 can hold.
            Every non-empty row sums to 1 within (k + 2) 2^-24 + 1e-4.
  softmax pullback   de = y (dy - s), s = sum_row y dy, run on the kernel's own y = ref (1 + delta), |delta| <= 1e-4.  With
            A = sum_row |ref dy|:  |s - s_ref| <= B_s = (k + 2) 2^-24 A (1 + 1e-4) + 1e-4 A  (the float32 sum of the terms it was
            given, plus those terms' own error), and de = fl(y fl(dy - s)) adds two roundings, so
            |de - de_ref| <= 1e-4 |de_ref| + ref (1 + 1e-4) (B_s + 2 2^-24 (|dy| + |s_ref| + B_s)).
            With integer y and dy (no softmax, the same kernel) s and de are exact and must match bit for bit.

Measured on the MI355X, worst err / bound over every case of this file (teardown_module prints the table under `pytest -s`):
  linear    gather pullback 0.33   propagate + 0.47   mean 0.60   dx 0.62   de (a row per edge) 0.65   de (a scalar per edge) 0.30
            apply_edges dot 0.28   dxi 0.43   dxj 0.46
  integer   every sum, dot product, dx and de: the same bits; the mean 0.25 of its 2 ulp
  softmax   y 0.040   row sums 0.004   equal logits 0.021   pullback 0.012
  The nearest are the one- and two-entry rows under the mean (k + 2 = 3 allows three roundings and the term, 1 / deg and the scaling
  are three; de = (dout / deg) x is two of its three): nothing above two thirds, as the count of roundings says.
  Every launch form came up in both column types at dpl 1 2 4 8 16 32 64 and at one, two and three (misaligned 256: four) column
  chunks; the softmax at dpl 1 2 4 8 64 and one to three chunks; rows of every ladder length by target (A) and by source (B).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from ngpde_amd import _lib
import test_mp_primitive_forms_gpu as P
from test_mp_primitive_forms_gpu import EPS, TINY, In, Out, exact, lin, ok, p, rng_for, same_bits, seg_sum, stream

gpu = pytest.mark.gpu
SUM, MEAN = _lib.AGGR["sum"], _lib.AGGR["mean"]

F4_WIDTHS = {4: 1, 8: 2, 12: 4, 16: 4, 20: 8, 32: 8, 36: 16, 64: 16, 68: 32, 128: 32, 132: 64, 256: 64, 260: 64, 516: 64}
SCALAR_WIDTHS = {1: 1, 2: 2, 3: 4, 5: 8, 7: 8, 13: 16, 21: 32, 33: 64, 63: 64, 65: 64, 130: 64}
WIDTHS = list(F4_WIDTHS) + list(SCALAR_WIDTHS)
MIS_WIDTHS = (64, 256)
HEADS = (1, 2, 3, 4, 5, 8, 33, 64, 65, 130)
IN_DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
N_NODES, N_SOURCES = 33, 30
KINDS = ("normal", "int")

WORST = {}                                      # family -> worst err / bound seen
CASES = set()                                   # (entry, column type, dpl, column chunks) of every launch checked
LENGTHS = set()                                 # row lengths, by target and by source, of every graph a launch walked


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------

def lanes(w):
    dpl = 1
    while dpl < w and dpl < 64:
        dpl *= 2
    return dpl


def aligned(*ptrs):
    return all(q is None or q % 16 == 0 for q in ptrs)


def form_of(d, vec):
    """(column type, dpl, column chunks) of a row of d floats"""
    w = d // 4 if vec else d
    return ("f4" if vec else "float", lanes(w), -(-w // lanes(w)))


def gather_vec(w, *ptrs):
    return w % 4 == 0 and aligned(*ptrs)


def ew_of(d, e_width):
    return 0 if e_width == 0 else 1 if e_width == 1 and d != 1 else 2


def emul_form(d, ew, X, out, x_own=None, de=None, e=None):
    return form_of(d, d % 4 == 0 and aligned(X, out, x_own, de) and (ew != 2 or aligned(e)))


def dot_form(d, A, B):
    return form_of(d, d % 4 == 0 and aligned(A, B))


def want_form(d, misaligned=False):
    return form_of(d, d in F4_WIDTHS and not misaligned)


def note(entry, form):
    CASES.add((entry,) + form)
    return form


def test_width_tables_cover_every_lane_layout():
    # every dpl from 1 to 64 in both column types; clamped lanes (12, 20, 3, 5); two and three column chunks with a clamped tail
    assert {d: lanes(d // 4) for d in F4_WIDTHS} == F4_WIDTHS and {d: lanes(d) for d in SCALAR_WIDTHS} == SCALAR_WIDTHS
    assert all(d % 4 == 0 for d in F4_WIDTHS) and all(d % 4 for d in SCALAR_WIDTHS)
    assert set(F4_WIDTHS.values()) == set(SCALAR_WIDTHS.values()) == {1, 2, 4, 8, 16, 32, 64}
    assert want_form(12) == ("f4", 4, 1) and want_form(20) == ("f4", 8, 1) and want_form(260) == ("f4", 64, 2)
    assert want_form(516) == ("f4", 64, 3) and want_form(65) == ("float", 64, 2) and want_form(130) == ("float", 64, 3)
    assert want_form(64, True) == ("float", 64, 1) and want_form(256, True) == ("float", 64, 4)
    assert emul_form(64, 1, 0, 16, e=4) == ("f4", 16, 1) and emul_form(64, 2, 0, 16, e=4) == ("float", 64, 1)
    assert {lanes(h) for h in HEADS} == {1, 2, 4, 8, 64} and ew_of(1, 1) == 2 and ew_of(2, 1) == 1 and ew_of(1, 0) == 0
    for dpl in (1, 2, 4, 8, 16, 32, 64):          # rows of slots and 4 slots entries, and one either side
        slots = 64 // dpl
        assert {slots, slots + 1, 4 * slots, 4 * slots + 1}.issubset(IN_DEGREES) and {slots - 1, 4 * slots - 1}.issubset(IN_DEGREES)
    assert max(IN_DEGREES) == 300


# ---- graphs -----------------------------------------------------------------------------------------------------------------------------

class Gr(P.Gr):
    """the shared graph restatement (p order and by-source order), attached to the library on first use of .ptr, so that the graphs
    also serve the tests that run without a GPU; attach() holds the by-target and the by-source lists to the restatement"""

    def __init__(self, s, t, n):
        super().__init__(s, t, n, attach=False)

    def __getattr__(self, name):                   # (only reached while .ptr / .handle / .g do not exist yet)
        if name not in ("ptr", "handle", "g"):
            raise AttributeError(name)
        self.attach()
        LENGTHS.update(int(k) for k in self.indeg)
        LENGTHS.update(int(k) for k in self.outdeg)
        return self.__dict__[name]


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        z = np.zeros(0, dtype=np.int64)
        if name == "edgeless":
            _GRAPHS[name] = Gr(z, z, 5)
        elif name == "one":
            _GRAPHS[name] = Gr(z, z, 1)
        else:
            rng = np.random.default_rng(31)
            t = np.repeat(np.arange(len(IN_DEGREES)), IN_DEGREES)
            s = rng.integers(0, N_SOURCES, t.size)
            k = rng.permutation(t.size)
            s, t = (s[k], t[k]) if name == "A" else (t[k], s[k])
            _GRAPHS[name] = Gr(s, t, N_NODES)
    return _GRAPHS[name]


def teardown_module(module):
    _GRAPHS.clear()
    if WORST:
        print("\nworst err / bound per family:")
        for fam in sorted(WORST):
            print(f"  {fam:40s} {WORST[fam]:.3f}")
        print("launch forms checked (entry: column type dpl x column chunks):")
        for entry in sorted({c[0] for c in CASES}):
            print(f"  {entry:28s}", " ".join(f"{t}{d}x{n}" for _, t, d, n in sorted(c for c in CASES if c[0] == entry)))
        print("row lengths walked:", " ".join(str(k) for k in sorted(LENGTHS)))


def test_graphs_are_what_the_cases_need():
    a, b = graph("A"), graph("B")
    assert a.n == 33 and a.n % 4 != 0 and a.E == sum(IN_DEGREES) == 1827
    assert list(a.indeg[:25]) == IN_DEGREES and not a.indeg[25:].any() and list(b.outdeg[:25]) == IN_DEGREES
    assert (a.s == a.t).any() and np.unique(a.s * 33 + a.t).size < a.E                    # self loops, repeated edges
    assert not np.array_equal(a.perm, np.arange(a.E)) and not np.array_equal(b.perm_s, np.arange(b.E))
    assert (a.outdeg == 0).any() and (b.indeg == 0).any() and a.outdeg.max() > 8 and b.indeg.max() > 8
    assert graph("edgeless").n == 5 and graph("edgeless").E == 0 and graph("one").n == 1 and graph("one").E == 0
    for prod, d, vec in GATHER_SPANS:                                                 # the flat walk's (deg, w) products
        w = d // 4 if vec else d
        assert prod % w == 0 and prod // w in IN_DEGREES and (d % 4 == 0) == vec


# ---- bounds and comparisons -----------------------------------------------------------------------------------------------------------

def within(out, ref, bound, fam, what, worst=WORST):
    return P.within(out, ref, bound, fam, what, worst)


def integer_exact(out, ref, ab, what):
    """the float64 sum of integer terms, every partial sum below 2^24: float32 must give the same number in any order"""
    assert np.max(ab, initial=0.0) < 2.0 ** 24, what
    assert np.array_equal(ref, np.rint(ref))
    exact(out, ref.astype(np.float32), what)


def check_sum(out, ref, k, ab, kind, fam, what, worst=WORST):
    if kind == "int":
        integer_exact(out, ref, ab, what)
    else:
        within(out, ref, lin(k, ab), fam, what, worst)


def check_mean(out, total, k, ab, kind, fam, what, worst=WORST):
    """total: the float64 sum; k: the count per row (0: the mean is 0)"""
    k = np.broadcast_to(k, total.shape)
    if kind == "int":
        assert np.max(ab, initial=0.0) < 2.0 ** 24, what
        r32 = np.where(k > 0, (np.float32(1.0) / np.maximum(k, 1).astype(np.float32)).astype(np.float64), 0.0)
        ref = total * r32                                                # exact in float64: two 24-bit factors
        within(out, ref, 2.0 * np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64), fam + ", integer (2 ulp)", what, worst)
    else:
        within(out, total / np.maximum(k, 1), lin(k, ab) / np.maximum(k, 1), fam, what, worst)


def draw(kind, rng, *shape):
    return rng.integers(-2, 3, size=shape).astype(np.float64) if kind == "int" else rng.normal(size=shape)


def drop_row(x, idx, row):
    """x without the first entry of segment `row`: what a kernel that skips one entry would have summed"""
    keep = np.ones(len(idx), dtype=bool)
    keep[np.flatnonzero(idx == row)[0]] = False
    return x[keep], idx[keep]


def test_the_checkers_reject_a_dropped_row():
    # no kernel: each family's checker is given the result of a sum that lost one entry of a 64-entry row, and must refuse it
    g, d, scratch = graph("A"), 8, {}
    row = IN_DEGREES.index(64)
    for kind in KINDS:
        x = draw(kind, rng_for("mutation", kind), g.E, d).astype(np.float32).astype(np.float64)
        x[x == 0] = 1.0                                                  # (a dropped zero changes nothing)
        ref, ab = seg_sum(x, g.t, g.n), seg_sum(np.abs(x), g.t, g.n)
        bad = seg_sum(*drop_row(x, g.t, row), g.n).astype(np.float32)
        check_sum(ref.astype(np.float32), ref, g.indeg[:, None], ab, kind, "mutation", kind, scratch)
        with pytest.raises(AssertionError):
            check_sum(bad, ref, g.indeg[:, None], ab, kind, "mutation", kind, scratch)
        with pytest.raises(AssertionError):
            check_mean(bad / np.maximum(g.indeg, 1)[:, None].astype(np.float32), ref, g.indeg[:, None], ab, kind, "mutation", kind, scratch)
    # exact: a gather that repeats the previous entry in place of one
    xi = x.astype(np.float32)[g.tp]
    bad = xi.copy()
    bad[g.rowptr[row] + 5] = xi[g.rowptr[row] - 1]
    exact(xi, xi, "copy", bits=True)
    with pytest.raises(AssertionError):
        exact(bad, xi, "copy", bits=True)
    # softmax: the denominator lost one of 64 entries
    e = rng_for("mutation softmax").normal(size=(g.E, 2))
    y, yb = softmax_ref(g, e), softmax_ref(g, e, drop=row)
    within(y.astype(np.float32), y, 1e-4 * y, "mutation", "softmax", scratch)
    with pytest.raises(AssertionError):
        within(yb.astype(np.float32), y, 1e-4 * y, "mutation", "softmax", scratch)
    assert "mutation" in scratch and not any("mutation" in k for k in WORST)


# ---- 1. ngpde_gather_forward / _backward -----------------------------------------------------------------------------------------------

GATHER_SPANS = [(255, 1, False), (256, 1, False), (257, 1, False), (255, 85, False), (513, 57, False), (255, 4, True), (256, 16, True),
                (256, 64, True), (257, 4, True), (255, 68, True), (513, 228, True)]    # (deg x w, d, float4 columns)


def table(items):
    arr = (C.c_void_p * max(len(items), 1))()
    for i, x in enumerate(items):
        arr[i] = p(x)
    return arr


def int_table(vals):
    return (C.c_int32 * max(len(vals), 1))(*[int(v) for v in vals])


def gather_fwd(g, xs, widths, sides, mis=(), tables=(True, True)):
    """sides[k] = (want xi, want xj); mis: names like "xi2" placed 4 bytes in; tables: pass the xi / xj table at all"""
    xi = [Out(g.E, w, mis=f"xi{k}" in mis) if si else None for k, (w, (si, _)) in enumerate(zip(widths, sides))]
    xj = [Out(g.E, w, mis=f"xj{k}" in mis) if sj else None for k, (w, (_, sj)) in enumerate(zip(widths, sides))]
    vec = [gather_vec(w, p(x), p(a), p(b)) for w, x, a, b in zip(widths, xs, xi, xj)]
    ok(_lib.load().ngpde_gather_forward(g.ptr, len(xs), table(xs), int_table(widths), table(xi) if tables[0] else None,
                                        table(xj) if tables[1] else None, stream()))
    for k, (w, x, a, b) in enumerate(zip(widths, xs, xi, xj)):
        if a is not None or b is not None:
            note("gather_forward", form_of(w, vec[k]))
        for o, idx, on in ((a, g.tp, tables[0]), (b, g.sp, tables[1])):
            if o is not None and on:
                exact(o, x.f[idx], f"gather array {k} w={w}", bits=True)
            elif o is not None:
                assert o.untouched()
        assert x is None or x.unchanged()
    return vec


def gather_bwd(g, widths, dxi, dxj, kind, want=None, mis=(), tables=(True, True)):
    dx = [None if want is not None and not want[k] else Out(g.n, w, mis=f"dx{k}" in mis) for k, w in enumerate(widths)]
    gi, gj = (dxi if tables[0] else [None] * len(widths)), (dxj if tables[1] else [None] * len(widths))
    vec = [gather_vec(w, p(a), p(b), p(o)) for w, a, b, o in zip(widths, gi, gj, dx)]
    ok(_lib.load().ngpde_gather_backward(g.ptr, len(widths), int_table(widths), table(dxi) if tables[0] else None,
                                         table(dxj) if tables[1] else None, table(dx), stream()))
    for k, (w, a, b, o) in enumerate(zip(widths, gi, gj, dx)):
        if o is None:
            continue
        note("gather_backward", form_of(w, vec[k]))
        zero = np.zeros((g.n, w))
        ref = (zero if a is None else seg_sum(a.r, g.tp, g.n)) + (zero if b is None else seg_sum(b.r, g.sp, g.n))
        ab = (zero if a is None else seg_sum(np.abs(a.r), g.tp, g.n)) + (zero if b is None else seg_sum(np.abs(b.r), g.sp, g.n))
        cnt = (0 if a is None else g.indeg) + (0 if b is None else g.outdeg) + np.zeros(g.n, dtype=np.int64)
        check_sum(o, ref, cnt[:, None], ab, kind, "gather pullback", f"dx array {k} w={w} {kind}")
        assert not o.get()[cnt == 0].any()
    return vec


def gather_bwd_values(g, d, kind, name):
    rng = rng_for("gather bwd", name, d, kind)
    return draw(kind, rng, g.E, d), draw(kind, rng, g.E, d)


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_gather_one_array(d):
    # both sides; xi only and xj only, through a NULL table and through a NULL entry; the pullback of each
    for name in ("A", "B"):
        g = graph(name)
        x = In(rng_for("gather", name, d).normal(size=(g.n, d)))
        for sides, tables in (((True, True), (True, True)), ((True, False), (True, True)), ((False, True), (True, True)),
                              ((True, False), (True, False)), ((False, True), (False, True))):
            assert gather_fwd(g, [x], [d], [sides], tables=tables) == [d in F4_WIDTHS]
        for kind in KINDS:
            dxi, dxj = (In(v) for v in gather_bwd_values(g, d, kind, name))
            for a, b, tables in ((dxi, dxj, (True, True)), (dxi, None, (True, True)), (None, dxj, (True, True)),
                                 (dxi, dxj, (True, False)), (dxi, dxj, (False, True)), (None, None, (False, False))):
                assert gather_bwd(g, [d], [a], [b], kind, tables=tables) == [d in F4_WIDTHS]
            assert dxi.unchanged() and dxj.unchanged()


@gpu
def test_gather_flat_walk_spans():
    # rows whose (entries x columns) is 255, 256, 257 and 513: the 256-pair step of gather_row, in both column types
    g = graph("A")
    for prod, d, vec in GATHER_SPANS:
        x = In(rng_for("spans", d).normal(size=(g.n, d)))
        assert gather_fwd(g, [x], [d], [(True, True)]) == [vec]


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_gather_several_arrays_in_one_launch(name):
    g = graph(name)
    widths = [1, 12, 64, 130]
    rng = rng_for("gather4", name)
    xs = [In(rng.normal(size=(g.n, w))) for w in widths]
    both = [(True, True)] * 4
    assert gather_fwd(g, xs, widths, both) == [False, True, True, False]
    for mis, vec in ((("xi2",), [False, True, False, False]), (("xj2",), [False, True, False, False]), (("xj1",), [False, False, True, False])):
        assert gather_fwd(g, xs, widths, both, mis=mis) == vec           # one output 4 bytes in: that array alone falls back
    xm = [xs[0], In(xs[1].f, mis=True), xs[2], xs[3]]                    # an input 4 bytes in
    assert gather_fwd(g, xm, widths, both) == [False, False, True, False]
    # single entries NULL; an array with neither output takes no part and its x may be NULL
    assert gather_fwd(g, xs[:3] + [None], widths, [(False, True), (True, True), (True, False), (False, False)]) == [False, True, True, False]
    ok(_lib.load().ngpde_gather_forward(g.ptr, 0, None, None, None, None, stream()))                      # n = 0
    ok(_lib.load().ngpde_gather_backward(g.ptr, 0, None, None, None, None, stream()))
    for kind in KINDS:
        dxi, dxj = [In(draw(kind, rng, g.E, w)) for w in widths], [In(draw(kind, rng, g.E, w)) for w in widths]
        assert gather_bwd(g, widths, dxi, dxj, kind) == [False, True, True, False]
        assert gather_bwd(g, widths, dxi, dxj, kind, mis=("dx2",)) == [False, True, False, False]
        dm = [dxi[0], dxi[1], In(dxi[2].f, mis=True), dxi[3]]
        assert gather_bwd(g, widths, dm, dxj, kind) == [False, True, False, False]
        # dxi-only and dxj-only entries, and an array whose dx is NULL (skipped)
        assert gather_bwd(g, widths, [dxi[0], None, dxi[2], dxi[3]], [None, dxj[1], dxj[2], dxj[3]], kind,
                          want=[True, True, True, False]) == [False, True, True, False]


@gpu
@pytest.mark.parametrize("d", MIS_WIDTHS)
def test_gather_misaligned_pointers(d):
    # d = 64 (one chunk) and 256 (four chunks of 64 lanes): each row array in turn 4 bytes in -> the float walk, the same bits
    for name in ("A", "B"):
        g = graph(name)
        rng = rng_for("gather mis", name, d)
        vals = rng.normal(size=(g.n, d))
        for mis in ((), ("x",), ("xi0",), ("xj0",)):
            assert gather_fwd(g, [In(vals, "x" in mis)], [d], [(True, True)], mis=mis) == [not mis]
        gi, gj = rng.normal(size=(g.E, d)), rng.normal(size=(g.E, d))
        for mis in ((), ("dxi",), ("dxj",), ("dx0",)):
            assert gather_bwd(g, [d], [In(gi, "dxi" in mis)], [In(gj, "dxj" in mis)], "normal", mis=mis) == [not mis]


# ---- 2. ngpde_propagate_emul_forward / _backward ---------------------------------------------------------------------------------------

def e_of(e, d):
    return 1.0 if e is None else e.r                                      # [E][1] broadcasts over the row


def emul_fwd(g, d, e_width, aggr, x, e, kind, mis=()):
    out = Out(g.n, d, mis="out" in mis)
    form = note("propagate_emul_forward", emul_form(d, ew_of(d, e_width), p(x), out.ptr, e=p(e)))
    ok(_lib.load().ngpde_propagate_emul_forward(g.ptr, d, e_width, aggr, p(x), p(e), out.ptr, stream()))
    what = f"propagate d={d} e_width={e_width} aggr={aggr} {kind} mis={mis}"
    terms = (e_of(e, d) * x.r[g.s]) if g.E else np.zeros((0, d))
    total, ab = seg_sum(terms, g.t, g.n), seg_sum(np.abs(terms), g.t, g.n)
    if aggr == SUM:
        check_sum(out, total, g.indeg[:, None], ab, kind, "propagate +", what)
    else:
        check_mean(out, total, g.indeg[:, None], ab, kind, "propagate mean", what)
    assert not out.get()[g.indeg == 0].any(), what
    return out, form


def emul_bwd(g, d, e_width, aggr, x, e, dout, kind, with_dx=True, with_de=True, mis=(), null_x=False):
    ew = ew_of(d, e_width)
    dx, de = Out(g.n, d, mis="dx" in mis), Out(g.E, max(e_width, 1), mis="de" in mis)
    dxp, dep = dx.ptr if with_dx else None, de.ptr if with_de else None
    xp = None if null_x else p(x)
    forms = []
    if with_dx or (with_de and ew == 2):
        forms.append(note("propagate_emul_backward", emul_form(d, ew, p(dout), dxp, xp if ew == 2 else None, dep if ew == 2 else None, p(e))))
    if with_de and ew == 1:
        forms.append(note("propagate_emul_backward de", dot_form(d, p(dout), xp)))
    ok(_lib.load().ngpde_propagate_emul_backward(g.ptr, d, e_width, aggr, xp, p(e), p(dout), dxp, dep, stream()))
    what = f"propagate pullback d={d} e_width={e_width} aggr={aggr} {kind} dx={with_dx} de={with_de} mis={mis}"
    rdeg = (np.float32(1.0) / np.maximum(g.indeg, 1).astype(np.float32)).astype(np.float64) if aggr == MEAN else np.ones(g.n)
    gt = dout.r[g.t] * rdeg[g.t][:, None]                                 # dout[t_e] (/ deg t_e), one row per edge
    inexact = "normal" if aggr == MEAN else kind                          # (1 / deg is no integer: the linear bound, whatever the draw)
    if with_dx:
        terms = e_of(e, d) * gt
        check_sum(dx, seg_sum(terms, g.s, g.n), g.outdeg[:, None], seg_sum(np.abs(terms), g.s, g.n), inexact, "propagate dx", "dx " + what)
        assert not dx.get()[g.outdeg == 0].any(), what
    else:
        assert dx.untouched(), what
    if with_de and g.E:
        terms = gt * x.r[g.s]
        if ew == 2:
            check_sum(de, terms, 1, np.abs(terms), inexact, "propagate de, a row per edge", "de " + what)
        else:
            ab = np.abs(terms).sum(1, keepdims=True)
            if inexact == "int":
                integer_exact(de, terms.sum(1, keepdims=True), ab, "de " + what)
            else:
                within(de, terms.sum(1, keepdims=True), (d + 1 + 4) * EPS * ab, "propagate de, a scalar per edge", "de " + what)
    else:
        assert de.untouched(), what
    return forms


def emul_values(g, d, e_width, kind, key):
    rng = rng_for("emul", key, d, e_width, kind)
    x, dout = draw(kind, rng, g.n, d), draw(kind, rng, g.n, d)
    return x, draw(kind, rng, g.E, e_width) if e_width else None, dout


def emul_inputs(g, d, e_width, kind, key, mis=()):
    x, e, dout = emul_values(g, d, e_width, kind, key)
    return In(x, "x" in mis), In(e, "e" in mis) if e_width else None, In(dout, "dout" in mis)


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_propagate_emul(d):
    for name, e_width, kind in itertools.product(("A", "B"), (0, 1, d), KINDS):
        g = graph(name)
        x, e, dout = emul_inputs(g, d, e_width, kind, name)
        ew = ew_of(d, e_width)
        for aggr in (SUM, MEAN):
            _, form = emul_fwd(g, d, e_width, aggr, x, e, kind)
            assert form == want_form(d), (name, e_width, aggr)
            for with_dx, with_de in ((True, True), (True, False), (False, True), (False, False)):
                if with_de and e_width == 0:
                    continue                                              # (de without e is refused: test_status_codes)
                forms = emul_bwd(g, d, e_width, aggr, x, e, dout, kind, with_dx, with_de, null_x=not with_de)
                assert forms == [want_form(d)] * ((with_dx or (with_de and ew == 2)) + (with_de and ew == 1)), (name, e_width, aggr)
        assert x.unchanged() and dout.unchanged() and (e is None or e.unchanged())


EMUL_RULE = {  # which misaligned arrays take each launch out of the float4 form: (forward, by-source walk, de's dot kernel)
    0: (("x", "out"), ("dout", "dx"), ()),
    1: (("x", "out"), ("dout", "dx"), ("dout", "x")),
    2: (("x", "out", "e"), ("dout", "dx", "x", "de", "e"), ()),
}


@gpu
@pytest.mark.parametrize("d", MIS_WIDTHS)
def test_propagate_emul_misaligned_pointers(d):
    g = graph("A")
    for e_width, aggr in itertools.product((0, 1, d), (SUM, MEAN)):
        ew = ew_of(d, e_width)
        fwd_rule, walk_rule, dot_rule = EMUL_RULE[ew]
        for m in ("", "x", "e", "out", "dout", "dx", "de"):
            if (m == "e" and not e_width) or (m == "de" and not e_width):
                continue
            mis = (m,) if m else ()
            x, e, dout = emul_inputs(g, d, e_width, "normal", "mis", mis)
            _, form = emul_fwd(g, d, e_width, aggr, x, e, "normal", mis)
            assert form == want_form(d, m in fwd_rule), (e_width, m)
            forms = emul_bwd(g, d, e_width, aggr, x, e, dout, "normal", True, bool(e_width), mis)
            assert forms == [want_form(d, m in walk_rule)] + ([want_form(d, m in dot_rule)] if ew == 1 else []), (e_width, m)


@gpu
def test_propagate_emul_graphs_without_edges():
    for name, d in itertools.product(("edgeless", "one"), (4, 3, 1)):
        g = graph(name)
        for e_width, aggr in itertools.product((0, 1, d), (SUM, MEAN)):
            x, e, dout = emul_inputs(g, d, e_width, "normal", name)
            emul_fwd(g, d, e_width, aggr, None, None, "normal")                                # zeros; x and e are not read
            out = Out(g.n, d)
            ok(_lib.load().ngpde_propagate_emul_forward(g.ptr, d, e_width, aggr, x.ptr, p(e), out.ptr, stream()))
            exact(out, np.zeros((g.n, d)), "out")
            dx, de = Out(g.n, d), Out(4, max(e_width, 1))
            ok(_lib.load().ngpde_propagate_emul_backward(g.ptr, d, e_width, aggr, x.ptr, p(e), dout.ptr, dx.ptr, de.ptr if e_width else None,
                                                         stream()))
            exact(dx, np.zeros((g.n, d)), "dx")
            assert de.untouched()


# ---- 3. ngpde_apply_edges_dot_forward / _backward --------------------------------------------------------------------------------------

def dot_fwd(g, d, xi, xj, kind, mis=()):
    out = Out(g.E, mis="out" in mis)
    form = note("apply_edges_dot_forward", dot_form(d, p(xi), p(xj)))
    ok(_lib.load().ngpde_apply_edges_dot_forward(g.ptr, d, p(xi), p(xj), out.ptr, stream()))
    terms = xi.r[g.t] * xj.r[g.s]                                         # COO order
    what = f"xi_dot_xj d={d} {kind} mis={mis}"
    if kind == "int":
        integer_exact(out, terms.sum(1), np.abs(terms).sum(1), what)
    else:
        within(out, terms.sum(1), (d + 1 + 4) * EPS * np.abs(terms).sum(1), "apply_edges dot", what)
    return form


def dot_bwd(g, d, xi, xj, dout, kind, with_dxi=True, with_dxj=True, mis=(), null_unused=False):
    dxi, dxj = Out(g.n, d, mis="dxi" in mis), Out(g.n, d, mis="dxj" in mis)
    ew = 2 if d == 1 else 1
    xip, xjp = (None if null_unused and not with_dxj else p(xi)), (None if null_unused and not with_dxi else p(xj))
    forms = [note("apply_edges_dot_backward", emul_form(d, ew, node, o.ptr, e=p(dout)))
             for on, node, o in ((with_dxi, xjp, dxi), (with_dxj, xip, dxj)) if on]
    ok(_lib.load().ngpde_apply_edges_dot_backward(g.ptr, d, xip, xjp, p(dout), dxi.ptr if with_dxi else None,
                                                  dxj.ptr if with_dxj else None, stream()))
    what = f"xi_dot_xj pullback d={d} {kind} dxi={with_dxi} dxj={with_dxj} mis={mis}"
    for on, o, other, idx, far, deg, nm in ((with_dxi, dxi, xj, g.t, g.s, g.indeg, "dxi"), (with_dxj, dxj, xi, g.s, g.t, g.outdeg, "dxj")):
        if not on:
            assert o.untouched(), what
            continue
        terms = dout.r[:, None] * other.r[far]
        check_sum(o, seg_sum(terms, idx, g.n), deg[:, None], seg_sum(np.abs(terms), idx, g.n), kind, f"apply_edges dot {nm}", f"{nm} {what}")
        assert not o.get()[deg == 0].any(), what
    return forms


def dot_values(g, d, kind, name):
    rng = rng_for("dot", name, d, kind)
    return draw(kind, rng, g.n, d), draw(kind, rng, g.n, d), draw(kind, rng, g.E)


@gpu
@pytest.mark.parametrize("d", WIDTHS)
def test_apply_edges_dot(d):
    for name, kind in itertools.product(("A", "B"), KINDS):
        g = graph(name)
        xi, xj, dout = (In(v) for v in dot_values(g, d, kind, name))
        for a, b in ((xi, xj), (xi, xi)):                                 # different arrays, and the same one
            assert dot_fwd(g, d, a, b, kind) == want_form(d)
            assert dot_bwd(g, d, a, b, dout, kind) == [want_form(d)] * 2
        assert dot_bwd(g, d, xi, xj, dout, kind, with_dxj=False, null_unused=True) == [want_form(d)]
        assert dot_bwd(g, d, xi, xj, dout, kind, with_dxi=False, null_unused=True) == [want_form(d)]
        assert dot_bwd(g, d, xi, xj, dout, kind, False, False) == []
        assert xi.unchanged() and xj.unchanged() and dout.unchanged()


@gpu
@pytest.mark.parametrize("d", MIS_WIDTHS)
def test_apply_edges_dot_misaligned_pointers(d):
    g = graph("B")
    rng = rng_for("dot mis", d)
    vi, vj, vo = rng.normal(size=(g.n, d)), rng.normal(size=(g.n, d)), rng.normal(size=g.E)
    for m in ("", "xi", "xj", "out", "dout", "dxi", "dxj"):
        mis = (m,) if m else ()
        xi, xj, dout = In(vi, m == "xi"), In(vj, m == "xj"), In(vo, m == "dout")
        assert dot_fwd(g, d, xi, xj, "normal", mis) == want_form(d, m in ("xi", "xj")), m
        assert dot_bwd(g, d, xi, xj, dout, "normal", mis=mis) == [want_form(d, m in ("xj", "dxi")), want_form(d, m in ("xi", "dxj"))], m


@gpu
def test_apply_edges_dot_zero_width_and_no_edges():
    g = graph("A")
    out = Out(g.E)
    ok(_lib.load().ngpde_apply_edges_dot_forward(g.ptr, 0, None, None, out.ptr, stream()))           # d = 0: the empty dot product
    exact(out, np.zeros(g.E), "d = 0")
    dxi, dxj = Out(g.n, 1), Out(g.n, 1)
    ok(_lib.load().ngpde_apply_edges_dot_backward(g.ptr, 0, None, None, None, dxi.ptr, dxj.ptr, stream()))
    assert dxi.untouched() and dxj.untouched()
    for name in ("edgeless", "one"):
        g = graph(name)
        out, x = Out(4), In(np.ones((g.n, 4)))
        ok(_lib.load().ngpde_apply_edges_dot_forward(g.ptr, 4, x.ptr, x.ptr, out.ptr, stream()))
        assert out.untouched()
        dxi, dxj = Out(g.n, 4), Out(g.n, 4)
        ok(_lib.load().ngpde_apply_edges_dot_backward(g.ptr, 4, x.ptr, x.ptr, None, dxi.ptr, dxj.ptr, stream()))
        exact(dxi, np.zeros((g.n, 4)), "dxi")
        exact(dxj, np.zeros((g.n, 4)), "dxj")


# ---- 4. ngpde_softmax_edge_neighbors_forward / _backward -------------------------------------------------------------------------------

def seg_max(x, idx, n):
    out = np.full((n,) + x.shape[1:], -np.inf)
    np.maximum.at(out, idx, x)
    return out


def softmax_ref(g, e, drop=None):
    """float64 softmax of the logits e [E][H] (COO order) over each target's incoming edges; drop: that row's sum loses an entry"""
    z = np.exp(e - seg_max(e, g.t, g.n)[g.t])
    zs, ts = (z, g.t) if drop is None else drop_row(z, g.t, drop)
    return z / seg_sum(zs, ts, g.n)[g.t]


def softmax_fwd(g, h, e, every=True):
    y = Out(g.E, h)
    note("softmax_edge_neighbors_forward", form_of(h, False))
    ok(_lib.load().ngpde_softmax_edge_neighbors_forward(g.ptr, h, e.ptr, y.ptr, stream()))
    ref = softmax_ref(g, e.r)
    rep = ref >= TINY
    assert rep.all() or not every, f"h={h}: {int((~rep).sum())} reference entries below float32's smallest normal"
    got = y.get()
    assert np.isfinite(got).all()
    within(got[rep], ref[rep], 1e-4 * ref[rep], "softmax_edge y", f"softmax h={h}")
    sums = seg_sum(got.astype(np.float64), g.t, g.n)[g.indeg > 0]
    within(sums, np.ones_like(sums), (g.indeg[g.indeg > 0][:, None] + 2) * EPS + 1e-4, "softmax_edge row sums", f"row sums h={h}")
    return y, ref


def softmax_bwd(g, h, yptr, dy):
    de = Out(g.E, h)
    note("softmax_edge_neighbors_backward", form_of(h, False))
    ok(_lib.load().ngpde_softmax_edge_neighbors_backward(g.ptr, h, yptr, dy.ptr, de.ptr, stream()))
    return de


def softmax_logits(g, h, key, scale=3.0):
    """the logits of test_softmax_edge_neighbors: normal draws, and on graph A a row whose logits are all equal"""
    e = rng_for("softmax", key, h).normal(size=(g.E, h)) * scale
    if key == "A":
        e[g.t == IN_DEGREES.index(17)] = 1.25                             # y = 1 / 17
    spread = seg_max(e, g.t, g.n) + seg_max(-e, g.t, g.n)                 # max - min per row and head
    assert spread[g.indeg > 0].max() < 60.0
    return e


def softmax_int_values(g, h, name):
    rng = rng_for("softmax int", name, h)
    return draw("int", rng, g.E, h), draw("int", rng, g.E, h)


@gpu
@pytest.mark.parametrize("h", HEADS)
def test_softmax_edge_neighbors(h):
    for name in ("A", "B"):
        g = graph(name)
        ein = In(softmax_logits(g, h, name))
        y, ref = softmax_fwd(g, h, ein)
        if name == "A":
            within(y.get()[g.t == IN_DEGREES.index(17)], np.full((17, h), 1.0 / 17), 3 * EPS / 17, "softmax_edge equal logits", f"h={h}")
            assert (y.get()[g.t == IN_DEGREES.index(1)] == 1.0).all()     # a single incoming edge
        # the pullback on the kernel's own y (bound: the docstring's derivation)
        dy = In(rng_for("softmax dy", name, h).normal(size=(g.E, h)))
        de = softmax_bwd(g, h, y.ptr, dy)
        k = g.indeg[:, None]
        A, s_ref = seg_sum(np.abs(ref * dy.r), g.t, g.n), seg_sum(ref * dy.r, g.t, g.n)
        Bs = (lin(k, A * (1 + 1e-4)) + 1e-4 * A)[g.t]
        de_ref = ref * (dy.r - s_ref[g.t])
        bound = 1e-4 * np.abs(de_ref) + ref * (1 + 1e-4) * (Bs + 2 * EPS * (np.abs(dy.r) + np.abs(s_ref[g.t]) + Bs))
        within(de, de_ref, bound, "softmax_edge de", f"de {name} h={h}")
        # integer y and dy: the row sum and de are exact
        yi, dyi = (In(v) for v in softmax_int_values(g, h, name))
        s = seg_sum(yi.r * dyi.r, g.t, g.n)
        integer_exact(softmax_bwd(g, h, yi.ptr, dyi), yi.r * (dyi.r - s[g.t]), 2 * (2 + seg_sum(np.abs(yi.r * dyi.r), g.t, g.n)), f"int de h={h}")
        assert ein.unchanged() and dy.unchanged()


@gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_softmax_edge_neighbors_large_logits(name):
    # logits 40 either side of the row's centre: finite, and within the bound wherever float32 can hold the reference at all
    g = graph(name)
    for h in (1, 4, 65):
        rng = rng_for("softmax 40", name, h)
        e = In(rng.choice([-40.0, 40.0], size=(g.E, h)) + rng.normal(size=(g.E, h)))
        y, ref = softmax_fwd(g, h, e, every=False)
        de = softmax_bwd(g, h, y.ptr, In(np.ones((g.E, h))))
        assert np.isfinite(de.get()).all()


@gpu
def test_softmax_edge_neighbors_graphs_without_edges():
    for name in ("edgeless", "one"):
        g = graph(name)
        x, y = In(np.ones((4, 2))), Out(4, 2)
        ok(_lib.load().ngpde_softmax_edge_neighbors_forward(g.ptr, 2, x.ptr, y.ptr, stream()))
        ok(_lib.load().ngpde_softmax_edge_neighbors_backward(g.ptr, 2, x.ptr, x.ptr, y.ptr, stream()))
        assert y.untouched()


# ---- the conditions the references must meet (no GPU) -----------------------------------------------------------------------------------

def test_reference_conditions_hold_for_every_case():
    # the inputs of the GPU tests, rebuilt from their seeds: every integer case keeps sum|term| below 2^24 (so float32 is exact in any
    # order), and every softmax reference entry of test_softmax_edge_neighbors is above float32's smallest normal
    def small(*abs_sums):
        assert all(np.max(a, initial=0.0) < 2.0 ** 24 for a in abs_sums)

    for name in ("A", "B"):
        g = graph(name)
        for d in WIDTHS:
            dxi, dxj = gather_bwd_values(g, d, "int", name)
            small(seg_sum(np.abs(dxi), g.tp, g.n) + seg_sum(np.abs(dxj), g.sp, g.n))
            for e_width in (0, 1, d):
                x, e, dout = emul_values(g, d, e_width, "int", name)
                ev = 1.0 if e is None else e
                small(seg_sum(np.abs(ev * x[g.s]), g.t, g.n), seg_sum(np.abs(ev * dout[g.t]), g.s, g.n),      # out, dx
                      np.abs(dout[g.t] * x[g.s]).sum(1))                                                       # de, either width
            xi, xj, dout = dot_values(g, d, "int", name)
            small(np.abs(xi[g.t] * xj[g.s]).sum(1), np.abs(xi[g.t] * xi[g.s]).sum(1))
            for a in (xi, xj):
                small(seg_sum(np.abs(dout[:, None] * a[g.s]), g.t, g.n), seg_sum(np.abs(dout[:, None] * a[g.t]), g.s, g.n))
        for h in HEADS:
            y, dy = softmax_int_values(g, h, name)
            small(2 * (2 + seg_sum(np.abs(y * dy), g.t, g.n)))
            e = softmax_logits(g, h, name).astype(np.float32).astype(np.float64)
            ref = softmax_ref(g, e)
            assert (ref >= TINY).all() and (name != "A" or np.allclose(ref[g.t == IN_DEGREES.index(17)], 1.0 / 17, rtol=1e-12, atol=0))
    assert 300 * 516 * 4 < 2 ** 24                                           # the longest row, the widest array, the largest product


# ---- 5. status codes -------------------------------------------------------------------------------------------------------------------

@gpu
def test_status_codes():
    # the documented order: a negative width, then a refused aggregation, then a NULL graph; nothing is written by a refused call
    lib, g, d = _lib.load(), graph("A"), 8
    x, e, dout = emul_inputs(g, d, d, "normal", "status")
    outs = [Out(g.n, d), Out(g.E, d), Out(g.E)]
    o_node, o_edge, o_flat = (o.ptr for o in outs)
    MAXA, MUL = _lib.AGGR["max"], _lib.AGGR["mul"]

    def refused(status, code, word):
        msg = lib.ngpde_last_error().decode()
        assert status == code and word in msg, (status, code, msg)
        assert all(o.untouched() for o in outs)

    for bad in (MAXA, MUL, 17):
        refused(lib.ngpde_propagate_emul_forward(None, -1, d, bad, x.ptr, e.ptr, o_node, stream()), _lib.ERR_DIMENSION_MISMATCH, "negative width")
        refused(lib.ngpde_propagate_emul_forward(None, d, d, bad, x.ptr, e.ptr, o_node, stream()), _lib.ERR_INVALID_ARGUMENT, "aggregation")
        refused(lib.ngpde_propagate_emul_backward(None, -1, d, bad, x.ptr, e.ptr, dout.ptr, o_node, o_edge, stream()),
                _lib.ERR_DIMENSION_MISMATCH, "negative width")
        refused(lib.ngpde_propagate_emul_backward(None, d, d, bad, x.ptr, e.ptr, dout.ptr, o_node, o_edge, stream()),
                _lib.ERR_INVALID_ARGUMENT, "aggregation")
    refused(lib.ngpde_propagate_emul_forward(None, d, d, SUM, x.ptr, e.ptr, o_node, stream()), _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    refused(lib.ngpde_propagate_emul_backward(None, d, d, MEAN, x.ptr, e.ptr, dout.ptr, o_node, o_edge, stream()),
            _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    for e_width in (2, d - 1, d + 1, -1):                                 # an e that is neither absent, a scalar nor a row per edge
        refused(lib.ngpde_propagate_emul_forward(g.ptr, d, e_width, SUM, x.ptr, e.ptr, o_node, stream()), _lib.ERR_DIMENSION_MISMATCH, "e has")
        refused(lib.ngpde_propagate_emul_backward(g.ptr, d, e_width, SUM, x.ptr, e.ptr, dout.ptr, o_node, o_edge, stream()),
                _lib.ERR_DIMENSION_MISMATCH, "e has")
    refused(lib.ngpde_propagate_emul_backward(g.ptr, d, 0, SUM, x.ptr, None, dout.ptr, o_node, o_edge, stream()),
            _lib.ERR_INVALID_ARGUMENT, "de without e")
    # gather: the number of arrays, then a negative width, then the graph
    five, w5 = table([x] * 5), int_table([d] * 5)
    o5 = table([outs[1]] * 5)
    refused(lib.ngpde_gather_forward(g.ptr, 5, five, w5, o5, o5, stream()), _lib.ERR_INVALID_ARGUMENT, "arrays")
    refused(lib.ngpde_gather_backward(g.ptr, 5, w5, five, five, table([outs[0]] * 5), stream()), _lib.ERR_INVALID_ARGUMENT, "arrays")
    refused(lib.ngpde_gather_forward(g.ptr, -1, five, w5, o5, o5, stream()), _lib.ERR_INVALID_ARGUMENT, "arrays")
    wneg = int_table([d, -1])
    refused(lib.ngpde_gather_forward(None, 2, five, wneg, o5, o5, stream()), _lib.ERR_DIMENSION_MISMATCH, "negative width")
    refused(lib.ngpde_gather_backward(None, 2, wneg, five, five, table([outs[0]] * 2), stream()), _lib.ERR_DIMENSION_MISMATCH, "negative width")
    refused(lib.ngpde_gather_forward(None, 2, five, w5, o5, o5, stream()), _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    refused(lib.ngpde_gather_backward(None, 2, w5, five, five, table([outs[0]] * 2), stream()), _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    refused(lib.ngpde_gather_forward(g.ptr, 2, None, w5, o5, o5, stream()), _lib.ERR_INVALID_ARGUMENT, "NULL array table")
    # apply_edges and the softmax take no aggregation: a negative width, then the graph
    refused(lib.ngpde_apply_edges_dot_forward(None, -1, x.ptr, x.ptr, o_flat, stream()), _lib.ERR_DIMENSION_MISMATCH, "negative width")
    refused(lib.ngpde_apply_edges_dot_forward(None, d, x.ptr, x.ptr, o_flat, stream()), _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    refused(lib.ngpde_apply_edges_dot_backward(None, -1, x.ptr, x.ptr, dout.ptr, o_node, o_node, stream()), _lib.ERR_DIMENSION_MISMATCH, "negative width")
    refused(lib.ngpde_apply_edges_dot_backward(None, d, x.ptr, x.ptr, dout.ptr, o_node, o_node, stream()), _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    refused(lib.ngpde_softmax_edge_neighbors_forward(None, -1, e.ptr, o_edge, stream()), _lib.ERR_DIMENSION_MISMATCH, "negative width")
    refused(lib.ngpde_softmax_edge_neighbors_forward(None, d, e.ptr, o_edge, stream()), _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    refused(lib.ngpde_softmax_edge_neighbors_backward(None, -1, e.ptr, e.ptr, o_edge, stream()), _lib.ERR_DIMENSION_MISMATCH, "negative width")
    refused(lib.ngpde_softmax_edge_neighbors_backward(None, d, e.ptr, e.ptr, o_edge, stream()), _lib.ERR_INVALID_ARGUMENT, "graph is NULL")
    # NULL operands an entry needs
    refused(lib.ngpde_propagate_emul_forward(g.ptr, d, d, SUM, x.ptr, None, o_node, stream()), _lib.ERR_INVALID_ARGUMENT, "NULL argument")
    refused(lib.ngpde_propagate_emul_backward(g.ptr, d, 1, SUM, None, e.ptr, dout.ptr, o_node, o_edge, stream()), _lib.ERR_INVALID_ARGUMENT, "NULL argument")
    refused(lib.ngpde_apply_edges_dot_backward(g.ptr, d, x.ptr, None, dout.ptr, o_node, None, stream()), _lib.ERR_INVALID_ARGUMENT, "NULL argument")
    refused(lib.ngpde_gather_forward(g.ptr, 1, table([None]), w5, o5, o5, stream()), _lib.ERR_INVALID_ARGUMENT, "is NULL")


# ---- 6. reproducibility ----------------------------------------------------------------------------------------------------------------

@gpu
def test_every_entry_gives_the_same_bits_twice():
    g, d = graph("A"), 68
    x, e, dout = emul_inputs(g, d, d, "normal", "twice")
    w = In(rng_for("twice w").normal(size=(g.E, 1)))
    lib = _lib.load()

    def once():
        outs = [Out(g.n, d), Out(g.n, d), Out(g.E, d), Out(g.E, 1), Out(g.E), Out(g.n, d), Out(g.n, d), Out(g.E, d), Out(g.E, d), Out(g.n, d)]
        ok(lib.ngpde_propagate_emul_forward(g.ptr, d, d, MEAN, x.ptr, e.ptr, outs[0].ptr, stream()))
        ok(lib.ngpde_propagate_emul_backward(g.ptr, d, d, MEAN, x.ptr, e.ptr, dout.ptr, outs[1].ptr, outs[2].ptr, stream()))
        ok(lib.ngpde_propagate_emul_backward(g.ptr, d, 1, SUM, x.ptr, w.ptr, dout.ptr, None, outs[3].ptr, stream()))
        ok(lib.ngpde_apply_edges_dot_forward(g.ptr, d, x.ptr, dout.ptr, outs[4].ptr, stream()))
        ok(lib.ngpde_apply_edges_dot_backward(g.ptr, d, x.ptr, dout.ptr, w.ptr, outs[5].ptr, outs[6].ptr, stream()))
        ok(lib.ngpde_softmax_edge_neighbors_forward(g.ptr, d, e.ptr, outs[7].ptr, stream()))
        ok(lib.ngpde_softmax_edge_neighbors_backward(g.ptr, d, outs[7].ptr, e.ptr, outs[8].ptr, stream()))
        ok(lib.ngpde_gather_backward(g.ptr, 1, int_table([d]), table([e]), table([outs[7]]), table([outs[9]]), stream()))
        return outs

    for k, (a, b) in enumerate(zip(once(), once())):
        same_bits(a, b, f"output {k}")


# ---- 7. what the launches above covered ------------------------------------------------------------------------------------------------

ROW_ENTRIES = ("gather_forward", "gather_backward", "propagate_emul_forward", "propagate_emul_backward", "propagate_emul_backward de",
               "apply_edges_dot_forward", "apply_edges_dot_backward")


@gpu
def test_every_lane_layout_and_row_length_was_launched():
    # the last test of the file, over what the tests before it recorded (run the file as a whole): every entry in both column types at
    # every dpl and at one, two and three column chunks; the softmax at every dpl its heads give; every ladder length by target and
    # by source
    every = {1, 2, 4, 8, 16, 32, 64}
    for entry in ROW_ENTRIES:
        for typ in ("f4", "float"):
            got = {(dpl, chunks) for e, t, dpl, chunks in CASES if e == entry and t == typ}
            floor = every - {1} if (entry, typ) == ("propagate_emul_backward de", "float") else every     # (d = 1 is the EW 2 route)
            assert {dpl for dpl, _ in got} >= floor and {chunks for _, chunks in got} >= {1, 2, 3}, (entry, typ, sorted(got))
        assert (entry, "float", 64, 4) in CASES, entry                    # d = 256 with a pointer 4 bytes in
    for entry in ("softmax_edge_neighbors_forward", "softmax_edge_neighbors_backward"):
        got = {(dpl, chunks) for e, _, dpl, chunks in CASES if e == entry}
        assert got >= {(1, 1), (2, 1), (4, 1), (8, 1), (64, 1), (64, 2), (64, 3)}, (entry, sorted(got))
    a, b = graph("A"), graph("B")
    assert set(IN_DEGREES) <= LENGTHS and set(IN_DEGREES) <= set(a.indeg) and set(IN_DEGREES) <= set(b.outdeg)
