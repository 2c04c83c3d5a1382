"""The message-passing primitives (csrc/mp_kernels.hip behind api_mp.hip) against float64 across their forms.

Every entry is called through the C ABI with raw pointers, so that NULL operands and misaligned pointers reach it.  Per-edge arrays
are in p order (np.argsort(t, kind="stable")): the library's rowptr / col / eid are compared with that restatement before anything
else is (Gr.__init__).  Dispatch, restated below and asserted in every case (vec_form, bias_act_form, colsum_stages):

  ngpde_edge_combine_forward    edge_combine_fwd4_kernel<DPL> iff h % 4 == 0, h <= 256 and P, Q, E, a_out, z_out are each NULL or
                                16-byte aligned; else edge_combine_fwd_kernel (lanes stride the features by 64).
  ngpde_edge_combine_backward   edge_combine_bwd_target4_kernel<DPL> under the same rule over da, z, dz, dP; else
                                edge_combine_bwd_target_kernel.  dQ is always edge_sum_by_source_kernel (8 entries per batch), whatever
                                its alignment.
  ngpde_segment_reduce_forward  segment_sum4_kernel<DPL> for sum / mean under the same rule over M, out; max / min / product and
                                everything else segment_reduce_fwd_kernel.  The pullback is one scalar kernel.
  DPL = dpl_for(h / 4): lanes per entry, 64 / DPL entry slots, four entries in flight per lane.
      h      4  12  16 | 20  32 | 36  64 | 68 100 128 | 132 256 |  1  3  65 130 260 | 64 with any pointer 4 bytes in
      h / 4  1   3   4 |  5   8 |  9  16 | 17  25  32 |  33  64 |
      form   DPL 4     | DPL 8  | DPL 16 | DPL 32     | DPL 64  |  scalar           | scalar
  ngpde_edge_permute, ngpde_gno_contract_forward / _backward, ngpde_activation_forward, ngpde_spectral_weights and the dz part of
  ngpde_bias_act_backward have one form each.
  ngpde_bias_act_forward        bias_act4_kernel iff d % 4 == 0 and a, addend, bias, y, save_z are each NULL or 16-byte aligned
                                (d = 4, 64, 128 aligned); else bias_act1_kernel (d = 7, 65, and every d 4 bytes in).
  ngpde_bias_act_backward       dbias = launch_colsum2: one stage (colsum_kernel, workspace untouched) iff n <= 512, else two
                                (colsum_partial_kernel writes all 128 x d partial sums).  The workspace is checked for exactly that.

Graphs: A has in-degrees 0 1 2 3 4 5 7 8 9 15 16 17 31 32 33 63 64 65 127 128 129 200 (SLOTS, 4 SLOTS and +-1 for every DPL, the
8-batches of the by-source sum) on 37 nodes, sources drawn with replacement from nodes 0 .. 33, COO list shuffled; B is A reversed
(the same row lengths by source); and an edgeless graph of 5 nodes.

References are float64 numpy of the operation itself, compared element by element:
  exact     copies, max / min and their pullbacks, dz of identity / relu / z = NULL, the sum's pullback: the same bits.
  linear    float32 sums of k terms in any order: |out - ref| <= (k + 2) 2^-24 sum|term_i|  (k - 1 roundings of partial sums that
            never exceed sum|term_i|, the mean's division, the cast).  gno dh: cout-term dot products summed over k edges:
            (cout + k + 4) 2^-24 sum|terms|.
  product   relative 2 k 2^-24 for a row of k entries, plus the smallest float32 normal.
  act       anything through a non-linear activation: 1e-5 + 1e-4 |ref|  (per element).  Cotangents of those cases
            are drawn from [-1, 1], so the bound of act' carries over to dz = da act'(z).  Sums of such values (dP, dQ, dbias) add
            the linear bound of the sum to the sum of their terms' bounds.
  spectral  1e-4 |ref| + 1e-5 against the float64 formula at the float64 arguments.
Outputs start as NaN between guard words; arrays an entry must not touch (NULL-gated outputs' neighbours, failed calls, the edgeless
graph) must come back as they were.

Measured on the MI355X, worst err / bound over every case of this file (teardown_module prints the table under `pytest -s`):
  linear    z = P + Q + E 0.39   dP 0.31   dQ 0.31   segment sum 0.29   mean 0.48   mean pullback 0.63   gno m 0.53   dK 0.33
            dh 0.17   bias_act z 0.37   dbias 0.27   (dP / dQ / dbias over act' terms: 0.03 / 0.02 / 0.001)
  product   forward 0.29   pullback 0.32                                spectral weights 0.024
  act       sweep (800 022 points: normal draws at scales 1, 3, 10, the grid on [-30, 30], +-0 .. +-1e4), act | act':
              tanh 0.012 | 0.038   sigmoid 0.001 | 0.009   swish 0.002 | 0.009   gelu 0.031 | 0.197   leakyrelu 0.001 | 0.000
              elu 0.004 | 0.001    softplus 0.006 | 0.001   -- every value finite; identity and relu exact
            through the kernels (edge_combine, bias_act; inputs of order 1), act | act':
              tanh 0.020 | 0.035   sigmoid 0.002 | 0.006   swish 0.006 | 0.003   gelu 0.031 | 0.099   leakyrelu 0.012 | 0.000
              elu 0.013 | 0.001    softplus 0.006 | 0.001
  The worst case is gelu' near z = -5 (2e-6 absolute), as the float32 emulation of the v_exp / v_rcp / v_log forms predicted;
  nothing comes nearer than a fifth of the bound, so device_utils.h's forms stay as they are.
"""
import ctypes as C
import itertools
import math
import zlib

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from oracle import ngpde_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
GUARD = 64                                      # guard floats before and behind every output (256 bytes: keeps the alignment)
SENTINEL = -1234.5
WS_GUARD = 256
ACTS = list(_lib.ACT)
EXACT_DERIV = ("identity", "relu")              # act' in {0, 1}: dz = da act'(z) is exact
AGGRS = ("sum", "mean", "max", "min", "mul")
KCOLSUM_CHUNKS = 128

F4_WIDTHS = {4: 4, 12: 4, 16: 4, 20: 8, 32: 8, 36: 16, 64: 16, 68: 32, 100: 32, 128: 32, 132: 64, 256: 64}
SCALAR_WIDTHS = (1, 3, 65, 130, 260)
WIDTHS = list(F4_WIDTHS) + list(SCALAR_WIDTHS)
ACT_WIDTHS = (16, 32, 64, 128, 256, 65)          # one 16-byte width per DPL, and the scalar form
IN_DEGREES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200]

WORST = {}                                      # family -> worst err / bound seen
WORST_ABS = {}                                  # activation -> largest |err| of (act, act') over the sweep


# ---- the dispatch, restated -----------------------------------------------------------------------------------------------------------

def dpl_for(c4n):
    return 4 if c4n <= 4 else 8 if c4n <= 8 else 16 if c4n <= 16 else 32 if c4n <= 32 else 64


def aligned(*ptrs):
    return all(p is None or p % 16 == 0 for p in ptrs)


def vec_form(h, *ptrs):
    """("f4", DPL) or ("scalar", None) for the three row kernels, from the width and the pointers the dispatch looks at"""
    return ("f4", dpl_for(h // 4)) if h % 4 == 0 and h <= 256 and aligned(*ptrs) else ("scalar", None)


def want_form(h, misaligned=False):
    return ("f4", F4_WIDTHS[h]) if h in F4_WIDTHS and not misaligned else ("scalar", None)


def bias_act_form(d, *ptrs):
    return "f4" if d % 4 == 0 and aligned(*ptrs) else "scalar"


def colsum_stages(n):
    return 1 if n <= 4 * KCOLSUM_CHUNKS else 2


def test_width_table_covers_every_lane_layout():
    # all five DPL values, each at full, partial and just-over-half occupancy; the scalar form below 4, off a multiple of 4, past 256
    assert {w: dpl_for(w // 4) for w in F4_WIDTHS} == F4_WIDTHS
    by_dpl = {d: sorted(w // 4 for w in F4_WIDTHS if F4_WIDTHS[w] == d) for d in (4, 8, 16, 32, 64)}
    for d, c4 in by_dpl.items():
        assert c4[-1] == d and c4[0] < d and (d == 4 or c4[0] == d // 2 + 1), (d, c4)
    assert all(vec_form(h, 0, None, 16) == ("scalar", None) for h in SCALAR_WIDTHS) and 260 % 4 == 0
    assert vec_form(64, 0, 4) == ("scalar", None) and vec_form(64, 0, None) == ("f4", 16)
    for d in (4, 8, 16, 32, 64):                  # rows of SLOTS, 4 SLOTS and +-1 entries for every DPL; the by-source batch of 8
        slots = 64 // d
        assert {slots, 4 * slots, 4 * slots + 1}.issubset(IN_DEGREES) and (4 * slots - 1 in IN_DEGREES or slots == 1)
    assert {7, 8, 9}.issubset(IN_DEGREES)


# ---- graphs -----------------------------------------------------------------------------------------------------------------------------

class _Raw:
    """a device buffer of the library seen through __cuda_array_interface__ (only ever copied to the host)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}


def read_i32(ptr, count):
    if count == 0:
        return np.zeros(0, dtype=np.int32)
    assert ptr
    return torch.as_tensor(_Raw(ptr, 4 * count), device=DEV).cpu().numpy().view(np.int32)


class Gr:
    """a graph, its p order and its by-source order restated, and the library's handle -- whose by-target and by-source lists must
    equal the restatement (attach=False: numpy only, until attach() is called)"""

    def __init__(self, s, t, n, attach=True):
        self.s, self.t, self.n, self.E = np.asarray(s, dtype=np.int64), np.asarray(t, dtype=np.int64), n, len(s)
        self.perm = np.argsort(self.t, kind="stable")           # p -> position in the COO list
        self.sp, self.tp = self.s[self.perm], self.t[self.perm]
        self.perm_s = np.argsort(self.s, kind="stable")         # the same by source
        self.indeg, self.outdeg = np.bincount(self.t, minlength=n), np.bincount(self.s, minlength=n)
        self.rowptr = np.concatenate([[0], np.cumsum(self.indeg)])
        self.rowptr_s = np.concatenate([[0], np.cumsum(self.outdeg)])
        if attach:
            self.attach()

    def attach(self):
        n, lib = self.n, _lib.load()
        self.g = ng.GNNGraph(self.s, self.t, num_nodes=n, index_base=0)
        self.handle = self.g.handle()
        self.ptr = self.handle.ptr
        for fn, rowptr, col, eid in ((lib.ngpde_graph_csr_by_target, self.rowptr, self.sp, self.perm),
                                     (lib.ngpde_graph_csr_by_source, self.rowptr_s, self.t[self.perm_s], self.perm_s)):
            rp, cl, ei = C.c_void_p(), C.c_void_p(), C.c_void_p()
            _lib.check(fn(self.ptr, C.byref(rp), C.byref(cl), C.byref(ei)))
            assert np.array_equal(read_i32(rp.value, n + 1), rowptr), "rowptr"
            assert np.array_equal(read_i32(cl.value, self.E), col), "col"
            assert np.array_equal(read_i32(ei.value, self.E), eid), "eid"


_GRAPHS = {}


def graph(name):
    if name not in _GRAPHS:
        if name == "edgeless":
            z = np.zeros(0, dtype=np.int64)
            _GRAPHS[name] = Gr(z, z, 5)
        else:
            rng = np.random.default_rng(20)
            t = np.repeat(np.arange(len(IN_DEGREES)), IN_DEGREES)
            s = rng.integers(0, 34, t.size)
            k = rng.permutation(t.size)
            s, t = (s[k], t[k]) if name == "A" else (t[k], s[k])
            _GRAPHS[name] = Gr(s, t, 37)
    return _GRAPHS[name]


def teardown_module(module):
    _GRAPHS.clear()
    if WORST:
        print("\nworst err / bound per family:")
        for fam in sorted(WORST):
            print(f"  {fam:34s} {WORST[fam]:.3f}")
        for act, (e, de) in WORST_ABS.items():
            print(f"  largest |err| over the sweep, {act:10s} act {e:.2e}   act' {de:.2e}")


def test_graphs_are_what_the_cases_need():
    a, b, e = graph("A"), graph("B"), graph("edgeless")
    assert a.n == 37 and a.n % 4 != 0 and a.E == sum(IN_DEGREES) == 959
    assert list(a.indeg[:22]) == IN_DEGREES and not a.indeg[22:].any() and list(b.outdeg[:22]) == IN_DEGREES
    assert not a.outdeg[34:].any() and not a.indeg[34:].any() and not b.outdeg[34:].any() and not b.indeg[34:].any()
    assert (a.s == a.t).any() and np.unique(a.s * 37 + a.t).size < a.E                    # self loops, repeated edges
    assert not np.array_equal(a.perm, np.arange(a.E)) and not np.array_equal(b.perm, np.arange(b.E))
    assert (a.outdeg == 0).any() and (b.indeg == 0).any() and b.indeg.max() > 8 and a.outdeg.max() > 8
    assert e.n == 5 and e.E == 0


# ---- buffers ----------------------------------------------------------------------------------------------------------------------------

class In:
    """float32 device copy of `a`, optionally 4 bytes into its allocation; .f the float32 values, .r the same in float64"""

    def __init__(self, a, mis=False):
        self.f = np.ascontiguousarray(a, dtype=np.float32)
        self.r = self.f.astype(np.float64)
        off = 1 if mis else 0
        self.full = torch.zeros(self.f.size + off + 4, device=DEV)
        self.t = self.full[off:off + self.f.size]
        self.t.copy_(torch.from_numpy(self.f.reshape(-1)))
        self.ptr = self.full.data_ptr() + 4 * off
        assert self.ptr % 16 == 4 * off

    def unchanged(self):
        return np.array_equal(self.t.cpu().numpy().view(np.int32), self.f.reshape(-1).view(np.int32))


class Out:
    """NaN-filled device output of `shape` between guard words, optionally 4 bytes into its allocation"""

    def __init__(self, *shape, mis=False):
        self.shape, self.size = shape, int(np.prod(shape))
        self.lo = GUARD + (1 if mis else 0)
        self.full = torch.full((self.lo + self.size + GUARD,), SENTINEL, device=DEV)
        self.full[self.lo:self.lo + self.size] = math.nan
        self.ptr = self.full.data_ptr() + 4 * self.lo
        assert self.ptr % 16 == (4 if mis else 0)

    def get(self):
        """the float32 values, after checking the guards"""
        torch.cuda.synchronize()
        full = self.full.cpu().numpy()
        assert (full[:self.lo] == SENTINEL).all() and (full[self.lo + self.size:] == SENTINEL).all(), "guard words overwritten"
        return full[self.lo:self.lo + self.size].reshape(self.shape)

    def untouched(self):
        return bool(np.isnan(self.get()).all())


class Ws:
    """workspace of exactly `nbytes` (all-ones words: NaN) with canary bytes behind it"""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self.full = torch.full((self.nbytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.full[self.nbytes:] = 0xA5
        self.ptr = self.full.data_ptr()

    def state(self, used=None):
        """"untouched", "written" (the first `used` bytes hold no all-ones word any more) or "partly"; the canary must be intact"""
        torch.cuda.synchronize()
        b = self.full.cpu().numpy()
        assert (b[self.nbytes:] == 0xA5).all(), "wrote past the workspace"
        if (b[:self.nbytes] == 0xFF).all():
            return "untouched"
        used = self.nbytes if used is None else used
        return "written" if not (b[:used - used % 4].view(np.uint32) == 0xFFFFFFFF).any() else "partly"


def p(x):
    return None if x is None else x.ptr


def stream():
    return _lib.current_stream()


def ok(status):
    _lib.check(status)
    torch.cuda.synchronize()


# ---- bounds and comparisons -----------------------------------------------------------------------------------------------------------

def lin(k, abs_sum):
    return (k + 2) * EPS * abs_sum


def nl(ref):
    return 1e-5 + 1e-4 * np.abs(ref)


def sum_of_bounded(k, abs_sum, slack_sum):
    """a float32 sum of k terms, each off by at most its share of slack_sum"""
    return slack_sum + lin(k, abs_sum + slack_sum)


def within(out, ref, bound, fam, what, worst=None):
    """every element within its bound of the float64 ref, non-finite entries the same; records the worst err / bound of `fam` (in
    `worst`: another module's table)"""
    worst = WORST if worst is None else worst
    got = (out.get() if isinstance(out, Out) else np.asarray(out)).astype(np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), ref.shape)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(got[~fin], ref[~fin]), f"{what}: non-finite entries differ"
    err, b = np.abs(got[fin] - ref[fin]), bound[fin]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / b)
    top = float(ratio.max(initial=0.0))
    worst[fam] = max(worst.get(fam, 0.0), top)
    if not top <= 1.0:
        k = int(np.argmax(ratio))
        where = np.argwhere(fin)[k]
        raise AssertionError(f"{what} [{fam}]: {int((ratio > 1).sum())} of {ratio.size} elements out of bound; worst at {tuple(where)}: "
                             f"got {got[fin][k]!r} ref {ref[fin][k]!r} err {err[k]:.3e} bound {b[k]:.3e}")
    return float(err.max(initial=0.0))


def exact(out, ref32, what, bits=False):
    """every element equal to the float32 array ref32 (bits: the very same bits, for copies; otherwise -0 == +0)"""
    got = out.get() if isinstance(out, Out) else np.asarray(out)
    ref32 = np.ascontiguousarray(ref32, dtype=np.float32)
    assert got.shape == ref32.shape, (what, got.shape, ref32.shape)
    same = got.view(np.int32) == ref32.view(np.int32) if bits else got == ref32
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} elements differ, first at {tuple(np.argwhere(~same)[0])}"


def same_bits(a, b, what):
    a, b = (x.get() if isinstance(x, Out) else x for x in (a, b))
    assert np.array_equal(a.view(np.int32), b.view(np.int32)), what


def seg_sum(x, idx, n):
    """float64 sums of the rows of x by segment idx (sorted, then reduceat: the arrays of the forms files reach a million elements)"""
    out = np.zeros((n,) + x.shape[1:], dtype=np.float64)
    counts = np.bincount(idx, minlength=n)
    ne = counts > 0
    if ne.any():
        out[ne] = np.add.reduceat(np.asarray(x, dtype=np.float64)[np.argsort(idx, kind="stable")], (np.cumsum(counts) - counts)[ne], axis=0)
    return out


def rng_for(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


# ---- 1. ngpde_edge_permute ------------------------------------------------------------------------------------------------------------

def permute(g, d, inverse, src):
    dst = Out(g.E, d)
    ok(_lib.load().ngpde_edge_permute(g.ptr, d, int(inverse), p(src), dst.ptr, stream()))
    return dst


@pytest.mark.parametrize("name", ["A", "B"])
def test_edge_permute(name):
    g = graph(name)
    for d in (1, 3, 64, 130):
        rng = rng_for("permute", name, d)
        coo = In(rng.normal(size=(g.E, d)))
        fwd = permute(g, d, False, coo)
        exact(fwd, coo.f[g.perm], f"forward d={d}", bits=True)                      # dst[p] = src[eid[p]]
        por = In(rng.normal(size=(g.E, d)))
        back = np.empty_like(por.f)
        back[g.perm] = por.f                                             # dst[eid[p]] = src[p]
        exact(permute(g, d, True, por), back, f"inverse d={d}", bits=True)
        exact(permute(g, d, True, In(fwd.get())), coo.f, f"inverse o forward d={d}", bits=True)
        assert coo.unchanged() and por.unchanged()


# ---- 2. ngpde_edge_combine_forward ----------------------------------------------------------------------------------------------------

def operands(g, h, key, mis=(), scale=1.0):
    rng = rng_for("operands", key, h)
    return dict(P=In(scale * rng.normal(size=(g.n, h)), "P" in mis), Q=In(scale * rng.normal(size=(g.n, h)), "Q" in mis),
                E=In(scale * rng.normal(size=(max(g.E, 1), h))[:g.E], "E" in mis))


def combine_fwd(g, h, act, P, Q, E, with_z=True, mis=()):
    a, z = Out(g.E, h, mis="a" in mis), Out(g.E, h, mis="z" in mis) if with_z else None
    form = vec_form(h, p(P), p(Q), p(E), a.ptr, p(z))
    ok(_lib.load().ngpde_edge_combine_forward(g.ptr, h, _lib.ACT[act], p(P), p(Q), p(E), a.ptr, p(z), stream()))
    return a, z, form


def combine_ref(g, P, Q, E):
    terms = [x for x in (None if P is None else P.r[g.tp], None if Q is None else Q.r[g.sp], None if E is None else E.r) if x is not None]
    return sum(terms), sum(np.abs(x) for x in terms), len(terms)


@pytest.mark.parametrize("h", WIDTHS)
def test_edge_combine_forward_operand_sets(h):
    # every non-empty subset of {P, Q, E}, with and without z_out; a single operand under the identity is a copy
    for name in ("A", "B"):
        g = graph(name)
        ops = operands(g, h, name)
        for mask, with_z in itertools.product(range(1, 8), (True, False)):
            P, Q, E = (ops[k] if mask >> i & 1 else None for i, k in enumerate("PQE"))
            a, z, form = combine_fwd(g, h, "identity", P, Q, E, with_z)
            what = f"{name} h={h} operands={mask:03b} z_out={with_z}"
            assert form == want_form(h), what
            zr, ab, k = combine_ref(g, P, Q, E)
            for o in (a, z) if with_z else (a,):
                if k == 1:
                    exact(o, zr.astype(np.float32), what, bits=True)
                else:
                    within(o, zr, lin(k, ab), "combine z = P + Q + E", what)
        assert all(x.unchanged() for x in ops.values())


@pytest.mark.parametrize("act", ACTS)
def test_edge_combine_forward_activations(act):
    for h, name in itertools.product(ACT_WIDTHS, ("A", "B")):
        g = graph(name)
        ops = operands(g, h, (name, act))
        a, z, form = combine_fwd(g, h, act, ops["P"], ops["Q"], ops["E"])
        what = f"{name} h={h} {act}"
        assert form == want_form(h), what
        zr, ab, k = combine_ref(g, ops["P"], ops["Q"], ops["E"])
        within(z, zr, lin(k, ab), "combine z = P + Q + E", what)
        if act in EXACT_DERIV:                                           # 1-Lipschitz and exact: z's bound carries over
            within(a, O.act(act, zr), lin(k, ab), "combine z = P + Q + E", what)
        else:
            within(a, O.act(act, zr), nl(O.act(act, zr)), f"through act {act}", what)


COMBINE_FWD_PTRS = ("P", "Q", "E", "a", "z")


def test_edge_combine_forward_misaligned_pointers():
    # h = 64: aligned -> DPL 16; every array 4 bytes in, and each of the five pointers alone -> the scalar form, which adds in the
    # same order: the same bits
    for name in ("A", "B"):
        g = graph(name)
        for act in ("identity", "tanh"):
            ops = operands(g, 64, name)
            a0, z0, form = combine_fwd(g, 64, act, ops["P"], ops["Q"], ops["E"])
            assert form == ("f4", 16)
            zr, ab, k = combine_ref(g, ops["P"], ops["Q"], ops["E"])
            within(z0, zr, lin(k, ab), "combine z = P + Q + E", f"{name} aligned")
            for mis in [COMBINE_FWD_PTRS] + [(m,) for m in COMBINE_FWD_PTRS]:
                o = operands(g, 64, name, mis)
                a, z, form = combine_fwd(g, 64, act, o["P"], o["Q"], o["E"], mis=mis)
                assert form == want_form(64, misaligned=True), mis
                same_bits(z, z0, f"{name} {act} z, misaligned {mis}")
                same_bits(a, a0, f"{name} {act} a, misaligned {mis}")


# ---- 3. ngpde_edge_combine_backward ---------------------------------------------------------------------------------------------------

def combine_bwd(g, h, act, da, z, with_dp=True, with_dq=True, mis=()):
    dz, dP, dQ = Out(g.E, h, mis="dz" in mis), Out(g.n, h, mis="dP" in mis), Out(g.n, h, mis="dQ" in mis)
    form = vec_form(h, p(da), p(z), dz.ptr, dP.ptr if with_dp else None)
    ok(_lib.load().ngpde_edge_combine_backward(g.ptr, h, _lib.ACT[act], p(da), p(z), dz.ptr, dP.ptr if with_dp else None,
                                               dQ.ptr if with_dq else None, stream()))
    assert with_dp or dP.untouched()
    assert with_dq or dQ.untouched()
    return dz, dP if with_dp else None, dQ if with_dq else None, form


def check_combine_bwd(g, act, da, z, dz, dP, dQ, what):
    """dz = da act'(z) (z = NULL: da), dP = its sums by target, dQ = by source"""
    if z is None or act in EXACT_DERIV:
        dz32 = da.f if z is None else da.f * O.dact(act, z.f).astype(np.float32)
        exact(dz, dz32, f"dz {what}", bits=z is None or act == "identity")
        dzr, slack = dz32.astype(np.float64), np.zeros_like(da.r)
        fam = "exact dz"
    else:
        dzr = da.r * O.dact(act, z.r)
        slack = nl(dzr)
        within(dz, dzr, slack, f"through act' {act}", f"dz {what}")
        fam = "act' terms"
    for o, idx, deg, nm in ((dP, g.tp, g.indeg, "dP"), (dQ, g.sp, g.outdeg, "dQ")):
        if o is None:
            continue
        bound = sum_of_bounded(deg[:, None], seg_sum(np.abs(dzr), idx, g.n), seg_sum(slack, idx, g.n))
        within(o, seg_sum(dzr, idx, g.n), bound, f"combine {nm}, {fam}", f"{nm} {what}")
        assert not o.get()[deg == 0].any(), f"{nm} of rows without entries {what}"


@pytest.mark.parametrize("h", WIDTHS)
def test_edge_combine_backward_operand_sets(h):
    # z NULL (identity, whatever act says) and given (relu: dz exact), dP and dQ each NULL and given
    for name in ("A", "B"):
        g = graph(name)
        rng = rng_for("combine bwd", name, h)
        da, z = In(rng.normal(size=(g.E, h))), In(rng.normal(size=(g.E, h)))
        for zz, with_dp, with_dq in itertools.product((None, z), (True, False), (True, False)):
            act = "tanh" if zz is None else "relu"
            dz, dP, dQ, form = combine_bwd(g, h, act, da, zz, with_dp, with_dq)
            what = f"{name} h={h} z={'given' if zz is not None else 'NULL'} dP={with_dp} dQ={with_dq}"
            assert form == want_form(h), what
            check_combine_bwd(g, act, da, zz, dz, dP, dQ, what)
        assert da.unchanged() and z.unchanged()


@pytest.mark.parametrize("act", ACTS)
def test_edge_combine_backward_activations(act):
    for h, name in itertools.product(ACT_WIDTHS, ("A", "B")):
        g = graph(name)
        rng = rng_for("combine bwd act", name, h, act)
        da, z = In(rng.uniform(-1, 1, size=(g.E, h))), In(rng.normal(size=(g.E, h)))
        dz, dP, dQ, form = combine_bwd(g, h, act, da, z)
        assert form == want_form(h)
        check_combine_bwd(g, act, da, z, dz, dP, dQ, f"{name} h={h} {act}")


def test_edge_combine_backward_misaligned_pointers():
    # h = 64: da, z, dz, dP each alone and all together 4 bytes in -> the scalar form; dQ is not part of the rule
    for name in ("A", "B"):
        g = graph(name)
        rng = rng_for("combine bwd mis", name)
        vals_da, vals_z = rng.uniform(-1, 1, size=(g.E, 64)), rng.normal(size=(g.E, 64))
        for act in ("relu", "swish"):
            for mis in [(), ("da", "z", "dz", "dP", "dQ"), ("da",), ("z",), ("dz",), ("dP",), ("dQ",)]:
                da, z = In(vals_da, "da" in mis), In(vals_z, "z" in mis)
                dz, dP, dQ, form = combine_bwd(g, 64, act, da, z, mis=mis)
                assert form == (("f4", 16) if mis in ((), ("dQ",)) else ("scalar", None)), mis
                check_combine_bwd(g, act, da, z, dz, dP, dQ, f"{name} {act} misaligned {mis}")


# ---- 4. ngpde_segment_reduce_forward / _backward ---------------------------------------------------------------------------------------

def draw_messages(g, h, aggr, rng):
    if aggr in ("max", "min"):
        return rng.integers(-1, 3, size=(g.E, h)).astype(np.float64)     # deliberate ties
    if aggr == "mul":
        m = rng.uniform(0.9, 1.1, size=(g.E, h))
        rows = np.flatnonzero(g.indeg >= 3)[:2]
        assert rows.size == 2
        m[g.rowptr[rows[0]]] = 0.0                                        # a row holding a single zero
        m[g.rowptr[rows[1]]:g.rowptr[rows[1]] + 2] = 0.0                  # and one holding two
        return m
    return rng.normal(size=(g.E, h))


def reduce_fwd(g, d, aggr, M, mis=()):
    out = Out(g.n, d, mis="out" in mis)
    form = vec_form(d, p(M), out.ptr) if aggr in ("sum", "mean") else ("scalar", None)
    ok(_lib.load().ngpde_segment_reduce_forward(g.ptr, d, _lib.AGGR[aggr], p(M), out.ptr, stream()))
    return out, form


def reduce_bwd(g, d, aggr, M, out, dout):
    dM = Out(g.E, d)
    ok(_lib.load().ngpde_segment_reduce_backward(g.ptr, d, _lib.AGGR[aggr], p(M), p(out), p(dout), dM.ptr, stream()))
    return dM


EMPTY_ROW = dict(sum=0.0, mean=0.0, max=-np.inf, min=np.inf, mul=1.0)


def check_reduce_fwd(g, aggr, M, out, what):
    ref = O.scatter(aggr, M.r.T, g.tp, g.n).T
    deg = g.indeg[:, None]
    if aggr in ("max", "min"):
        exact(out, ref.astype(np.float32), what)
    elif aggr == "mul":
        within(out, ref, 2 * deg * EPS * np.abs(ref) + TINY, "segment product", what)
    else:
        ab = seg_sum(np.abs(M.r), g.tp, g.n)
        within(out, ref, lin(deg, ab) / (np.maximum(deg, 1) if aggr == "mean" else 1), f"segment {aggr}", what)
    got = out.get()[g.indeg == 0]
    assert got.size and (got == EMPTY_ROW[aggr]).all(), f"empty rows {what}"
    return ref


def check_reduce_bwd(g, aggr, M, ref_out, dout, dM, what):
    ref = O.scatter_pullback(aggr, M.r.T, g.tp, g.n, ref_out.T, dout.r.T).T
    deg = g.indeg[g.tp][:, None]
    if aggr in ("sum", "max", "min"):
        exact(dM, ref.astype(np.float32), what)
    elif aggr == "mean":
        within(dM, ref, lin(1, np.abs(ref)), "segment mean pullback", what)
    else:
        within(dM, ref, 2 * deg * EPS * np.abs(ref) + TINY, "segment product pullback", what)
        assert np.isfinite(dM.get()).all()


@pytest.mark.parametrize("h", WIDTHS)
def test_segment_reduce(h):
    for name, aggr in itertools.product(("A", "B"), AGGRS):
        g = graph(name)
        rng = rng_for("segment", name, h, aggr)
        M, dout = In(draw_messages(g, h, aggr, rng)), In(rng.normal(size=(g.n, h)))
        what = f"{name} h={h} {aggr}"
        out, form = reduce_fwd(g, h, aggr, M)
        assert form == (want_form(h) if aggr in ("sum", "mean") else ("scalar", None)), what
        ref = check_reduce_fwd(g, aggr, M, out, what)
        with np.errstate(invalid="ignore"):
            ref_in = In(ref)                                              # the float64 result, rounded: exact for max / min
        dM = reduce_bwd(g, h, aggr, M, ref_in, dout)
        check_reduce_bwd(g, aggr, M, ref, dout, dM, "pullback " + what)
        assert M.unchanged() and dout.unchanged()


def test_segment_reduce_product_rows_with_zeros():
    # one zero: that entry's gradient is the product of the others, the others' is 0; two zeros: all 0 -- finite, no division
    g = graph("A")
    rng = rng_for("zeros")
    m = draw_messages(g, 3, "mul", rng)
    rows = np.flatnonzero(g.indeg >= 3)[:2]
    M, dout = In(m), In(np.ones((g.n, 3)))
    out, _ = reduce_fwd(g, 3, "mul", M)
    assert not out.get()[rows].any()
    dM = reduce_bwd(g, 3, "mul", M, In(out.get()), dout).get()
    r0, r1 = (slice(g.rowptr[r], g.rowptr[r + 1]) for r in rows)
    assert (dM[r0][0] > 0.5).all() and not dM[r0][1:].any() and not dM[r1].any()
    others = np.prod(M.r[r0][1:], axis=0)
    within(dM[r0][0], others, 2 * g.indeg[rows[0]] * EPS * others + TINY, "segment product pullback", "the single zero's gradient")


def test_segment_reduce_misaligned_pointers():
    for name, aggr in itertools.product(("A", "B"), ("sum", "mean")):
        g = graph(name)
        vals = rng_for("segment mis", name).normal(size=(g.E, 64))
        for mis in [(), ("M", "out"), ("M",), ("out",)]:
            M = In(vals, "M" in mis)
            out, form = reduce_fwd(g, 64, aggr, M, mis)
            assert form == want_form(64, misaligned=bool(mis)), mis
            check_reduce_fwd(g, aggr, M, out, f"{name} {aggr} misaligned {mis}")


# ---- 5. ngpde_gno_contract_forward / _backward ----------------------------------------------------------------------------------------

def gno_fwd(g, cin, cout, K, hf):
    m = Out(g.E, cout)
    ok(_lib.load().ngpde_gno_contract_forward(g.ptr, cin, cout, p(K), p(hf), m.ptr, stream()))
    return m


def gno_bwd(g, cin, cout, K, hf, dm, with_dk=True, with_dh=True, short=0, expect=_lib.OK):
    dK, dh = Out(g.E, cin * cout), Out(g.n, cin)
    ws = Ws(g.E * cin * 4 - short)
    st = _lib.load().ngpde_gno_contract_backward(g.ptr, cin, cout, p(K), p(hf), p(dm), dK.ptr if with_dk else None,
                                                 dh.ptr if with_dh else None, ws.ptr, ws.nbytes, stream())
    torch.cuda.synchronize()
    assert st == expect, (st, _lib.load().ngpde_last_error())
    assert ws.state() in (("written",) if with_dh and st == _lib.OK and g.E else ("untouched",))
    return dK, dh


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("cin", [1, 3, 16])
def test_gno_contract(cin, name):
    g = graph(name)
    for cout in (1, 63, 64, 65, 130):
        rng = rng_for("gno", name, cin, cout)
        K, hf, dm = In(rng.normal(size=(g.E, cin * cout))), In(rng.normal(size=(g.n, cin))), In(rng.normal(size=(g.E, cout)))
        what = f"{name} cin={cin} cout={cout}"
        K3, hs = K.r.reshape(g.E, cin, cout), hf.r[g.sp]                  # K_p[o + cout i]
        within(gno_fwd(g, cin, cout, K, hf), np.einsum("pio,pi->po", K3, hs), lin(cin, np.einsum("pio,pi->po", np.abs(K3), np.abs(hs))),
               "gno m", "m " + what)
        dK, dh = gno_bwd(g, cin, cout, K, hf, dm)
        dKr = (hs[:, :, None] * dm.r[:, None, :]).reshape(g.E, cin * cout)
        within(dK, dKr, lin(1, np.abs(dKr)), "gno dK", "dK " + what)
        per_edge, per_edge_abs = np.einsum("pio,po->pi", K3, dm.r), np.einsum("pio,po->pi", np.abs(K3), np.abs(dm.r))
        bound = (cout + g.outdeg[:, None] + 4) * EPS * seg_sum(per_edge_abs, g.sp, g.n)
        within(dh, seg_sum(per_edge, g.sp, g.n), bound, "gno dh", "dh " + what)
        assert not dh.get()[g.outdeg == 0].any()
        # dk and dh are each nullable: the other one keeps its bits, the absent one is not written
        dK1, dh1 = gno_bwd(g, cin, cout, K, hf, dm, with_dh=False)
        same_bits(dK1, dK, "dK with dh = NULL " + what)
        assert dh1.untouched()
        dK2, dh2 = gno_bwd(g, cin, cout, K, hf, dm, with_dk=False)
        same_bits(dh2, dh, "dh with dk = NULL " + what)
        assert dK2.untouched()
        # a workspace one byte short: NGPDE_ERR_WORKSPACE, nothing written
        dK3, dh3 = gno_bwd(g, cin, cout, K, hf, dm, short=1, expect=_lib.ERR_WORKSPACE)
        assert dK3.untouched() and dh3.untouched()
        assert K.unchanged() and hf.unchanged() and dm.unchanged()


# ---- the edgeless graph ---------------------------------------------------------------------------------------------------------------

def test_edgeless_graph():
    g, lib, h = graph("edgeless"), _lib.load(), 8
    x, node = In(np.ones((4, h))), In(np.ones((g.n, h)))
    # edge_permute, edge_combine_forward, gno_contract_forward, segment_reduce_backward: OK, nothing written
    o = Out(4, h)
    ok(lib.ngpde_edge_permute(g.ptr, h, 0, x.ptr, o.ptr, stream()))
    ok(lib.ngpde_edge_permute(g.ptr, h, 1, x.ptr, o.ptr, stream()))
    ok(lib.ngpde_edge_combine_forward(g.ptr, h, _lib.ACT["tanh"], node.ptr, node.ptr, x.ptr, o.ptr, o.ptr, stream()))
    ok(lib.ngpde_gno_contract_forward(g.ptr, 2, 4, x.ptr, node.ptr, o.ptr, stream()))
    ok(lib.ngpde_segment_reduce_backward(g.ptr, h, _lib.AGGR["sum"], x.ptr, node.ptr, node.ptr, o.ptr, stream()))
    assert o.untouched()
    # edge_combine_backward: dP = dQ = 0 over the 5 nodes, per-edge pointers NULL
    for hh in (8, 7):
        dP, dQ = Out(g.n, hh), Out(g.n, hh)
        ok(lib.ngpde_edge_combine_backward(g.ptr, hh, _lib.ACT["tanh"], None, None, None, dP.ptr, dQ.ptr, stream()))
        exact(dP, np.zeros((g.n, hh)), "dP")
        exact(dQ, np.zeros((g.n, hh)), "dQ")
        for aggr in AGGRS:                                                # segment_reduce_forward with m = NULL: the neutral elements
            out = Out(g.n, hh)
            ok(lib.ngpde_segment_reduce_forward(g.ptr, hh, _lib.AGGR[aggr], None, out.ptr, stream()))
            exact(out, np.full((g.n, hh), EMPTY_ROW[aggr]), aggr)
    # gno_contract_backward with dh given: zeros, dk untouched, no workspace needed
    dK, dh = Out(4, 8), Out(g.n, 2)
    ok(lib.ngpde_gno_contract_backward(g.ptr, 2, 4, None, None, None, dK.ptr, dh.ptr, None, 0, stream()))
    exact(dh, np.zeros((g.n, 2)), "dh")
    assert dK.untouched()


# ---- 6. bias_act and the activations ---------------------------------------------------------------------------------------------------

def bias_act_fwd(n, d, act, a, addend, bias, with_z, mis=False):
    y, z = Out(n, d, mis=mis), Out(n, d, mis=mis) if with_z else None
    form = bias_act_form(d, p(a), p(addend), p(bias), y.ptr, p(z))
    ok(_lib.load().ngpde_bias_act_forward(n, d, _lib.ACT[act], p(a), p(addend), p(bias), y.ptr, p(z), stream()))
    return y, z, form


@pytest.mark.parametrize("mis", [False, True])
@pytest.mark.parametrize("d", [4, 64, 128, 7, 65])
def test_bias_act_forward(d, mis):
    n = 37
    rng = rng_for("bias_act", d, mis)
    a, addend, bias = In(rng.normal(size=(n, d)), mis), In(rng.normal(size=(n, d)), mis), In(rng.normal(size=d), mis)
    for mask, act in itertools.product(range(8), ACTS):
        ad, bi, with_z = addend if mask & 1 else None, bias if mask & 2 else None, bool(mask & 4)
        y, z, form = bias_act_fwd(n, d, act, a, ad, bi, with_z, mis)
        what = f"d={d} misaligned={mis} addend={ad is not None} bias={bi is not None} save_z={with_z} {act}"
        assert form == ("f4" if d % 4 == 0 and not mis else "scalar"), what
        terms = [a.r] + ([ad.r] if ad else []) + ([np.broadcast_to(bi.r, (n, d))] if bi else [])
        zr, bound = sum(terms), lin(len(terms), sum(np.abs(x) for x in terms))
        if with_z and len(terms) == 1:
            exact(z, zr, what, bits=True)
        elif with_z:
            within(z, zr, bound, "bias_act z", what)
        if act in EXACT_DERIV:
            within(y, O.act(act, zr), bound, "bias_act z", what)
        else:
            within(y, O.act(act, zr), nl(O.act(act, zr)), f"through act {act}", what)
    assert a.unchanged() and addend.unchanged() and bias.unchanged()


def bias_act_bwd(n, d, act, dy, z, with_db=True, ws_bytes=None, dz_alias=None, expect=_lib.OK):
    lib = _lib.load()
    dz, db = Out(max(n, 1), d), Out(d)
    need = lib.ngpde_bias_act_workspace_bytes(d)
    assert need == KCOLSUM_CHUNKS * d * 4
    ws = Ws(need if ws_bytes is None else ws_bytes)
    dzp = dz_alias.ptr if dz_alias is not None else dz.ptr if n else None
    st = lib.ngpde_bias_act_backward(n, d, _lib.ACT[act], p(dy), p(z), dzp, db.ptr if with_db else None,
                                     ws.ptr if ws.nbytes else None, ws.nbytes, stream())
    torch.cuda.synchronize()
    assert st == expect, (st, lib.ngpde_last_error())
    return dz, db, ws


def test_bias_act_backward_activations():
    n, d = 37, 65
    for act in ACTS:
        rng = rng_for("bias_act bwd", act)
        dy, z = In(rng.uniform(-1, 1, size=(n, d))), In(rng.normal(size=(n, d)))
        dz, db, ws = bias_act_bwd(n, d, act, dy, z)
        assert colsum_stages(n) == 1 and ws.state() == "untouched"
        if act in EXACT_DERIV:
            dz32 = dy.f * O.dact(act, z.f).astype(np.float32)
            exact(dz, dz32, act)
            dzr, slack, fam = dz32.astype(np.float64), np.zeros((n, d)), "exact dz"
        else:
            dzr = dy.r * O.dact(act, z.r)
            slack, fam = nl(dzr), "act' terms"
            within(dz, dzr, slack, f"through act' {act}", act)
        within(db, dzr.sum(0), sum_of_bounded(n, np.abs(dzr).sum(0), slack.sum(0)), f"dbias, {fam}", f"dbias {act}")
        dz2, db2, _ = bias_act_bwd(n, d, act, dy, z, with_db=False, ws_bytes=0)     # dbias = NULL needs no workspace
        same_bits(dz2, dz, act)
        assert db2.untouched()


@pytest.mark.parametrize("d", [1, 63, 64, 65, 130])
def test_bias_act_backward_column_sums(d):
    # one stage up to 512 rows (the workspace stays as it was), two above (all 128 x d partial sums written); n = 0 gives zeros
    for n in (0, 1, 3, 4, 5, 512, 513, 1000, 2051):
        rng = rng_for("dbias", n, d)
        dy = In(rng.normal(size=(n, d))) if n else None
        dz, db, ws = bias_act_bwd(n, d, "identity", dy, None)
        assert ws.state() == ("untouched" if colsum_stages(n) == 1 else "written"), (n, d, ws.state())
        if n == 0:
            exact(db, np.zeros(d), f"n=0 d={d}")
            assert dz.untouched()
            continue
        exact(dz, dy.f, f"dz n={n} d={d}", bits=True)
        within(db, dy.r.sum(0), lin(n, np.abs(dy.r).sum(0)), "dbias, exact dz", f"dbias n={n} d={d}")
        assert dy.unchanged()


@pytest.mark.parametrize("n,d", [(5, 64), (513, 65)])
def test_bias_act_backward_identity_in_place(n, d):
    # dz aliasing dy under the identity: nothing to compute, dbias from the array as it is
    vals = rng_for("alias", n, d).normal(size=(n, d))
    both = Out(n, d)
    both.full[both.lo:both.lo + both.size] = torch.as_tensor(vals.astype(np.float32).reshape(-1), device=DEV)
    dz, db, ws = bias_act_bwd(n, d, "identity", both, None, dz_alias=both)
    exact(both, vals.astype(np.float32), "dy = dz", bits=True)
    assert dz.untouched() and ws.state() == ("untouched" if colsum_stages(n) == 1 else "written")
    r = vals.astype(np.float32).astype(np.float64)
    within(db, r.sum(0), lin(n, np.abs(r).sum(0)), "dbias, exact dz", f"in place n={n}")


def test_bias_act_backward_needs_its_workspace():
    n, d = 600, 64
    dy, z = In(np.ones((n, d))), In(np.ones((n, d)))
    need = _lib.load().ngpde_bias_act_workspace_bytes(d)
    for nbytes in (0, need - 1):
        dz, db, ws = bias_act_bwd(n, d, "tanh", dy, z, ws_bytes=nbytes, expect=_lib.ERR_WORKSPACE)
        assert dz.untouched() and db.untouched() and ws.state() == "untouched"


def sweep():
    """200 000 normal draws at three scales, a 200 001-point grid on [-30, 30], and the edges of the exp2 / rcp / log2 forms"""
    rng = np.random.default_rng(8)
    special = [0.0, 1e-6, 1e-3, 20.0, 44.0, 88.0, 89.0, 100.0, 1e3, 1e4]
    parts = [rng.normal(size=200000) * s for s in (1.0, 3.0, 10.0)] + [np.linspace(-30.0, 30.0, 200001),
                                                                      np.array(special + [-v for v in special] + [20.000002])]
    return np.concatenate(parts).astype(np.float32)


_SWEEP = []


def sweep_in():
    if not _SWEEP:
        _SWEEP.append(In(sweep()))
    return _SWEEP[0]


@pytest.mark.parametrize("act", ACTS)
def test_activation_sweep(act):
    # act through ngpde_activation_forward, act' through ngpde_bias_act_backward with dy = 1: finite, and within the parity bound
    z = sweep_in()
    n = z.f.size
    a = Out(n)
    ok(_lib.load().ngpde_activation_forward(n, _lib.ACT[act], z.ptr, a.ptr, stream()))
    ones = In(np.ones(n))
    dz, _, _ = bias_act_bwd(n, 1, act, ones, z, with_db=False, ws_bytes=0)
    with np.errstate(all="ignore"):
        ar, dr = O.act(act, z.r), O.dact(act, z.r)
    assert np.isfinite(ar).all() and np.isfinite(dr).all()
    if act in EXACT_DERIV:
        assert np.array_equal(a.get(), ar.astype(np.float32)) and np.array_equal(dz.get().reshape(-1), dr.astype(np.float32))
    else:
        WORST_ABS[act] = (within(a, ar, nl(ar), f"sweep act {act}", f"{act}"),
                          within(dz.get().reshape(-1), dr, nl(dr), f"sweep act' {act}", f"{act}'"))
    assert z.unchanged()


# ---- 7. ngpde_spectral_weights ---------------------------------------------------------------------------------------------------------

def spectral(n, e):
    w = Out(e.f.size)
    ok(_lib.load().ngpde_spectral_weights(e.f.size, n, e.ptr, w.ptr, stream()))
    return w


@pytest.mark.parametrize("n", [8, 100, 101])
def test_spectral_weights(n):
    # the layer's own arguments: e = x_t - x_s on the n-point grid, rounded to float32 for the device
    e64 = O.spectral_graph(n).edata["e"].reshape(-1)
    ref = np.cos(e64 * n / 2) / np.tan(e64 / 2) / 2
    within(spectral(n, In(e64)), ref, 1e-4 * np.abs(ref) + 1e-5, "spectral weights", f"n={n}")


# ---- 8. reproducibility ------------------------------------------------------------------------------------------------------------------

def test_every_entry_gives_the_same_bits_twice():
    g, h, lib = graph("A"), 68, _lib.load()
    rng = rng_for("twice")
    ops = operands(g, h, "twice")
    da, z, dout = In(rng.normal(size=(g.E, h))), In(rng.normal(size=(g.E, h))), In(rng.normal(size=(g.n, h)))
    K, hf, dm = In(rng.normal(size=(g.E, 3 * h))), In(rng.normal(size=(g.n, 3))), In(rng.normal(size=(g.E, h)))
    rows, bias = In(rng.normal(size=(1000, h))), In(rng.normal(size=h))
    e = In(O.spectral_graph(8).edata["e"].reshape(-1))

    def once():
        outs = [permute(g, h, False, z), permute(g, h, True, z)]
        outs += combine_fwd(g, h, "tanh", ops["P"], ops["Q"], ops["E"])[:2]
        outs += combine_bwd(g, h, "tanh", da, z)[:3]
        for aggr in AGGRS:
            M = In(draw_messages(g, h, aggr, rng_for("twice", aggr)))
            out, _ = reduce_fwd(g, h, aggr, M)
            outs += [out, reduce_bwd(g, h, aggr, M, In(out.get()), dout)]
        outs += [gno_fwd(g, 3, h, K, hf)] + list(gno_bwd(g, 3, h, K, hf, dm))
        outs += bias_act_fwd(1000, h, "gelu", rows, rows, bias, True)[:2]
        outs += bias_act_bwd(1000, h, "gelu", rows, rows)[:2]
        a = Out(1000, h)
        ok(lib.ngpde_activation_forward(1000 * h, _lib.ACT["softplus"], rows.ptr, a.ptr, stream()))
        return outs + [a, spectral(8, e)]

    first, second = once(), once()
    assert len(first) == len(second) == 26
    for k, (x, y) in enumerate(zip(first, second)):
        with np.errstate(invalid="ignore"):
            same_bits(x, y, f"output {k}")
