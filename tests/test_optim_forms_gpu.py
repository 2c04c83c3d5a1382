"""The flat-vector kernels of csrc/optim.hip across their launch envelope: ngpde_adam_step, ngpde_rprop_step, ngpde_accumulate_many
and -- past their grid caps and with `out` aliasing a term -- ngpde_rk_stage_combine, ngpde_rk_dense_output and its pullback.

The C entries are called directly.  Every output and every in-place array is a window of a larger allocation with 64 sentinel floats
on both sides (Window); the bytes outside the window and every read-only input must keep their bits.  The references and the derived
bounds are test_flat_kernel_bounds.py's, where each bound is shown sufficient without a GPU: Adam and the combination against float64
under a counted bound, Rprop and acc += g bit for bit against the numpy float32 restatement, the dense-output kernels bit for bit
against the chained combinations they restate."""
import ctypes as C

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from ngpde_amd import node as NODE
from test_flat_kernel_bounds import (ADAM_BETAS, ADAM_EDGE, N_SCRIPTS, RPROP, D, F, accumulate_f32, adam_consts, adam_plant_edges,
                                     adam_ref, adam_state, bits, combine_ref, ratio, rprop_gradients, rprop_trace)
from test_node_adaptive_gpu import offset_tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -842150451            # 0xCDCDCDCD: as a float, -4.3e8
GUARD = 64                       # floats on either side of a window (256 bytes: the window keeps the alignment `off` gives it)


class Window:
    """n floats inside a larger allocation, `off` floats past a 256-byte boundary, GUARD sentinel floats before and after.  Starts
    from `data`, or from the sentinel (an output: an element the kernel does not write shows)."""

    def __init__(self, data=None, n=None, off=0):
        if data is not None:
            data = np.ascontiguousarray(data, dtype=F).reshape(-1)
            n = data.size
        self.n, self.lo = n, GUARD + off
        self.raw = torch.full((self.lo + n + GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
        self.i = self.raw[self.lo:self.lo + n]
        self.t = self.i.view(torch.float32)
        if data is not None:
            self.t.copy_(torch.from_numpy(data))
        assert (self.ptr - 4 * off) % 256 == 0 and self.ptr % 4 == 0

    @property
    def ptr(self):
        return self.raw.data_ptr() + 4 * self.lo

    def bits(self):
        return self.i.cpu().numpy()

    def host(self):
        return self.t.cpu().numpy()

    def guards_intact(self):
        return bool((self.raw[:self.lo] == SENTINEL).all()) and bool((self.raw[self.lo + self.n:] == SENTINEL).all())

    def untouched(self):
        """an output window nothing was written to"""
        return self.guards_intact() and bool((self.i == SENTINEL).all())


GEN = torch.Generator().manual_seed(0)


def readonly(data, off=0):
    """a read-only input at `off` floats past a 256-byte boundary, and the snapshot of its bits"""
    data = np.ascontiguousarray(data, dtype=F).reshape(-1)
    t = offset_tensor(data.size, off, GEN)
    t.copy_(torch.from_numpy(data))
    return t, t.view(torch.int32).clone()


def unchanged(pair):
    t, snap = pair
    return torch.equal(t.view(torch.int32), snap)


def lib():
    return _lib.load()


def sync():
    torch.cuda.synchronize()


def offsets(n):
    """aligned; and, where the size would allow 16-byte accesses, every pointer one float past a 16-byte boundary"""
    return (0, 1) if n % 4 == 0 else (0,)


def same_bits(window, expect):
    return np.array_equal(window.bits(), bits(expect).reshape(-1))


# ---- Adam ------------------------------------------------------------------------------------------------------------------------

ADAM_N = [1, 255, 256, 257, 2048 * 256 + 3]       # the last: past the grid cap of 2048 x 256 threads, the loop's second trip
EPS = 1e-8


def adam_call(n, x, g, m, v, eta, b1, b2, step, gs, eps=EPS):
    return lib().ngpde_adam_step(n, x, g, m, v, eta, b1, b2, eps, step, gs, _lib.current_stream())


def adam_device(state, off, eta, b1, b2, step, gs):
    """one step on the device from the float32 state: (x, m, v) as numpy, guards and the gradient checked"""
    x, g, m, v = state
    X, M, V, G = Window(x, off=off), Window(m, off=off), Window(v, off=off), readonly(g, off)
    _lib.check(adam_call(x.size, X.ptr, G[0].data_ptr(), M.ptr, V.ptr, eta, b1, b2, step, gs))
    sync()
    assert X.guards_intact() and M.guards_intact() and V.guards_intact() and unchanged(G)
    return X.host(), M.host(), V.host()


@pytest.mark.parametrize("betas", range(len(ADAM_BETAS)), ids=["0.5-0.75", "0-0.5", "0.9-0.999"])
@pytest.mark.parametrize("n", ADAM_N)
def test_adam_one_step_against_float64(n, betas):
    (b1, b2), dc = ADAM_BETAS[betas]
    rng = np.random.default_rng(1000 * betas + n % 1000)
    worst = 0.0
    for off in offsets(n):
        for step, gs in ((1, 1.0), (2, 1.0 / 3.0), (12 if dc == 0.0 else 100, 1.0), (7, 1.0 / 3.0)):
            state = adam_state(rng, n)
            eta = float(10.0 ** rng.uniform(-4, -1))
            got = adam_device(state, off, eta, b1, b2, step, gs)
            # the defaults' c1, c2 carry the rounding of the float power: 2^-23 absolute each (ADAM_BETAS), through 1 / c1, 1 / sqrt(c2)
            ref, bnd = adam_ref(*state, eta, b1, b2, EPS, step, gs, dc, dc)
            for name, a, r, b in zip("xmv", got, ref, bnd):
                rt = ratio(a, r, b)
                worst = max(worst, rt)
                assert rt <= 1.0, (name, off, step, gs, rt)
    print("adam: worst |device - float64| / bound", n, (b1, b2), worst)


@pytest.mark.parametrize("n", ADAM_N)
def test_adam_grad_scale_is_the_premultiplied_gradient_bit_for_bit(n):
    rng = np.random.default_rng(n)
    for off in offsets(n):
        x, g, m, v = adam_state(rng, n)
        a = adam_device((x, g, m, v), off, 0.01, 0.9, 0.999, 3, 0.25)
        b = adam_device((x, F(0.25) * g, m, v), off, 0.01, 0.9, 0.999, 3, 1.0)
        for p, q in zip(a, b):
            assert np.array_equal(bits(p), bits(q))
        assert not np.array_equal(bits(a[0]), bits(x))


@pytest.mark.parametrize("n", [257, 2048 * 256 + 3])
def test_adam_edge_elements(n):
    rng = np.random.default_rng(n + 1)
    x, g, m, v = adam_state(rng, n)
    spots = [100] + ([n - 40] if n > 1000 else [])
    bad = [i for at in spots for i in adam_plant_edges(x, g, m, v, at)]
    assert sorted(bad) == sorted(at + ADAM_EDGE[k] for at in spots for k in ("nan", "inf"))       # the only elements left out below
    dc = 2.0 ** -23                                              # default betas at step 2: the power's rounding, as above
    got = adam_device((x, g, m, v), 0, 0.01, 0.9, 0.999, 2, 1.0)
    ref, bnd = adam_ref(x, g, m, v, 0.01, 0.9, 0.999, EPS, 2, 1.0, dc, dc)
    keep = np.ones(n, bool)
    keep[bad] = False
    for name, a, r, b in zip("xmv", got, ref, bnd):
        assert not np.any(np.isfinite(a[bad])), name             # NaN and inf gradients poison their own element of x, m and v ...
        assert np.all(np.isfinite(a[keep])), name                # ... and no other
        assert ratio(a[keep], r[keep], b[keep]) <= 1.0, name
    for at in spots:
        z, t, t0 = (at + ADAM_EDGE[k] for k in ("zero", "tiny", "tiny_from_zero"))
        assert bits(got[0])[z] == bits(x)[z] and bits(got[1])[z] == 0 and bits(got[2])[z] == 0
        assert np.isfinite(got[0][t]) and got[2][t0] == 0.0 and 0.0 < got[0][t0] < 1e-20


def test_adam_first_step_closed_form_and_late_step():
    n = 1000
    rng = np.random.default_rng(7)
    x, g, _, _ = adam_state(rng, n)
    zero = np.zeros(n, F)
    eta = 0.05
    for b1, b2 in ((0.9, 0.999), (0.5, 0.75)):
        # t = 1 from m = v = 0: m / c1 = g and v / c2 = g^2, so x1 = x - eta g / (|g| + eps).  powf(beta, 1) = beta and 1 - beta are
        # exact in float32 for these betas: no allowance on c1, c2
        got = adam_device((x, g, zero, zero), 0, eta, b1, b2, 1, 1.0)
        ref, bnd = adam_ref(x, g, zero, zero, eta, b1, b2, EPS, 1, 1.0)
        g64, e64 = g.astype(D), D(F(eta))
        closed = x.astype(D) - e64 * g64 / (np.abs(g64) + D(F(EPS)))
        # the closed form and adam_ref are the same number up to a few float64 roundings of the update
        assert np.all(np.abs(closed - ref[0]) <= 16 * 2.0 ** -52 * (np.abs(x) + e64))
        assert ratio(got[0], closed, bnd[0] + 16 * 2.0 ** -52 * (np.abs(x) + e64)) <= 1.0
    # step 10000 with the defaults: 0.9^10000 underflows, c1 is exactly 1; c2 keeps the power's allowance
    c1, c2 = adam_consts(0.9, 0.999, 10000)
    assert c1 == F(1) and c2 < F(1)
    x, g, m, v = adam_state(rng, n)
    got = adam_device((x, g, m, v), 0, eta, 0.9, 0.999, 10000, 1.0)
    ref, bnd = adam_ref(x, g, m, v, eta, 0.9, 0.999, EPS, 10000, 1.0, 0.0, 2.0 ** -23)
    for a, r, b in zip(got, ref, bnd):
        assert ratio(a, r, b) <= 1.0


def test_adam_refused_arguments_write_nothing():
    rng = np.random.default_rng(8)
    n = 300
    x, g, m, v = adam_state(rng, n)
    X, M, V, G = Window(x), Window(m), Window(v), readonly(g)
    before = [w.bits() for w in (X, M, V)]
    bad = _lib.ERR_INVALID_ARGUMENT
    gp = G[0].data_ptr()
    assert adam_call(n, X.ptr, gp, M.ptr, V.ptr, 0.01, 0.9, 0.999, 0, 1.0) == bad                 # step counts from 1
    assert adam_call(-1, X.ptr, gp, M.ptr, V.ptr, 0.01, 0.9, 0.999, 1, 1.0) == bad
    for k in range(4):
        args = [X.ptr, gp, M.ptr, V.ptr]
        args[k] = None
        assert adam_call(n, *args, 0.01, 0.9, 0.999, 1, 1.0) == bad
    assert adam_call(0, None, None, None, None, 0.01, 0.9, 0.999, 1, 1.0) == _lib.OK
    assert adam_call(0, X.ptr, gp, M.ptr, V.ptr, 0.01, 0.9, 0.999, 1, 1.0) == _lib.OK
    sync()
    assert all(w.guards_intact() for w in (X, M, V)) and unchanged(G)
    assert all(np.array_equal(w.bits(), b) for w, b in zip((X, M, V), before))


# ---- Rprop -----------------------------------------------------------------------------------------------------------------------

def rprop_call(n, x, g, gprev, step, gs, p=RPROP):
    return lib().ngpde_rprop_step(n, x, g, gprev, step, p["shrink"], p["grow"], p["step_min"], p["step_max"], gs, _lib.current_stream())


@pytest.mark.parametrize("grad_scale", [1.0, 0.25, 1.0 / 3.0], ids=["1", "1/4", "1/3"])
@pytest.mark.parametrize("n", ADAM_N)
def test_rprop_twelve_steps_bit_for_bit(n, grad_scale):
    x0 = np.random.default_rng(n).normal(size=n).astype(F)
    seen = {}
    for shift in (range(N_SCRIPTS) if n < N_SCRIPTS else (0,)):          # a single element walks every script in turn
        grads = rprop_gradients(n, shift, n + shift)
        trace, events = rprop_trace(x0, grads, grad_scale)
        for k, val in events.items():
            seen[k] = seen.get(k, False) or val
        for off in offsets(n):
            X, P, S = Window(x0, off=off), Window(np.zeros(n, F), off=off), Window(np.full(n, RPROP["eta"], F), off=off)
            for t, (g, (xt, gt, st)) in enumerate(zip(grads, trace)):
                G = readonly(g, off)
                _lib.check(rprop_call(n, X.ptr, G[0].data_ptr(), P.ptr, S.ptr, grad_scale))
                sync()
                assert unchanged(G)
                assert same_bits(X, xt) and same_bits(P, gt) and same_bits(S, st), (shift, off, t)
            assert X.guards_intact() and P.guards_intact() and S.guards_intact()
    # the sequences did what they are for: both limits reached exactly, a flip zeroed the remembered gradient and the next step kept
    # the size, 0.0 and -0.0 gradients, a product that underflowed to 0
    assert seen and all(seen.values()), seen


def test_rprop_refused_arguments_write_nothing():
    n = 300
    x = np.random.default_rng(9).normal(size=n).astype(F)
    X, P, S, G = Window(x), Window(np.zeros(n, F)), Window(np.full(n, 1e-3, F)), readonly(x)
    before = [w.bits() for w in (X, P, S)]
    gp = G[0].data_ptr()
    assert rprop_call(-1, X.ptr, gp, P.ptr, S.ptr, 1.0) == _lib.ERR_INVALID_ARGUMENT
    for k in range(4):
        args = [X.ptr, gp, P.ptr, S.ptr]
        args[k] = None
        assert rprop_call(n, *args, 1.0) == _lib.ERR_INVALID_ARGUMENT
    assert rprop_call(0, None, None, None, None, 1.0) == _lib.OK
    sync()
    assert all(w.guards_intact() for w in (X, P, S)) and unchanged(G)
    assert all(np.array_equal(w.bits(), b) for w, b in zip((X, P, S), before))


# ---- ngpde_accumulate_many ---------------------------------------------------------------------------------------------------------

MANY_COUNTS = [0, 1, 255, 256, 257]
MANY_BIG = 1024 * 256 + 3            # past the cap of 1024 x 256 threads per array
TAIL = 5                             # floats of the accumulator past counts[k]: they must keep their bits


def combine_call(count, c_self, base, terms, coefs, out):
    arr = (C.c_void_p * max(len(terms), 1))(*terms)
    cf = (C.c_float * max(len(coefs), 1))(*coefs)
    return lib().ngpde_rk_stage_combine(count, c_self, base, len(terms), arr, cf, out, _lib.current_stream())


def many_members(n_arrays, big_at, seed):
    """per member (count, acc data [count + TAIL] | None, g data | None, off): the counts cycle through MANY_COUNTS, every other
    zero-count member is a pair of NULL pointers, every third member sits one float off alignment"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n_arrays):
        c = MANY_BIG if k == big_at else MANY_COUNTS[(k + 1) % 5]
        if c == 0 and k % 2 == 0:
            out.append((0, None, None, 0))
            continue
        acc = (rng.normal(size=c + TAIL) * 10.0 ** rng.integers(-3, 3, c + TAIL)).astype(F)
        g = (rng.normal(size=c) * 10.0 ** rng.integers(-3, 3, c)).astype(F)
        g[: c // 7] = -acc[: c // 7]                   # exact cancellations
        out.append((c, acc, g, 1 if k % 3 == 1 else 0))
    return out


def many_call(members, accs, gs, counts=None):
    n = len(members)
    a = (C.c_void_p * max(n, 1))(*[w.ptr if w is not None else None for w in accs])
    g = (C.c_void_p * max(n, 1))(*[t[0].data_ptr() if t is not None else None for t in gs])
    c = (C.c_int64 * max(n, 1))(*(counts if counts is not None else [m[0] for m in members]))
    return lib().ngpde_accumulate_many(n, a, g, c, _lib.current_stream())


def many_buffers(members):
    accs = [Window(m[1], off=m[3]) if m[1] is not None else None for m in members]
    gs = [readonly(m[2], m[3]) if m[2] is not None else None for m in members]
    return accs, gs


@pytest.mark.parametrize("n_arrays,big_at", [(0, None), (1, None), (1, 0), (24, None), (24, 3), (24, 23), (25, None), (25, 3), (25, 24),
                                             (49, None), (49, 3), (49, 48)])
def test_accumulate_many_bit_for_bit(n_arrays, big_at):
    members = many_members(n_arrays, big_at, 100 * n_arrays + (big_at or 0))
    if n_arrays >= 24:
        assert any(m[1] is None for m in members) and any(m[0] == 0 and m[1] is not None for m in members) and any(m[3] for m in members)
    accs, gs = many_buffers(members)
    if n_arrays == 0:
        assert lib().ngpde_accumulate_many(0, None, None, None, _lib.current_stream()) == _lib.OK
        return
    _lib.check(many_call(members, accs, gs))
    sync()
    for k, ((c, acc, g, off), A, G) in enumerate(zip(members, accs, gs)):
        if A is None:
            continue
        assert A.guards_intact() and unchanged(G), k
        expect = np.concatenate([accumulate_f32(acc[:c], g), acc[c:]])          # the float32 sum; elements past the count untouched
        assert same_bits(A, expect), k
        if c:                                            # and what the header promises: the combination out = 1 * acc + 1 * g in place
            B = Window(acc, off=off)
            _lib.check(combine_call(c, 1.0, B.ptr, [G[0].data_ptr()], [1.0], B.ptr))
            sync()
            assert B.guards_intact() and np.array_equal(B.bits(), A.bits()), k


@pytest.mark.parametrize("at", [2, 30])                  # in the first launch's 24 arrays, and behind them
def test_accumulate_many_refuses_a_negative_count_before_any_launch(at):
    members = many_members(49, None, at)
    accs, gs = many_buffers(members)
    before = [w.bits() if w is not None else None for w in accs]
    counts = [m[0] for m in members]
    counts[at] = -1
    assert many_call(members, accs, gs, counts) == _lib.ERR_INVALID_ARGUMENT
    counts[at], gs_null = members[at][0], list(gs)
    live = next(k for k in range(at, 49) if members[k][0] > 0)
    gs_null[live] = None                                 # a NULL array with a positive count
    assert many_call(members, accs, gs_null, counts) == _lib.ERR_INVALID_ARGUMENT
    sync()
    for w, b in zip(accs, before):                       # nothing was written: not even the arrays ahead of the refused one
        assert w is None or (w.guards_intact() and np.array_equal(w.bits(), b))


# ---- the Runge-Kutta launches past their caps, and aliasing ----------------------------------------------------------------------

PAST_CAP = [4096 * 256 + 3,          # odd: the scalar path, two trips of its 4096 x 256 threads
            4 * 4096 * 256 + 4]      # 16-byte aligned: the float4 path, two trips
IDS = ["scalar", "float4"]


def big_inputs(count, k, seed):
    gen = torch.Generator().manual_seed(seed)
    ts = [offset_tensor(count, 0, gen) for _ in range(k)]
    assert all(t.data_ptr() % 16 == 0 for t in ts)
    return ts, [t.view(torch.int32).clone() for t in ts]


@pytest.mark.parametrize("n_terms", [0, 2, 8])
@pytest.mark.parametrize("count", PAST_CAP, ids=IDS)
def test_stage_combine_past_the_grid_cap_against_float64(count, n_terms):
    ts, snaps = big_inputs(count, n_terms + 1, count + n_terms)
    base, terms = ts[0], ts[1:]
    coefs = [float(c) for c in np.random.default_rng(n_terms).normal(size=n_terms)]
    ref, bnd = combine_ref(0.75, base.double(), [t.double() for t in terms], coefs)       # float64 on the device; (n_terms + 1) u2
    for off in offsets(count):                           # off = 1: the aligned count through the scalar path (four trips)
        out = Window(n=count, off=off)
        _lib.check(combine_call(count, 0.75, base.data_ptr(), [t.data_ptr() for t in terms], coefs, out.ptr))
        sync()
        err = (out.t.double() - ref).abs()
        assert out.guards_intact() and bool((err <= bnd).all()), (off, float((err / bnd).max()))
        print("combine: worst |device - float64| / bound", count, n_terms, off, float((err / bnd).max()))
    assert all(torch.equal(t.view(torch.int32), s) for t, s in zip(ts, snaps))


@pytest.mark.parametrize("n_terms", [2, 8])
@pytest.mark.parametrize("count", PAST_CAP, ids=IDS)
def test_stage_combine_out_may_alias_a_term(count, n_terms):
    ts, snaps = big_inputs(count, n_terms + 1, 3 * count + n_terms)
    base, terms = ts[0], ts[1:]
    coefs = [float(c) for c in np.random.default_rng(n_terms + 10).normal(size=n_terms)]
    plain = Window(n=count)
    _lib.check(combine_call(count, 0.75, base.data_ptr(), [t.data_ptr() for t in terms], coefs, plain.ptr))
    for pos in (0, n_terms - 1):
        alias = Window(n=count)
        alias.t.copy_(terms[pos])
        ptrs = [t.data_ptr() for t in terms]
        ptrs[pos] = alias.ptr
        _lib.check(combine_call(count, 0.75, base.data_ptr(), ptrs, coefs, alias.ptr))
        sync()
        assert alias.guards_intact() and plain.guards_intact() and torch.equal(alias.i, plain.i), pos
    assert all(torch.equal(t.view(torch.int32), s) for t, s in zip(ts, snaps))


@pytest.mark.parametrize("count", PAST_CAP, ids=IDS)
def test_dense_output_and_pullback_past_the_grid_cap_are_the_combines(count):
    m, stages = 2, 7
    ts, snaps = big_inputs(count, 1 + stages + m, 5 * count)
    u, ks, douts = ts[0], ts[1:1 + stages], ts[1 + stages:]
    rng = np.random.default_rng(count)
    rows = [[float(F(c)) for c in rng.normal(size=stages) * 0.3] for _ in range(m)]
    cf = (C.c_float * (stages * m))(*[c for r in rows for c in r])
    karr = (C.c_void_p * stages)(*[k.data_ptr() for k in ks])
    outs = [Window(n=count) for _ in range(m)]
    oarr = (C.c_void_p * m)(*[o.ptr for o in outs])
    _lib.check(lib().ngpde_rk_dense_output(count, u.data_ptr(), stages, karr, m, cf, oarr, _lib.current_stream()))
    sync()
    for j in range(m):
        assert outs[j].guards_intact() and torch.equal(outs[j].t, NODE._combine(u, 1.0, ks, rows[j])), j
    del outs
    # the pullback: kbar_i = sum_j rows[j][i] dout_j written from nothing, ubar += sum_j dout_j
    ubar0 = offset_tensor(count, 0, torch.Generator().manual_seed(count + 1))
    ubar = Window(n=count)
    ubar.t.copy_(ubar0)
    kbar = [Window(n=count) for _ in range(stages)]
    darr = (C.c_void_p * m)(*[d.data_ptr() for d in douts])
    kbarr = (C.c_void_p * stages)(*[k.ptr for k in kbar])
    _lib.check(lib().ngpde_rk_dense_output_pullback(count, m, darr, stages, cf, ubar.ptr, kbarr, _lib.current_stream()))
    sync()
    for i in range(stages):
        assert kbar[i].guards_intact() and torch.equal(kbar[i].t, NODE._combine(None, 1.0, douts, [rows[j][i] for j in range(m)])), i
    assert ubar.guards_intact() and torch.equal(ubar.t, NODE._combine(ubar0, 1.0, douts, [1.0] * m))
    assert all(torch.equal(t.view(torch.int32), s) for t, s in zip(ts, snaps))
