"""The references and the error bounds of the flat-vector kernels (csrc/optim.hip, csrc/row_blocks.hip), as functions the GPU tests
import (test_optim_forms_gpu.py, test_row_blocks_forms_gpu.py), and -- here, without a GPU -- the proof that each bound is
sufficient: the kernel's rule restated operation by operation in numpy float32 stays inside the bound taken against float64.

Bounds are counted, never fitted, in units of u2 = 2^-23 (twice the float32 unit roundoff, which covers the second-order terms;
as test_graph_matrices_gpu.py): one rounded operation is within u2 / 2 of its exact result, so a count of k operations spends at
most k / 2 of a `k * u2` allowance.  The library is built with -ffp-contract=off: the kernels round every product and every sum as
numpy does, and fmaf only where the source says so.

Rules that only copy, compare, or round ONCE per element (Rprop's products, acc + g, x * scale, the row-block copies, the transpose,
the row index) have no bound: the GPU tests hold them bit for bit to the numpy float32 restatement.  What is shown here for those is
that the float32 restatement is the float64 rule rounded once per operation (rounding a float64 sum, product or quotient of float32
values to float32 gives the correctly rounded float32 result: 53 >= 2 * 24 + 2 bits)."""
import numpy as np
import pytest

from oracle import ngpde_oracle as O

U2 = 2.0 ** -23
TINY = 2.0 ** -126          # the smallest normal float32: what one operation can lose when its result leaves the normal range
F, D = np.float32, np.float64


def bits(a):
    """the bit patterns of a float32 array (to compare -0.0, NaN payloads and sentinels exactly)"""
    return np.ascontiguousarray(a, dtype=F).view(np.int32)


# ---- Adam ------------------------------------------------------------------------------------------------------------------------

def adam_consts(beta1, beta2, step):
    """(c1, c2) as ngpde_adam_step forms them on the host: 1 - powf(beta, step) in float"""
    t = F(step)
    return F(1) - np.power(F(beta1), t), F(1) - np.power(F(beta2), t)


def adam_f32(x, g, m, v, eta, beta1, beta2, eps, step, grad_scale):
    """adam_kernel restated in numpy float32, operation by operation: one step from the state (x, m, v) -> (x, m, v)"""
    x, g, m, v = (np.asarray(a, F) for a in (x, g, m, v))
    c1, c2 = adam_consts(beta1, beta2, step)
    eta, b1, b2, eps, gs = F(eta), F(beta1), F(beta2), F(eps), F(grad_scale)
    with np.errstate(all="ignore"):
        gi = gs * g
        mi = b1 * m + (F(1) - b1) * gi
        vi = b2 * v + (F(1) - b2) * gi * gi
        xn = x - mi / c1 / (np.sqrt(vi / c2) + eps) * eta
    assert xn.dtype == F and mi.dtype == F and vi.dtype == F
    return xn, mi, vi


def adam_ref(x, g, m, v, eta, beta1, beta2, eps, step, grad_scale, dc1=0.0, dc2=0.0):
    """One Adam step in float64 from the float32 state, and the float32 rounding bound of every output: ((x, m, v), (bx, bm, bv)).

    The scalars are the float32 values the entry receives.  c1 = 1 - beta1^step and c2 are taken exactly; dc1 / dc2 is the absolute
    error the caller grants the entry's float c1 / c2 (0 where the power is exact in float32).

    Counted operations of the kernel, each within u2 / 2 relative (plus TINY absolute where a result leaves the normal range):
      m:   gs * g, (1 - b1), its product with g, b1 * m, the sum: every term through at most 4  ->  3 u2 on |b1 m| + |(1 - b1) g|
      v:   gs * g (entering twice), (1 - b2), two products, b2 * v, the sum: at most 6          ->  5 u2 on  b2 v  +  (1 - b2) g^2
      den: v / c2 and the root (half of v's relative error and of the quotient's, one for the root) and the sum with eps:
           the error of v carried through the root exactly, plus 2 u2 on the denominator (the quotient and the root spend 3/4 u2 of
           the root, the sum 1/2 u2 of root + eps)
      upd: m / c1, the quotient by den, the product with eta                                      ->  3 u2 on |update|
      x:   the subtraction                                                                         ->  u2 (|x| + |update|)
    The TINY terms: m's four operations lose at most TINY each; v's lose TINY each and the one on gs * g enters g^2 as 2 |g| TINY;
    the three of the update are scaled by what follows them (eta / den, eta, 1)."""
    x, g, m, v = (np.asarray(a, F).astype(D) for a in (x, g, m, v))
    eta, b1, b2, eps, gs = (D(F(a)) for a in (eta, beta1, beta2, eps, grad_scale))
    c1, c2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    with np.errstate(all="ignore"):
        gi = gs * g
        t1, t2 = b1 * m, (1.0 - b1) * gi
        m1 = t1 + t2
        bm = 3 * U2 * (np.abs(t1) + np.abs(t2)) + 4 * TINY
        s1, s2 = b2 * v, (1.0 - b2) * gi * gi
        v1 = s1 + s2
        bv = 5 * U2 * (np.abs(s1) + np.abs(s2)) + (4 + 2 * np.abs(gi)) * TINY
        q = v1 / c2
        dq = bv / (c2 - dc2) + q * dc2 / (c2 - dc2)
        r = np.sqrt(q)
        dr = np.maximum(r - np.sqrt(np.maximum(q - dq, 0.0)), np.sqrt(q + dq) - r)      # the root of q -+ dq, exactly
        den = r + eps
        dden = dr + 2 * U2 * den + TINY
        mh = m1 / c1
        dmh = bm / (c1 - dc1) + np.abs(mh) * dc1 / (c1 - dc1)
        den_lo = den - dden
        assert np.all(den_lo[np.isfinite(den_lo)] > 0)
        upd = mh / den * eta
        dupd = eta * (dmh / den_lo + np.abs(mh) * dden / (den * den_lo)) + 3 * U2 * np.abs(upd) + (eta / den_lo + eta + 1) * TINY
        x1 = x - upd
        bx = dupd + U2 * (np.abs(x) + np.abs(upd)) + TINY
    return (x1, m1, v1), (bx, bm, bv)


# The defaults (0.9, 0.999): beta^step is not a float32 number, so the entry's c1 and c2 carry the rounding of powf (under one
# unit in the last place of a value below 1: 2^-24) and of the subtraction from 1 (2^-25): at most 2^-23 absolute on each.
ADAM_BETAS = [((0.5, 0.75), 0.0), ((0.0, 0.5), 0.0), ((0.9, 0.999), 2.0 ** -23)]


def adam_state(rng, n):
    """a random state and gradient: magnitudes 1e-6 .. 1e2 with random signs (v >= 0), 5 % zero gradients, 10 % zero moments"""
    mag = lambda: 10.0 ** rng.uniform(-6, 2, n)
    sgn = lambda: rng.choice([-1.0, 1.0], n)
    x, g, m, v = mag() * sgn(), mag() * sgn(), mag() * sgn(), mag()
    g[rng.random(n) < 0.05] = 0.0
    z = rng.random(n) < 0.10
    m[z], v[z] = 0.0, 0.0
    return tuple(a.astype(F) for a in (x, g, m, v))


def ratio(got, ref, bound):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0; every element must be finite)"""
    err = np.abs(np.asarray(got, D) - ref)
    assert np.all(np.isfinite(err)) and np.all(np.isfinite(bound)) and np.all(bound >= 0)
    return float(np.max(np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1e-300)), initial=0.0))


def test_adam_float32_rule_is_inside_the_bound():
    rng = np.random.default_rng(0)
    worst = {"x": 0.0, "m": 0.0, "v": 0.0}
    for trial in range(200):
        (b1, b2), dc = ADAM_BETAS[trial % 3]
        step, gs, eta = int(rng.integers(1, 12)), (1.0, 0.25, 1.0 / 3.0)[trial % 3 if trial % 2 else (trial // 3) % 3], 10.0 ** rng.uniform(-4, -1)
        x, g, m, v = adam_state(rng, 512)
        got = adam_f32(x, g, m, v, eta, b1, b2, 1e-8, step, gs)
        ref, bnd = adam_ref(x, g, m, v, eta, b1, b2, 1e-8, step, gs, dc, dc)
        for name, a, r, b in zip("xmv", got, ref, bnd):
            worst[name] = max(worst[name], ratio(a, r, b))
        if dc == 0.0:                                    # the exact powers: float c1, c2 are the reference's
            c1, c2 = adam_consts(b1, b2, step)
            assert D(c1) == 1.0 - D(F(b1)) ** step and D(c2) == 1.0 - D(F(b2)) ** step
    print("adam worst |f32 - f64| / bound:", worst)
    assert max(worst.values()) <= 1.0
    assert worst["x"] <= 0.55           # the issue's measurement of this count (0.50): the count has not drifted


def test_adam_bound_refuses_slightly_wrong_rules():
    # what the bound is for: a rule that differs from Adam in one place must leave it
    rng = np.random.default_rng(1)
    x, g, m, v = adam_state(rng, 4096)
    eta, b1, b2, eps, step = 0.01, 0.5, 0.75, 1e-8, 3
    ref, bnd = adam_ref(x, g, m, v, eta, b1, b2, eps, step, 1.0)
    c1, c2 = adam_consts(b1, b2, step)
    gi, b1f, b2f = g, F(b1), F(b2)
    mi = b1f * m + (F(1) - b1f) * gi
    vi = b2f * v + (F(1) - b2f) * gi * gi
    wrong = {
        "eps inside the root": x - mi / c1 / np.sqrt(vi / c2 + F(eps)) * F(eta),
        "no c2": x - mi / c1 / (np.sqrt(vi) + F(eps)) * F(eta),
        "c1 of the step before": x - mi / adam_consts(b1, b2, step - 1)[0] / (np.sqrt(vi / c2) + F(eps)) * F(eta),
        "update 16 units in the last place off": x - (mi / c1 / (np.sqrt(vi / c2) + F(eps)) * F(eta)) * F(1 + 16 * U2),
    }
    for name, xw in wrong.items():
        err = np.abs(xw.astype(D) - ref[0])
        assert np.any(err > bnd[0]), name
    assert ratio(b1f * m + gi, ref[1], bnd[1]) > 1 and ratio(b2f * v + (F(1) - b2f) * gi, ref[2], bnd[2]) > 1


ADAM_EDGE = {"zero": 3, "tiny": 7, "tiny_from_zero": 8, "nan": 11, "inf": 13}      # offsets of the planted elements from `at`


def adam_plant_edges(x, g, m, v, at):
    """plant the edge elements at at + ADAM_EDGE[.] among the ordinary ones (in place); returns the non-finite positions"""
    z, t, t0, nan, inf = (at + ADAM_EDGE[k] for k in ("zero", "tiny", "tiny_from_zero", "nan", "inf"))
    g[z], m[z], v[z] = 0.0, 0.0, 0.0                     # nothing to do: x keeps its bits
    g[t], g[t0] = F(1e-30), F(-1e-30)                    # g * g underflows; the second from x = m = v = 0: the float32 v stays 0 and
    x[t0], m[t0], v[t0] = 0.0, 0.0, 0.0                  # the step, far below 1e-20, is all there is of x
    g[nan], g[inf] = np.nan, np.inf
    return [nan, inf]


def test_adam_edge_elements_in_the_float32_rule():
    rng = np.random.default_rng(2)
    x, g, m, v = adam_state(rng, 64)
    bad = adam_plant_edges(x, g, m, v, 20)
    got = adam_f32(x, g, m, v, 0.01, 0.9, 0.999, 1e-8, 2, 1.0)
    ref, bnd = adam_ref(x, g, m, v, 0.01, 0.9, 0.999, 1e-8, 2, 1.0, 2.0 ** -23, 2.0 ** -23)
    keep = np.ones(64, bool)
    keep[bad] = False
    for a, r, b in zip(got, ref, bnd):
        assert not np.any(np.isfinite(a[bad])) and np.all(np.isfinite(a[keep]))
        assert ratio(a[keep], r[keep], b[keep]) <= 1.0
    z, t = 20 + ADAM_EDGE["zero"], 20 + ADAM_EDGE["tiny_from_zero"]
    assert bits(got[0])[z] == bits(x)[z]
    assert got[2][t] == 0.0 and ref[2][t] > 0.0 and 0.0 < got[0][t] < 1e-20      # v underflowed in float32 and the step was still taken


# ---- Rprop -----------------------------------------------------------------------------------------------------------------------

RPROP = dict(eta=1e-3, shrink=0.5, grow=1.2, step_min=1e-4, step_max=2e-3)       # both limits are reached inside 12 steps
RPROP_STEPS = 12
N_SCRIPTS = 6


def rprop_gradients(n, shift, seed):
    """[RPROP_STEPS][n] float32 gradients; element i follows script (i + shift) % N_SCRIPTS:
    0 one sign throughout (the step size grows to step_max), 1 alternating signs (every flip shrinks it: down to step_min; the
    remembered gradient is zeroed and the step after a flip keeps the size), 2 every other gradient 0.0, 3 every other gradient -0.0,
    4 gradients of 1e-30 (gprev * g underflows to 0: the size never moves), 5 random magnitudes and signs"""
    rng = np.random.default_rng(seed)
    t = np.arange(RPROP_STEPS)[:, None]
    script = ((np.arange(n) + shift) % N_SCRIPTS)[None, :]
    mag = (0.5 + rng.random((RPROP_STEPS, n)))
    g = np.where(script == 0, mag, 0.0)
    g = np.where(script == 1, mag * np.where(t % 2 == 0, 1.0, -1.0), g)
    g = np.where(script == 2, np.where(t % 2 == 0, mag, 0.0), g)
    g = np.where(script == 3, np.where(t % 2 == 0, -mag, -0.0), g)
    g = np.where(script == 4, 1e-30 * mag, g)
    g = np.where(script == 5, rng.normal(size=(RPROP_STEPS, n)) * 10.0 ** rng.integers(-3, 3, (RPROP_STEPS, n)), g)
    return g.astype(F)


def rprop_trace(x, grads, grad_scale, p=RPROP):
    """the float32 rule (oracle.rprop_step) over the gradient sequence: the list of (x, gprev, step) after every step, and which
    of the events the sequence must produce it did produce"""
    state = O.rprop_init(x, p["eta"])
    ev = dict.fromkeys(["step_max", "step_min", "flip_zeroes_then_keeps", "zero_grad", "negative_zero_grad", "product_underflows"], False)
    out, x = [], np.asarray(x, F)
    flipped = np.zeros(x.shape, bool)
    for g in grads:
        gi = F(grad_scale) * g
        g_old, s0 = state["g"], state["step"]
        prod = g_old * gi
        x, state = O.rprop_step(x, g, state, (p["shrink"], p["grow"]), (p["step_min"], p["step_max"]), grad_scale=grad_scale)
        assert x.dtype == F and state["g"].dtype == F and state["step"].dtype == F
        ev["step_max"] |= bool(np.any((state["step"] == F(p["step_max"])) & (s0 * F(p["grow"]) > F(p["step_max"]))))
        ev["step_min"] |= bool(np.any((state["step"] == F(p["step_min"])) & (s0 * F(p["shrink"]) < F(p["step_min"]))))
        ev["flip_zeroes_then_keeps"] |= bool(np.any(flipped & (gi != 0) & (bits(state["step"]) == bits(s0))))
        flipped = prod < 0
        assert np.all(bits(state["g"])[flipped] == 0)                      # a flip remembers +0.0
        ev["zero_grad"] |= bool(np.any((g == 0) & ~np.signbit(g)))
        ev["negative_zero_grad"] |= bool(np.any((g == 0) & np.signbit(g) & np.signbit(state["g"])))
        ev["product_underflows"] |= bool(np.any((prod == 0) & (g_old != 0) & (gi != 0) & (state["step"] == s0)))
        out.append((x.copy(), state["g"].copy(), state["step"].copy()))
    return out, ev


def rprop_ref(x, g, gprev, step, grad_scale, p=RPROP):
    """one step of the rule in float64, every product and the subtraction rounded once to float32"""
    r = lambda a: np.asarray(a, D).astype(F).astype(D)
    x, g, gprev, s = (np.asarray(a, F).astype(D) for a in (x, g, gprev, step))
    gi = r(D(F(grad_scale)) * g)
    prod = r(gprev * gi)
    s = np.where(prod > 0, np.minimum(r(s * D(F(p["grow"]))), D(F(p["step_max"]))),
                 np.where(prod < 0, np.maximum(r(s * D(F(p["shrink"]))), D(F(p["step_min"]))), s))
    keep = np.where(prod < 0, 0.0, gi)
    return r(x - s * np.sign(keep)).astype(F), keep.astype(F), s.astype(F)


@pytest.mark.parametrize("grad_scale", [1.0, 0.25, 1.0 / 3.0])
def test_rprop_float32_rule_is_the_rounded_float64_rule_and_the_sequences_do_their_work(grad_scale):
    n = 600
    x0 = np.random.default_rng(3).normal(size=n).astype(F)
    grads = rprop_gradients(n, 0, 4)
    trace, ev = rprop_trace(x0, grads, grad_scale)
    assert all(ev.values()), ev
    x, gp, s = x0, np.zeros(n, F), np.full(n, RPROP["eta"], F)
    for g, (xt, gt, st) in zip(grads, trace):
        x, gp, s = rprop_ref(x, g, gp, s, grad_scale)
        assert np.array_equal(bits(x), bits(xt)) and np.array_equal(bits(gp), bits(gt)) and np.array_equal(bits(s), bits(st))
    # a single element sees every event over the shifts (what the GPU test does for n < N_SCRIPTS)
    seen = dict.fromkeys(ev, False)
    for shift in range(N_SCRIPTS):
        for k, val in rprop_trace(x0[:1], rprop_gradients(1, shift, 4), grad_scale)[1].items():
            seen[k] |= val
    assert all(seen.values()), seen


# ---- the Runge-Kutta combination -------------------------------------------------------------------------------------------------

def combine_ref(c_self, base, terms, coefs):
    """out = c_self * base + sum_k coefs[k] * terms[k] in float64 and its float32 bound; base / terms are float64 arrays (numpy, or
    torch tensors on any device), the scalars the float32 values the entry receives.  The kernel rounds n_terms + 1 times: the product
    with c_self, then one fmaf per term; each leaves at most u2 / 2 of the running magnitude, which |c b| + sum |c_k t_k| bounds:
    (n_terms + 1) * u2 of it holds with the second-order terms."""
    like = base if base is not None else terms[0]
    v = float(F(c_self)) * base if base is not None else 0.0 * like
    mag = abs(v)
    for c, t in zip(coefs, terms):
        v = v + float(F(c)) * t
        mag = mag + abs(float(F(c)) * t)
    return v, (len(terms) + 1) * U2 * mag + TINY


def combine_f32(c_self, base, terms, coefs):
    """rk_combine_kernel restated: 1 rounded product, then fmaf per term (the float64 product of two float32 values is exact; its
    float64 sum with a float32 value, rounded to float32, is the fused result up to a double rounding the bound has room for)"""
    v = F(c_self) * np.asarray(base, F) if base is not None else np.zeros_like(terms[0], dtype=F)
    for c, t in zip(coefs, terms):
        v = (D(F(c)) * np.asarray(t, F).astype(D) + v.astype(D)).astype(F)
    return v


@pytest.mark.parametrize("n_terms", [0, 1, 2, 8])
def test_combine_float32_rule_is_inside_the_bound(n_terms):
    rng = np.random.default_rng(n_terms)
    n = 5000
    base = (rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, n)).astype(F)
    terms = [(rng.normal(size=n) * 10.0 ** rng.integers(-3, 3, n)).astype(F) for _ in range(n_terms)]
    coefs = [float(c) for c in rng.normal(size=n_terms)]
    ref, bnd = combine_ref(0.75, base.astype(D), [t.astype(D) for t in terms], coefs)
    worst = ratio(combine_f32(0.75, base, terms, coefs), ref, bnd)
    print("combine worst ratio:", n_terms, worst)
    assert worst <= 1.0
    if n_terms:                                          # and it is a bound on THIS rule: a dropped term leaves it
        assert ratio(combine_f32(0.75, base, terms[:-1], coefs[:-1]), ref, bnd) > 1.0


# ---- acc + g and x * scale: one rounded operation ----------------------------------------------------------------------------------

def accumulate_f32(acc, g):
    """accumulate_many_kernel: fmaf(1, g, 1 * acc) = the float32 sum"""
    return np.asarray(acc, F) + np.asarray(g, F)


def rows_scale_f32(x, scale):
    return np.asarray(x, F) * np.asarray(scale, F)[:, None]


def test_single_operation_rules_are_the_rounded_float64_result():
    rng = np.random.default_rng(5)
    a = (rng.normal(size=4000) * 10.0 ** rng.integers(-20, 20, 4000)).astype(F)
    g = (rng.normal(size=4000) * 10.0 ** rng.integers(-20, 20, 4000)).astype(F)
    g[:100] = -a[:100]
    assert np.array_equal(bits(accumulate_f32(a, g)), bits((a.astype(D) + g.astype(D)).astype(F)))
    x, s = a.reshape(1000, 4), g[:1000]
    with np.errstate(over="ignore"):
        assert np.array_equal(bits(rows_scale_f32(x, s)), bits((x.astype(D) * s.astype(D)[:, None]).astype(F)))


# ---- row blocks ------------------------------------------------------------------------------------------------------------------

BLOCK_HEIGHTS = {1: (150, 7), 3: (50, 7), 64: (5, 2), 67: (5, 2)}       # (dh, dp) per width: total_rows * width crosses 256 unevenly
MAX_SEG = 16


def row_block_spec(kind, width):
    """(src_rows, out_rows, segments) of the recombinations the layers ask for; a segment is (out, dst_row0, src_row0, n_rows, sign).
    The source is the [in][out] weight of phi's first layer, its row blocks stacked in the order the layer reads them."""
    dh, dp = BLOCK_HEIGHTS[width]
    de, dth = 3, 1
    if kind == "explicit":            # [wa; wb; wc] -> [wa; -wc] / [wb; wc]
        oa, ob, oc = 0, dh, 2 * dh
        return 2 * dh + dp, [dh + dp, dh + dp], [(0, 0, oa, dh, 1.0), (0, dh, oc, dp, -1.0), (1, 0, ob, dh, 1.0), (1, dh, oc, dp, 1.0)]
    if kind == "vmh":                 # [wa - wb; -wc] / [wb; wc]: two segments cover the first dh rows of output 0
        oa, ob, oc = 0, dh, 2 * dh
        return 2 * dh + dp, [dh + dp, dh + dp], [(0, 0, oa, dh, 1.0), (0, 0, ob, dh, -1.0), (0, dh, oc, dp, -1.0), (1, 0, ob, dh, 1.0),
                                                 (1, dh, oc, dp, 1.0)]
    if kind == "mppde":               # [wa; wb; wc; wd; we] -> [wa; wc; we] / [wb; -wc] / [wd]
        oa, ob, oc, od, oe = 0, dh, 2 * dh, 2 * dh + dp, 2 * dh + dp + de
        return oe + dth, [dh + dp + dth, dh + dp, de], [(0, 0, oa, dh, 1.0), (0, dh, oc, dp, 1.0), (0, dh + dp, oe, dth, 1.0),
                                                        (1, 0, ob, dh, 1.0), (1, dh, oc, dp, -1.0), (2, 0, od, de, 1.0)]
    if kind == "gno":                 # [wa; wb; wd] -> [wa] / [wb] / [wd]
        return 2 * dh + de, [dh, dh, de], [(0, 0, 0, dh, 1.0), (1, 0, dh, dh, 1.0), (2, 0, 2 * dh, de, 1.0)]
    if kind == "limits":              # four outputs, the second empty; 16 segments, one of no rows; overlaps up to 3 deep; rows no
        r = dh                        # segment covers (the tail of output 0, the middle of output 2); source rows nothing reads
        segs = [(0, 0, 0, r - 2, 1.0), (0, 1, 3, r - 4, -1.0), (0, 2, 1, 2, 1.0), (2, 0, r, 2, -1.0), (2, 4, 0, r - 2, 1.0),
                (2, 4, 2, 3, 1.0), (3, 0, 2 * r, 3, -1.0), (3, 2, 0, 1, 1.0), (2, 1, 5, 0, 1.0), (3, 0, 1, 1, 1.0),
                (0, 0, 2 * r + 2, 1, -1.0), (2, r + 1, 7, 1, 1.0), (2, 4, r + 1, 2, -1.0), (3, 1, r, 2, 1.0), (0, r - 3, 9, 1, 1.0),
                (2, 5, 2 * r, 2, 1.0)]
        return 2 * r + 6, [r, 0, r + 2, 3], segs
    raise KeyError(kind)


ROW_BLOCK_KINDS = ["explicit", "vmh", "mppde", "gno", "limits"]


def _blocks(dtype, width, src, out_rows, segs):
    outs = [np.zeros((r, width), dtype) for r in out_rows]
    mags = [np.zeros((r, width), D) for r in out_rows]
    covers = [np.zeros(r, np.int64) for r in out_rows]
    for o, d0, s0, n, sign in segs:             # per element: the segments in order, from 0.f (row_blocks_gather_kernel)
        outs[o][d0:d0 + n] += dtype(sign) * src[s0:s0 + n]
        mags[o][d0:d0 + n] += np.abs(src[s0:s0 + n])
        covers[o][d0:d0 + n] += 1
    return outs, mags, covers


def row_blocks_gather_f32(width, src, out_rows, segs):
    return _blocks(F, width, np.asarray(src, F), out_rows, segs)[0]


def row_blocks_gather_ref(width, src, out_rows, segs):
    """float64 outputs and bounds: an entry k segments cover is a float32 sum of k signed copies taken in order from 0: (k - 1) u2 of
    sum |copies| (0 for a single cover: an exact signed copy)"""
    outs, mags, covers = _blocks(D, width, np.asarray(src, F).astype(D), out_rows, segs)
    return outs, [np.maximum(c - 1, 0)[:, None] * U2 * m for c, m in zip(covers, mags)], covers


def _pull(dtype, width, src_rows, douts, segs):
    dsrc, mag, reads = np.zeros((src_rows, width), dtype), np.zeros((src_rows, width), D), np.zeros(src_rows, np.int64)
    for o, d0, s0, n, sign in segs:             # per element: the segments in order, from 0.f (row_blocks_scatter_kernel)
        if douts[o] is None:                    # a NULL gradient counts as zero
            continue
        dsrc[s0:s0 + n] += dtype(sign) * douts[o][d0:d0 + n].astype(dtype)
        mag[s0:s0 + n] += np.abs(douts[o][d0:d0 + n])
        reads[s0:s0 + n] += 1
    return dsrc, mag, reads


def row_blocks_scatter_f32(width, src_rows, douts, segs):
    return _pull(F, width, src_rows, douts, segs)[0]


def row_blocks_scatter_ref(width, src_rows, douts, segs):
    dsrc, mag, reads = _pull(D, width, src_rows, douts, segs)
    return dsrc, np.maximum(reads - 1, 0)[:, None] * U2 * mag, reads


def adjoint_gap_bound(w, d_list, gather_bounds, scatter_bound, n_terms):
    """|<gather(W), D> - <W, scatter(D)>| with both sides summed in float64 from float32 gather / scatter results: the exact
    operators are adjoint, so the gap is the float32 rounding of each side weighted by the other factor, plus the two float64 sums"""
    gap = sum(float((np.abs(d) * b).sum()) for d, b in zip(d_list, gather_bounds) if d is not None) + float((np.abs(w) * scatter_bound).sum())
    return gap + n_terms * 2.0 ** -52 * (sum(float(np.abs(d).sum()) for d in d_list if d is not None) + 1.0) * float(np.abs(w).max() + 1.0)


def row_block_data(kind, width, seed):
    src_rows, out_rows, segs = row_block_spec(kind, width)
    rng = np.random.default_rng(seed)
    src = rng.normal(size=(src_rows, width)).astype(F)
    douts = [rng.normal(size=(r, width)).astype(F) for r in out_rows]
    return src_rows, out_rows, segs, src, douts


def adjoint_sides(src, douts, outs, dsrc):
    left = sum(float((o.astype(D) * d.astype(D)).sum()) for o, d in zip(outs, douts) if d is not None)
    return left, float((src.astype(D) * dsrc.astype(D)).sum())


@pytest.mark.parametrize("width", [1, 3, 64, 67])
@pytest.mark.parametrize("kind", ROW_BLOCK_KINDS)
def test_row_block_float32_rules_are_inside_the_bounds(kind, width):
    src_rows, out_rows, segs, src, douts = row_block_data(kind, width, width)
    total = sum(out_rows) * width
    assert total > 256 and total % 256 != 0 and len(segs) <= MAX_SEG
    if kind == "limits":
        assert len(segs) == MAX_SEG and len(out_rows) == 4 and out_rows[1] == 0 and any(s[3] == 0 for s in segs)
    for o, d0, s0, n, _ in segs:
        assert 0 <= d0 and d0 + n <= out_rows[o] and 0 <= s0 and s0 + n <= src_rows
    outs = row_blocks_gather_f32(width, src, out_rows, segs)
    ref, bnd, covers = row_blocks_gather_ref(width, src, out_rows, segs)
    worst = 0.0
    for a, r, b, c in zip(outs, ref, bnd, covers):
        worst = max(worst, ratio(a, r, b))
        assert np.array_equal(a[c == 1], r[c == 1].astype(F)) and not np.any(a[c == 0])
    if kind in ("vmh", "limits"):
        assert max(int(c.max(initial=0)) for c in covers) >= 2
    if kind == "limits":
        assert any(np.any(c == 0) for c in covers) and max(int(c.max(initial=0)) for c in covers) >= 3
    for drop in (None, 0):
        dl = [None if k == drop else d for k, d in enumerate(douts)]
        dsrc = row_blocks_scatter_f32(width, src_rows, dl, segs)
        dref, dbnd, reads = row_blocks_scatter_ref(width, src_rows, dl, segs)
        worst = max(worst, ratio(dsrc, dref, dbnd))
        assert not np.any(dsrc[reads == 0])
        left, right = adjoint_sides(src, dl, outs, dsrc)
        assert abs(left - right) <= adjoint_gap_bound(src, dl, bnd, dbnd, total + src_rows * width)
    print("row blocks worst ratio:", kind, width, worst)
    assert worst <= 1.0
    if kind == "limits":
        assert np.any(reads == 0)


# ---- rows by an index list ---------------------------------------------------------------------------------------------------------

def rows_index_f32(src, index, n_rows, scatter):
    """gather: dst[o][i] = src[o][index[i]] ([outer][n_index][d]); scatter: dst[o][index[i]] = src[o][i] ([outer][n_rows][d]), every
    other row zero.  An entry outside [0, n_rows) names no row: a zero row in the gather, skipped in the scatter."""
    src, index = np.asarray(src, F), np.asarray(index, np.int64)
    ok = (index >= 0) & (index < n_rows)
    if scatter:
        dst = np.zeros((src.shape[0], n_rows, src.shape[2]), F)
        dst[:, index[ok]] = src[:, ok]
    else:
        dst = np.zeros((src.shape[0], len(index), src.shape[2]), F)
        dst[:, ok] = src[:, index[ok]]
    return dst


OUT_OF_RANGE = (-1, None, 2 ** 40, -2 ** 40)          # None stands for n_rows itself


def index_list(n_rows, n_index, seed, out_of_range):
    """n_index distinct rows in random order; with out_of_range, entries 0, the middle and the last name no row"""
    idx = np.random.default_rng(seed).permutation(n_rows)[:n_index].astype(np.int64)
    if out_of_range:
        for k, at in enumerate(sorted({0, n_index // 2, n_index - 1} & set(range(n_index)))):
            idx[at] = n_rows if OUT_OF_RANGE[k] is None else OUT_OF_RANGE[k]
    return idx


@pytest.mark.parametrize("n_index", [0, 1, 257, 300])
def test_rows_index_restatement_gathers_scatters_and_is_its_own_adjoint(n_index):
    rng = np.random.default_rng(n_index)
    n_rows, outer, d = 300, 3, 5
    x = rng.normal(size=(outer, n_rows, d)).astype(F)
    y = rng.normal(size=(outer, n_index, d)).astype(F)
    for oor in (False, True):
        idx = index_list(n_rows, n_index, n_index, oor)
        gx, sy = rows_index_f32(x, idx, n_rows, False), rows_index_f32(y, idx, n_rows, True)
        assert gx.shape == y.shape and sy.shape == x.shape
        for i, j in enumerate(idx):
            assert np.array_equal(gx[:, i], x[:, j] if 0 <= j < n_rows else np.zeros((outer, d), F))
        assert float((gx.astype(D) * y).sum()) == pytest.approx(float((x.astype(D) * sy).sum()), rel=1e-12, abs=1e-12)
        named = np.zeros(n_rows, bool)
        named[idx[(idx >= 0) & (idx < n_rows)]] = True
        assert not np.any(sy[:, ~named]) and int(named.sum()) == n_index - (min(n_index, 3) if oor else 0)
    if n_index == n_rows:
        perm = index_list(n_rows, n_rows, 9, False)
        assert np.array_equal(rows_index_f32(rows_index_f32(x, perm, n_rows, True), perm, n_rows, False), x)
