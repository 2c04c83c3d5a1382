"""GNOConv's matrix-pipe kernels against float64 across their shape envelope (src/layers.jl:509-547).

The layer-entry tests (test_layer_abi_gpu.py) compare the entries with the composed layer, which runs the same launches; here every
form is compared with a plain float64 computation of the same operation:
  a. ngpde_gno_gform_aggregate  (csrc/gno_gform.hip: G_i = Z_i^T H_i, hsum_i, z_out) at every `in`, both chunk sizes, every act1
     instantiation, every operand set, rows of 0 .. 129 edges;
  b. ngpde_gno_gform_transform  (G W2 + hsum B2 + h W + bias) on partial 128-row and 128-column tiles, every split, every optional term;
  c. the by-source entries (csrc/gno_mfma.hip: ngpde_gno_message_forward, ngpde_gno_apply_*, ngpde_gno_message_backward_from_nodes)
     at every supported (out, k);
  d. the GNOConv layer end to end against O.gno_conv / O.gno_conv_backward, one case per plan form;
  e. the 4 GB guard of the aggregate-then-transform form;
  f. the ABI queries' answers and the layer entry's workspace sizes, pinned to tests/golden/gno_forms.json.

Which form a layer case must show comes from tests/gno_forms_spec.py, the restatement of csrc/gno_forms.h, where every choice is made.

Tolerances are the suite's: forward 1e-4 * max|ref| + 1e-5, gradients 5e-4 relative.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib
from oracle import ngpde_oracle as O
import gno_forms_spec as S
from test_mp_gpu import check_grads, close, mlp_grad_pairs, omlp, prep

pytestmark = pytest.mark.gpu
DEV = "cuda"
K64 = 64
SWITCHES = S.SWITCHES


def clear_switches(monkeypatch):
    # the suite may run under one of these (tools/switch_matrix.sh): every case here names the form it tests
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)


def dv(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def nan_buf(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def p_order(t):
    """edge order of the per-edge arrays: by target, COO order inside a row"""
    return np.argsort(t, kind="stable")


# ---- a. the aggregate of the aggregate-then-transform form ------------------------------------------------------------------------

DEGREES = (0, 1, 3, 4, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)


def degree_graph(seed):
    """one graph holding every in-degree of DEGREES (and isolated nodes), targets in random COO order"""
    rng = np.random.default_rng(seed)
    N = 40
    nodes = rng.permutation(N)[:len(DEGREES)]
    t = np.concatenate([np.full(d, n) for n, d in zip(nodes, DEGREES)])
    s = rng.integers(0, N, t.size)
    perm = rng.permutation(t.size)
    return s[perm], t[perm], N


@pytest.mark.parametrize("chunk", [16, 32])
@pytest.mark.parametrize("cin", [32, 64, 128])
def test_gform_aggregate_against_float64(cin, chunk, monkeypatch):
    # G_i[k][i'] = sum_{e -> i} z_e[k] h_{s_e}[i'], hsum_i = sum_{e -> i} h_{s_e} (both / deg when mean), z_e = act1(P[t_e] + Q[s_e] + E_e)
    # kept in p order.  act1 tanh / swish take the kernel's run-time activation; 16-edge chunks at in = 32 have more staging rows
    # than edges (a full chunk's rows 16 .. 31 are clamped copies of its last edge)
    clear_switches(monkeypatch)
    monkeypatch.setenv("NGPDE_GNO_GFORM_CHUNK", str(chunk))
    lib = _lib.load()
    rng = np.random.default_rng(100 + cin + chunk)
    s, t, N = degree_graph(7)
    E = s.size
    handle = ng.GNNGraph(s, t, num_nodes=N, index_base=0).handle()
    order = p_order(t)
    sp, tp = s[order], t[order]
    deg = np.bincount(t, minlength=N)
    h = rng.normal(size=(N, cin)).astype(np.float32)
    th = dv(h)
    H = h.astype(np.float64)[sp]                                       # [E][in], p order
    A = np.zeros((N, E))                                               # target incidence: A[t_e][e] = 1
    A[tp, np.arange(E)] = 1.0
    hsum = A @ H
    P, Q, Et = (rng.normal(size=(N, K64)).astype(np.float32), rng.normal(size=(N, K64)).astype(np.float32),
                rng.normal(size=(E, K64)).astype(np.float32))
    tP, tQ, tE = dv(P), dv(Q), dv(Et)
    operand_sets = {"PQE": (True, True, True), "PQ": (True, True, False), "E": (False, False, True)}
    case = 0
    for mean in (0, 1):
        div = np.maximum(deg, 1)[:, None] if mean else np.ones((N, 1))
        for act1 in ("identity", "relu", "tanh", "swish"):
            for ops, (hp, hq, he) in operand_sets.items():
                pre = np.zeros((E, K64))
                if hp:
                    pre += P[tp]
                if hq:
                    pre += Q[sp]
                if he:
                    pre += Et
                z = O.act(act1, pre)                                   # [E][k], p order
                Gr = (A @ (z[:, :, None] * H[:, None, :]).reshape(E, K64 * cin)).reshape(N, K64, cin) / div[:, :, None]
                hr = hsum / div
                for want_hs, want_z in ((True, True), (False, True), (True, False), (False, False)):
                    G, hs, zo = nan_buf(N, K64 * cin), nan_buf(N, cin), nan_buf(E, K64)
                    _lib.check(lib.ngpde_gno_gform_aggregate(handle.ptr, cin, K64, _lib.ACT[act1], mean, _lib.ptr(tP) if hp else None,
                                                             _lib.ptr(tQ) if hq else None, _lib.ptr(tE) if he else None, _lib.ptr(th),
                                                             _lib.ptr(G), _lib.ptr(hs) if want_hs else None, _lib.ptr(zo) if want_z else None,
                                                             _lib.current_stream()))
                    what = f"in={cin} chunk={chunk} mean={mean} act1={act1} ops={ops} hsum={want_hs} z_out={want_z}"
                    close(G.view(N, K64, cin), Gr, what="G " + what)
                    if want_hs:
                        close(hs, hr, what="hsum " + what)
                    else:
                        assert bool(torch.isnan(hs).all()), what
                    if want_z:
                        close(zo, z, what="z_out " + what)
                    else:
                        assert bool(torch.isnan(zo).all()), what
                    case += 1
    assert case == 2 * 4 * 3 * 4


# ---- b. the transform -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cout", [4, 20, 48, 144, 256])
@pytest.mark.parametrize("N", [1, 127, 128, 129, 300])
def test_gform_transform_against_float64(N, cout, monkeypatch):
    # y = act.(G W2' + hsum B2 + h W + bias), zt = the pre-activation: the contraction split into nsplit slabs, the b2 term and W h two
    # more slabs of the same launch, the slab reduction fused with the tail (16-byte stores, or 4-byte ones when y / zt are not aligned)
    clear_switches(monkeypatch)
    lib = _lib.load()
    cin = 32 if N % 2 else 64
    Kc = cin * K64
    rng = np.random.default_rng(N * 1000 + cout)
    G, W2 = rng.normal(size=(N, Kc)).astype(np.float32), (rng.normal(size=(Kc, cout)) / np.sqrt(Kc)).astype(np.float32)
    hs, b2 = rng.normal(size=(N, cin)).astype(np.float32), rng.normal(size=cin * cout).astype(np.float32)
    h, w = rng.normal(size=(N, cin)).astype(np.float32), rng.normal(size=(cin, cout)).astype(np.float32)
    bias = rng.normal(size=cout).astype(np.float32)
    tG, tW2, ths, tb2, th, tw, tbias = (dv(a) for a in (G, W2, hs, b2, h, w, bias))
    f64 = lambda a: a.astype(np.float64)
    base = f64(G) @ f64(W2)
    b2term = f64(hs) @ f64(b2).reshape(cin, cout)                      # B2[i'][o] = b2[o + out i']
    hw = f64(h) @ f64(w)
    splits = int(lib.ngpde_gno_gform_splits(N, cin, K64, cout))
    assert 1 <= splits <= 32
    acts = ("identity", "relu", "tanh", "swish")
    i = 0
    for nsplit in sorted({1, splits, 32}):
        slabs = torch.empty((nsplit + 2, N, cout), device=DEV)
        for with_b2 in (True, False):
            for with_h in (True, False):
                for with_bias in (True, False):
                    act = acts[i % 4]
                    off = (i // 4) % 2                                 # y and zt one float past a 16-byte boundary: the 4-byte path
                    i += 1
                    ybuf, zbuf = nan_buf(N * cout + 4), nan_buf(N * cout + 4)
                    y, zt = ybuf[off:off + N * cout], zbuf[off:off + N * cout]
                    _lib.check(lib.ngpde_gno_gform_transform(N, cin, K64, cout, _lib.ACT[act], _lib.ptr(tG), _lib.ptr(tW2),
                                                             _lib.ptr(ths) if with_b2 else None, _lib.ptr(tb2) if with_b2 else None,
                                                             _lib.ptr(th) if with_h else None, _lib.ptr(tw) if with_h else None,
                                                             _lib.ptr(tbias) if with_bias else None, _lib.ptr(y), _lib.ptr(zt),
                                                             _lib.ptr(slabs), nsplit, _lib.current_stream()))
                    zr = base + (b2term if with_b2 else 0.0) + (hw if with_h else 0.0) + (f64(bias) if with_bias else 0.0)
                    what = f"N={N} out={cout} nsplit={nsplit} b2={with_b2} h={with_h} bias={with_bias} act={act} offset={off}"
                    close(zt.view(N, cout), zr, what="zt " + what)
                    close(y.view(N, cout), O.act(act, zr), what="y " + what)
                    # nothing written around the outputs
                    assert bool(torch.isnan(ybuf[:off]).all() and torch.isnan(ybuf[off + N * cout:]).all()), what
                    assert bool(torch.isnan(zbuf[:off]).all() and torch.isnan(zbuf[off + N * cout:]).all()), what
    # without zt
    y = nan_buf(N, cout)
    slabs = torch.empty((splits + 2, N, cout), device=DEV)
    _lib.check(lib.ngpde_gno_gform_transform(N, cin, K64, cout, _lib.ACT["tanh"], _lib.ptr(tG), _lib.ptr(tW2), _lib.ptr(ths), _lib.ptr(tb2),
                                             _lib.ptr(th), _lib.ptr(tw), _lib.ptr(tbias), _lib.ptr(y), None, _lib.ptr(slabs), splits,
                                             _lib.current_stream()))
    close(y, np.tanh(base + b2term + hw + f64(bias)), what="y without zt")


# ---- c. the by-source matrix-pipe entries -------------------------------------------------------------------------------------------

def by_source_graph(seed):
    """isolated nodes (the last 9), and node 5 the source of 400 edges: a by-source row far beyond one staging batch"""
    rng = np.random.default_rng(seed)
    N = 200
    s = np.concatenate([rng.integers(0, N - 9, 1200), np.full(400, 5)])
    t = rng.integers(0, N - 9, s.size)
    perm = rng.permutation(s.size)
    return s[perm], t[perm], N


def per_source(sp, N):
    idx = np.argsort(sp, kind="stable")
    bounds = np.searchsorted(sp[idx], np.arange(N + 1))
    return [idx[bounds[j]:bounds[j + 1]] for j in range(N)]


@pytest.mark.parametrize("k", [16, 32, 64])
@pytest.mark.parametrize("cout", [16, 48, 128, 256])
def test_by_source_entries_against_float64(cout, k, monkeypatch):
    # m_e = T_{s_e} z_e + Bh_{s_e} (T [N][out][k]), z_e = act1(P[t_e] + Q[s_e] + E_e); aggregated by target with + / mean / max.
    # Pullbacks: ngpde_gno_message_backward_from_nodes from the node gradient (+ / mean), ngpde_segment_reduce_backward +
    # ngpde_gno_apply_backward (max), ngpde_gno_apply_* on a given z
    clear_switches(monkeypatch)
    lib = _lib.load()
    assert lib.ngpde_gno_message_supported(cout, k) == 1
    apply_ok = lib.ngpde_gno_apply_supported(cout, k) == 1      # (256 x 64: T_j beyond the apply entries' LDS limit)
    assert apply_ok == (cout * k < 256 * 64)
    rng = np.random.default_rng(cout * 100 + k)
    s, t, N = by_source_graph(3)
    E = s.size
    handle = ng.GNNGraph(s, t, num_nodes=N, index_base=0).handle()
    order = p_order(t)
    sp, tp = s[order], t[order]
    groups = per_source(sp, N)
    deg = np.maximum(np.bincount(t, minlength=N), 1)
    P, Q, Et = (rng.normal(size=(N, k)).astype(np.float32), rng.normal(size=(N, k)).astype(np.float32), rng.normal(size=(E, k)).astype(np.float32))
    T = (rng.normal(size=(N, cout, k)) / np.sqrt(k)).astype(np.float32)
    Bh = rng.normal(size=(N, cout)).astype(np.float32)
    R = rng.normal(size=(N, cout)).astype(np.float32)
    tP, tQ, tE, tT, tBh, tR = (dv(a) for a in (P, Q, Et, T, Bh, R))
    T64 = T.astype(np.float64)
    st = _lib.current_stream()
    for act1 in ("identity", "relu"):
        pre = P[tp].astype(np.float64) + Q[sp] + Et
        z = O.act(act1, pre)
        dact = O.dact(act1, pre)
        for with_bh in (True, False):
            what = f"out={cout} k={k} act1={act1} Bh={with_bh}"
            m = np.zeros((E, cout))
            for j, ix in enumerate(groups):
                m[ix] = z[ix] @ T64[j].T
            if with_bh:
                m += Bh[sp]
            zo, mo = nan_buf(E, k), nan_buf(E, cout)
            _lib.check(lib.ngpde_gno_message_forward(handle.ptr, cout, k, _lib.ACT[act1], _lib.ptr(tP), _lib.ptr(tQ), _lib.ptr(tE), _lib.ptr(tT),
                                                     _lib.ptr(tBh) if with_bh else None, _lib.ptr(zo), _lib.ptr(mo), st))
            close(zo, z, what="z_out " + what)
            close(mo, m, what="m " + what)
            # the same message from a given z (ngpde_gno_apply_forward)
            ma = nan_buf(E, cout)
            rc = lib.ngpde_gno_apply_forward(handle.ptr, cout, k, _lib.ptr(tT), _lib.ptr(tBh) if with_bh else None, _lib.ptr(zo), _lib.ptr(ma), st)
            if apply_ok:
                _lib.check(rc)
                close(ma, m, what="apply m " + what)
            else:
                assert rc == _lib.ERR_UNSUPPORTED and bool(torch.isnan(ma).all()), what
            for aggr in ("+", "mean", "max"):
                agg = O.scatter(aggr, m.T, tp, N).T                  # [N][out]; an empty max stays -inf
                ag = nan_buf(N, cout)
                _lib.check(lib.ngpde_segment_reduce_forward(handle.ptr, cout, _lib.AGGR[aggr], _lib.ptr(mo), _lib.ptr(ag), st))
                fin = np.isfinite(agg)
                assert np.array_equal(torch.isfinite(ag).cpu().numpy(), fin), what
                close(ag.cpu().numpy()[fin], agg[fin], what=f"agg {aggr} " + what)
                if aggr == "max":   # which message is a target's largest: the kernel's own (float64 and float32 may order near-ties apart)
                    dm = O.scatter_pullback(aggr, mo.cpu().double().numpy().T, tp, N, ag.cpu().double().numpy().T, R.T.astype(np.float64)).T
                else:
                    dm = O.scatter_pullback(aggr, m.T, tp, N, agg.T, R.T.astype(np.float64)).T       # [E][out]
                dT, dBh, dq, da = np.zeros((N, cout, k)), np.zeros((N, cout)), np.zeros((N, k)), np.zeros((E, k))
                for j, ix in enumerate(groups):
                    dT[j] = dm[ix].T @ z[ix]
                    dBh[j] = dm[ix].sum(axis=0)
                    da[ix] = dm[ix] @ T64[j]
                dpre = da * dact
                for j, ix in enumerate(groups):
                    dq[j] = dpre[ix].sum(axis=0)
                dTo, dBho, dzo = nan_buf(N, cout * k), nan_buf(N, cout), nan_buf(E, k)
                if aggr == "max":
                    assert lib.ngpde_gno_message_backward_from_nodes(handle.ptr, cout, k, _lib.AGGR[aggr], _lib.ACT[act1], _lib.ptr(tT), _lib.ptr(zo),
                                                                     _lib.ptr(tR), _lib.ptr(dTo), None, _lib.ptr(dzo), None, st) == _lib.ERR_UNSUPPORTED
                    dmo = nan_buf(E, cout)
                    _lib.check(lib.ngpde_segment_reduce_backward(handle.ptr, cout, _lib.AGGR[aggr], _lib.ptr(mo), _lib.ptr(ag), _lib.ptr(tR),
                                                                 _lib.ptr(dmo), st))
                    close(dmo, dm, rtol=5e-4, what="dm max " + what)
                    rc = lib.ngpde_gno_apply_backward(handle.ptr, cout, k, _lib.ptr(tT), _lib.ptr(zo), _lib.ptr(dmo), _lib.ptr(dTo),
                                                      _lib.ptr(dBho), _lib.ptr(dzo), st)
                    if not apply_ok:
                        assert rc == _lib.ERR_UNSUPPORTED, what
                        continue
                    _lib.check(rc)
                    close(dzo, da, rtol=5e-4, what="apply dz " + what)            # (apply_backward: the gradient of its z)
                else:
                    dqo = nan_buf(N, k)
                    _lib.check(lib.ngpde_gno_message_backward_from_nodes(handle.ptr, cout, k, _lib.AGGR[aggr], _lib.ACT[act1], _lib.ptr(tT),
                                                                         _lib.ptr(zo), _lib.ptr(tR), _lib.ptr(dTo),
                                                                         _lib.ptr(dBho) if with_bh else None, _lib.ptr(dzo), _lib.ptr(dqo), st))
                    close(dzo, dpre, rtol=5e-4, what=f"dz {aggr} " + what)      # (the gradient of the pre-activation)
                    close(dqo, dq, rtol=5e-4, what=f"dq {aggr} " + what)
                close(dTo.view(N, cout, k), dT, rtol=5e-4, what=f"dT {aggr} " + what)
                if with_bh or aggr == "max":
                    close(dBho, dBh, rtol=5e-4, what=f"dBh {aggr} " + what)
                else:
                    assert bool(torch.isnan(dBho).all()), what
    # outside the matrix-pipe kernels' envelope the fused entries refuse instead of computing something else
    for co, kk in ((cout + 8, k), (cout, 48), (272, k)):
        assert lib.ngpde_gno_message_supported(co, kk) == 0
        assert lib.ngpde_gno_message_forward(handle.ptr, co, kk, 1, _lib.ptr(tP), None, None, _lib.ptr(tT), None, None, _lib.ptr(tR), st) == _lib.ERR_UNSUPPORTED
        assert lib.ngpde_gno_message_backward_from_nodes(handle.ptr, co, kk, 0, 1, _lib.ptr(tT), _lib.ptr(tE), _lib.ptr(tR), _lib.ptr(tT), None,
                                                         None, None, st) == _lib.ERR_UNSUPPORTED


# ---- d. the layer end to end ----------------------------------------------------------------------------------------------------------

def layer_graph(N, deg, seed, edata=0, node_data=True, isolated=0):
    """`deg` incoming edges per node (the last `isolated` nodes none; deg = None: 6 N random edges), 2-d positions and one more node
    feature (or none: an edge-only graph), as the library's graph and the oracle's"""
    rng = np.random.default_rng(seed)
    if deg is None:
        s, t = rng.integers(0, N, 6 * N), rng.integers(0, N - isolated, 6 * N)
    else:
        t = np.repeat(np.arange(N - isolated), deg)
        s = rng.integers(0, N, t.size)
        perm = rng.permutation(t.size)
        s, t = s[perm], t[perm]
    kw = {}
    if node_data:
        kw["ndata"] = {"x": rng.random((2, N)), "f0": rng.normal(size=(1, N))}
    if edata:
        kw["edata"] = {"e": rng.normal(size=(edata, s.size))}
    g = ng.GNNGraph(s, t, num_nodes=N, index_base=0, **{k: {n: v.astype(np.float32) for n, v in d.items()} for k, d in kw.items()})
    og = O.Graph(s, t, num_nodes=N, index_base=0, **{k: {n: v.astype(np.float32).astype(np.float64) for n, v in d.items()} for k, d in kw.items()})
    return g, og, 3 if node_data else 0


# (name, in, out, k, aggr, first, b2, N, deg, edata, node data, chunk, form in training, form in inference, phi)
# phi: "2" = Dense(., k, first), Dense(k, in out); "1" = Dense(., in out, first) alone; "3" = Dense(., 32, first), Dense(32, k, relu),
# Dense(k, in out); "2-relu" = "2" with relu on the last layer (K_e is no longer linear in z_e: the literal contraction)
LAYER_CASES = [
    ("gform-train-in32-chunk16", 32, 48, 64, "+", "relu", True, 150, 64, 0, True, 16, "gform", "gform", "2"),
    ("gform-train-in64-mean", 64, 16, 64, "mean", "identity", True, 130, 70, 1, True, 32, "gform", "gform", "2"),
    ("gform-infer-in128", 128, 16, 64, "mean", "relu", True, 200, 20, 0, True, 32, "fused-agg", "gform", "2"),
    ("gform-infer-in32-chunk16", 32, 128, 64, "+", "identity", True, 129, 24, 2, True, 16, "fused-agg", "gform", "2"),
    ("by-source-sum-k16", 64, 48, 16, "+", "relu", True, 300, None, 0, True, 32, "fused-agg", "fused-agg", "2"),
    ("by-source-mean-k32", 32, 128, 32, "mean", "identity", True, 257, None, 2, True, 32, "fused-agg", "fused-agg", "2"),
    ("message-max", 32, 16, 64, "max", "relu", True, 257, None, 0, True, 32, "fused-msg", "fused-msg", "2"),
    ("edge-only", 32, 48, 64, "mean", "relu", True, 100, 70, 3, False, 32, "gform", "gform", "2"),
    ("no-b2", 128, 16, 64, "+", "relu", False, 100, 66, 0, True, 32, "gform", "gform", "2"),
    ("phi-one-layer", 8, 12, 16, "+", "tanh", True, 129, 5, 1, True, 32, "literal", "literal", "1"),
    ("phi-three-layers", 16, 20, 24, "mean", "swish", True, 130, None, 0, True, 32, "reassoc", "reassoc", "3"),
    ("last-layer-relu", 8, 16, 64, "+", "relu", True, 129, 5, 0, True, 32, "literal", "literal", "2-relu"),
]


def phi_dims_acts(shape, d0, k, cin, cout, first):
    """widths and activations of phi's Dense layers for a case's phi column"""
    if shape == "1":
        return [d0, cin * cout], [first]
    if shape == "3":
        return [d0, 32, k, cin * cout], [first, "relu", "identity"]
    return [d0, k, cin * cout], [first, "relu" if shape == "2-relu" else "identity"]


def plan_form(N, E, cin, cout, dims, acts, b2, aggr, training):
    """the layer entry's form (csrc/gno_forms.h: gno_layer_form) by its restatement, under the environment of the moment"""
    return S.layer_form_name(S.layer_form(N, E, cin, cout, len(acts), dims[-2], _lib.ACT[acts[0]], _lib.ACT[acts[-1]], b2, _lib.AGGR[aggr], training))


@pytest.mark.parametrize("case", LAYER_CASES, ids=[c[0] for c in LAYER_CASES])
def test_gno_layer_forms_against_float64(case, monkeypatch):
    # output, dx and every parameter gradient of GNOConv through the layer entry against the literal float64 layer (O.gno_conv:
    # K materialised, batched_mul, scatter): one case per plan form, node counts off the 128-row tiles, nodes without incoming edges
    name, cin, cout, k, aggr, first, b2, N, deg, de, nd, chunk, f_train, f_infer, shape = case
    clear_switches(monkeypatch)
    monkeypatch.setenv("NGPDE_GNO_GFORM_CHUNK", str(chunk))
    g, og, ds = layer_graph(N, deg, 31, edata=de, node_data=nd, isolated=0 if deg is not None else 3)
    E = g.num_edges
    assert E * cin * cout <= 2.5e7                                       # (the literal oracle's [in out][E] arrays)
    dims, acts = phi_dims_acts(shape, 2 * ds + de, k, cin, cout, first)
    assert plan_form(N, E, cin, cout, dims, acts, b2, aggr, True) == f_train, name
    assert plan_form(N, E, cin, cout, dims, acts, b2, aggr, False) == f_infer, name
    lib = _lib.load()                                                     # the library's queries say what the restatement says of this case
    for training in (False, True):
        f = S.layer_form(N, E, cin, cout, len(acts), dims[-2], _lib.ACT[acts[0]], _lib.ACT[acts[-1]], b2, _lib.AGGR[aggr], training)
        assert lib.ngpde_gno_apply_supported(cout, dims[-2]) == int(f["apply"]["apply_entry"]), name
        assert lib.ngpde_gno_message_supported(cout, dims[-2]) == int(f["apply"]["message_entry"]), name
        assert lib.ngpde_gno_gform_preferred(N, E, cin, dims[-2], cout, int(training)) == int(f["by_target"]["preferred"]), name
        assert lib.ngpde_gno_gform_splits(N, cin, dims[-2], cout) == f["by_target"]["nsplit"], name
    phi = ng.Chain(*[ng.Dense(dims[l], dims[l + 1], acts[l], **({"bias": b2} if l + 1 == len(acts) else {})) for l in range(len(acts))])
    layer = ng.GNOConv((cin, cout), phi, "tanh", initialgraph=g, aggr=aggr)
    ps0, st = ng.setup(41, layer)
    ps = prep(ps0, 41)
    x = torch.randn(cin, N, device=DEV)
    W = ps["linear"]["weight"].detach().cpu().double().numpy()
    b = ps["linear"]["bias"].detach().cpu().double().numpy()
    yo, c = O.gno_conv(x.cpu().double().numpy(), omlp(phi, ps["ϕ"]), W, b, og, cin, cout, "tanh", aggr)
    with torch.no_grad():
        yi, _ = layer(x, ps, st)
    close(yi, yo, what=f"{name} inference y")
    xg = x.clone().requires_grad_(True)
    y, _ = layer(xg, ps, st)
    close(y, yo, what=f"{name} training y")
    R = np.random.default_rng(42).normal(size=yo.shape)
    (y * torch.as_tensor(R, dtype=torch.float32, device=DEV)).sum().backward()
    gr = O.gno_conv_backward(c, R)
    n1, o1 = mlp_grad_pairs(ps["ϕ"], gr["phi"], phi)
    names = n1 + [("linear.weight", ps["linear"]["weight"]), ("linear.bias", ps["linear"]["bias"])]
    check_grads(ps, (names, o1 + [gr["weight"], gr["bias"]]), xg, gr["x"])


# ---- e. the 4 GB guard ------------------------------------------------------------------------------------------------------------

def test_gform_guard_covers_the_q_rows(monkeypatch):
    # Q rows are 64 floats (256 bytes) fetched with 32-bit byte offsets: at in = 32 the Q table, not h, reaches 4 GB first (2^24 nodes)
    clear_switches(monkeypatch)
    lib = _lib.load()
    E = 1 << 30
    assert lib.ngpde_gno_gform_preferred(1 << 24, E, 32, 64, 64, 0) == 0
    assert lib.ngpde_gno_gform_preferred(1 << 23, E, 32, 64, 64, 0) == 1
    assert lib.ngpde_gno_gform_preferred(1 << 23, E, 64, 64, 64, 0) == 1
    assert lib.ngpde_gno_gform_preferred(1 << 23, E, 128, 64, 64, 0) == 0
    assert lib.ngpde_gno_gform_preferred((1 << 23) - 1, E, 128, 64, 64, 0) == 1


# ---- f. the queries' answers and the layer workspace sizes, pinned to the build before csrc/gno_forms.h ------------------------------

FORMS_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gno_forms.json")
QUERY_OUTS = (0, 1, 4, 15, 16, 17, 112, 128, 129, 144, 240, 256, 257, 272)
QUERY_KS = (0, 1, 8, 15, 16, 17, 32, 33, 48, 64, 65, 128, 256, 257)
QUERY_INS = (0, 16, 32, 48, 64, 96, 128, 256)
QUERY_NS = (0, 1, 127, 128, 129, 4096, 1 << 20, (1 << 23) - 1, 1 << 23, 1 << 24)
QUERY_SETTINGS = [None] + [(name, "1") for name in S.PATH_SWITCHES] + [(S.GNO_GFORM_CHUNK, v) for v in ("16", "32", "7")]
LAYER_SETTINGS = QUERY_SETTINGS[:4]                                        # unswitched and each path switch alone
DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"                            # ngpde_gno_gform_splits: one character per answer (at most 32)
AS_UNSWITCHED = "as unswitched"


def hexbits(vals):
    """yes / no answers, four per hexadecimal digit, first answer in the highest bit (the last digit padded with zero bits)"""
    bits = "".join("1" if v else "0" for v in vals)
    bits += "0" * (-len(bits) % 4)
    return f"{int(bits, 2):0{len(bits) // 4}x}"


def query_edge_counts(N):
    return (0, 1, 64 * N - 1, 64 * N, 1 << 30)


def gno_descriptor(case, ds, dev_ptr):
    """ngpde_gno_layer_t of a layer case: the size query reads the widths and tests the pointers for NULL"""
    name, cin, cout, k, aggr, first, b2, N, deg, de, nd, chunk, f_train, f_infer, shape = case
    dims, acts = phi_dims_acts(shape, 2 * ds + de, k, cin, cout, first)
    d = _lib.GnoLayer()
    d.in_chs, d.out_chs, d.aggr, d.act = cin, cout, _lib.AGGR[aggr], _lib.ACT["tanh"]
    d.h = d.weight = d.bias = dev_ptr
    d.node_feat, d.node_feat_width = (dev_ptr, ds) if ds else (None, 0)
    d.edge_feat, d.edge_feat_width = (dev_ptr, de) if de else (None, 0)
    d.phi.n_layers = len(acts)
    for l, w in enumerate(dims):
        d.phi.dims[l] = w
    for l, a in enumerate(acts):
        d.phi.act[l] = _lib.ACT[a]
        d.phi.weight[l] = dev_ptr
        d.phi.bias[l] = dev_ptr if (b2 or l + 1 < len(acts)) else None
    return d


def query_answers(monkeypatch):
    """the five queries over the boundary grid under every switch setting, and ngpde_gno_layer_workspace_bytes of every layer case
    [inference, training] unswitched and under each path switch, as the library answers now.  Yes / no answers as hexbits, groups
    separated by blanks: apply / message_supported one group per out (over k), gform_supported one per in (over k), gform_preferred
    per N one group per (E, training) over in x (k, out) with (k, out) = every k x 128 and 64 x every out, gform_splits per N one group
    per in over k x out.  A table that a switch leaves as it is without it says so instead of repeating it."""
    lib = _lib.load()
    digits = lambda vals: "".join(DIGITS[int(v)] for v in vals)
    ko = [(k, 128) for k in QUERY_KS] + [(64, out) for out in QUERY_OUTS]
    queries = {}
    for setting in QUERY_SETTINGS:
        clear_switches(monkeypatch)
        if setting:
            monkeypatch.setenv(*setting)
        q = {"apply_supported": " ".join(hexbits(lib.ngpde_gno_apply_supported(o, k) for k in QUERY_KS) for o in QUERY_OUTS),
             "message_supported": " ".join(hexbits(lib.ngpde_gno_message_supported(o, k) for k in QUERY_KS) for o in QUERY_OUTS),
             "gform_supported": " ".join(hexbits(lib.ngpde_gno_gform_supported(i, k) for k in QUERY_KS) for i in QUERY_INS),
             "gform_preferred": {f"N={N}": " ".join(hexbits(lib.ngpde_gno_gform_preferred(N, E, i, k, o, tr) for i in QUERY_INS for k, o in ko)
                                                    for E in query_edge_counts(N) for tr in (0, 1)) for N in QUERY_NS},
             "gform_splits": {f"N={N}": " ".join(digits(lib.ngpde_gno_gform_splits(N, i, k, o) for k in QUERY_KS for o in QUERY_OUTS) for i in QUERY_INS)
                              for N in QUERY_NS}}
        if setting:
            q = {name: (AS_UNSWITCHED if table == queries[""][name] else table) for name, table in q.items()}
        queries["=".join(setting) if setting else ""] = q
    layers = {"=".join(setting) if setting else "": {} for setting in LAYER_SETTINGS}
    dummy = torch.zeros(16, device=DEV)
    for case in LAYER_CASES:
        g, _, ds = layer_graph(case[7], case[8], 31, edata=case[9], node_data=case[10], isolated=0 if case[8] is not None else 3)
        handle = g.handle()
        d = gno_descriptor(case, ds, dummy.data_ptr())
        for setting in LAYER_SETTINGS:
            clear_switches(monkeypatch)
            if setting:
                monkeypatch.setenv(*setting)
            layers["=".join(setting) if setting else ""][case[0]] = [int(lib.ngpde_gno_layer_workspace_bytes(handle.ptr, C.byref(d), tr)) for tr in (0, 1)]
    clear_switches(monkeypatch)
    return {"queries": queries, "layer_workspace_bytes": layers}


def test_queries_answer_what_the_build_before_the_forms_header_answered(monkeypatch):
    # which kernel runs never shows in a float64 comparison; what the ABI queries and the layer's workspace size say about it does.
    # tests/golden/gno_forms.json holds their answers from the library as it was before the choices moved into csrc/gno_forms.h (the
    # field "recorded_from" names the commit; tools/record_forms.py --family gno wrote it).  No kernel of the family is launched here.
    want = json.load(open(FORMS_GOLDEN))
    got = query_answers(monkeypatch)
    assert set(got["queries"]) == set(want["queries"]) == {""} | {"=".join(s) for s in QUERY_SETTINGS[1:]}
    for setting, q in got["queries"].items():
        assert set(q) == set(want["queries"][setting])
        for name, table in q.items():
            rec = want["queries"][setting][name]
            rows, rec_rows = (table, rec) if isinstance(table, dict) and isinstance(rec, dict) else ({"": table}, {"": rec})
            wrong = [(key, row, rec_rows.get(key)) for key, row in rows.items() if row != rec_rows.get(key)]
            assert not wrong and len(rows) == len(rec_rows), f"{setting or 'unswitched'} {name} (row, now, recorded): {wrong[:2]}"
    assert got["layer_workspace_bytes"] == want["layer_workspace_bytes"]
    sizes = got["layer_workspace_bytes"]
    assert all(0 < a <= b for per in sizes.values() for a, b in per.values())
    assert all(sizes[""] != sizes[s] for s in sizes if s)                      # every path switch moves at least one layout
    # the switches act where they are meant to: each path switch on its own tables, the chunk switch on no query
    changed = {setting: {name for name, table in q.items() if table != AS_UNSWITCHED} for setting, q in got["queries"].items() if setting}
    assert changed == {"NGPDE_NO_GNO_MFMA=1": {"message_supported"}, "NGPDE_NO_GNO_GFORM=1": {"gform_supported", "gform_preferred"},
                       "NGPDE_GNO_MATERIALIZE=1": set(), "NGPDE_GNO_GFORM_CHUNK=16": set(), "NGPDE_GNO_GFORM_CHUNK=32": set(),
                       "NGPDE_GNO_GFORM_CHUNK=7": set()}
