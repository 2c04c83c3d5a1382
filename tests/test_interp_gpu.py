"""Two-set search and k-NN interpolation on the device (include/ngpde_interp.h, ngpde_amd.interp) against the numpy restatements of
tests/interp_spec.py.

Search: idx, d2, ptr and nbr equal the float32 brute-force lists BIT FOR BIT (no tolerance) over dims 1-3, k in {1, 3, 8, 128},
N in {k, 200}, M in {1, 63, 64, 65, 130}, and in the named regimes -- queries outside the data's box (some more than 100 cells away),
empty rings, ties cut by k, coincident points, batches (with the refusal that names the short graph) and the radius limits -- each
of which asserts its regime on the reference before the device output is looked at.

Interpolation: the float64 reference takes the LIBRARY's float32 idx and d2.  Forward, D in {1, 3, 64, 65, 130}:
    |y - ref| <= (2k + 4) 2^-24 max_j |x[idx_j]|          per entry
(one rounding per weight, one per product, k - 1 per sum in two sums, one division; the weights are positive, so W has no
cancellation; two units for second-order terms).  Pullback:
    |xbar_i - ref| <= (T_i + 2k + 4) 2^-24 sum |w ybar| + T_i 2^-126 max |ybar|,    T_i = the slots of point i, counted here
(the second term covers normalised weights in the denormal range, which occur beside a coincident point).  The inputs have points no
query names (their rows must be exactly 0 in an output pre-filled with NaN) and a point named by >= 64 queries.
Reached on the MI355X (every run prints its own): the forward at most 0.27 of its bound (k = 3, d = 65), the pullback at most 0.25
(k = 3, d = 130; max T = 73 and 75, 89 and 22 untouched points for k = 3 and 8).

Also: the same inputs give the same bits twice; torch.autograd through itp(x) equals the C entry; forward + backward captured into
one HIP graph replay to the eager bits; every stream-taking entry of the header runs on a side stream behind still-running
producer work (the method of tests/test_streams_gpu.py: stale NaN / zero inputs that the side stream overwrites behind a delay, a
deliberately mis-streamed control first) and equals the NULL-stream result bitwise; every array argument of the four public
functions is swept over float64, bfloat16 (exact values), stride 2, offset 1 and numpy input with equal outputs.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib

import interp_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
I = ng.interp
U = 2.0 ** -24



def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def search_both(pts, qs, k, r, gp=None, gq=None):
    """the device's (idx, d2, ptr, nbr) in the C layouts, through the Python entries; points / queries are [n][dim] here"""
    kw = {} if gp is None else dict(graph_indicator=dev(gp), query_graph_indicator=dev(gq))
    idx, d2 = I.knn(dev(pts).T, dev(qs).T, k, **kw)
    al = I.inrange(dev(pts).T, dev(qs).T, r, **kw)
    assert al.eid is None and len(al) == len(qs)
    return host(idx.T), host(d2.T), host(al.ptr), host(al.neighbors)


def assert_search(pts, qs, k, r, gp=None, gq=None, ref=None):
    want_idx, want_d2 = ref or S.knn_brute(pts, qs, k, gp, gq)
    want_ptr, want_nbr = S.radius_brute(pts, qs, r, gp, gq)
    idx, d2, ptr, nbr = search_both(pts, qs, k, r, gp, gq)
    assert same_bits(idx, want_idx), np.argwhere(idx != want_idx)[:5]
    assert same_bits(d2, want_d2), np.argwhere(d2 != want_d2)[:5]
    assert same_bits(ptr, want_ptr) and same_bits(nbr, want_nbr)
    return want_idx, want_d2, want_ptr, want_nbr


# ---- search: the sweep ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8, 128])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_search_equals_brute_force_across_sizes(dim, k):
    rng = np.random.default_rng(100 * dim + k)
    for n in (k, 200):
        pts = rng.random((n, dim)).astype(np.float32)
        for m in (1, 63, 64, 65, 130):
            qs = (rng.random((m, dim)) * 1.5 - 0.25).astype(np.float32)          # a third outside the box
            qs[0] = 0.5
            r = float(np.sqrt(S.dist2(pts, qs[:1]))[0].min()) * 1.5 + 0.05       # query 0 has a hit, and not every pair is one
            idx, d2, ptr, nbr = assert_search(pts, qs, k, r)
            assert idx.shape == (m, k) and ptr[-1] > 0 and (n * m < 1000 or ptr[-1] < n * m) and len(np.unique(idx[0])) == k


# ---- search: the named regimes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_queries_outside_the_box(dim):
    rng = np.random.default_rng(7 + dim)
    n, m, k, r = 200, 64, 3, 0.3
    pts = rng.random((n, dim)).astype(np.float32)
    qs = rng.random((m, dim)).astype(np.float32)
    out = np.arange(m) % 4 == 0                                                   # a quarter outside, on every side in turn
    for j in np.flatnonzero(out):
        side = (j // 4) % (2 * dim)
        qs[j, side // 2] = -0.2 - rng.random() if side % 2 == 0 else 1.2 + rng.random()
    qs[4] = -1e4                                                                  # far: a cell is at most twice the box's extent
    qs[8] = 1e4
    lo, hi = pts.min(0), pts.max(0)
    outside = ((qs < lo) | (qs > hi)).any(1)
    assert outside.sum() >= m // 4 and all(((qs[:, d] < lo[d]).any() and (qs[:, d] > hi[d]).any()) for d in range(dim))
    assert np.abs(qs[4] - lo).min() > 100 * 2 * (hi - lo).max()
    idx, d2, ptr, nbr = assert_search(pts, qs, k, r)
    assert ptr[5] == ptr[4] and ptr[-1] > 0 and np.isfinite(d2).all()             # the far query's row is empty, others are not
    # and at magnitudes where the far squares overflow: distances of inf, ordered by index
    qs[8] = 3e19
    idx, d2, ptr, nbr = assert_search(pts, qs, k, r)
    assert np.isinf(d2[8]).all() and idx[8].tolist() == [0, 1, 2]


def test_empty_rings_between_the_queries_and_the_cluster():
    rng = np.random.default_rng(3)
    k = 8
    near = 1.0 - rng.random((3, 2)) * 0.05                                        # three points in the queries' corner
    cluster = rng.random((197, 2)) * 0.05                                         # everything else in the opposite corner
    pts = np.concatenate([cluster, near]).astype(np.float32)
    qs = (1.0 - rng.random((40, 2)) * 0.1).astype(np.float32)
    ref = S.knn_brute(pts, qs, k)
    cell = np.sqrt(0.5 * k / len(pts))                                            # the k-NN grid's edge on the unit box (knn_want)
    assert (ref[1][:, 2] < (2 * cell) ** 2).all() and (ref[1][:, 3] > (5 * cell) ** 2).all()   # 3 within 2 cells, the 4th beyond 5
    assert_search(pts, qs, k, 0.2, ref=ref)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_ties_are_cut_by_index(k):
    g = np.arange(5) * 0.25
    pts = np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    c = np.arange(4) * 0.25 + 0.125
    qs = np.stack(np.meshgrid(c, c, indexing="ij"), -1).reshape(-1, 2).astype(np.float32)
    full = np.sort(S.dist2(pts, qs), axis=1)
    assert len(qs) == 16 and (full[:, 2] == full[:, 3]).all() and (full[:, 0] == full[:, 3]).all()
    assert full[0, 0] < np.float32(0.18) * np.float32(0.18) < full[0, 4]
    idx, d2, ptr, nbr = assert_search(pts[::-1].copy(), qs, k, 0.18)               # (reversed: index order is not scan order)
    assert (np.diff(idx, axis=1) > 0).all() and (ptr[1:] - ptr[:-1] == 4).all()    # the four tied corners, ascending by index


def test_coincident_points():
    rng = np.random.default_rng(5)
    pts = rng.random((200, 3)).astype(np.float32)
    pts[50:60] = pts[40:50]                                                       # coincident data points as well
    qs = pts[30:95].copy()
    ref = S.knn_brute(pts, qs, 3)
    assert (ref[1][:, 0] == 0).all() and (ref[1][10:20, 1] == 0).all() and (ref[1][:, 2] > 0).all()
    idx, d2, ptr, nbr = assert_search(pts, qs, 3, 0.0, ref=ref)                    # r = 0 with coincident pairs
    assert ptr[-1] == 65 + 2 * 10 and idx[10].tolist()[:2] == [40, 50]


def batch_sets(k, short_by):
    rng = np.random.default_rng(11)
    sizes = (40, 30, k - short_by)                                                # graph 3 holds k - short_by points
    gp = np.repeat([1, 2, 3], sizes)
    gq = np.repeat([1, 3], (50, 20))                                              # graph 2 has points and no queries
    perm_p, perm_q = rng.permutation(len(gp)), rng.permutation(len(gq))           # members interleaved, not block by block
    gp, gq = gp[perm_p], gq[perm_q]
    pts = rng.random((len(gp), 2)).astype(np.float32)
    qs = (rng.random((len(gq), 2)) * 1.2 - 0.1).astype(np.float32)
    return pts, qs, gp.astype(np.int64), gq.astype(np.int64)


def test_batches_search_inside_their_own_graph():
    k = 5
    pts, qs, gp, gq = batch_sets(k, 0)
    idx, d2, ptr, nbr = assert_search(pts, qs, k, 0.25, gp, gq)
    assert (gp[idx] == gq[:, None]).all() and (gp == 2).any() and not (gq == 2).any() and ptr[-1] > 0
    plain = S.knn_brute(pts, qs, k)[0]
    assert (plain != idx).any()                                                   # the indicators matter on these inputs


def test_a_graph_one_point_short_is_refused_by_name():
    k = 5
    pts, qs, gp, gq = batch_sets(k, 1)
    with pytest.raises(ValueError, match="fewer than k = 5"):
        S.knn_brute(pts, qs, k, gp, gq)
    with pytest.raises(ng.ArgumentError, match=r"graph 3 has queries and 4 points, fewer than k = 5"):
        I.knn(dev(pts).T, dev(qs).T, k, graph_indicator=dev(gp), query_graph_indicator=dev(gq))
    # a graph with queries and no points: refused for k-NN, empty rows for the radius search
    gq2 = gq.copy()
    gq2[:3] = 4
    with pytest.raises(ng.ArgumentError, match=r"graph 4 has queries and 0 points"):
        I.knn(dev(pts).T, dev(qs).T, 2, graph_indicator=dev(gp), query_graph_indicator=dev(gq2))
    want_ptr, want_nbr = S.radius_brute(pts, qs, 0.3, gp, gq2)
    assert (want_ptr[1:4] == want_ptr[0:3]).all() and want_ptr[-1] > 0
    al = I.inrange(dev(pts).T, dev(qs).T, 0.3, graph_indicator=dev(gp), query_graph_indicator=dev(gq2))
    assert same_bits(host(al.ptr), want_ptr) and same_bits(host(al.neighbors), want_nbr)


def test_radius_limits():
    rng = np.random.default_rng(13)
    pts = rng.random((150, 2)).astype(np.float32)
    qs = rng.random((65, 2)).astype(np.float32)
    qs[3] = (5.0, 5.0)                                                            # no hit within 0.2
    want = S.radius_brute(pts, qs, 0.2)
    assert want[0][4] == want[0][3] and want[0][1] > want[0][0]
    al = I.inrange(dev(pts).T, dev(qs).T, 0.2)
    assert same_bits(host(al.ptr), want[0]) and same_bits(host(al.neighbors), want[1]) and al[3].numel() == 0
    al = I.inrange(dev(pts).T, dev(qs).T, float("inf"))                           # r = inf: every point, ascending
    assert host(al.ptr).tolist() == list(range(0, 150 * 65 + 1, 150)) and al[64].tolist() == list(range(150))
    # capacity one short: refused, and nothing is written
    lib = _lib.load()
    p, q = dev(pts), dev(qs)
    total = int(want[0][-1])
    found = C.c_int64(0)
    args = (150, 65, 2, _lib.ptr(p), _lib.ptr(q), 0.2, None, None, 1, 1, 0)
    assert lib.ngpde_radius_query(*args, 0, None, None, C.byref(found), None) == 0 and found.value == total
    ptr = torch.full((66,), -7, dtype=torch.int32, device=DEV)
    nbr = torch.full((total + 64,), -7, dtype=torch.int32, device=DEV)
    st = lib.ngpde_radius_query(*args, total - 1, _lib.ptr(ptr), _lib.ptr(nbr), C.byref(found), None)
    assert st == _lib.ERR_INVALID_ARGUMENT and f"{total} pairs, the output array holds {total - 1}" in lib.ngpde_last_error().decode()
    torch.cuda.synchronize()
    assert (nbr == -7).all() and (ptr == -7).all()
    assert lib.ngpde_radius_query(*args, total, _lib.ptr(ptr), _lib.ptr(nbr), C.byref(found), None) == 0
    assert same_bits(host(nbr[:total]), want[1]) and (nbr[total:] == -7).all() and same_bits(host(ptr), want[0])


# ---- interpolation ---------------------------------------------------------------------------------------------------------------------
def interp_sets(k, seed=21):
    """200 points, 130 queries in 2-D: 70 queries crowd outside one corner (they name the same k points: a hub), the rest are
    spread over the box; query 0 coincides with a data point"""
    rng = np.random.default_rng(seed)
    pts = rng.random((200, 2)).astype(np.float32)
    qs = np.concatenate([2.0 + 0.01 * rng.random((70, 2)), rng.random((60, 2))]).astype(np.float32)
    qs[100] = pts[17]
    return pts, qs


@pytest.fixture(scope="module", params=[3, 8])
def fitted(request):
    k = request.param
    pts, qs = interp_sets(k)
    itp = I.KNNInterpolator(dev(pts).T, dev(qs).T, k)
    idx, d2, w = host(itp.idx.T), host(itp.d2.T), host(itp.weights.T)
    want = S.knn_brute(pts, qs, k)
    assert same_bits(idx, want[0]) and same_bits(d2, want[1])
    T = np.bincount(idx.reshape(-1), minlength=len(pts))
    assert (T == 0).any() and T.max() >= 64 and d2[100, 0] == 0 and (d2[100, 1:] > 0).all()
    w64 = S.interp_weights(d2, np.float64)
    assert np.abs(w - w64).max() <= (k + 2) * U and np.abs(w.sum(1) - 1).max() <= (k + 2) * U
    assert 0 < w[100, 1] < 2.0 ** -100                                            # beside the coincident point: tiny normalised weights
    return dict(k=k, n=len(pts), m=len(qs), itp=itp, idx=idx, d2=d2, w=w, w64=w64, T=T, pts=pts, qs=qs)


@pytest.mark.parametrize("d", [1, 3, 64, 65, 130])
def test_forward_within_the_rounding_bound(fitted, d):
    f = fitted
    rng = np.random.default_rng(d)
    x = rng.standard_normal((f["n"], d)).astype(np.float32)
    ref = S.interp_forward(f["idx"], f["w64"], x, np.float64)
    y = host(f["itp"](dev(x).T).T)
    assert y.shape == ref.shape and y.dtype == np.float32
    bound = (2 * f["k"] + 4) * U * np.abs(x[f["idx"]]).max(1)
    factor = float((np.abs(y - ref) / bound).max())
    print(f"forward k={f['k']} d={d}: |y - ref| reaches {factor:.3f} of the bound")
    assert factor <= 1.0
    again = host(f["itp"](dev(x).T).T)
    assert same_bits(y, again)


@pytest.mark.parametrize("d", [1, 3, 64, 65, 130])
def test_pullback_within_the_rounding_bound(fitted, d):
    f = fitted
    lib = _lib.load()
    k, n, m, T = f["k"], f["n"], f["m"], f["T"]
    rng = np.random.default_rng(50 + d)
    ybar = rng.standard_normal((m, d)).astype(np.float32)
    ref = S.interp_backward(f["idx"], f["w64"], ybar, n, np.float64)
    mag = np.zeros((n, d))
    np.add.at(mag, f["idx"].reshape(-1), np.abs(f["w64"].reshape(-1, 1) * np.repeat(ybar.astype(np.float64), k, axis=0)))
    bound = (T[:, None] + 2 * k + 4) * U * mag + T[:, None] * 2.0 ** -126 * np.abs(ybar).max()
    ptr, slot = f["itp"].transpose()
    want_rows = S.transpose_rows(f["idx"], n)
    assert same_bits(host(ptr), want_rows[0]) and same_bits(host(slot), want_rows[1])
    xbar = torch.full((n, d), float("nan"), dtype=torch.float32, device=DEV)
    yb = dev(ybar)
    assert lib.ngpde_knn_interp_backward(n, m, k, d, _lib.ptr(ptr), _lib.ptr(slot), _lib.ptr(f["itp"]._w), _lib.ptr(yb), _lib.ptr(xbar),
                                         _lib.current_stream()) == 0
    got = host(xbar)
    assert (got[T == 0] == 0).all() and not np.isnan(got).any()
    touched = T > 0
    factor = float((np.abs(got - ref)[touched] / bound[touched]).max())
    print(f"pullback k={k} d={d}: |xbar - ref| reaches {factor:.3f} of the bound (max T = {T.max()}, {int((T == 0).sum())} untouched)")
    assert factor <= 1.0
    # torch.autograd through itp(x) is the same launch
    x = torch.zeros((d, n), dtype=torch.float32, device=DEV, requires_grad=True)
    f["itp"](x).backward(yb.T)
    assert same_bits(host(x.grad.T), got)


def test_the_same_inputs_give_the_same_bits(fitted):
    f = fitted
    other = I.KNNInterpolator(dev(f["pts"]).T, dev(f["qs"]).T, f["k"])
    for a, b in ((other.idx, f["itp"].idx), (other.d2, f["itp"].d2), (other.weights, f["itp"].weights)):
        assert same_bits(host(a), host(b))
    rows = other.matrix_rows()
    assert rows[0] is other.idx and rows[1] is other.weights and tuple(rows[1].shape) == (f["k"], f["m"])
    x = dev(np.random.default_rng(1).standard_normal((7, f["n"])).astype(np.float32))
    assert same_bits(host(other(x)), host(f["itp"](x)))
    assert same_bits(host(I.knn_interpolate(x, dev(f["pts"]).T, dev(f["qs"]).T, f["k"])), host(f["itp"](x)))


def test_forward_and_backward_replay_from_one_hip_graph(fitted):
    f = fitted
    lib = _lib.load()
    k, n, m, d = f["k"], f["n"], f["m"], 33
    itp = f["itp"]
    ptr, slot = itp.transpose()                                                   # built ahead of the capture: it allocates
    rng = np.random.default_rng(9)
    x, ybar = dev(rng.standard_normal((n, d)).astype(np.float32)), dev(rng.standard_normal((m, d)).astype(np.float32))
    y, xbar = torch.empty((m, d), device=DEV), torch.empty((n, d), device=DEV)

    def both():
        s = _lib.current_stream()
        assert lib.ngpde_knn_interp_weights(m, k, _lib.ptr(itp._d2), _lib.ptr(w), s) == 0
        assert lib.ngpde_knn_interp_forward(n, m, k, d, _lib.ptr(itp._idx), _lib.ptr(w), _lib.ptr(x), _lib.ptr(y), s) == 0
        assert lib.ngpde_knn_interp_backward(n, m, k, d, _lib.ptr(ptr), _lib.ptr(slot), _lib.ptr(w), _lib.ptr(ybar), _lib.ptr(xbar), s) == 0

    w = torch.empty((m, k), device=DEV)
    both()
    torch.cuda.synchronize()
    eager = [host(t).copy() for t in (w, y, xbar)]
    assert same_bits(eager[0], f["w"])
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for t in (w, y, xbar):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for t, e in zip((w, y, xbar), eager):
        assert same_bits(host(t), e)


# ---- streams: every stream-taking entry behind still-running producer work ---------------------------------------------------------------
def header_stream_entries():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ngpde_interp.h")).read(), flags=re.S)
    return sorted(name for name, args in re.findall(r"\b(ngpde_[a-z0-9_]+)\s*\(([^)]*)\)", src) if "ngpde_stream_t" in args)


def stream_cases():
    """name -> (inputs, call): call(inputs, stream) runs the entry on `stream` and returns (statuses, outputs)"""
    lib = _lib.load()
    rng = np.random.default_rng(17)
    n, m, k, d, dim = 300, 200, 4, 48, 2
    pts, qs = rng.random((n, dim)).astype(np.float32), rng.random((m, dim)).astype(np.float32)
    gp, gq = (np.arange(n) % 2).astype(np.int32), (np.arange(m) % 2).astype(np.int32)          # 0-based ids: zeros are valid too
    idx, d2 = S.knn_brute(pts, qs, k, gp, gq)
    w = S.interp_weights(d2)
    ptr, slot = S.transpose_rows(idx, n)
    x, ybar = rng.standard_normal((n, d)).astype(np.float32), rng.standard_normal((m, d)).astype(np.float32)
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=DEV)
    f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=DEV)
    P = _lib.ptr

    def knn_query(a, s):
        oi, od = i32(m, k), f32(m, k)
        return [lib.ngpde_knn_query(n, m, dim, P(a["pts"]), P(a["qs"]), k, P(a["gp"]), P(a["gq"]), 2, 0, 0, P(oi), P(od), s)], [oi, od]

    def radius_query(a, s):
        found = C.c_int64(0)
        head = (n, m, dim, P(a["pts"]), P(a["qs"]), 0.1, P(a["gp"]), P(a["gq"]), 2, 0, 0)
        cap = int(S.radius_brute(pts, qs, 0.1, gp, gq)[0][-1])
        op, on = i32(m + 1), i32(cap)
        st = [lib.ngpde_radius_query(*head, 0, None, None, C.byref(found), s)]
        counted = found.value
        st.append(lib.ngpde_radius_query(*head, cap, P(op), P(on), C.byref(found), s))
        return st, [op, on, torch.tensor([counted, found.value])]

    def weights(a, s):
        o = f32(m, k)
        return [lib.ngpde_knn_interp_weights(m, k, P(a["d2"]), P(o), s)], [o]

    def forward(a, s):
        o = f32(m, d)
        return [lib.ngpde_knn_interp_forward(n, m, k, d, P(a["idx"]), P(a["w"]), P(a["x"]), P(o), s)], [o]

    def transpose(a, s):
        nbytes = lib.ngpde_knn_interp_transpose_workspace_bytes(n, m, k)
        ws, op, os_ = torch.empty(nbytes, dtype=torch.uint8, device=DEV), i32(n + 1), i32(m * k)
        return [lib.ngpde_knn_interp_transpose(n, m, k, P(a["idx"]), P(op), P(os_), P(ws), nbytes, s)], [op, os_]

    def backward(a, s):
        o = f32(n, d)
        return [lib.ngpde_knn_interp_backward(n, m, k, d, P(a["ptr"]), P(a["slot"]), P(a["w"]), P(a["ybar"]), P(o), s)], [o]

    sets = dict(pts=pts, qs=qs, gp=gp, gq=gq)
    return {
        "ngpde_knn_query": (sets, knn_query),
        "ngpde_radius_query": (sets, radius_query),
        "ngpde_knn_interp_weights": (dict(d2=d2), weights),
        "ngpde_knn_interp_forward": (dict(idx=idx, w=w, x=x), forward),
        "ngpde_knn_interp_transpose": (dict(idx=idx), transpose),
        "ngpde_knn_interp_backward": (dict(ptr=ptr, slot=slot, w=w, ybar=ybar), backward),
    }


CASES = None


def case(name):
    global CASES
    if CASES is None:
        CASES = stream_cases()
    return CASES[name]


class Side:
    """a side stream that does not run in order with the NULL stream, and a calibrated delay (torch.cuda._sleep)"""

    def __init__(self):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(20_000_000)
        b.record()
        torch.cuda.synchronize()
        self.cycles_per_ms = 20_000_000 / a.elapsed_time(b)
        assert 1e3 < self.cycles_per_ms < 1e8
        self.stream = None

    def run(self, inputs, call, stream, ms=20.0):
        """the inputs arrive on the side stream behind a delay, in buffers that hold NaN / zeros until then; `call` gets `stream`"""
        real = {k: dev(v) for k, v in inputs.items()}
        stale = {k: (torch.full_like(v, float("nan")) if v.is_floating_point() else torch.zeros_like(v)) for k, v in real.items()}
        torch.cuda.synchronize()
        with torch.cuda.stream(self.stream):
            torch.cuda._sleep(int(ms * self.cycles_per_ms))
            for k in stale:
                stale[k].copy_(real[k])
            st, out = call(stale, self.stream.cuda_stream if stream == "side" else None)
        self.stream.synchronize()
        torch.cuda.synchronize()
        return st, [host(o).copy() for o in out]


def expected(name):
    inputs, call = case(name)
    st, out = call({k: dev(v) for k, v in inputs.items()}, None)
    torch.cuda.synchronize()
    assert st == [0] * len(st), (name, _lib.load().ngpde_last_error())
    return [host(o).copy() for o in out]


@pytest.fixture(scope="module")
def side():
    """the control: ONE deliberately mis-streamed call (stream = NULL while its inputs arrive on the side stream) must differ from the
    expected result; up to 8 streams are tried for one that does not share the NULL stream's order"""
    s = Side()
    name = "ngpde_knn_interp_weights"
    want = expected(name)
    for _ in range(8):
        s.stream = torch.cuda.Stream()
        st, got = s.run(*case(name), stream="null")
        if not all(same_bits(g, w) for g, w in zip(got, want)):
            return s
    pytest.fail("no side stream out of order with the NULL stream: the stream cases could not fail")


def test_the_stream_cases_cover_the_header():
    assert sorted(stream_cases()) == header_stream_entries() and len(header_stream_entries()) == 6


@pytest.mark.parametrize("name", ["ngpde_knn_query", "ngpde_radius_query", "ngpde_knn_interp_weights", "ngpde_knn_interp_forward",
                                  "ngpde_knn_interp_transpose", "ngpde_knn_interp_backward"])
def test_entry_runs_on_the_stream_it_is_given(side, name):
    want = expected(name)
    st, got = side.run(*case(name), stream="side")
    assert st == [0] * len(st), (name, _lib.load().ngpde_last_error())
    assert len(got) == len(want) and all(same_bits(g, w) for g, w in zip(got, want)), name


# ---- every array argument over dtype, stride, offset and numpy ------------------------------------------------------------------------------
def variants(t):
    """the same values as float64, bfloat16, with stride 2, at storage offset 1 and as a numpy array"""
    assert torch.equal(t.to(torch.bfloat16).to(t.dtype), t), "the sweep's values must be exact in bfloat16"
    wide = torch.zeros(t.shape[:-1] + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    flat[1:] = t.reshape(-1)
    shifted = flat[1:].view(t.shape)
    assert wide[..., ::2].stride(-1) == 2 and shifted.storage_offset() == 1
    return {"float64": t.double(), "bfloat16": t.to(torch.bfloat16), "stride 2": wide[..., ::2], "offset 1": shifted,
            "numpy": t.cpu().numpy()}


def sweep_inputs():
    rng = np.random.default_rng(23)
    n, m = 40, 33
    pts = torch.as_tensor(rng.integers(0, 16, (2, n)) / 8.0, dtype=torch.float32, device=DEV)       # eighths: exact in bfloat16
    qs = torch.as_tensor(rng.integers(-4, 20, (2, m)) / 8.0, dtype=torch.float32, device=DEV)
    gp = torch.as_tensor(np.arange(n) % 2 + 1, dtype=torch.int64, device=DEV)
    gq = torch.as_tensor(np.arange(m) % 2 + 1, dtype=torch.int64, device=DEV)
    x = torch.as_tensor(rng.integers(-8, 9, (5, n)) / 4.0, dtype=torch.float32, device=DEV)
    return dict(points=pts, queries=qs, graph_indicator=gp, query_graph_indicator=gq, x=x)


def outputs_of(fn, a):
    kw = dict(graph_indicator=a["graph_indicator"], query_graph_indicator=a["query_graph_indicator"])
    if fn == "knn":
        return list(I.knn(a["points"], a["queries"], 3, **kw))
    if fn == "inrange":
        al = I.inrange(a["points"], a["queries"], 0.5, **kw)
        return [al.ptr, al.neighbors]
    if fn == "KNNInterpolator":
        itp = I.KNNInterpolator(a["points"], a["queries"], 3, **kw)
        return [itp.idx, itp.weights, itp(a["x"])]
    return [I.knn_interpolate(a["x"], a["points"], a["queries"], 3, **kw)]


@pytest.mark.parametrize("fn", ["knn", "inrange", "KNNInterpolator", "knn_interpolate"])
def test_every_array_argument_in_every_form(fn):
    base = sweep_inputs()
    want = outputs_of(fn, base)
    assert all(w.numel() > 0 for w in want)
    names = [k for k in base if k != "x" or fn in ("KNNInterpolator", "knn_interpolate")]
    for name in names:
        for form, value in variants(base[name]).items():
            got = outputs_of(fn, dict(base, **{name: value}))
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and torch.equal(g, w), (fn, name, form)
