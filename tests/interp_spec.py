"""Numpy restatements of the two-set search and the k-NN interpolation (include/ngpde_interp.h), for tests/test_interp_host.py
(which pins them against plain Python loops) and tests/test_interp_gpu.py (which holds the device to them).  Imports numpy only.

Layouts are the C ABI's: points [n][dim], queries [m][dim], idx / d2 / w [m][k], x [n][d], y [m][d]; graph ids are plain integers
(any base, the same on both sides) or None; positions are 0-based.
"""
import numpy as np

FLT_MIN = np.float32(2.0 ** -126)


def dist2(points, queries):
    """[m][n] float32: the sum over the coordinates, in order, of (q - p)^2, every operation rounded to float32 (no FMA)"""
    p, q = np.asarray(points, np.float32), np.asarray(queries, np.float32)
    d2 = np.zeros((q.shape[0], p.shape[0]), np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for c in range(p.shape[1]):
            df = q[:, None, c] - p[None, :, c]
            d2 = d2 + df * df
    return d2


def _candidates(n, m, point_graph, query_graph):
    if point_graph is None and query_graph is None:
        return [np.arange(n)] * m
    gp = np.zeros(n, np.int64) if point_graph is None else np.asarray(point_graph).reshape(-1)
    gq = np.zeros(m, np.int64) if query_graph is None else np.asarray(query_graph).reshape(-1)
    return [np.flatnonzero(gp == g) for g in gq]


def knn_brute(points, queries, k, point_graph=None, query_graph=None):
    """(idx int32 [m][k], d2 float32 [m][k]): the k smallest (d2, index) pairs among the points of the query's graph, nearest
    first.  Raises ValueError naming the first query whose graph holds fewer than k points."""
    d2 = dist2(points, queries)
    m, n = d2.shape
    idx, out = np.zeros((m, k), np.int32), np.zeros((m, k), np.float32)
    for q, cand in enumerate(_candidates(n, m, point_graph, query_graph)):
        if cand.size < k:
            raise ValueError(f"query {q}: its graph holds {cand.size} points, fewer than k = {k}")
        order = cand[np.argsort(d2[q, cand], kind="stable")[:k]]      # stable: equal distances keep ascending index
        idx[q], out[q] = order, d2[q, order]
    return idx, out


def radius_brute(points, queries, r, point_graph=None, query_graph=None):
    """(ptr int32 [m + 1], nbr int32): rows by query, neighbours ascending; a pair is connected iff d2 <= r*r in float32"""
    d2 = dist2(points, queries)
    m, n = d2.shape
    with np.errstate(over="ignore", under="ignore"):
        r2 = np.float32(r) * np.float32(r)
    rows = [cand[d2[q, cand] <= r2] for q, cand in enumerate(_candidates(n, m, point_graph, query_graph))]
    ptr = np.zeros(m + 1, np.int32)
    ptr[1:] = np.cumsum([len(row) for row in rows])
    nbr = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return ptr, nbr


def interp_weights(d2, dtype=np.float32):
    """normalised weights [m][k] in `dtype` from float32 d2 (ascending per row): c_j = max(d2_j, FLT_MIN), w_j = c_0 / c_j (all 1
    where c_0 is inf), W = the sum in ascending j from 0; returns w_j / W"""
    d2 = np.asarray(d2, np.float32)
    c = np.maximum(d2, FLT_MIN).astype(dtype)
    with np.errstate(invalid="ignore", under="ignore"):
        w = c[:, :1] / c
    w[np.isinf(c[:, 0])] = 1
    W = np.zeros(d2.shape[0], dtype)
    for j in range(d2.shape[1]):
        W = W + w[:, j]
    with np.errstate(under="ignore"):
        return (w / W[:, None]).astype(dtype)


def interp_forward(idx, w, x, dtype=np.float32):
    """y [m][d] = sum_j w[q][j] * x[idx[q][j]] in ascending j from 0, products and sums rounded to `dtype`"""
    idx, w, x = np.asarray(idx), np.asarray(w, dtype), np.asarray(x, dtype)
    y = np.zeros((idx.shape[0], x.shape[1]), dtype)
    with np.errstate(under="ignore"):
        for j in range(idx.shape[1]):
            y = y + w[:, j:j + 1] * x[idx[:, j]]
    return y


def transpose_rows(idx, n):
    """(ptr [n + 1], slot [m * k]): slot[ptr[i] : ptr[i + 1]] are the positions q * k + j with idx[q][j] == i, ascending"""
    flat = np.asarray(idx).reshape(-1)
    slot = np.argsort(flat, kind="stable").astype(np.int32)
    ptr = np.searchsorted(flat[slot], np.arange(n + 1)).astype(np.int32)
    return ptr, slot


def interp_backward(idx, w, ybar, n, dtype=np.float32):
    """xbar [n][d]: xbar_i = the sum over the slots of point i, in ascending slot order from 0, of w[slot] * ybar[slot // k]"""
    idx, w, ybar = np.asarray(idx), np.asarray(w, dtype), np.asarray(ybar, dtype)
    k = idx.shape[1]
    ptr, slot = transpose_rows(idx, n)
    xbar = np.zeros((n, ybar.shape[1]), dtype)
    wf = w.reshape(-1)
    with np.errstate(under="ignore"):
        for i in range(n):
            acc = np.zeros(ybar.shape[1], dtype)
            for s in slot[ptr[i]:ptr[i + 1]]:
                acc = acc + wf[s] * ybar[s // k]
            xbar[i] = acc
    return xbar
