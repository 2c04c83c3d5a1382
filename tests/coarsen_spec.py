"""Numpy restatements of the coarsening block's rules (include/ngpde_coarsen.h), written from the header's words and sharing no code
with the library: what tests/test_coarsen_gpu.py holds the device results to."""
import numpy as np

F = np.float32
TILE_MAX_POINTS = 16384
TILE_THREADS = 1024


def d2_to(p, q):
    """the float rule: the sum over the coordinates, in order, of (p - q)^2, every operation rounded to float32; p [n][dim], q [dim]"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        dx = (p[:, 0] - q[0]).astype(F)
        s = (dx * dx).astype(F)
        for c in range(1, p.shape[1]):
            dc = (p[:, c] - q[c]).astype(F)
            s = (s + (dc * dc).astype(F)).astype(F)
    return s


def fps_graph(p, k, start=0, ties=None):
    """one graph: p float32 [n][dim]; (idx int32 [k], d2 float32 [k]).  ties: a list that receives, per round, how many unselected points
    attain the round's maximum"""
    p = np.ascontiguousarray(p, dtype=F)
    n = len(p)
    key = np.full(n, np.inf, dtype=F)
    idx, d2 = np.zeros(k, np.int32), np.zeros(k, F)
    for r in range(k):
        if r == 0:
            s = int(start)
        else:
            s = int(np.argmax(key))                     # the first of the largest keys: equal keys go to the smallest index
            if ties is not None:
                ties.append(int(np.sum(key == key[s])))
        idx[r], d2[r] = s, key[s]
        if r + 1 < k:
            live = key >= 0
            key[live] = np.minimum(key[live], d2_to(p[live], p[s]))
            key[s] = F(-1)
    return idx, d2


def fps_brute(points, ptr, ks, starts=None):
    """a batch: points [n][dim], ptr [G + 1], ks [G], starts global positions [G] or None; graphs concatenated"""
    idx, d2 = [], []
    for g in range(len(ptr) - 1):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        if ks[g] == 0:
            continue
        s = 0 if starts is None else int(starts[g]) - lo
        i, d = fps_graph(points[lo:hi], int(ks[g]), s)
        idx.append(i + lo)
        d2.append(d)
    if not idx:
        return np.zeros(0, np.int32), np.zeros(0, F)
    return np.concatenate(idx).astype(np.int32), np.concatenate(d2).astype(F)


def bits_holding(top):
    return int(top).bit_length()


def grid_cluster_brute(points, size, ptr, origin=None):
    """points float32 [n][dim]; size [dim]; ptr [G + 1]; origin [dim] or None (every graph's own minimum).  A dict of labels, count, ptr,
    order, graph_indicator (1-based) -- or a string naming the refusal"""
    p = np.ascontiguousarray(points, dtype=F)
    n, dim = p.shape
    size = np.broadcast_to(np.asarray(size, dtype=F), (dim,))
    G = len(ptr) - 1
    graph = np.repeat(np.arange(G), np.diff(ptr))
    if not np.isfinite(p).all():
        return "non-finite"
    cells = np.zeros((n, dim), np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(G):
            lo, hi = int(ptr[g]), int(ptr[g + 1])
            if lo == hi:
                continue
            o = p[lo:hi].min(axis=0) if origin is None else np.asarray(origin, dtype=F)
            q = np.floor(((p[lo:hi] - o).astype(F) / size).astype(F))
            if (q < 0).any():
                return "below"
            if not (q < 2147483648.0).all():
                return "too small"
            cells[lo:hi] = q.astype(np.int64)
    bits = sum(bits_holding(cells[:, c].max(initial=0)) for c in range(dim)) + bits_holding(G - 1)
    if bits > 63:
        return "too small"
    keys = [tuple([int(graph[i])] + [int(cells[i, c]) for c in reversed(range(dim))]) for i in range(n)]      # (graph, c_z, c_y, c_x)
    uniq = sorted(set(keys))
    number = {k: j for j, k in enumerate(uniq)}
    labels = np.array([number[k] for k in keys], dtype=np.int32)
    order = np.argsort(labels, kind="stable").astype(np.int32)
    counts = np.bincount(labels, minlength=len(uniq))
    return dict(labels=labels, count=len(uniq), ptr=np.concatenate(([0], np.cumsum(counts))).astype(np.int32), order=order,
                graph_indicator=np.array([k[0] + 1 for k in uniq], dtype=np.int32))


def pool_ref(x, labels, count, aggr):
    """x [N][D] float32, float64 arithmetic: (out [count][D] float64, sum of |x| per entry [count][D], sizes [count])"""
    x64 = np.asarray(x, dtype=np.float64)
    d = x64.shape[1]
    out = np.zeros((count, d))
    mag = np.zeros((count, d))
    sizes = np.bincount(labels, minlength=count)
    if aggr in ("+", "mean"):
        np.add.at(out, labels, x64)
        np.add.at(mag, labels, np.abs(x64))
        if aggr == "mean":
            out = out / sizes[:, None]
            mag = mag / sizes[:, None]
    else:
        out[:] = -np.inf if aggr == "max" else np.inf
        (np.maximum if aggr == "max" else np.minimum).at(out, labels, x64)
    return out, mag, sizes


def pool_backward_ref(x, out, dout, labels, sizes, aggr):
    """the header's pullback in float32: dx [N][D]"""
    g = np.asarray(dout, dtype=F)[labels]
    if aggr == "mean":
        return (g / sizes[labels].astype(F)[:, None]).astype(F)
    if aggr in ("max", "min"):
        return np.where(np.asarray(x, dtype=F) == np.asarray(out, dtype=F)[labels], g, F(0)).astype(F)
    return g


def pool_graph_ref(s, t, w, labels, count):
    """relabel, drop loops, unique (s, t) by source then target with summed weights (float64)"""
    cs, ct = labels[s], labels[t]
    keep = cs != ct
    cs, ct, w = cs[keep], ct[keep], np.asarray(w, dtype=np.float64)[keep]
    code = cs.astype(np.int64) * count + ct
    uniq, inv = np.unique(code, return_inverse=True)
    ws = np.zeros(len(uniq))
    np.add.at(ws, inv, w)
    return (uniq // count).astype(np.int64), (uniq % count).astype(np.int64), ws
