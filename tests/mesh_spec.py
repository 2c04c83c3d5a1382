"""The Delaunay rule of include/ngpde_mesh.h restated in numpy, float64, by brute force over all pairs (O(N^3), N <= 150), the
triangles read off its rows, the margin that says how far a triangulation's decisions are from a tie, and the max_edge_length
filter in float32.  tests/test_mesh_host.py checks these against Qhull and against lattices; tests/test_mesh_gpu.py holds the
device to them.
"""
import numpy as np

TIE_BOUND = 12.0 * 2.0 ** -53          # NGPDE_DELAUNAY_TIE_BOUND
SPEC_TIE = 1e-12                       # the restatement's own tie tolerance, relative


def edges_brute(points, tol=SPEC_TIE):
    """points float32 [n][2].  i ~ j iff the part of their bisector that is no nearer to any third point is not empty: the
    bisector is q / 2 + t perp(q) with q = p_j - p_i, and a point k allows t * c <= b with c = perp(q) . q_k and
    b = (|q_k|^2 - q . q_k) / 2.  Returns the sorted set of directed pairs (i, j) as an int array [E][2]."""
    p = np.asarray(points, np.float32).astype(np.float64)
    n = len(p)
    out = []
    for i in range(n):
        q = p - p[i]                                                   # [n][2]
        n2 = (q * q).sum(1)
        c = -q[:, 1:2] * q[None, :, 0] + q[:, 0:1] * q[None, :, 1]     # [j][k]
        b = 0.5 * (n2[None, :] - q @ q.T)                              # [j][k]
        scale = np.sqrt(n2)[:, None] * np.sqrt(n2)[None, :]
        other = np.ones((n, n), bool)
        other[:, i] = False
        other[np.arange(n), np.arange(n)] = False
        flat = np.abs(c) <= tol * scale                                # k collinear with i and j
        blocked = (other & flat & (b < -tol * scale)).any(1)           # ... and between them
        with np.errstate(divide="ignore", invalid="ignore"):
            t = b / c
        hi = np.where(other & ~flat & (c > 0), t, np.inf).min(1)
        lo = np.where(other & ~flat & (c < 0), t, -np.inf).max(1)
        with np.errstate(invalid="ignore"):
            ok = ~blocked & ((lo <= hi) | (lo - hi <= tol * (1.0 + np.abs(lo) + np.abs(hi))))
        ok[i] = False
        out += [(i, j) for j in np.flatnonzero(ok)]
    return np.array(sorted(out), np.int64).reshape(-1, 2)


def rows_of(edges, n):
    rows = [[] for _ in range(n)]
    for i, j in np.asarray(edges).tolist():
        rows[i].append(j)
    return [sorted(r) for r in rows]


def triangles_from_rows(points, edges):
    """The header's rule: for an edge (i, j) with i < j, k is the neighbour of i that follows j counter-clockwise among those
    strictly left of i -> j; (i, j, k) is a triangle iff k > i and k is in j's row.  Sorted lexicographically."""
    p = np.asarray(points, np.float32).astype(np.float64)
    rows = rows_of(edges, len(p))
    sets = [set(r) for r in rows]
    cross = lambda a, b: a[0] * b[1] - a[1] * b[0]
    tri = []
    for i, row in enumerate(rows):
        for j in row:
            if j < i:
                continue
            qj = p[j] - p[i]
            best = None
            for k in row:
                qk = p[k] - p[i]
                if k == j or not cross(qj, qk) > 0:
                    continue
                if best is None or cross(qk, p[best] - p[i]) > 0:
                    best = k
            if best is not None and best > i and best in sets[j]:
                tri.append((i, j, best))
    return np.array(sorted(tri), np.int64).reshape(-1, 3)


def canonical_triangles(points, simplices):
    """a triangulation's simplices as the header writes them: smallest index first, counter-clockwise, sorted"""
    p = np.asarray(points, np.float32).astype(np.float64)
    out = []
    for a, b, c in np.asarray(simplices).tolist():
        if (p[b, 0] - p[a, 0]) * (p[c, 1] - p[a, 1]) - (p[b, 1] - p[a, 1]) * (p[c, 0] - p[a, 0]) < 0:
            b, c = c, b
        while a != min(a, b, c):
            a, b, c = b, c, a
        out.append((a, b, c))
    return np.array(sorted(out), np.int64).reshape(-1, 3)


def edges_of_simplices(simplices):
    s = np.asarray(simplices, np.int64)
    e = np.concatenate([s[:, [0, 1]], s[:, [1, 2]], s[:, [2, 0]]])
    e = np.concatenate([e, e[:, ::-1]])
    return np.unique(e, axis=0)


def min_margin(points, simplices):
    """The smallest normalised in-circle margin over the interior edges of a triangulation.  For an edge (a, b) between the
    triangles (a, b, c) and (b, a, d) and each of the four points as the origin o, with u, v, w the other three translated to o,
        D = |w|^2 (u x v) + |u|^2 (v x w) + |v|^2 (w x u),     margin = |D| / (|u||v||w| (|u| + |v| + |w|)),
    the quantity NGPDE_DELAUNAY_TIE_BOUND bounds.  A device decision on these points is outside its doubt zone when this is well
    above the bound."""
    p = np.asarray(points, np.float32).astype(np.float64)
    s = np.asarray(simplices, np.int64)
    opposite = {}
    for t in s.tolist():
        for r in range(3):
            a, b, c = t[r], t[(r + 1) % 3], t[(r + 2) % 3]
            opposite.setdefault((min(a, b), max(a, b)), []).append(c)
    quads = np.array([(a, b, cs[0], cs[1]) for (a, b), cs in opposite.items() if len(cs) == 2], np.int64)
    best = np.inf
    for o in range(4):
        rest = [k for k in range(4) if k != o]
        u, v, w = (p[quads[:, k]] - p[quads[:, o]] for k in rest)
        x = lambda a, b: a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
        nu, nv, nw = (np.sqrt((a * a).sum(1)) for a in (u, v, w))
        d = nw ** 2 * x(u, v) + nu ** 2 * x(v, w) + nv ** 2 * x(w, u)
        best = min(best, float((np.abs(d) / (nu * nv * nw * (nu + nv + nw))).min()))
    return best


def within(points, pairs, r):
    """the neighbour search's float32 rule: d2 = (dx*dx) + (dy*dy), every operation rounded to float32, d2 <= r*r"""
    p = np.asarray(points, np.float32)
    pairs = np.asarray(pairs, np.int64)
    d = p[pairs[:, 0]] - p[pairs[:, 1]]
    d2 = (np.float32(0) + d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]
    return d2 <= np.float32(r) * np.float32(r)


def filter_edges(points, edges, r):
    return np.asarray(edges)[within(points, edges, r)].reshape(-1, 2)


def filter_triangles(points, tri, r):
    tri = np.asarray(tri).reshape(-1, 3)
    keep = within(points, tri[:, [0, 1]], r) & within(points, tri[:, [1, 2]], r) & within(points, tri[:, [2, 0]], r)
    return tri[keep]


# ---- the clouds both test files use ------------------------------------------------------------------------------------------------
def cloud(kind, seed, n=150):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        p = rng.random((n, 2))
    elif kind == "clustered":
        centres = rng.random((6, 2))
        p = centres[rng.integers(0, 6, n)] + 0.04 * rng.standard_normal((n, 2))
    elif kind == "circle":            # n - 1 points on a circle and its centre, which every one of them is joined to
        a = np.sort(rng.random(n - 1)) * 2 * np.pi
        p = np.concatenate([np.stack([np.cos(a), np.sin(a)], 1), np.zeros((1, 2))])
    else:
        raise ValueError(kind)
    return p.astype(np.float32)


def lattice(nx, ny):
    return np.array([(x, y) for x in range(nx) for y in range(ny)], np.float32)


def stencil8(nx, ny):
    """the 8-neighbour stencil of the nx x ny lattice in lattice()'s numbering"""
    out = []
    for x in range(nx):
        for y in range(ny):
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    if (dx or dy) and 0 <= x + dx < nx and 0 <= y + dy < ny:
                        out.append((x * ny + y, (x + dx) * ny + y + dy))
    return np.array(sorted(out), np.int64)
