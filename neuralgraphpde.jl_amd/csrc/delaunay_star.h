// delaunay_star.h -- the geometry of the Delaunay builder (delaunay.hip): one point's star as its Voronoi cell, clipped by one
// bisector at a time.  Includes nothing from HIP, so tests/host/delaunay_star_check.cpp runs the same code as the kernels against a
// brute force in exact integer arithmetic.
//
// The rule (include/ngpde_mesh.h).  i and j are joined iff some closed disk has p_i and p_j on its boundary and no other point of
// the graph strictly inside.  The centre of such a disk is a point of the plane that is as near to p_j as to p_i and no nearer to
// any other point: the closed Voronoi cells of i and j meet.  So the star of i is the set of j whose bisector touches the cell of i.
//
// Coordinates.  Everything is translated to the star's own point: q_j = p_j - p_i, formed in double from the float coordinates
// (one rounding each; exact whenever the two exponents are within 29 of each other).  The bisector of j is the line
//   L_j = (q_x, q_y, -h),  h = (q_x^2 + q_y^2) / 2,        the cell's side of it is   s_j(v) = h w - q_x x - q_y y >= 0
// for a homogeneous point v = (x, y, w), w >= 0.  w = 0 is a direction: an unbounded cell has such vertices, so a hull point needs no
// bounding box.  The line at infinity is L = (0, 0, -1), its side s = w.  The cell is a cyclic list of vertices, counter-clockwise,
// every vertex with the line (`tag`) of the edge that LEAVES it; it starts as the whole plane, the four axis directions joined by
// edges at infinity.
//
// Expressions.  A vertex is the intersection of its two lines, computed from the LINES and never from earlier vertices, so every
// vertex carries the error of one step however many clips came before:
//   v = L_a x L_b:   x = h_a b_y - h_b a_y,   y = h_b a_x - h_a b_x,   w = a_x b_y - a_y b_x          (negated where w < 0)
// and s_j(v) = h_j w - j_x x - j_y y is half the in-circle determinant of (p_i, p_a, p_b, p_j)
//   D = |j|^2 (a x b) + |a|^2 (b x j) + |b|^2 (j x a),   s = D / 2.
// Forward error bound.  With u = 2^-53 and every operation rounded once (the library is compiled with -ffp-contract=off): each
// monomial of D, such as j_x j_x a_x b_y, is a product of four coordinates.  Between the float inputs and the result it passes at
// most 11 roundings: 4 differences, 3 products, and 4 of the sums (one inside |j|^2 or h, one inside the 2 x 2 determinant, two that
// add the three terms); halving is exact.  So |computed s - s| <= ((1 + u)^11 - 1) P < 12 u P with P the sum of the monomials'
// absolute values, and P <= |a||b||j| (|a| + |b| + |j|) / 2 by Cauchy-Schwarz on each 2 x 2 determinant.  The bound used is
//   E_j(v) = 6 u |j| (ab |j| + abs),   ab >= |a||b|,   abs >= |a||b|(|a| + |b|)      (both kept per vertex, rounded up to float),
// i.e. |D| <= kTieBound * |a||b||j|(|a| + |b| + |j|) with kTieBound = 12 u: NGPDE_DELAUNAY_TIE_BOUND of the header.  For a direction
// (w = 0) s = -(j_x x + j_y y) with x, y one coordinate each: 3 roundings, E = 4 u (|j_x x| + |j_y y|).
// Decisions.  A vertex is cut by j iff s_j(v) < -E_j(v) (and see is_cut for a direction): a margin inside the bound is a tie, and ties keep the vertex, so the kept
// cell contains the true one.  j is a neighbour iff s_j(v) <= E_j(v) at a FINITE vertex, or its line is the edge between two
// opposite directions (a bisector that meets the cell only at infinity belongs to no disk: the third of three collinear points is no neighbour).
// A decision that exact arithmetic makes by more than the bound therefore comes out right, and a tie keeps the edge.  What is NOT
// claimed: where some decision of a star is a tie, later vertices are intersections with a kept line that exact arithmetic would
// have cut, so other near-ties of the same star may be kept that a different candidate order would drop; the result is a function
// of the points because the candidate order (cells, then sorted position) is.
// Stop.  After the cells within `ring` rings every unvisited point is at least reach(ring) away (neighbor_grid.h, ring bound), its
// bisector at least reach / 2.  If every vertex is finite and within rho of the point, the cell lies in the disk of radius rho
// (it is the hull of its vertices), and a bisector farther than rho cannot touch it.  rho^2 = (x^2 + y^2) / w^2 is compared with a
// relative slack of 2^-10, far above the float rounding of reach^2 (2^-22) and the vertices' own; a vertex whose w is noise has
// a huge rho and only delays the stop.  A direction among the vertices means no stop before the grid is exhausted.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define NGPDE_STAR_HD __host__ __device__ __forceinline__
#else
#define NGPDE_STAR_HD inline
#endif

namespace ngpde {
namespace star {

constexpr double kU = 0x1p-53;
constexpr double kTieBound = 12.0 * kU;   // NGPDE_DELAUNAY_TIE_BOUND
constexpr int32_t kTagInfinity = -1;

struct Line {
  double x, y, h, n;   // q, |q|^2 / 2, |q|
  int32_t tag;         // the candidate's name (its sorted position); kTagInfinity for the line at infinity
};

struct Vertex {
  double x, y, w;
  float ab, abs;       // >= |a||b| and >= |a||b|(|a| + |b|) of its two lines (unused where w == 0)
  int32_t tag;         // line of the edge that leaves it
};

NGPDE_STAR_HD Line line_to(float ax, float ay, float bx, float by, int32_t tag) {
  Line l;
  l.x = (double)bx - (double)ax;
  l.y = (double)by - (double)ay;
  const double n2 = l.x * l.x + l.y * l.y;
  l.h = 0.5 * n2;
  l.n = sqrt(n2);
  l.tag = tag;
  return l;
}
NGPDE_STAR_HD bool coincident(const Line &l) { return l.x == 0.0 && l.y == 0.0; }

NGPDE_STAR_HD float round_up(double v) { return (float)(v * (1.0 + 0x1p-20)); }   // >= v: the float rounding is within 2^-24

// s_j(v) and its bound
NGPDE_STAR_HD void side(const Vertex &v, const Line &l, double *s, double *e) {
  if (v.w == 0.0) {
    const double a = l.x * v.x, b = l.y * v.y;
    *s = -(a + b);
    *e = 4.0 * kU * (fabs(a) + fabs(b));
  } else {
    *s = l.h * v.w - l.x * v.x - l.y * v.y;
    *e = 6.0 * kU * l.n * ((double)v.ab * l.n + (double)v.abs);
  }
}
// Is vertex v cut by l?  `prev` is the vertex before it, line_of(tag) rebuilds a line of the cell.  A direction that l passes
// through within the bound is the far end of an edge parallel to l, and the direction alone cannot say on which side of l that
// edge runs: it is cut iff one of its two edges is a finite line whose foot point q_e / 2 lies beyond l,
//   s_l(q_e / 2) = h_l - (l_x e_x + l_y e_y) / 2 < -6 u (h_l + (|l_x e_x| + |l_y e_y|) / 2)            (5 roundings per monomial).
// This is what makes the nearer of two collinear points on one side replace the farther one whatever order they come in.
template <class LineOf>
NGPDE_STAR_HD bool is_cut(const Vertex &prev, const Vertex &v, const Line &l, LineOf &&line_of) {
  double s, e;
  side(v, l, &s, &e);
  if (s < -e) return true;
  if (v.w != 0.0 || s > e) return false;
  for (int which = 0; which < 2; ++which) {
    const int32_t tag = which ? v.tag : prev.tag;
    if (tag == kTagInfinity) continue;
    const Line f = line_of(tag);
    const double a = 0.5 * (l.x * f.x), b = 0.5 * (l.y * f.y);
    if (l.h - a - b < -6.0 * kU * (l.h + fabs(a) + fabs(b))) return true;
  }
  return false;
}

// v and the vertex after it, `next`: does the line reach v, or is it the edge from v to next?  An edge between two directions is
// an edge only where they are opposite (a strip or a half-plane: collinear points); between equal directions it has been cut down
// to nothing at infinity.
NGPDE_STAR_HD bool touches(const Vertex &v, const Vertex &next, const Line &l) {
  if (v.w == 0.0) return v.tag == l.tag && next.w == 0.0 && v.x * next.x + v.y * next.y < 0.0;
  double s, e;
  side(v, l, &s, &e);
  return s <= e;
}

// the whole plane: vertex k of 4
NGPDE_STAR_HD Vertex plane_corner(int k) {
  Vertex v;
  v.x = k == 0 ? 1.0 : (k == 2 ? -1.0 : 0.0);
  v.y = k == 1 ? 1.0 : (k == 3 ? -1.0 : 0.0);
  v.w = 0.0;
  v.ab = v.abs = 0.f;
  v.tag = kTagInfinity;
  return v;
}

// The new vertex where line l crosses the edge (of line e) that runs from `in` (kept) to `out` (cut); `tag` names the edge that
// leaves it.  The sign of a homogeneous triple is free: a finite vertex takes w > 0, a direction the side of the edge's own
// ends.  Two lines that are parallel within the rounding of w meet in a direction.
NGPDE_STAR_HD Vertex cross_vertex(const Line &e, const Line &l, const Vertex &in, const Vertex &out, int32_t tag) {
  Vertex v;
  v.tag = tag;
  v.ab = v.abs = 0.f;
  if (e.tag == kTagInfinity) {
    v.x = l.y;
    v.y = -l.x;
    v.w = 0.0;
  } else {
    v.x = e.h * l.y - l.h * e.y;
    v.y = l.h * e.x - e.h * l.x;
    const double p = e.x * l.y, m = e.y * l.x;
    v.w = p - m;
    if (fabs(v.w) <= 4.0 * kU * (fabs(p) + fabs(m))) v.w = 0.0;
  }
  if (v.w == 0.0) {
    double t;
    if (out.w == 0.0) {   // the crossing lies at infinity between (or at) the directions `in` and `out`, which are within 90 degrees
      t = (v.x * out.x + v.y * out.y) / sqrt(out.x * out.x + out.y * out.y);
      if (in.w == 0.0) t += (v.x * in.x + v.y * in.y) / sqrt(in.x * in.x + in.y * in.y);
    } else {
      double si, ei, so, eo;
      side(in, l, &si, &ei);
      side(out, l, &so, &eo);
      if (si < 0.0) si = 0.0;
      t = v.x * (si * out.x - so * in.x) + v.y * (si * out.y - so * in.y);
    }
    if (t < 0.0) {
      v.x = -v.x;
      v.y = -v.y;
    }
  } else {
    if (v.w < 0.0) {
      v.x = -v.x;
      v.y = -v.y;
      v.w = -v.w;
    }
    v.ab = round_up(e.n * l.n);
    v.abs = round_up(e.n * l.n * (e.n + l.n));
  }
  return v;
}

// rho^2 of a vertex (inf for a direction)
NGPDE_STAR_HD double rho2(const Vertex &v) {
  if (v.w == 0.0) return INFINITY;
  return (v.x * v.x + v.y * v.y) / (v.w * v.w);
}
// the stop: no point at float distance^2 >= reach2 can touch a cell whose vertices have rho^2 <= r2max
NGPDE_STAR_HD bool certified(double r2max, float reach2) { return 4.0 * r2max * (1.0 + 0x1p-10) < (double)reach2; }

// The run of cut vertices, found from the flags alone.  The cut vertices of a convex cell are consecutive; the run taken is the
// one from the first cut vertex whose predecessor is kept to the LAST cut vertex before that predecessor, so that flags which
// contradict convexity (ties beside roundings) still leave a valid cyclic list.  a = first cut, len = length; false: nothing is cut
// (or, never in exact arithmetic, everything is).
template <class Cut>
NGPDE_STAR_HD bool cut_run(int m, Cut &&cut, int *a, int *len) {
  int first = -1;
  bool prev = cut(m - 1);
  for (int k = 0; k < m; ++k) {
    const bool c = cut(k);
    if (c && !prev && first < 0) first = k;
    prev = c;
  }
  if (first < 0) return false;
  int l = 1;
  for (int t = 1; t < m - 1; ++t) {
    int k = first + t;
    if (k >= m) k -= m;
    if (cut(k)) l = t + 1;
  }
  *a = first;
  *len = l;
  return true;
}

enum ClipResult { kUnchanged = 0, kClipped = 1, kOverflow = -1 };

// One clip step, by one thread.  P: the cell, P.get(k) / P.set(k, v) for 0 <= k < cap; m its size; line_of(tag) rebuilds a
// line of the cell from its name.  kOverflow: the clipped cell needs more than `cap` vertices; nothing was written.
template <class Cell, class LineOf>
NGPDE_STAR_HD ClipResult clip(Cell &P, int *m_io, int cap, const Line &l, LineOf &&line_of) {
  const int m = *m_io;
  int a, len;
  if (!cut_run(m, [&](int k) { return is_cut(P.get(k == 0 ? m - 1 : k - 1), P.get(k), l, line_of); }, &a, &len)) return kUnchanged;
  const int m_new = m - len + 2;
  if (m_new > cap) return kOverflow;
  int b = a + len - 1;
  const bool wraps = b >= m;
  if (wraps) b -= m;
  const Vertex u = P.get(a == 0 ? m - 1 : a - 1), va = P.get(a), vb = P.get(b), vn = P.get(b + 1 == m ? 0 : b + 1);
  const Line eu = u.tag == kTagInfinity ? Line{0, 0, 0, 0, kTagInfinity} : line_of(u.tag);
  const Line eb = vb.tag == kTagInfinity ? Line{0, 0, 0, 0, kTagInfinity} : line_of(vb.tag);
  const Vertex A = cross_vertex(eu, l, u, va, l.tag);
  const Vertex B = cross_vertex(eb, l, vn, vb, vb.tag);
  if (wraps) {   // kept: b+1 .. a-1
    const int cnt = m - len;
    for (int k = 0; k < cnt; ++k) P.set(k, P.get(k + b + 1));
    P.set(cnt, A);
    P.set(cnt + 1, B);
  } else {       // kept: 0 .. a-1 and b+1 .. m-1
    const int delta = 2 - len;
    if (delta < 0)
      for (int k = b + 1; k < m; ++k) P.set(k + delta, P.get(k));
    else if (delta > 0)
      for (int k = m - 1; k > b; --k) P.set(k + delta, P.get(k));
    P.set(a, A);
    P.set(a + 1, B);
  }
  *m_io = m_new;
  return kClipped;
}

}  // namespace star
}  // namespace ngpde
