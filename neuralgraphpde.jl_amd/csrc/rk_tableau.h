// rk_tableau.h -- the explicit Runge-Kutta tableaus of the device-resident solvers and the coefficient tables their kernels read.
// Host only (no HIP include: tests/host/rk_tables_check.cpp builds it with a plain C++ compiler).  Every table entry is
// (float)(dt * x) with the product formed in double, exactly as the generic solver passes it to ngpde_rk_stage_combine; every
// slot a formula below does not name is +0.0.
#pragma once

#include <vector>

#include "../../include/ngpde.h"

namespace ngpde {

struct Tableau {
  int S;
  std::vector<std::vector<double>> a;  // a[i][j], j < i
  std::vector<double> b;
};

inline Tableau make_tableau(int which) {
  Tableau t;
  if (which == NGPDE_TABLEAU_EULER) {
    t.S = 1;
    t.a = {{}};
    t.b = {1.0};
    return t;
  }
  // Tsitouras 5(4) as used by OrdinaryDiffEq.Tsit5 (graph_node.md:48); fixed step: only the 5th-order
  // weights are needed, and they equal the 7th stage row (FSAL), so this is a 6-stage explicit scheme.
  t.S = 6;
  t.a = {{},
         {0.161},
         {-0.008480655492356989, 0.335480655492357},
         {2.8971530571054935, -6.359448489975075, 4.3622954328695815},
         {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525},
         {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383}};
  t.b = {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774};
  return t;
}

// Forward table of the GCN and VMH solvers, out[42].  Stage i's epilogue forms the NEXT stage's input (after the last stage: the
// step update), so its row is a[i + 1] (b for i = S - 1): the weight of k_j, j < i, at out[i * 6 + j], of its own k_i at out[36 + i].
inline void rk_forward6(const Tableau &tb, double dt, float *out) {
  for (int k = 0; k < 42; ++k) out[k] = 0.f;
  for (int i = 0; i < tb.S; ++i) {
    const std::vector<double> &row = (i == tb.S - 1) ? tb.b : tb.a[i + 1];
    for (int j = 0; j < i; ++j) out[i * 6 + j] = (float)(dt * row[j]);
    out[36 + i] = (float)(dt * row[i]);
  }
}

// Adjoint table of the GAT and VMH solvers, out[S][8]: out[i][i] = dt b_i, out[i][j] (j > i) = dt a[j][i].
inline void rk_adjoint8(const Tableau &tb, double dt, float *out) {
  for (int k = 0; k < tb.S * 8; ++k) out[k] = 0.f;
  for (int i = 0; i < tb.S; ++i) {
    out[i * 8 + i] = (float)(dt * tb.b[i]);
    for (int j = i + 1; j < tb.S; ++j) out[i * 8 + j] = (float)(dt * tb.a[j][i]);
  }
}

}  // namespace ngpde
