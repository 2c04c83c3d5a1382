// rk_tables_check.cpp -- stand-alone print-out of csrc/rk_tableau.h's coefficient tables (built with ASan + UBSan by
// tests/test_rk_tables_host.py, which compares every float bit for bit with numpy's float32(float64(dt) * x)).
// One line per table:  <forward6|adjoint8> <euler|tsit5> <dt index> <hex floats...>   for dt = 0.02, 1 / 50 and 0.1f widened to double.
// The tables are heap blocks of exactly the documented size, filled with NaN bit patterns first: a slot the functions leave alone or a
// write past the end shows.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rk_tableau.h"

using namespace ngpde;

namespace {

void print(const char *table, const char *name, int k, const std::vector<float> &v) {
  std::printf("%s %s %d", table, name, k);
  for (float x : v) std::printf(" %a", (double)x);
  std::printf("\n");
}

}  // namespace

int main() {
  const double one = 1.0, fifty = 50.0;
  const float tenth = 0.1f;
  const double dts[3] = {0.02, one / fifty, (double)tenth};
  const int which[2] = {NGPDE_TABLEAU_EULER, NGPDE_TABLEAU_TSIT5};
  const char *names[2] = {"euler", "tsit5"};
  for (int t = 0; t < 2; ++t) {
    const Tableau tb = make_tableau(which[t]);
    for (int k = 0; k < 3; ++k) {
      std::vector<float> fwd(42), adj((size_t)tb.S * 8);
      std::memset(fwd.data(), 0xff, fwd.size() * sizeof(float));
      std::memset(adj.data(), 0xff, adj.size() * sizeof(float));
      rk_forward6(tb, dts[k], fwd.data());
      rk_adjoint8(tb, dts[k], adj.data());
      print("forward6", names[t], k, fwd);
      print("adjoint8", names[t], k, adj);
    }
  }
  return 0;
}
