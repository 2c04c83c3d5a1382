// dense_forms_check.cpp -- prints the decisions of csrc/dense_forms.h for the cases on its standard input (built with ASan + UBSan by
// tests/test_dense_forms_host.py, which writes the cases and compares every line with tests/dense_forms_spec.py).  Includes the
// header alone: the choice of a Dense kernel needs neither HIP nor a device.  Addresses are plain integers and never dereferenced.
//
// A case, one line of whitespace-separated integers behind the entry's name:
//   <entry> n  nseg {address width row_div} x nseg  nseg_b {address width row_div} x nseg_b  d1 d2  identity bias
//           weight y z dy workspace  dseg x 4
//   fwd (d1 = dout), bwd (d1 = dout), pair_fwd (d1, d2 = the sides' dout), chain (d1 = dmid, d2 = dout), pair_bwd (d1 = dout)
// The answer, one line: the kernel names in launch order ("-": no launch) and the decision's numbers ("-": not part of this form).
// The Dense switches are read from the environment as the library reads them.
#include <cstdarg>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "dense_forms.h"

namespace ngpde {
int32_t fail(int32_t code, const char *, ...) { return code; }   // (workspace.h only declares it; nothing here fails)
}  // namespace ngpde

using namespace ngpde;

namespace {

struct Table {
  SegTable t;
  int din = 0;
};
bool read_table(std::istream &in, Table &tb) {
  int nseg = 0;
  if (!(in >> nseg) || nseg < 0 || nseg > 4) return false;
  const float *ptr[4] = {nullptr, nullptr, nullptr, nullptr};
  int32_t width[4] = {0, 0, 0, 0}, row_div[4] = {0, 0, 0, 0};
  for (int i = 0; i < nseg; ++i) {
    unsigned long long a = 0;
    if (!(in >> a >> width[i] >> row_div[i]) || width[i] < 0) return false;
    ptr[i] = reinterpret_cast<const float *>(static_cast<uintptr_t>(a));
  }
  if (nseg) tb.din = fill_seg_table(tb.t, nseg, ptr, width, row_div);
  return true;
}

std::string join(const KernelNames &names) {
  std::string s;
  for (const char *k : names) s += (s.empty() ? "" : ",") + std::string(k);
  return s.empty() ? "-" : s;
}
std::string num(bool present, long long v) { return present ? std::to_string(v) : "-"; }

}  // namespace

int main() {
  std::string line;
  long long lineno = 0;
  while (std::getline(std::cin, line)) {
    ++lineno;
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string entry;
    long long n = 0;
    Table a, b;
    int d1 = 0, d2 = 0, identity = 0, bias = 0;
    unsigned long long addr[5] = {0, 0, 0, 0, 0}, dseg_addr[4] = {0, 0, 0, 0};
    bool ok = static_cast<bool>(in >> entry >> n) && read_table(in, a) && read_table(in, b) && static_cast<bool>(in >> d1 >> d2 >> identity >> bias);
    for (int i = 0; ok && i < 5; ++i) ok = static_cast<bool>(in >> addr[i]);
    for (int i = 0; ok && i < 4; ++i) ok = static_cast<bool>(in >> dseg_addr[i]);
    if (!ok) {
      std::fprintf(stderr, "line %lld: cannot read the case: %s\n", lineno, line.c_str());
      return 2;
    }
    auto at = [](unsigned long long v) { return reinterpret_cast<float *>(static_cast<uintptr_t>(v)); };
    const float *weight = at(addr[0]), *y = at(addr[1]), *z = at(addr[2]), *dy = at(addr[3]);
    float *workspace = at(addr[4]);
    float *dseg[4] = {at(dseg_addr[0]), at(dseg_addr[1]), at(dseg_addr[2]), at(dseg_addr[3])};

    if (entry == "fwd") {
      const DenseFwd p = dense_fwd_plan(n, a.t, a.din, d1, weight, y, z);
      const bool wide = p.form == DenseFwdForm::Stream || p.form == DenseFwdForm::Wide;
      std::printf("%s din_main=%s grid=%s\n", join(p.names()).c_str(), num(wide, p.din_main).c_str(), num(p.form == DenseFwdForm::Small, p.grid).c_str());
    } else if (entry == "bwd") {
      const SegGrad g = seg_grads(a.t, dseg);
      const DenseBwd p = dense_bwd_plan(n, a.t, g, a.din, d1, identity != 0, bias != 0, weight, dy, workspace);
      const bool stream = p.form == DenseBwdForm::Stream, small = p.form == DenseBwdForm::Small, composed = p.form == DenseBwdForm::Composed;
      const bool input = composed && p.input.form != DenseInputForm::None;
      std::printf("%s grid=%s n_main=%s nchunk=%s rpc=%s oper=%s nz=%s workspace=%zu\n", join(p.names()).c_str(),
                  num(stream || small, stream ? p.stream.grid : p.small_grid).c_str(), num(stream, p.stream.n_main).c_str(),
                  num(composed, p.weight.nchunk).c_str(), num(composed, p.weight.rpc).c_str(), num(input, p.input.oper).c_str(),
                  num(input, p.input.nz).c_str(), dense_bwd_workspace_bytes(n, a.din, d1));
    } else if (entry == "pair_fwd") {
      const DensePairFwd p = dense_pair_fwd_plan(n, a.t, a.din, d1, b.t, b.din, d2);
      std::printf("%s fused=%d\n", join(p.names()).c_str(), p.fused ? 1 : 0);
    } else if (entry == "chain") {
      const DenseChainFwd p = dense_chain_fwd_plan(n, a.t, a.din, d1, d2);
      std::printf("%s n_main=%d\n", join(p.names()).c_str(), p.n_main);
    } else if (entry == "pair_bwd") {
      const DensePairBwd p = dense_pair_bwd_plan(n, a.t, a.din, b.t, b.din, d1);
      std::printf("%s grid=%d workspace=%zu\n", join(p.names()).c_str(), p.grid, p.workspace_bytes);
    } else {
      std::fprintf(stderr, "line %lld: unknown entry %s\n", lineno, entry.c_str());
      return 2;
    }
  }
  return 0;
}
