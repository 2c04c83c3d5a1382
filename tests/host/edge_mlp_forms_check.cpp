// edge_mlp_forms_check.cpp -- prints the decisions of csrc/edge_mlp_forms.h for the cases on its standard input (built with ASan +
// UBSan by tests/test_edge_mlp_forms_host.py, which writes the cases and compares every line with tests/edge_mlp_forms_spec.py).
// Includes the header alone: the choice of a message-MLP kernel needs neither HIP nor a device, and nothing here is a pointer to data.
//
// A case, one line of whitespace-separated integers behind the entry's name (fwd, bwd or layer):
//   <entry>  graph has_norm halo_ok max_halo n_tiles n_nodes n_edges   h1 act1 n_tail tables {dout act} x 4 aggr
//            P Q Eterm save_z dQ dE  training
//   tables = 0: the tail layers' tables are NULL.  Four {dout act} pairs, so that n_tail = 4 has something to (not) read.
// The answer, one line: the decision's fields, the kernel names in launch order ("-": no launch), numbers that are no part of an
// unsupported call as "-".  The switches are read from the environment as the library reads them.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "edge_mlp_forms.h"

namespace ngpde {
int32_t fail(int32_t code, const char *, ...) { return code; }   // (workspace.h only declares it; nothing here fails)
}  // namespace ngpde

using namespace ngpde;

namespace {

std::string join(const EdgeKernelNames &names) {
  std::string s;
  for (const std::string &k : names) s += (s.empty() ? "" : ",") + k;
  return s.empty() ? "-" : s;
}
std::string num(bool present, unsigned long long v) { return present ? std::to_string(v) : "-"; }

}  // namespace

int main() {
  std::string line;
  long long lineno = 0;
  while (std::getline(std::cin, line)) {
    ++lineno;
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string entry;
    int graph = 0, has_norm = 0, halo_ok = 0, tables = 0, bits[6] = {0, 0, 0, 0, 0, 0}, training = 0;
    int h1 = 0, act1 = 0, n_tail = 0, aggr = 0;
    int32_t dout[4] = {0, 0, 0, 0}, act[4] = {0, 0, 0, 0};
    TileGeom g;
    bool ok = static_cast<bool>(in >> entry >> graph >> has_norm >> halo_ok >> g.max_halo >> g.n_tiles >> g.n_nodes >> g.n_edges >> h1 >> act1 >> n_tail >>
                                tables);
    for (int l = 0; ok && l < 4; ++l) ok = static_cast<bool>(in >> dout[l] >> act[l]);
    ok = ok && static_cast<bool>(in >> aggr);
    for (int i = 0; ok && i < 6; ++i) ok = static_cast<bool>(in >> bits[i]);
    ok = ok && static_cast<bool>(in >> training) && n_tail <= 4;
    if (!ok) {
      std::fprintf(stderr, "line %lld: cannot read the case: %s\n", lineno, line.c_str());
      return 2;
    }
    g.graph = graph != 0; g.has_norm = has_norm != 0; g.halo_ok = halo_ok != 0;
    EdgeMlpDesc d = edge_mlp_desc(h1, act1, n_tail, tables ? dout : nullptr, tables ? act : nullptr, aggr);
    d.P = bits[0] != 0; d.Q = bits[1] != 0; d.Eterm = bits[2] != 0; d.save_z = bits[3] != 0; d.dQ = bits[4] != 0; d.dE = bits[5] != 0;

    if (entry == "fwd") {
      const EdgeFwd p = edge_mlp_fwd_plan(g, d);
      const bool on = p.form != EdgeFwdForm::None;
      std::printf("supported=%d %s threads=%s lds=%s per_xcd=%s grid=%s\n", p.supported ? 1 : 0, join(p.names()).c_str(), num(on, p.threads).c_str(),
                  num(on, p.lds).c_str(), num(on, p.per_xcd).c_str(), num(on, p.grid).c_str());
    } else if (entry == "bwd") {
      const EdgeBwd p = edge_mlp_bwd_plan(g, d);
      std::printf("supported=%d %s threads=%s lds=%s grid=%s edge_buffer=%d dE_missing=%d workspace=%zu\n", p.supported ? 1 : 0, join(p.names()).c_str(),
                  num(p.launch, p.threads).c_str(), num(p.launch, p.lds).c_str(), num(p.launch, p.grid).c_str(), p.edge_buffer ? 1 : 0,
                  p.dE_missing ? 1 : 0, p.workspace_bytes);
    } else if (entry == "layer") {
      const EdgeMsgPath m = edge_layer_msg_path(g, d, training != 0);
      std::printf("fused_msg=%d fused_bwd=%d need_dE=%d workspace=%zu\n", m.fused_msg ? 1 : 0, m.fused_bwd ? 1 : 0, m.need_dE ? 1 : 0, m.bwd_workspace_bytes);
    } else {
      std::fprintf(stderr, "line %lld: unknown entry %s\n", lineno, entry.c_str());
      return 2;
    }
  }
  return 0;
}
