// gno_forms_check.cpp -- prints the decisions of csrc/gno_forms.h for the cases on its standard input (built with ASan + UBSan by
// tests/test_gno_forms_host.py, which writes the cases and compares every line with tests/gno_forms_spec.py).  Includes the header
// alone: the choice of a GNOConv kernel needs neither HIP nor a device, and nothing here is a pointer to data.
//
// A case, one line of whitespace-separated integers behind the function's name:
//   apply  out k
//   gform  N E in k out act1 training
//   layer  N E in out phi_layers k act1 last_act b2 aggr training
//   lds_max                                   (the largest dynamic LDS of the matrix-pipe pullback over its envelope)
// The answer, one line: the decision's fields and the kernel names in launch order ("-": none).  The switches are read from the
// environment as the library reads them.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "gno_forms.h"

using namespace ngpde;

namespace {

std::string join(const GnoKernelNames &names) {
  std::string s;
  for (const std::string &k : names) s += (s.empty() ? "" : ",") + k;
  return s.empty() ? "-" : s;
}
const char *kind_name(GnoApplyKind k) { return k == GnoApplyKind::Mfma ? "mfma" : k == GnoApplyKind::Valu ? "valu" : "unsupported"; }

}  // namespace

int main() {
  std::string line;
  long long lineno = 0;
  while (std::getline(std::cin, line)) {
    ++lineno;
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string fn;
    in >> fn;
    bool ok = true;
    if (fn == "apply") {
      int out = 0, k = 0;
      ok = static_cast<bool>(in >> out >> k);
      if (ok) {
        const GnoApplyForm f = gno_apply_form(out, k);
        const std::string none = "-";   // the message entries' launches: the forward with its input formed in the kernel, the pullback from nodes
        std::printf("kind=%s apply_entry=%d message_entry=%d fwd=%s bwd=%s msg_fwd=%s msg_bwd=%s kp_log2=%d rows_per_thread=%d nob=%d lds_fwd=%zu lds_bwd=%zu\n", kind_name(f.kind),
                    f.apply_entry ? 1 : 0, f.message_entry ? 1 : 0, join(f.fwd_names()).c_str(), join(f.bwd_names()).c_str(),
                    (f.message_entry ? join(f.fwd_names(true)) : none).c_str(), (f.message_entry ? join(f.bwd_names(true)) : none).c_str(), f.kp_log2,
                    f.rows_per_thread, f.nob, f.lds_fwd, f.lds_bwd);
      }
    } else if (fn == "gform") {
      long long N = 0, E = 0;
      int cin = 0, k = 0, out = 0, act1 = 0, training = 0;
      ok = static_cast<bool>(in >> N >> E >> cin >> k >> out >> act1 >> training);
      if (ok) {
        const GnoGform f = gno_gform_form(N, E, cin, k, out, act1, training != 0);
        std::printf("supported=%d rows_ok=%d preferred=%d chunk=%d act1=%s nsplit=%d %s\n", f.supported ? 1 : 0, f.rows_ok ? 1 : 0, f.preferred ? 1 : 0, f.chunk,
                    gno_act1_name(f.act1), f.nsplit, join(f.names()).c_str());
      }
    } else if (fn == "layer") {
      long long N = 0, E = 0;
      int cin = 0, out = 0, layers = 0, k = 0, act1 = 0, last = 0, b2 = 0, aggr = 0, training = 0;
      ok = static_cast<bool>(in >> N >> E >> cin >> out >> layers >> k >> act1 >> last >> b2 >> aggr >> training);
      if (ok) {
        const GnoLayerForm f = gno_layer_form(N, E, cin, out, layers, k, act1, last, b2 != 0, aggr, training != 0);
        std::printf("reassoc=%d has_b2=%d fused_msg=%d fused_agg=%d gform=%d n_mid=%d nsplit=%d fwd=%s bwd=%s\n", f.reassoc ? 1 : 0, f.has_b2 ? 1 : 0,
                    f.fused_msg ? 1 : 0, f.fused_agg ? 1 : 0, f.gform ? 1 : 0, f.n_mid, f.nsplit, join(f.fwd_names()).c_str(), join(f.bwd_names()).c_str());
      }
    } else if (fn == "lds_max") {
      std::printf("max_pullback_lds=%zu\n", gno_mfma_bwd_lds_max());
    } else {
      std::fprintf(stderr, "line %lld: unknown function %s\n", lineno, fn.c_str());
      return 2;
    }
    if (!ok) {
      std::fprintf(stderr, "line %lld: cannot read the case: %s\n", lineno, line.c_str());
      return 2;
    }
  }
  return 0;
}
