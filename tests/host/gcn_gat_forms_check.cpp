// gcn_gat_forms_check.cpp -- prints the decisions of csrc/gcn_forms.h and csrc/gat_forms.h for the cases on its standard input (built
// with ASan + UBSan by tests/test_gcn_gat_forms_host.py, which writes the cases and compares every line with
// tests/gcn_gat_forms_spec.py).  Includes the headers alone: the choice of a GCNConv or GATConv kernel needs neither HIP nor a device,
// and nothing here is a pointer to data.
//
// A case, one line of whitespace-separated integers behind the function's name.  GEOM stands for the seven fields of a TileGeom:
// graph has_norm halo_ok halo_ok_s self_loops n_nodes n_edges.
//   fused_fwd  GEOM d act pre own_first
//   fused_bwd  GEOM d act aggregate pre
//   fused_sizes n_nodes d                     (d one of the fused widths)
//   prescaled  GEOM d
//   layer      GEOM din dout act
//   gat_fwd    GEOM heads c
//   gat_bwd    GEOM heads c aligned
//   gat_layer  GEOM din heads c
// The answer, one line: the decision's fields and the kernel names in launch order ("-": none).  The switches are read from the
// environment as the library reads them.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "gat_forms.h"
#include "gcn_forms.h"

using namespace ngpde;

namespace {

std::string join(const std::vector<std::string> &names) {
  std::string s;
  for (const std::string &k : names) s += (s.empty() ? "" : ",") + k;
  return s.empty() ? "-" : s;
}
bool read_geom(std::istream &in, TileGeom &g) {
  int graph = 0, has_norm = 0, halo_ok = 0, halo_ok_s = 0, self_loops = 0;
  long long n = 0, e = 0;
  if (!(in >> graph >> has_norm >> halo_ok >> halo_ok_s >> self_loops >> n >> e)) return false;
  g.graph = graph != 0; g.has_norm = has_norm != 0; g.halo_ok = halo_ok != 0; g.halo_ok_s = halo_ok_s != 0; g.self_loops = self_loops != 0;
  g.n_nodes = n; g.n_edges = e;
  g.n_tiles = (int)((n + kTileRows - 1) / kTileRows);
  return true;
}
const char *kind_name(GcnKind k) { return k == GcnKind::Fused ? "fused" : k == GcnKind::AggregateFirst ? "aggregate_first" : "multiply_first"; }
const char *form_name(GatForm f) { return f == GatForm::Tiled ? "tiled" : f == GatForm::Blocked ? "blocked" : "row"; }

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
    TileGeom g;
    bool ok = true;
    if (fn == "fused_fwd") {
      int d = 0, act = 0, pre = 0, own = 0;
      ok = read_geom(in, g) && (in >> d >> act >> pre >> own);
      if (ok) {
        const GcnFusedFwd f = gcn_fused_fwd_form(g, d, act, pre != 0, own != 0);
        std::printf("supported=%d rows_ok=%d pre_ok=%d launch=%d act=%s halo=%d pre=%d own_first=%d grid=%d block=%d %s\n", f.supported ? 1 : 0, f.rows_ok ? 1 : 0,
                    f.pre_ok ? 1 : 0, f.launch ? 1 : 0, gcn_act_name(f.act), f.halo ? 1 : 0, f.pre ? 1 : 0, f.own_first ? 1 : 0, f.grid, f.block, join(f.names()).c_str());
      }
    } else if (fn == "fused_bwd") {
      int d = 0, act = 0, agg = 0, pre = 0;
      ok = read_geom(in, g) && (in >> d >> act >> agg >> pre);
      if (ok) {
        const GcnFusedBwd f = gcn_fused_bwd_form(g, d, act, agg != 0, pre != 0);
        std::printf("supported=%d rows_ok=%d pre_ok=%d launch=%d act=%s halo=%d pair=%d pre=%d grid=%d block=%d slabs=%d %s\n", f.supported ? 1 : 0, f.rows_ok ? 1 : 0,
                    f.pre_ok ? 1 : 0, f.launch ? 1 : 0, gcn_act_name(f.act), f.halo ? 1 : 0, f.pair ? 1 : 0, f.pre ? 1 : 0, f.grid, f.block, f.slabs, join(f.names()).c_str());
      }
    } else if (fn == "fused_sizes") {
      long long n = 0;
      int d = 0;
      ok = static_cast<bool>(in >> n >> d) && fused_supported(d, d);
      if (ok) std::printf("blocks=%d slabs=%d mask_bytes=%zu\n", fused_num_blocks(n), fused_num_slabs(n, d), fused_mask_bytes(n, d));
    } else if (fn == "prescaled") {
      int d = 0;
      ok = read_geom(in, g) && (in >> d);
      if (ok) std::printf("prescaled=%d\n", fused_prescaled_supported(g, d) ? 1 : 0);
    } else if (fn == "layer") {
      int din = 0, dout = 0, act = 0;
      ok = read_geom(in, g) && (in >> din >> dout >> act);
      if (ok) {
        const GcnLayerForm f = gcn_layer_form(g.n_nodes, din, dout);
        std::printf("kind=%s dp=%d nsplit=%d parts=%d colsum_two=%d needs_saved_agg=%d needs_x=%d ws=%zu,%zu,%zu fwd=%s bwd=%s bwd_dw_only=%s\n", kind_name(f.kind), f.dp,
                    f.nsplit, f.parts, f.colsum_two ? 1 : 0, f.needs_saved_agg ? 1 : 0, f.needs_x ? 1 : 0, gcn_workspace_bytes(f, false, false),
                    gcn_workspace_bytes(f, true, false), gcn_workspace_bytes(f, true, true), join(f.fwd_names(g, act)).c_str(),
                    join(f.bwd_names(g, act, true, true)).c_str(), join(f.bwd_names(g, act, false, false)).c_str());
      }
    } else if (fn == "gat_fwd") {
      int heads = 0, c = 0;
      ok = read_geom(in, g) && (in >> heads >> c);
      if (ok) {
        const GatFwd f = gat_fwd_form(g, heads, c);
        std::printf("form=%s tiled_supported=%d launch=%d %s\n", form_name(f.form), gat_tiled_supported(g, heads, c) ? 1 : 0, f.launch ? 1 : 0, join(f.names()).c_str());
      }
    } else if (fn == "gat_bwd") {
      int heads = 0, c = 0, aligned = 0;
      ok = read_geom(in, g) && (in >> heads >> c >> aligned);
      if (ok) {
        const GatBwd f = gat_bwd_form(g, heads, c, aligned != 0);
        GatBwdWs p;
        std::printf("form=%s launch=%d ws=%zu %s\n", form_name(f.form), f.launch ? 1 : 0, measure(gat_bwd_layout, g, heads, p) + kWsSlack, join(f.names()).c_str());
      }
    } else if (fn == "gat_layer") {
      int din = 0, heads = 0, c = 0;
      ok = read_geom(in, g) && (in >> din >> heads >> c);
      if (ok) {
        const GatLayer f = gat_layer_form(g, din, heads, c);
        std::printf("supported=%d node=%d h=%d n_tiles=%d src_wgs=%d ws=%zu fwd=%s bwd=%s\n", f.supported ? 1 : 0, gat_node_host_supported(g, heads, c) ? 1 : 0, f.h,
                    f.n_tiles, f.src_wgs, gat_layer_workspace_bytes(g, heads), join(f.fwd_names()).c_str(), join(f.bwd_names()).c_str());
      }
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
