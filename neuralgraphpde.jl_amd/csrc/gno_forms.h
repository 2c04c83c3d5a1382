// gno_forms.h -- which kernels every GNOConv call runs, decided in one place (host only, plain C++17: no HIP).
//
// The family behind ngpde_gno_* and ngpde_gno_layer_* (GNOConv, config C5) picks its kernels from widths, phi's shape, the
// aggregation, the graph's node and edge counts and four switches.  Every choice is a pure function here that returns a small plain
// struct -- the decision -- and the launchers (mp_kernels.hip, gno_mfma.hip, gno_gform.hip) and entries (api_mp.hip, api_layers.hip)
// execute a decision without judging the shape again.  A decision names the kernels it stands for, in launch order, and
// tests/host/gno_forms_check.cpp prints decisions for tests/test_gno_forms_host.py to compare, line by line, with the restatement the
// float64 tests take their forms from (tests/gno_forms_spec.py).  No function here touches the device or dereferences a data pointer.
//
// The message m_e = K_e h_{s_e} (K_e = reshape(phi(e), out, in)) of a layer, in the order the forms are tried (gno_layer_form):
//   by target     gno_gform_fwd_kernel<in, chunk, act1>, dense_gemm128_split_nn_kernel, gno_gform_finish_kernel
//                   the fused form's conditions and + / mean, k = kGK, in in {32, 64, 128}, out % 4 == 0, h and Q rows within 2^32 bytes,
//                   and in training at least kGformTrainEdgesPerNode edges per node; NGPDE_NO_GNO_GFORM unset.  chunk = 32, or 16 under
//                   NGPDE_GNO_GFORM_CHUNK=16; act1 instantiated for relu and identity, otherwise read at run time.  The node-level
//                   product's contraction is split gno_gform_splits() ways.  The pullback is the fused form's.
//   fused         gno_apply_mfma_fwd_kernel<k, true>
//                   the reassociated form's conditions, a two-layer phi, edges, act1 identity or relu, the matrix-pipe envelope.
//                   Pullback: gno_apply_mfma_bwd_kernel<k, NOB, true> from the node gradient (+ / mean), else the aggregation's
//                   pullback, the apply pullback (gno_apply_form) and the edge combination's
//   reassociated  ngpde_edge_combine_forward, phi's middle layers on [E] rows, the apply kernels (gno_apply_form)
//                   phi of two or more layers whose last has no activation, the VALU envelope; NGPDE_GNO_MATERIALIZE unset
//   literal       ngpde_edge_combine_forward, all of phi's further layers on [E] rows, gno_contract_fwd_kernel: everything else
// The apply kernels (gno_apply_form), in this order:
//   mfma        gno_apply_mfma_fwd_kernel<k, false> / gno_apply_mfma_bwd_kernel<k, NOB, NODE>: out a multiple of 16 in 16 .. 256, k in
//                 {16, 32, 64}; NOB = 8 up to out = 128, else 16; NGPDE_NO_GNO_MFMA unset
//   valu        gno_apply_fwd_kernel / gno_apply_bwd_kernel: out, k in 1 .. 256, at most kGnoMaxRowsPerThread rows of dT_j per thread
//                 and the pullback's LDS (T_j, a batch of z and dm rows) within kGnoValuLdsLimit
// The entries keep an asymmetry (GnoApplyForm::apply_entry / message_entry): ngpde_gno_apply_* accept a shape iff the VALU envelope
// holds, also where the matrix-pipe kernel would run it (256 x 64 is refused though ngpde_gno_message_* take it); ngpde_gno_message_*
// and ngpde_gno_message_backward_from_nodes accept iff the matrix-pipe envelope holds.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/ngpde.h"
#include "switches.h"

namespace ngpde {

// ---- the family's constants (the device files size their arrays with them) -----------------------------------------------------------
constexpr int kGnoBatch = 16;                 // VALU apply: edges of one source staged per LDS pass
constexpr int kGnoThreads = 256;              // threads of every workgroup of the family
constexpr int kGnoMaxDim = 256;               // VALU apply: out and k at most
constexpr int kGnoMaxRowsPerThread = 32;      // VALU pullback: rows of dT_j a thread keeps in registers
constexpr size_t kGnoValuLdsLimit = 60 * 1024;
constexpr int kET = 16;                       // matrix pipe: edges per MFMA tile
constexpr int kEB = 64;                       // edges staged per pass of the forward (4 tiles)
constexpr int kEBb = 32;                      // ... of the pullback (z and dm rows: 25 KB at 128 x 64)
constexpr int kGnoMfmaOutStep = 16, kGnoMfmaOutMax = 256;   // out in 16 .. 256 step 16; k in {16, 32, 64}
constexpr int kGnoMfmaNobSmall = 8, kGnoMfmaNobLarge = 16, kGnoMfmaNobSmallMaxOut = 128;   // register copy of T_j's columns: out / 16 at most
constexpr int kGK = 64;                       // by target: k (width of phi's hidden layer); in in {32, 64, 128}
constexpr int kGformChunk = 32, kGformChunkAlt = 16;        // edges per chunk: the default, NGPDE_GNO_GFORM_CHUNK=16
constexpr int64_t kGformTrainEdgesPerNode = 64;             // training: the form pays from here (its forward leaves no T behind)
constexpr uint64_t kGformRowBytesLimit = 1ull << 32;        // h and Q rows are fetched with 32-bit byte offsets
constexpr int kGformSplitTile = 128, kGformSplitTargetWgs = 512, kGformSplitMinK = 256, kGformSplitCap = 32;   // the node-level product's split

using GnoKernelNames = std::vector<std::string>;

// ---- the apply kernels ---------------------------------------------------------------------------------------------------------------
constexpr int gno_pad4(int v) { return (v + 3) & ~3; }
constexpr int gno_kp_log2(int kdim) {
  int l = 0;
  while ((1 << l) < kdim) ++l;
  return l;
}
// rows of dT_j per thread in the VALU pullback: ceil(pad4(out) / OG) rounded up to a multiple of 4
constexpr int gno_rows_per_thread(int cout, int kdim) {
  const int og = kGnoThreads >> gno_kp_log2(kdim);
  return gno_pad4((gno_pad4(cout) + og - 1) / og);
}
constexpr size_t gno_valu_lds(int cout, int kdim, bool bwd) {
  const int cP = gno_pad4(cout), kdP = gno_pad4(kdim);
  return ((size_t)kdP * (cP + 1) + (size_t)kGnoBatch * kdP + (bwd ? (size_t)kGnoBatch * cP : 0)) * sizeof(float);
}
constexpr bool gno_valu_envelope(int cout, int kdim) {
  if (cout <= 0 || kdim <= 0 || cout > kGnoMaxDim || kdim > kGnoMaxDim) return false;
  return gno_rows_per_thread(cout, kdim) <= kGnoMaxRowsPerThread && gno_valu_lds(cout, kdim, true) <= kGnoValuLdsLimit;
}
constexpr bool gno_mfma_shape(int cout, int kdim) {
  return cout % kGnoMfmaOutStep == 0 && cout >= kGnoMfmaOutStep && cout <= kGnoMfmaOutMax && (kdim == 16 || kdim == 32 || kdim == 64);
}
constexpr size_t gno_mfma_bwd_lds(int cout, int kdim) { return (size_t)(kEBb * (kdim + 4) + kEBb * (cout + 4)) * sizeof(float); }
constexpr size_t gno_mfma_bwd_lds_max() {
  size_t m = 0;
  for (int cout = kGnoMfmaOutStep; cout <= kGnoMfmaOutMax; cout += kGnoMfmaOutStep)
    for (int kdim = 16; kdim <= 64; kdim *= 2) m = gno_mfma_bwd_lds(cout, kdim) > m ? gno_mfma_bwd_lds(cout, kdim) : m;
  return m;
}
// the pullback's dynamic LDS stays below the 64 KB a kernel may ask for without raising its limit, anywhere in the envelope
static_assert(gno_mfma_bwd_lds_max() == 41984 && gno_mfma_bwd_lds_max() <= 64 * 1024, "gno_apply_mfma_bwd_kernel: LDS beyond the default limit");
inline bool gno_mfma_envelope(int cout, int kdim) { return !switch_on(Switch::NoGnoMfma) && gno_mfma_shape(cout, kdim); }

enum class GnoApplyKind { Unsupported, Valu, Mfma };
struct GnoApplyForm {
  GnoApplyKind kind = GnoApplyKind::Unsupported;   // what launch_gno_apply_fwd / _bwd run
  bool apply_entry = false;     // ngpde_gno_apply_* accept the shape: the VALU envelope, whichever kernel runs
  bool message_entry = false;   // ngpde_gno_message_* and _backward_from_nodes accept it: the matrix-pipe envelope
  int kdim = 0;
  int kp_log2 = 0, rows_per_thread = 0;   // Valu
  int nob = 0;                            // Mfma
  size_t lds_fwd = 0, lds_bwd = 0;        // dynamic LDS (Mfma forward: none)
  GnoKernelNames fwd_names(bool fused = false) const {
    if (kind == GnoApplyKind::Unsupported) return {};
    if (kind == GnoApplyKind::Valu) return {"gno_apply_fwd_kernel"};
    return {"gno_apply_mfma_fwd_kernel<" + std::to_string(kdim) + (fused ? ",true>" : ",false>")};
  }
  GnoKernelNames bwd_names(bool node = false) const {
    if (kind == GnoApplyKind::Unsupported) return {};
    if (kind == GnoApplyKind::Valu) return {"gno_apply_bwd_kernel"};
    return {"gno_apply_mfma_bwd_kernel<" + std::to_string(kdim) + "," + std::to_string(nob) + (node ? ",true>" : ",false>")};
  }
};
inline GnoApplyForm gno_apply_form(int cout, int kdim) {
  GnoApplyForm f;
  f.kdim = kdim;
  f.apply_entry = gno_valu_envelope(cout, kdim);
  f.message_entry = gno_mfma_envelope(cout, kdim);
  if (f.message_entry) {
    f.kind = GnoApplyKind::Mfma;
    f.nob = cout <= kGnoMfmaNobSmallMaxOut ? kGnoMfmaNobSmall : kGnoMfmaNobLarge;
    f.lds_bwd = gno_mfma_bwd_lds(cout, kdim);
  } else if (f.apply_entry) {
    f.kind = GnoApplyKind::Valu;
    f.kp_log2 = gno_kp_log2(kdim);
    f.rows_per_thread = gno_rows_per_thread(cout, kdim);
    f.lds_fwd = gno_valu_lds(cout, kdim, false);
    f.lds_bwd = gno_valu_lds(cout, kdim, true);
  }
  return f;
}

// ---- the by-target form --------------------------------------------------------------------------------------------------------------
enum class GnoAct1 { Relu, Identity, RunTime };   // the act1 the aggregate kernel is instantiated for
inline const char *gno_act1_name(GnoAct1 a) { return a == GnoAct1::Relu ? "relu" : a == GnoAct1::Identity ? "identity" : "runtime"; }
struct GnoGform {
  bool supported = false;   // the aggregate kernel takes (in, k)
  bool rows_ok = false;     // h and Q rows within kGformRowBytesLimit
  bool preferred = false;   // a layer takes this form
  int in_chs = 0, chunk = kGformChunk, nsplit = 1;
  GnoAct1 act1 = GnoAct1::RunTime;
  GnoKernelNames names() const {
    if (!supported) return {};
    return {"gno_gform_fwd_kernel<" + std::to_string(in_chs) + "," + std::to_string(chunk) + "," + gno_act1_name(act1) + ">", "dense_gemm128_split_nn_kernel",
            "gno_gform_finish_kernel"};
  }
};
inline bool gno_gform_supported(int in_chs, int kdim) {
  return !switch_on(Switch::NoGnoGform) && kdim == kGK && (in_chs == 32 || in_chs == 64 || in_chs == 128);
}
// enough workgroups for two per CU; every split a multiple of 16 of the contraction
inline int gno_gform_splits(int64_t n_nodes, int in_chs, int kdim, int cout) {
  const int64_t tiles = ((n_nodes + kGformSplitTile - 1) / kGformSplitTile) * ((cout + kGformSplitTile - 1) / kGformSplitTile);
  const int K = in_chs * kdim;
  int ns = (int)std::max<int64_t>(1, (kGformSplitTargetWgs + tiles - 1) / std::max<int64_t>(tiles, 1));
  ns = std::min(ns, std::max(1, K / kGformSplitMinK));
  return std::min(ns, kGformSplitCap);
}
// Inference: always (config 5: 0.279 -> 0.200 ms at radius 0.1, 0.191 -> 0.147 ms at 0.05).  Training: the pullback stays in the
// by-source form and needs T = W2 (x) h, which only that form's forward leaves behind -- one more node-level product (86 us at
// config 5) that this form's forward must win back on the edges: it does from about 64 edges per node (radius 0.1, 117 per node:
// forward + backward 0.895 -> 0.861 ms; radius 0.05, 34 per node: 0.623 -> 0.657 ms, so not there).
inline GnoGform gno_gform_form(int64_t n_nodes, int64_t n_edges, int in_chs, int kdim, int cout, int act1, bool training) {
  GnoGform f;
  f.in_chs = in_chs;
  f.supported = gno_gform_supported(in_chs, kdim);
  f.rows_ok = (uint64_t)n_nodes * (uint64_t)std::max(in_chs, kGK) * 4u < kGformRowBytesLimit;
  f.preferred = f.supported && cout % 4 == 0 && n_edges > 0 && f.rows_ok && (!training || n_edges >= kGformTrainEdgesPerNode * n_nodes);
  const char *chunk_env = switch_text(Switch::GnoGformChunk);   // (A/B runs) unset or any other value than 16 means the default
  f.chunk = chunk_env && std::atoi(chunk_env) == kGformChunkAlt ? kGformChunkAlt : kGformChunk;
  f.act1 = act1 == NGPDE_ACT_RELU ? GnoAct1::Relu : act1 == NGPDE_ACT_IDENTITY ? GnoAct1::Identity : GnoAct1::RunTime;
  f.nsplit = gno_gform_splits(n_nodes, in_chs, kdim, cout);
  return f;
}

// ---- a layer (make_gno_plan in api_layers.hip lays its workspace out by these bits; gno_plan_key hashes bits()) ------------------------
struct GnoLayerForm {
  bool reassoc = false, has_b2 = false, fused_msg = false, fused_agg = false;
  bool gform = false;      // aggregate-then-transform (gno_gform.hip): no [E][out] message, no T in the forward
  int n_mid = 0;           // Dense layers of phi evaluated on [E] rows by the primitives (reassociated: 1 .. L - 2; literal: 1 .. L - 1)
  int nsplit = 1;
  GnoApplyForm apply;      // reassociated: the apply kernels
  GnoGform by_target;      // gform: its instantiation
  uint64_t bits() const {
    return (uint64_t)reassoc | (uint64_t)fused_msg << 1 | (uint64_t)fused_agg << 2 | (uint64_t)has_b2 << 3 | (uint64_t)gform << 4 | (uint64_t)nsplit << 8 |
           (uint64_t)n_mid << 16;
  }
  // the message part on a graph with edges; a primitive whose kernel depends on its pointers' alignment stands by its entry's name
  GnoKernelNames fwd_names() const {
    if (gform) return by_target.names();
    if (fused_msg) return apply.fwd_names(true);
    GnoKernelNames k = {"ngpde_edge_combine_forward"};
    k.insert(k.end(), (size_t)std::max(n_mid, 0), "ngpde_dense_forward");
    if (!reassoc) k.push_back("gno_contract_fwd_kernel");
    else for (const std::string &s : apply.fwd_names()) k.push_back(s);
    return k;
  }
  GnoKernelNames bwd_names() const {
    if (fused_agg) return apply.bwd_names(true);
    GnoKernelNames k = {"ngpde_segment_reduce_backward"};
    if (!reassoc) k.push_back("gno_contract_bwd_kernel");
    else for (const std::string &s : apply.bwd_names()) k.push_back(s);
    k.insert(k.end(), (size_t)std::max(n_mid, 0), "ngpde_dense_backward");
    k.push_back("ngpde_edge_combine_backward");
    return k;
  }
};
inline GnoLayerForm gno_layer_form(int64_t n_nodes, int64_t n_edges, int in_chs, int cout, int phi_layers, int kdim, int act1, int last_act, bool b2,
                                   int aggr, bool training) {
  GnoLayerForm f;
  f.apply = gno_apply_form(cout, kdim);
  f.reassoc = phi_layers >= 2 && last_act == NGPDE_ACT_IDENTITY && !switch_on(Switch::GnoMaterialize) && f.apply.apply_entry;
  f.has_b2 = f.reassoc && b2;
  f.fused_msg = f.reassoc && phi_layers == 2 && n_edges > 0 && (act1 == NGPDE_ACT_IDENTITY || act1 == NGPDE_ACT_RELU) && f.apply.message_entry;
  f.fused_agg = f.fused_msg && (aggr == NGPDE_AGGR_SUM || aggr == NGPDE_AGGR_MEAN);
  // the edge index contracted first, per target: the forward needs neither T nor the [E][out] message (the pullback keeps the
  // by-source form and makes its own T)
  f.by_target = gno_gform_form(n_nodes, n_edges, in_chs, kdim, cout, act1, training);
  f.gform = f.fused_agg && f.by_target.preferred;
  f.n_mid = f.fused_msg ? 0 : (f.reassoc ? phi_layers - 2 : phi_layers - 1);
  f.nsplit = f.gform ? f.by_target.nsplit : 1;
  return f;
}

}  // namespace ngpde
