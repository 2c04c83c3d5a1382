// dense_forms.h -- which kernels every Dense call runs, decided in one place (host only, plain C++17: no HIP).
//
// The Dense family picks its kernels from the shape, the block table, the pointers' alignment and tile-count thresholds.  Every such
// choice is a pure function here that returns a small plain struct -- the decision -- and the launchers (dense_mfma.hip,
// dense_small_bwd.hip, dense_stream_bwd.hip) and entries (api_mp.hip) execute a decision without judging the shape again.  A
// decision names the kernels it stands for, in launch order (names()), and tests/host/dense_forms_check.cpp prints decisions for
// tests/test_dense_forms_host.py to compare, line by line, with the restatement the float64 tests use (tests/dense_forms_spec.py).
// No function here touches the device or reads what a data pointer points at: alignment enters through the addresses.  Grids that
// depend on the device's occupancy are launch-time values and no part of a decision.
//
// ngpde_dense_forward (dense_fwd_plan), in this order:
//   small    dense_small_fwd_kernel      17 <= din <= 64, 1 <= dout <= 64, 1 <= n <= 65 536
//   gemm128  dense_gemm128_fwd_kernel    one `vec` block of row_div 1, din % 16 == 0, dout % 4 == 0, dout >= 128, at least 512 tiles of
//                                        128 x 128, weight, y and save_z 16-byte aligned
//   stream   dense_stream64_fwd_kernel   at least 512 tiles of 128 x 64, din_main == 64, dout <= 64, every block before din_main `vec`
//                                        and inside it
//   wide     dense_wide_fwd_kernel       at least 512 tiles of 128 x 64 otherwise
//   general  dense_mfma_fwd_kernel       everything else
// ngpde_dense_backward (dense_bwd_plan), in this order: the streaming pullback (dense_stream_bwd_plan), the small pullback
// (dense_small_bwd_grid), else composed: dense_dz_kernel unless the activation is the identity, the weight pullback
// (dense_bwd_weight_plan), the input pullback split over the outputs (dense_bwd_input_split_plan: one block, > 1 split) or whole
// (dense_bwd_input_plan).  The pair and chain forwards (dense_pair_fwd_plan, dense_chain_fwd_plan) and the pair pullback
// (dense_pair_bwd_plan) each decide "one launch or not".
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "switches.h"
#include "workspace.h"

namespace ngpde {

// ---- block tables (taken by value by the kernels: layout and member order are part of the device code) -----------------------------
struct SegTable {   // virtual concatenation [X1 | X2 | ...] of up to 4 row-major blocks
  int n = 0;
  const float *ptr[4] = {nullptr, nullptr, nullptr, nullptr};
  int width[4] = {0, 0, 0, 0};
  int row_div[4] = {1, 1, 1, 1};   // block row = row / row_div (per-graph features repeated over a graph's rows)
  int offset[5] = {0, 0, 0, 0, 0};
  int vec[4] = {0, 0, 0, 0};       // block may be read with 16-byte loads (offset, width multiples of 4, base aligned)
};
struct SegGrad {
  int n = 0;
  float *ptr[4] = {nullptr, nullptr, nullptr, nullptr};
  int width[4] = {0, 0, 0, 0};
  int offset[5] = {0, 0, 0, 0, 0};
};

template <class... P>
inline bool aligned16(P... p) {   // every address a multiple of 16 (NULL is)
  return ((reinterpret_cast<uintptr_t>(p) | ...) & 15) == 0;
}

// the table of n_seg blocks (1..4, widths >= 0: the caller has checked); returns the total width
inline int fill_seg_table(SegTable &t, int n_seg, const float *const *seg_ptr, const int32_t *seg_width, const int32_t *seg_row_div) {
  t.n = n_seg;
  int off = 0;
  for (int i = 0; i < n_seg; ++i) {
    t.ptr[i] = seg_ptr[i];
    t.width[i] = seg_width[i];
    t.row_div[i] = (seg_row_div && seg_row_div[i] > 0) ? seg_row_div[i] : 1;
    t.offset[i] = off;
    t.vec[i] = (off % 4 == 0 && seg_width[i] % 4 == 0 && aligned16(seg_ptr[i])) ? 1 : 0;
    off += seg_width[i];
  }
  for (int i = n_seg; i <= 4; ++i) t.offset[i] = off;
  return off;
}

// where the blocks' gradients go: a block with row_div > 1 carries none (per-graph features: @ignore_derivatives in the layers)
inline SegGrad seg_grads(const SegTable &t, float *const *dseg) {
  SegGrad g;
  g.n = t.n;
  for (int b = 0; b < t.n; ++b) {
    g.ptr[b] = (dseg && t.row_div[b] == 1) ? dseg[b] : nullptr;
    g.width[b] = t.width[b];
  }
  for (int b = 0; b <= 4; ++b) g.offset[b] = t.offset[b];
  return g;
}
inline bool any_grad(const SegGrad &g) { return g.ptr[0] || g.ptr[1] || g.ptr[2] || g.ptr[3]; }

// ---- what the conditions measure in -------------------------------------------------------------------------------------------------
constexpr int kDenseRows64 = 64, kDenseRows128 = 128;   // rows of a tile
constexpr int kDenseCols64 = 64, kDenseCols128 = 128;   // columns of a tile; 64 is also the width of a streamed block
constexpr int kDenseK16 = 16, kDenseK32 = 32;           // features per K step
constexpr int kDenseNarrow = 4;                         // features beside the 64-wide blocks of a streaming form
constexpr int kDenseTrailing = 8;                       // features of trailing blocks that may leave the wide forward's K loop
constexpr int64_t kDenseSmallRows = 65536;              // the small forms: latency-bound row counts
constexpr int64_t kDenseStreamBwdRows = 32768;          // the streaming pullbacks: a resident wave of tiles ...
constexpr int64_t kDenseStreamBwdMaxRows = 1 << 24;     // ... and 32-bit byte offsets

using KernelNames = std::vector<const char *>;
inline int64_t dense_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// 128-row tiles once they alone give every CU two workgroups
inline bool dense_wide_tiles(int64_t n, int cols) {
  return !switch_on(Switch::DenseNarrow) && dense_cdiv(n, kDenseRows128) * dense_cdiv(cols, kDenseCols64) >= 512;
}

// ---- the counting functions ---------------------------------------------------------------------------------------------------------
// number of K splits worth taking for X[n][din] x W[din][dout]: only when the row tiles alone leave most of the chip idle and
// the contraction is long; every split gets a multiple of 16 features
inline int dense_fwd_splits(int64_t n, int din, int dout) {
  const int64_t tiles = dense_cdiv(n, kDenseRows64) * dense_cdiv(dout, kDenseCols64);
  if (tiles == 0 || tiles >= 256 || din < 256) return 1;   // (no rows: nothing to split, and no division by zero tiles)
  const int64_t want = (512 + tiles - 1) / tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, din / 64));
}
inline int dense_fwd_split_features(int din, int nsplit) { return ((din + nsplit - 1) / nsplit + kDenseK16 - 1) / kDenseK16 * kDenseK16; }
inline int dense_fwd_split_count(int din, int nsplit) {   // partial slabs launch_dense_seg_fwd_splitk actually writes
  const int kper = dense_fwd_split_features(din, nsplit);
  return (din + kper - 1) / kper;
}
// row chunks of the weight pullback: enough (tile x chunk) workgroups to cover the chip several times over (the chunk
// loop is a dependent global-load chain, ~16 rows per trip), at least 64 rows per chunk, at most 1024 partial slabs
inline int dense_weight_chunks(int64_t n, int din, int dout) {
  const int64_t tiles = std::max<int64_t>(1, dense_cdiv(din, kDenseRows64)) * std::max<int64_t>(1, dense_cdiv(dout, kDenseCols64));
  const int64_t want = (4096 + tiles - 1) / tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(1024, want), (n + 63) / 64));
}
// splits of the input pullback over the output features (see dense_mfma_bwd_input_kernel): 1 = none
inline int dense_bwd_input_splits(int64_t n, int din, int dout) {
  const int64_t tiles = dense_cdiv(n, kDenseRows128) * dense_cdiv(din, kDenseCols64);
  if (tiles == 0 || tiles >= 256 || dout < 512) return 1;   // (ngpde_dense_workspace_bytes asks for n = 0 too)
  // enough workgroups for a few rounds of the chip, each still with a dozen or more K steps (the partial slabs cost a pass too)
  return (int)std::max<int64_t>(1, std::min<int64_t>((2048 + tiles - 1) / tiles, dout / 256));
}
inline size_t dense_bwd_input_split_bytes(int64_t n, int din, int dout) {
  const int ns = dense_bwd_input_splits(n, din, dout);
  return ns > 1 ? (size_t)(ns - 1) * (size_t)n * din * sizeof(float) : 0;
}

// the Dense pullback's workspace: dz (the one-launch forms put their slabs there), the weight pullback's slabs, the split input
// pullback's partials
struct DenseBwdWs {
  float *dz, *partial, *split_part;
};
inline void dense_bwd_layout(Workspace &w, int64_t n, int32_t din, int32_t dout, DenseBwdWs &p) {
  p.dz = w.take<float>((size_t)std::max<int64_t>(n, 1) * dout);
  p.partial = w.take<float>((size_t)dense_weight_chunks(n, din, dout) * (din + 1) * dout);
  p.split_part = reinterpret_cast<float *>(w.take<char>(dense_bwd_input_split_bytes(n, din, dout)));
}
inline size_t dense_bwd_workspace_bytes(int64_t n, int32_t din, int32_t dout) {
  DenseBwdWs p;
  return measure(dense_bwd_layout, n, din, dout, p) + kWsSlack;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------
// the forward of at most 64 x 64 in one contraction pass: its grid, or 0 when the shape is not this form's (din <= 16 is ONE step of
// the general kernel)
inline int dense_small_fwd_grid(int64_t n, int din, int dout) {
  if (switch_on(Switch::DenseNoSmallFwd) || din < 17 || din > kDenseCols64 || dout < 1 || dout > kDenseCols64 || n < 1 || n > kDenseSmallRows) return 0;
  return (int)std::min<int64_t>(dense_cdiv(n, kDenseRows64), 1024);
}

enum class DenseFwdForm { None, Small, Gemm128, Stream, Wide, General };
struct DenseFwd {
  DenseFwdForm form = DenseFwdForm::None;
  int din_main = 0;   // Stream, Wide: the features inside the K loop
  int grid = 0;       // Small
  KernelNames names() const {
    switch (form) {
      case DenseFwdForm::None: return {};
      case DenseFwdForm::Small: return {"dense_small_fwd_kernel"};
      case DenseFwdForm::Gemm128: return {"dense_gemm128_fwd_kernel"};
      case DenseFwdForm::Stream: return {"dense_stream64_fwd_kernel"};
      case DenseFwdForm::Wide: return {"dense_wide_fwd_kernel"};
      case DenseFwdForm::General: break;
    }
    return {"dense_mfma_fwd_kernel"};
  }
};
inline DenseFwd dense_fwd_plan(int64_t n, const SegTable &segs, int din, int dout, const void *wt, const void *y, const void *save_z) {
  DenseFwd p;
  if (n == 0 || dout == 0) return p;
  if ((p.grid = dense_small_fwd_grid(n, din, dout))) {   // latency-bound row counts
    p.form = DenseFwdForm::Small;
    return p;
  }
  // wide outputs from one 16-byte-loadable block: 128 x 128 tiles
  if (!switch_on(Switch::DenseNoGemm128) && segs.n == 1 && segs.vec[0] && segs.row_div[0] == 1 && din % kDenseK16 == 0 && dout % 4 == 0 &&
      dout >= kDenseCols128 && dense_cdiv(n, kDenseRows128) * dense_cdiv(dout, kDenseCols128) >= 512 && aligned16(wt, y, save_z)) {
    p.form = DenseFwdForm::Gemm128;
    return p;
  }
  if (dense_wide_tiles(n, dout)) {
    // trailing narrow blocks (<= 8 features in total behind a multiple of 32) leave the K loop: see dense_wide_fwd_kernel
    p.din_main = din;
    for (int i = segs.n - 1; i >= 1 && din - segs.offset[i] <= kDenseTrailing; --i)
      if (segs.offset[i] % kDenseK32 == 0) p.din_main = segs.offset[i];
    // a 64-deep contraction over 16-byte-loadable blocks: the streaming form (whole input tile by LDS-DMA in one burst)
    bool stream_ok = !switch_on(Switch::DenseNoStream) && p.din_main == kDenseCols64 && dout <= kDenseCols64;
    for (int i = 0; i < segs.n && segs.offset[i] < p.din_main; ++i) stream_ok = stream_ok && segs.vec[i] && segs.offset[i + 1] <= p.din_main;
    p.form = stream_ok ? DenseFwdForm::Stream : DenseFwdForm::Wide;
    return p;
  }
  p.form = DenseFwdForm::General;
  return p;
}

// ---- the two-layer streaming forwards -----------------------------------------------------------------------------------------------
// leading blocks of exactly 64 features that LDS-DMA can fetch (row_div 1, 16-byte aligned); the rest must be narrow
inline int dense_stream_main_blocks(const SegTable &t, int din) {
  int nm = 0;
  while (nm < t.n && t.width[nm] == kDenseCols64 && t.row_div[nm] == 1 && t.vec[nm]) ++nm;
  return (nm >= 1 && din - kDenseCols64 * nm <= kDenseNarrow) ? nm : 0;
}
inline bool dense_stream2_enabled(int64_t n) { return !switch_on(Switch::DenseNoStream2) && dense_cdiv(n, kDenseRows128) >= 512; }

struct DensePairFwd {   // two outputs from one shared 64-wide block: one launch, or a dense_fwd_plan per side
  bool fused = false;
  KernelNames names() const { return fused ? KernelNames{"dense_pair_fwd_kernel"} : KernelNames{}; }
};
inline DensePairFwd dense_pair_fwd_plan(int64_t n, const SegTable &ta, int dina, int douta, const SegTable &tb, int dinb, int doutb) {
  return {dense_stream2_enabled(n) && douta <= kDenseCols64 && doutb <= kDenseCols64 && dense_stream_main_blocks(ta, dina) == 1 &&
          dense_stream_main_blocks(tb, dinb) == 1 && ta.ptr[0] == tb.ptr[0]};
}
struct DenseChainFwd {   // a two-layer chain: one launch over n_main 64-wide blocks, or (0) a dense_fwd_plan per layer
  int n_main = 0;
  KernelNames names() const {
    return n_main == 1 ? KernelNames{"dense_chain_fwd_kernel<1>"} : n_main == 2 ? KernelNames{"dense_chain_fwd_kernel<2>"} : KernelNames{};
  }
};
inline DenseChainFwd dense_chain_fwd_plan(int64_t n, const SegTable &t1, int din1, int dmid, int dout2) {
  const int nm = dense_stream_main_blocks(t1, din1);
  return {(dense_stream2_enabled(n) && dmid == kDenseCols64 && dout2 <= kDenseCols64 && (nm == 1 || nm == 2)) ? nm : 0};
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------
// The whole pullback as one streaming launch: 64 outputs, one or two blocks of exactly 64 features (row_div 1, 16-byte aligned, their
// gradient too), every other feature narrow (<= 4 in total) and without a gradient request, enough rows for a resident wave of tiles,
// and the slabs fit the dz area of the caller's workspace.  NGPDE_DENSE_NO_STREAM_BWD=1 keeps the composed path.
struct DenseStreamBwd {
  int grid = 0;   // 0: not applicable
  int n_main = 0;
  bool main[4] = {false, false, false, false};   // block b is one of the 64-wide blocks (else: narrow features)
};
inline DenseStreamBwd dense_stream_bwd_plan(int64_t n, const SegTable &t, const SegGrad &g, int din, int dout) {
  DenseStreamBwd s;
  if (switch_on(Switch::DenseNoStreamBwd) || dout != kDenseCols64 || n < kDenseStreamBwdRows || n > kDenseStreamBwdMaxRows) return {};
  int n_narrow = 0;
  for (int b = 0; b < t.n; ++b) {
    if (t.width[b] == kDenseCols64 && t.row_div[b] == 1 && aligned16(t.ptr[b], g.ptr[b])) {
      s.main[b] = true;
      ++s.n_main;
    } else {
      if (g.ptr[b]) return {};
      n_narrow += t.width[b];
    }
  }
  if (s.n_main < 1 || s.n_main > 2 || n_narrow > kDenseNarrow) return {};
  int grid = (int)std::min<int64_t>(dense_cdiv(n, kDenseRows64), 256 * 2);
  grid = (int)std::min<int64_t>(grid, n / (din + 1));   // slabs live in the [n][64] dz area of the workspace
  if (grid < 256) return {};
  s.grid = grid;
  return s;
}

// grid of the small one-launch pullback, or 0 when the shape is not its own: widths up to 64, few enough rows that the composed path's
// launches are latency-bound (beyond that its 16-byte / LDS-DMA loads win), and enough rows for the slabs to fit the [n][dout] dz
// area of the composed path's workspace (which this form does not use otherwise)
inline int dense_small_bwd_grid(int64_t n, int din, int dout) {
  if (switch_on(Switch::DenseNoSmallBwd) || din < 1 || din > kDenseCols64 || dout < 1 || dout > kDenseCols64 || n < 1 || n > kDenseSmallRows) return 0;
  const int64_t grid = std::min<int64_t>(std::min<int64_t>(dense_cdiv(n, kDenseRows64), 1024), n / (din + 1));
  return grid >= 1 ? (int)grid : 0;
}

// the weight pullback into nchunk slabs of rpc rows each + their reduction; 128 x 128 tiles for a wide layer without bias gradient
// (GNOConv's T): slabs in the layout dense_weight_reduce_kernel sums
enum class DenseWeightForm { None, Gemm128Split, Mfma };
struct DenseBwdWeight {
  DenseWeightForm form = DenseWeightForm::None;
  int nchunk = 0;
  int64_t rpc = 0;
  KernelNames names() const {
    if (form == DenseWeightForm::None) return {};
    return {form == DenseWeightForm::Gemm128Split ? "dense_gemm128_split_kernel<true,false>" : "dense_mfma_bwd_weight_kernel",
            "dense_weight_reduce_kernel"};
  }
};
inline DenseBwdWeight dense_bwd_weight_plan(int64_t n, const SegTable &segs, int din, int dout, const void *dz, bool has_db, const void *partial) {
  DenseBwdWeight p;
  if (dout == 0) return p;
  p.nchunk = dense_weight_chunks(n, din, dout);
  p.rpc = std::max<int64_t>(kDenseK16, dense_cdiv(dense_cdiv(n, p.nchunk), kDenseK16) * kDenseK16);
  const bool gemm128 = !switch_on(Switch::DenseNoGemm128) && !has_db && p.nchunk > 1 && segs.n == 1 && segs.vec[0] && segs.row_div[0] == 1 &&
                       din >= kDenseRows128 && din % 4 == 0 && dout >= kDenseCols128 && dout % 4 == 0 && n % kDenseK16 == 0 && n < (1 << 30) &&
                       aligned16(dz, partial);
  p.form = gemm128 ? DenseWeightForm::Gemm128Split : DenseWeightForm::Mfma;
  return p;
}

// the input pullback: split over the output features into nz ranges of oper (128 x 128 tiles -- GNOConv's T = W2 (x) h: 4096 x 128
// <= 8192 -- or the 128-row kernel; add: add_partials_kernel sums the ranges), or whole (128-row tiles, 64-row tiles below)
enum class DenseInputForm { None, Gemm128Split, WideSplit, Wide, Mfma };
struct DenseBwdInput {
  DenseInputForm form = DenseInputForm::None;
  int oper = 0, nz = 0;
  bool add = false;
  KernelNames names() const {
    KernelNames k;
    switch (form) {
      case DenseInputForm::None: break;
      case DenseInputForm::Gemm128Split: k.push_back("dense_gemm128_split_kernel<false,true>"); break;
      case DenseInputForm::WideSplit:
      case DenseInputForm::Wide: k.push_back("dense_wide_bwd_input_kernel"); break;
      case DenseInputForm::Mfma: k.push_back("dense_mfma_bwd_input_kernel"); break;
    }
    if (add) k.push_back("add_partials_kernel");
    return k;
  }
};
// a single block's, with dense_bwd_input_splits > 1; `part` holds dense_bwd_input_split_bytes
inline DenseBwdInput dense_bwd_input_split_plan(int64_t n, int din, int dout, const void *dz, const void *wt, const void *dx, const void *part) {
  DenseBwdInput p;
  if (n == 0 || din == 0) return p;
  const int ns = dense_bwd_input_splits(n, din, dout);
  p.oper = (int)(dense_cdiv(dense_cdiv(dout, ns), kDenseK32) * kDenseK32);
  p.nz = (dout + p.oper - 1) / p.oper;
  if (!switch_on(Switch::DenseNoGemm128) && p.nz > 1 && din >= kDenseCols128 && din % 4 == 0 && dout % kDenseK16 == 0 && p.oper % kDenseK16 == 0 &&
      n < (1 << 30) && aligned16(dz, wt, dx, part)) {
    p.form = DenseInputForm::Gemm128Split;
    p.add = true;
  } else {
    p.form = DenseInputForm::WideSplit;
    p.add = p.nz > 1;
  }
  return p;
}
inline DenseBwdInput dense_bwd_input_plan(int64_t n, int din, int dout) {
  DenseBwdInput p;
  if (n == 0 || din == 0) return p;
  p.form = dense_wide_tiles(n, din) ? DenseInputForm::Wide : DenseInputForm::Mfma;
  p.oper = dout;
  p.nz = 1;
  return p;
}

enum class DenseBwdForm { None, Stream, Small, Composed };
struct DenseBwd {
  DenseBwdForm form = DenseBwdForm::None;   // None: no rows (the entry zeroes the weight gradients)
  DenseStreamBwd stream;                    // Stream
  int small_grid = 0;                       // Small
  // Composed: the workspace's pieces, whether dz = dy . act'(z) is computed (else dz is dy itself), the two pullbacks
  DenseBwdWs ws = {nullptr, nullptr, nullptr};
  bool dz = false;
  DenseBwdWeight weight;
  DenseBwdInput input;
  KernelNames names() const {
    if (form == DenseBwdForm::None) return {};
    if (form == DenseBwdForm::Stream) return {stream.n_main == 1 ? "dense_stream64_bwd_kernel<1>" : "dense_stream64_bwd_kernel<2>", "dense_weight_reduce_kernel"};
    if (form == DenseBwdForm::Small) return {"dense_small_bwd_kernel", "dense_weight_reduce_kernel"};
    KernelNames k;
    if (dz) k.push_back("dense_dz_kernel");
    for (const KernelNames &part : {weight.names(), input.names()}) k.insert(k.end(), part.begin(), part.end());
    return k;
  }
};
inline DenseBwd dense_bwd_plan(int64_t n, const SegTable &t, const SegGrad &g, int din, int dout, bool act_identity, bool has_bias, const void *wt,
                               const void *dy, void *workspace) {
  DenseBwd p;
  if (n == 0) return p;
  if ((p.stream = dense_stream_bwd_plan(n, t, g, din, dout)).grid) {   // one streaming launch (slabs in the dz area)
    p.form = DenseBwdForm::Stream;
    return p;
  }
  if ((p.small_grid = dense_small_bwd_grid(n, din, dout))) {   // at most 64 x 64, latency-bound row counts: one launch too
    p.form = DenseBwdForm::Small;
    return p;
  }
  p.form = DenseBwdForm::Composed;
  Workspace w(workspace);
  dense_bwd_layout(w, n, din, dout, p.ws);
  p.dz = !act_identity;
  const void *dz = act_identity ? dy : p.ws.dz;
  p.weight = dense_bwd_weight_plan(n, t, din, dout, dz, has_bias, p.ws.partial);
  if (any_grad(g)) {
    if (t.n == 1 && dense_bwd_input_splits(n, din, dout) > 1)   // few rows, very wide output: split the contraction
      p.input = dense_bwd_input_split_plan(n, din, dout, dz, wt, g.ptr[0], p.ws.split_part);
    else
      p.input = dense_bwd_input_plan(n, din, dout);
  }
  return p;
}

// ---- the pair pullback: both sides one 64-wide leading block at the SAME address + narrow blocks, 64 outputs, no activation -----------
struct DensePairBwd {
  int grid = 0;   // 0: not applicable
  size_t workspace_bytes = 0;
  KernelNames names() const {
    return grid ? KernelNames{"dense_pair64_bwd_kernel", "dense_weight_reduce_kernel", "dense_weight_reduce_kernel"} : KernelNames{};
  }
};
inline bool dense_pair_side_ok(const SegTable &t, int din) {
  if (t.n < 1 || t.width[0] != kDenseCols64 || t.row_div[0] != 1 || !aligned16(t.ptr[0])) return false;
  return din - kDenseCols64 <= kDenseNarrow;
}
inline DensePairBwd dense_pair_bwd_plan(int64_t n, const SegTable &ta, int dina, const SegTable &tb, int dinb, int dout) {
  DensePairBwd p;
  if (dout != kDenseCols64 || switch_on(Switch::DenseNoStreamBwd) || n < kDenseStreamBwdRows || n > kDenseStreamBwdMaxRows) return p;
  if (!dense_pair_side_ok(ta, dina) || !dense_pair_side_ok(tb, dinb) || ta.ptr[0] != tb.ptr[0]) return p;
  p.grid = (int)std::min<int64_t>(dense_cdiv(n, kDenseRows64), 256 * 2);
  p.workspace_bytes = (size_t)p.grid * (dina + dinb + 2) * kDenseCols64 * sizeof(float) + 512;
  return p;
}

}  // namespace ngpde
