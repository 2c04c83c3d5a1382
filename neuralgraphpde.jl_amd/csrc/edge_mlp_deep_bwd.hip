// edge_mlp_deep_bwd.hip -- fused pullback of the edge-function layers' message path for message MLPs of THREE or FOUR Dense layers
//   m_i = aggr_{e: t_e = i} phi([h_i; h_j; ...]),  phi = Dense -> Dense -> Dense [-> Dense]
// (/root/reference/src/layers.jl:103-111, :313-326, :402-416; the VMH tutorial's phi = 4 => 60 => 60 => 60 => 40, tanh:
// /root/reference/docs/src/tutorials/VMH.md:75-83).  edge_mlp_fused.hip's pullback stops at two layers; deeper phi used to take the
// primitives' path: every layer's [E][h] pre-activations written by the forward and read back, ~12 launches.  Here, as there:
//   * the forward saves NOTHING per edge: a wave recomputes the chain z1 -> a1 -> z2 -> ... for its 16 edges in registers
//     (transposed products z^T = W^T a^T, whose result layout is again the operand layout: edge_mlp_fused.hip), keeping every
//     layer's activation and derivative;
//   * then walks back: dz_l = g . act_l'(z_l), db_l += dz_l, dW_l += a_{l-1}^T dz_l on the matrix pipe (operands transposed through
//     the wave's 4 KB of LDS), g <- W_l dz_l^T;
//   * dz1 is written once ([E][h1]: the gradient of the per-edge first-layer term and the input of the by-source sum) and summed
//     per target through LDS (dP).
// Registers are what this needs (three layers: 7 x 16 for activations / derivatives, 3 x 64 weight-gradient accumulators), so a
// workgroup is 4 waves with one wave per SIMD (512 registers per lane, accumulators in the AccVGPR half) and one workgroup per CU;
// both orientations of every tail weight stay in LDS (104 KB at three tail layers).  Sized for the tutorials' graphs (thousands of
// nodes: a launch is a handful of tiles per workgroup), not for BASELINE config 4, whose two-layer phi has its own kernels.
#include <algorithm>

#include "common.h"
#include "device_utils.h"
#include "edge_mlp_tile.h"

namespace ngpde {

namespace {

using Shape = TwoRowsPerGroup;   // (kT4, kChunk4, kMaxTail, kW, kTS, kRows: edge_mlp_forms.h)

struct DeepBwdK : EdgeTileArgs {
  int h1, act1, aggr, n_tail;
  int dout[kMaxTail], act[kMaxTail];
  const float *P, *Q, *Eterm, *dout_grad;
  const float *wt[kMaxTail], *bias[kMaxTail];
  float *dP, *dE;
  float *partial[kMaxTail];   // per tail layer: [n_workgroups][(din_l + 1)][dout_l]  (row din_l = bias gradient)
};

template <int NT>
__global__ __launch_bounds__(kT4, 1) void edge_mlp_deep_bwd_kernel(const DeepBwdK p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float *ldsQ = dyn;                                              // [halo_rows + 1][kTS]
  float *ldsP = ldsQ + (size_t)(p.halo_rows + 1) * kTS;           // [32][kTS]
  float *ldsS = ldsP + kRows * kTS;                               // [64][kTS]  wave-private transposes, then dz1 of the chunk
  float *ldsWf = ldsS + kChunk4 * kTS;                            // [NT][64 out][kTS]  W_l^T
  float *ldsWb = ldsWf + (size_t)NT * kW * kTS;                   // [NT][64 in][kTS]   W_l
  __shared__ int ldsOff[kRows + 1], ldsRs[kRows], ldsNode[kRows];
  __shared__ float ldsInv[kRows];
  __shared__ __attribute__((aligned(16))) unsigned ldsSlots[kRows * 8];
  __shared__ uint16_t ldsEdge[kRows * kSlotWidth];
  __shared__ __attribute__((aligned(16))) float ldsBias[NT * kW];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g16 = tid >> 4, q = tid & 15;
  const int ei = lane & 15, kq = lane >> 4;
  const int h1 = p.h1, zero_slot = p.halo_rows;

  const EdgeTileRange tr(p.n_tiles);

  // ---- once per workgroup: both orientations of every tail weight (zero-padded to 64 x 64), the biases, the all-zero halo row
#pragma unroll
  for (int l = 0; l < NT; ++l)
    stage_weights<kT4, true, true>(p.wt[l], p.bias[l], l == 0 ? h1 : p.dout[l - 1], p.dout[l], tid, ldsWf + (size_t)l * kW * kTS, ldsWb + (size_t)l * kW * kTS,
                                   ldsBias + l * kW);
  zero_halo_row(ldsQ, zero_slot, g16, q);

  // weight / bias gradient accumulators of this wave, per tail layer: tile (ct, mt) <-> inputs 16 ct .. + 15 x outputs 16 mt .. + 15
  f32x4 accW[NT][4][4];
  float4 dbacc[NT][4];
#pragma unroll
  for (int l = 0; l < NT; ++l)
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      dbacc[l][a] = f4_zero();
#pragma unroll
      for (int b = 0; b < 4; ++b) accW[l][a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }

  TileMeta<Shape> meta;
  int jt = tr.wg_in_xcd;
  if (jt < tr.range_len) fetch_meta(p, tr.range_lo + jt, g16, q, meta);

  for (; jt < tr.range_len; jt += tr.wgs_per_xcd) {
    const int4 sc0 = meta.sc0, sc1 = meta.sc1;
    {   // stage the tile: P rows and the distinct Q rows
      TileRows<Shape> rows;
      fetch_rows<true>(p.P, p.Q, h1, p.halo_rows, meta, g16, q, rows);
      stage_rows(rows, p.halo_rows, g16, q, ldsQ, ldsP);
    }
    stage_tile_degrees<true, true>(meta, g16, q, p.aggr == NGPDE_AGGR_MEAN, ldsOff, ldsSlots, ldsRs, ldsNode, ldsInv);
    const int jn = jt + tr.wgs_per_xcd;
    if (jn < tr.range_len) fetch_meta(p, tr.range_lo + jn, g16, q, meta);
    __syncthreads();
    scan_tile_degrees(ldsOff, tid);
    __syncthreads();
    int total, lo0, hi0, lo1, hi1;
    expand_tile_edges(ldsOff, ldsSlots, ldsEdge, g16, q, total, lo0, hi0, lo1, hi1);
    float4 racc0 = f4_zero(), racc1 = f4_zero();
    __syncthreads();

    for (int c0 = 0; c0 < total; c0 += kChunk4) {
      const bool wave_on = c0 + wave * 16 < total;   // wave-uniform
      const int k = c0 + wave * 16 + ei;
      const bool valid = k < total;
      float *mine = ldsS + (size_t)(wave * 16) * kTS;          // this wave's 16 rows of the staging tile
      float4 dz1[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
      if (wave_on) {
        int r, slot;
        size_t pe;
        lane_edge(ldsEdge, ldsOff, ldsRs, k, valid, zero_slot, r, slot, pe);
        const int dlast = p.dout[NT - 1];
        // incoming gradient rows of the edge's target (x 1 / deg for mean): issued now, used behind the recomputed chain
        float4 g[4];
        {
          const float *grow = p.dout_grad + (size_t)ldsNode[r] * dlast + 4 * kq;
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) g[mt] = (16 * mt + 4 * kq < dlast) ? *reinterpret_cast<const float4 *>(grow + 16 * mt) : f4_zero();
        }
        const float inv = valid ? ldsInv[r] : 0.f;
        // ---- the chain, recomputed: a[l] = input of tail layer l, d[l] = derivative of the activation that produced it
        // (d[0]: act1'(z1); d[l + 1]: act_l'(z_{l + 1})); padded features and edges beyond the tile are zero throughout
        float4 a[NT][4], d[NT + 1][4];
        first_layer(ldsP, ldsQ, p.Eterm, h1, p.act1, r, slot, pe, valid, kq, d[0], a[0]);
        f4n_dact<4>(p.act1, d[0]);
#pragma unroll
        for (int l = 0; l < NT; ++l) {
          const int din = l == 0 ? h1 : p.dout[l - 1], dw = p.dout[l];
          float4 z[4];
          dense_transposed<true>(ldsWf + (size_t)l * kW * kTS, ldsBias + l * kW, din, dw, ei, kq, a[l], z);
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) d[l + 1][mt] = z[mt];
          f4n_dact<4>(p.act[l], d[l + 1]);
          if (l + 1 < NT) {
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) a[l + 1][mt] = z[mt];
            f4n_act<4>(p.act[l], a[l + 1]);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
              if (!(valid && 16 * mt + 4 * kq < dw)) a[l + 1][mt] = f4_zero();
          }
        }
        // ---- back through the tail layers
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) g[mt] = (valid && 16 * mt + 4 * kq < dlast) ? f4_scale(inv, g[mt]) : f4_zero();
#pragma unroll
        for (int l = NT - 1; l >= 0; --l) {
          const int din = l == 0 ? h1 : p.dout[l - 1], dw = p.dout[l];
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) {
            g[mt] = f4_mul(g[mt], d[l + 1][mt]);                 // dz_{l+1}; zero for invalid edges / padded features
            dbacc[l][mt] = f4_add(dbacc[l][mt], g[mt]);
          }
          weight_grad_products<true>(mine, a[l], g, din, dw, ei, kq, accW[l]);   // dW_l += a_l^T dz
          // g <- W_l dz^T (transposed product): the gradient w.r.t. a_l
          float4 gn[4];
          dense_transposed<false>(ldsWb + (size_t)l * kW * kTS, nullptr, dw, din, ei, kq, g, gn);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) g[ct] = gn[ct];
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int f = 16 * ct + 4 * kq;
          dz1[ct] = (valid && f < h1) ? f4_mul(g[ct], d[0][ct]) : f4_zero();
          if (valid && f < h1 && p.dE) *reinterpret_cast<float4 *>(p.dE + pe * h1 + f) = dz1[ct];
        }
      }
      // ---- dz1 of the chunk -> LDS, lane group g16 sums the rows of targets g16 and g16 + 16 in edge order (= dP)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<float4 *>(&mine[ei * kTS + 16 * ct + 4 * kq]) = dz1[ct];
      __syncthreads();
      row_sum_chunk(ldsS, c0, kChunk4, lo0, hi0, q, racc0);
      row_sum_chunk(ldsS, c0, kChunk4, lo1, hi1, q, racc1);
      __syncthreads();
    }
    if (p.dP && 4 * q < h1) {
      if (sc0.x >= 0) *reinterpret_cast<float4 *>(p.dP + (size_t)sc0.x * h1 + 4 * q) = racc0;
      if (sc1.x >= 0) *reinterpret_cast<float4 *>(p.dP + (size_t)sc1.x * h1 + 4 * q) = racc1;
    }
  }

  // ---- per layer: fold the waves' accumulators into this workgroup's slab, wave by wave (fixed order), and write it out
#pragma unroll
  for (int l = 0; l < NT; ++l) {
    const int din = l == 0 ? h1 : p.dout[l - 1], dw = p.dout[l];
    float *slab = ldsS;                                            // [(din + 1)][dw] <= 65 x 64 floats <= [64][kTS]
    __syncthreads();
    for (int idx = tid; idx < (din + 1) * dw; idx += kT4) slab[idx] = 0.f;
    fold_bias_lanes(dbacc[l]);   // db: sum the 16 edge lanes of each k-quarter inside the wave first
    __syncthreads();
    for (int w = 0; w < kT4 / 64; ++w) {
      if (wave == w) fold_slab<true>(slab, din, dw, accW[l], dbacc[l], ei, kq);
      __syncthreads();
    }
    float *dst = p.partial[l] + (size_t)blockIdx.x * (din + 1) * dw;
    for (int idx = tid; idx < (din + 1) * dw; idx += kT4) dst[idx] = slab[idx];
  }
}

}  // namespace

int32_t launch_edge_mlp_deep_bwd(const ngpde_graph *g, const EdgeBwd &p, const EdgeMlpBwdArgs &a, hipStream_t stream) {
  NGPDE_REQUIRE(p.supported, NGPDE_ERR_UNSUPPORTED,
                "deep fused edge-MLP pullback needs widths <= 64 and multiples of 4, 2 or 3 layers after the first, + or mean "
                "aggregation and a graph whose tiles fit the LDS halo");
  if (!p.launch) return NGPDE_OK;   // no nodes
  if (int32_t st = check_workspace("deep fused edge-MLP pullback", a.workspace, a.workspace_bytes, p.workspace_bytes, 1)) return st;
  NGPDE_REQUIRE(!p.dE_missing, NGPDE_ERR_INVALID_ARGUMENT, "deep fused edge-MLP pullback: the [E][h1] buffer dE is required");
  const EdgeMlpDesc &d = a.d;
  const TileGeom t = tile_geom(g);
  DeepBwdK k;
  fill_tile_args(g, t, k);
  k.h1 = d.h1; k.act1 = d.act1; k.aggr = d.aggr; k.n_tail = d.n_tail;
  k.P = a.P; k.Q = a.Q; k.Eterm = a.Eterm; k.dout_grad = a.dout; k.dP = a.dP; k.dE = a.dE;
  Workspace w(a.workspace);
  EdgeBwdWs ws;
  edge_mlp_bwd_layout(w, t, d, p.form, ws);
  for (int l = 0; l < kMaxTail; ++l) {
    k.partial[l] = ws.partial[l];
    k.dout[l] = d.dout[l]; k.act[l] = d.act[l]; k.wt[l] = a.wt[l]; k.bias[l] = a.bias[l];   // (zero / NULL from n_tail on)
  }
  int32_t st = p.n_tail == 2 ? launch_with_lds(edge_mlp_deep_bwd_kernel<2>, p.grid, p.threads, p.lds, stream, k, "edge_mlp_deep_bwd_kernel")
                             : launch_with_lds(edge_mlp_deep_bwd_kernel<3>, p.grid, p.threads, p.lds, stream, k, "edge_mlp_deep_bwd_kernel");
  if (st) return st;
  for (int l = 0; l < p.n_tail; ++l)
    if ((st = launch_dense_weight_reduce(p.grid, d.din(l), d.dout[l], k.partial[l], a.dwt[l], a.dbias[l], stream))) return st;
  if (p.by_source && (st = launch_edge_sum_by_source(g, d.h1, a.dE, a.dQ, stream))) return st;
  return NGPDE_OK;
}

}  // namespace ngpde
