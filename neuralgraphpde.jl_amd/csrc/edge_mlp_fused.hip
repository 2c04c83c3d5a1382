// edge_mlp_fused.hip -- fused forward of the edge-function layers' message path
//   m_i = aggr_{e: t_e = i}  phi( [h_i; h_j; ...] )      (/root/reference/src/layers.jl:103-111, :313-326, :402-416)
// for message MLPs phi = Dense, Dense, ... up to 64 wide: one launch does
//   gather (LDS-staged distinct source rows of the tile) -> z1_e = P[t_e] + Q[s_e] + E_e -> act ->
//   the remaining Dense layers on fp32 MFMA with the weights resident in LDS -> in-tile segmented reduction,
// so no [E][h] array is written unless the caller asks for the pre-activations (training).  The reference
// materialises gather(x, t), gather(x, s), their vcat and every layer's activations over all E edges.
//
// A workgroup (8 waves) owns one 32-row tile of the locality schedule and walks the tile's edges in chunks of
// 64 (4 MFMA row tiles); per chunk and Dense layer each wave issues 32 v_mfma_f32_16x16x4_f32.  Row r of the
// tile is summed by lane group r in edge (= COO) order: no atomics, bitwise reproducible.
#include <algorithm>

#include "common.h"
#include "device_utils.h"
#include "edge_mlp_tile.h"
#include "stamps.h"

namespace ngpde {

namespace {

using Shape = RowPerGroup;   // (kT, kChunk = 8 waves x 16 edges, kGroups, kW, kTS: edge_mlp_forms.h)

struct EdgeMlpK : EdgeTileArgs {
  int h1, act1, aggr;
  const float *P, *Q, *Eterm;
  int n_tail;
  int din[3], dout[3], act[3];
  const float *wt[3], *bias[3];
  float *out;
  float *save_z[4];   // [0]: z1 [E][h1]; [k]: pre-activation of tail layer k [E][dout_k]; nullable
  NGPDE_STAMP_FIELD
};

// Register-chained message MLP.  A wave owns 16 edges of the chunk; lane (i = lane & 15, kq = lane >> 4) holds, for edge i,
// the features {16 ct + 4 kq + r : ct = 0..3, r = 0..3} of the current activation as four float4.  A Dense layer is
// evaluated TRANSPOSED, z^T = W^T a^T, with v_mfma_f32_16x16x4_f32(A = W^T tile from LDS, B = a^T from registers): the D
// layout of that product (row = output feature 4 kq + r, column = edge i) is again exactly this register layout, so the
// layers chain in registers -- no LDS round trip and no barrier between assemble, Dense layers, bias and activation.
// MFMA step (ct, r) contracts, in lane kq, feature 16 ct + 4 kq + r of both operands (the order of a sum's terms is free).
template <int NTAIL>
__global__ __launch_bounds__(kT, (NTAIL <= 1 ? 4 : 2)) void edge_mlp_fused_fwd_kernel(const EdgeMlpK p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float *ldsQ = dyn;                                              // [halo_rows + 1][kTS]  rows of Q the tile references
  float *ldsP = ldsQ + (size_t)(p.halo_rows + 1) * kTS;           // [32][kTS]             P rows of the tile's targets
  float *ldsWt = ldsP + kGroups * kTS;                            // [NTAIL][64 out][kTS]  tail weights, W^T
  float *ldsMsg = ldsWt + (size_t)NTAIL * kW * kTS;               // [kChunk][kTS]         messages of the chunk
  __shared__ int ldsOff[kGroups + 1], ldsRs[kGroups];
  __shared__ __attribute__((aligned(16))) unsigned ldsSlots[kGroups * 8];   // 32 slot bytes per row
  __shared__ uint8_t ldsRowOf[kGroups * kSlotWidth];                        // tile edge k -> row of the tile
  __shared__ __attribute__((aligned(16))) float ldsBias[(NTAIL > 0 ? NTAIL : 1) * kW];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = tid >> 4, q = tid & 15;           // staging / reduction role: group g <-> row g, lane q <-> features 4q..4q+3
  const int ei = lane & 15, kq = lane >> 4;         // MFMA role: edge ei of the wave's 16, k-quarter kq
  const int h1 = p.h1, zero_slot = p.halo_rows;

  const EdgeTileRange tr(p.n_tiles);   // persistent workgroup: strides through its XCD's range of tiles

  // ---- once per workgroup: tail weights as W^T rows (output j, contiguous inputs) and biases in LDS
  // (all loads of all layers first, unconditional from clamped addresses, pinned, then selected and written: a `cond ? load : 0` is an
  // exec-masked branch per load, and with one tile per workgroup -- a 3 000-node graph -- this prologue is most of the launch)
  {
    const int j = tid % kW, kg0 = tid / kW;   // output column j, input quads kg0 and kg0 + 8
    float t[NTAIL > 0 ? NTAIL : 1][2][4];
#pragma unroll
    for (int l = 0; l < NTAIL; ++l) {
      const int dinl = p.din[l], doutl = p.dout[l];
      const float *w = p.wt[l] + min(j, doutl - 1);
#pragma unroll
      for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int r = 0; r < 4; ++r) t[l][ps][r] = w[min(4 * (kg0 + 8 * ps) + r, dinl - 1) * doutl];
    }
#pragma unroll
    for (int l = 0; l < NTAIL; ++l)
#pragma unroll
      for (int ps = 0; ps < 2; ++ps)
#pragma unroll
        for (int r = 0; r < 4; ++r) asm volatile("" : "+v"(t[l][ps][r]));
#pragma unroll
    for (int l = 0; l < NTAIL; ++l) {
      const int dinl = p.din[l], doutl = p.dout[l];
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        const int k = 4 * (kg0 + 8 * ps);
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (k + r < dinl && j < doutl) ? t[l][ps][r] : 0.f;
        *reinterpret_cast<float4 *>(&ldsWt[l * kW * kTS + j * kTS + k]) = make_float4(v[0], v[1], v[2], v[3]);
      }
      if (tid < kW) ldsBias[l * kW + tid] = (p.bias[l] && tid < doutl) ? p.bias[l][tid] : 0.f;
    }
  }
  zero_halo_row(ldsQ, zero_slot, grp, q);

  TileMeta<Shape> meta;
  TileRows<Shape> rows;
  int jt = tr.wg_in_xcd;
  if (jt < tr.range_len) {
    fetch_meta(p, tr.range_lo + jt, grp, q, meta);
    fetch_rows<true>(p.P, p.Q, h1, p.halo_rows, meta, grp, q, rows);
  }
  const int last_w = (NTAIL > 0) ? p.dout[NTAIL - 1] : h1;

  for (; jt < tr.range_len; jt += tr.wgs_per_xcd) {
    const bool first_tile = (jt == tr.wg_in_xcd + 4 * tr.wgs_per_xcd);   // a tile in steady state (the fifth of the workgroup)
    if (first_tile) { NGPDE_STAMP(p.stamps, 16, 0, memtime); NGPDE_STAMP(p.stamps, 16, 8, memrealtime); }
    // ---- stage this tile (fetched under the previous tile's arithmetic)
    const int4 sc = meta.sc;
    stage_rows(rows, p.halo_rows, grp, q, ldsQ, ldsP);
    stage_tile_degrees<true>(meta, grp, q, ldsOff, ldsSlots, ldsRs);   // degrees; turned into offsets below
    // ---- next tile: metadata now (one L2 round trip, lands during the prefix sums), rows after the first chunk
    const int jn = jt + tr.wgs_per_xcd;
    const bool has_next = jn < tr.range_len;       // workgroup-uniform
    if (has_next) fetch_meta(p, tr.range_lo + jn, grp, q, meta);
    __syncthreads();
    scan_tile_degrees(ldsOff, tid);
    __syncthreads();
    int total, my_lo, my_hi;
    expand_tile_edges(ldsOff, ldsRowOf, grp, q, total, my_lo, my_hi);

    float4 racc;
    if (p.aggr == NGPDE_AGGR_MAX) racc = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    else if (p.aggr == NGPDE_AGGR_MIN) racc = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    else if (p.aggr == NGPDE_AGGR_MUL) racc = make_float4(1.f, 1.f, 1.f, 1.f);   // scatter(*): the neutral element (an empty neighbourhood gives 1)
    else racc = f4_zero();
    __syncthreads();
    if (first_tile) NGPDE_STAMP(p.stamps, 16, 1, memtime);

    bool rows_fetched = false;
    for (int c0 = 0; c0 < total; c0 += kChunk) {
      // ---- this lane's edge: row, halo slot, position in p order (a wave past the tile's last edge only joins the barriers)
      const bool wave_on = c0 + wave * 16 < total;   // wave-uniform
      const int k = c0 + wave * 16 + ei;
      const bool valid = k < total;
      int r, slot;
      size_t pe;
      lane_edge(ldsRowOf, ldsOff, ldsSlots, ldsRs, k, valid, zero_slot, r, slot, pe);
      // ---- a1 = act1(P[t] + Q[s] + E), features 16 ct + 4 kq .. + 3
      float4 a[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
      if (wave_on) {
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const int f = 16 * ct + 4 * kq;
        float4 z = f4_add(*reinterpret_cast<const float4 *>(&ldsP[r * kTS + f]), *reinterpret_cast<const float4 *>(&ldsQ[slot * kTS + f]));
        if (p.Eterm && valid && f < h1) z = f4_add(z, *reinterpret_cast<const float4 *>(p.Eterm + pe * h1 + f));
        if (p.save_z[0] && valid && f < h1) *reinterpret_cast<float4 *>(p.save_z[0] + pe * h1 + f) = z;
        a[ct] = z;
      }
      f4n_act<4>(p.act1, a);                           // one uniform activation switch for the 16 values
#pragma unroll
      for (int ct = 0; ct < 4; ++ct)
        if (!(valid && 16 * ct + 4 * kq < h1)) a[ct] = f4_zero();
      }
      if (c0 == 0 && first_tile) NGPDE_STAMP(p.stamps, 16, 2, memtime);
      if (has_next && !rows_fetched) {   // the next tile's rows: in flight across this tile's MFMAs
        fetch_rows<true>(p.P, p.Q, h1, p.halo_rows, meta, grp, q, rows);
        rows_fetched = true;
      }
      // ---- remaining Dense layers, transposed product on MFMA, chained in registers
      if (wave_on) {
#pragma unroll
      for (int l = 0; l < NTAIL; ++l) {
        const int dw = p.dout[l];
        const int n_ct = (p.din[l] + 15) >> 4, n_mt = (dw + 15) >> 4;   // uniform
        const float *wl = ldsWt + l * kW * kTS + ei * kTS + 4 * kq;
        f32x4 acc[4];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
          if (mt < n_mt) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
              if (ct < n_ct) {
                const float4 w4 = *reinterpret_cast<const float4 *>(wl + mt * 16 * kTS + 16 * ct);
                acc[mt] = mfma16(w4.x, a[ct].x, acc[mt]);
                acc[mt] = mfma16(w4.y, a[ct].y, acc[mt]);
                acc[mt] = mfma16(w4.z, a[ct].z, acc[mt]);
                acc[mt] = mfma16(w4.w, a[ct].w, acc[mt]);
              }
            }
          }
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const int f = 16 * mt + 4 * kq;
          const float4 b4 = *reinterpret_cast<const float4 *>(&ldsBias[l * kW + f]);
          const float4 z = make_float4(acc[mt][0] + b4.x, acc[mt][1] + b4.y, acc[mt][2] + b4.z, acc[mt][3] + b4.w);
          if (p.save_z[l + 1] && valid && f < dw) *reinterpret_cast<float4 *>(p.save_z[l + 1] + pe * dw + f) = z;
          a[mt] = z;
        }
        f4n_act<4>(p.act[l], a);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
          if (!(valid && 16 * mt + 4 * kq < dw)) a[mt] = f4_zero();
      }
      }
      if (c0 == 0 && first_tile) NGPDE_STAMP(p.stamps, 16, 3, memtime);
      // ---- messages of the chunk -> LDS, then lane group g sums the messages of row g in edge order
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
        *reinterpret_cast<float4 *>(&ldsMsg[(wave * 16 + ei) * kTS + 16 * mt + 4 * kq]) = a[mt];
      __syncthreads();
      if (c0 == 0 && first_tile) NGPDE_STAMP(p.stamps, 16, 4, memtime);
      row_fold_chunk(ldsMsg, c0, kChunk, my_lo, my_hi, q, racc, [&](float4 acc, float4 m) {
        if (p.aggr == NGPDE_AGGR_MAX) return make_float4(fmaxf(acc.x, m.x), fmaxf(acc.y, m.y), fmaxf(acc.z, m.z), fmaxf(acc.w, m.w));
        if (p.aggr == NGPDE_AGGR_MIN) return make_float4(fminf(acc.x, m.x), fminf(acc.y, m.y), fminf(acc.z, m.z), fminf(acc.w, m.w));
        if (p.aggr == NGPDE_AGGR_MUL) return f4_mul(acc, m);
        return f4_add(acc, m);
      });
      __syncthreads();
      if (c0 == 0 && first_tile) NGPDE_STAMP(p.stamps, 16, 5, memtime);
    }
    if (first_tile) NGPDE_STAMP(p.stamps, 16, 6, memtime);
    if (has_next && !rows_fetched) fetch_rows<true>(p.P, p.Q, h1, p.halo_rows, meta, grp, q, rows);   // a tile without edges
    if (sc.x >= 0 && 4 * q < last_w) {
      const int deg = my_hi - my_lo;
      if (p.aggr == NGPDE_AGGR_MEAN) racc = deg > 0 ? f4_scale(1.0f / (float)deg, racc) : f4_zero();
      *reinterpret_cast<float4 *>(p.out + (size_t)sc.x * last_w + 4 * q) = racc;
    }
    if (first_tile) { NGPDE_STAMP(p.stamps, 16, 7, memtime); NGPDE_STAMP(p.stamps, 16, 9, memrealtime); }
  }
}

// ---- fused pullback of the message path (0 or 1 Dense layer after the first) -------------------------------------------------
// Same tiling, staging and register layout as the forward kernel.  Per 16-edge wave slice, all in registers:
//   z1 = P[t] + Q[s] + E, a1 = act1(z1)                         (recomputed: nothing per-edge was saved by the forward)
//   z2^T = W2^T a1^T + b2            (MFMA, transposed product)   dz2 = g[t] * act2'(z2),  g = dout / deg (mean) or dout (+)
//   da1^T = W2 dz2^T                 (MFMA, transposed product)   dz1 = da1 * act1'(z1)
//   dW2 += a1^T dz2                  (MFMA over the wave's 16 edges; the two operands are transposed through a wave-private
//                                     4 KB LDS tile; 16 accumulator tiles per wave live for the whole kernel)
// dz1 goes to HBM once ([E][h1], p order: it is dE and the input of the by-source sum that gives dQ) and through LDS into
// the in-tile segmented sum that gives dP.  At the end the 8 waves fold their dW2 / db2 accumulators into one slab per
// workgroup in a fixed order; a reduce kernel sums the slabs.  No atomics.
struct EdgeMlpBwdK : EdgeTileArgs {
  int h1, act1, aggr, n_tail, dw, act2;   // dw = width of the tail layer's output (NTAIL = 1)
  const float *P, *Q, *Eterm, *wt, *bias, *dout;
  float *dP, *dE, *partial;   // partial: [n_workgroups][(h1 + 1)][dw]  (row h1 = bias gradient)
};

template <int NTAIL>
__global__ __launch_bounds__(kT, 2) void edge_mlp_fused_bwd_kernel(const EdgeMlpBwdK p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float *ldsQ = dyn;                                              // [halo_rows + 1][kTS]
  float *ldsP = ldsQ + (size_t)(p.halo_rows + 1) * kTS;           // [32][kTS]
  float *ldsG = ldsP + kGroups * kTS;                             // [32][kTS]  incoming gradient rows (already / deg for mean)
  float *ldsS = ldsG + kGroups * kTS;                             // [kChunk][kTS]  wave-private transposes, then dz1 of the chunk
  float *ldsWf = ldsS + kChunk * kTS;                             // [64 out][kTS]  W2^T   (NTAIL = 1)
  float *ldsWb = ldsWf + (NTAIL ? kW * kTS : 0);                  // [64 in][kTS]   W2
  float *ldsZc = ldsWb + (NTAIL ? kW * kTS : 0);                  // [32][kTS]  aggr = *: how many of the target's messages are zero, per feature;
                                                                  //            max / min: the target's extremum
  __shared__ int ldsOff[kGroups + 1], ldsRs[kGroups];
  __shared__ __attribute__((aligned(16))) unsigned ldsSlots[kGroups * 8];
  __shared__ uint8_t ldsRowOf[kGroups * kSlotWidth];
  __shared__ __attribute__((aligned(16))) float ldsBias[kW];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = tid >> 4, q = tid & 15;
  const int ei = lane & 15, kq = lane >> 4;
  const int h1 = p.h1, zero_slot = p.halo_rows, dw = NTAIL ? p.dw : p.h1;

  const EdgeTileRange tr(p.n_tiles);

  if (NTAIL) stage_weights<kT, true, true>(p.wt, p.bias, h1, dw, tid, ldsWf, ldsWb, ldsBias);   // W2^T, W2, b2
  zero_halo_row(ldsQ, zero_slot, grp, q);

  // dW2 accumulators of this wave: tile (ct, mt) <-> rows 16 ct .. + 15 (inputs) x columns 16 mt .. + 15 (outputs)
  f32x4 accW[4][4];
  float4 dbacc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    dbacc[a] = f4_zero();
#pragma unroll
    for (int b = 0; b < 4; ++b) accW[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  const bool mul = p.aggr == NGPDE_AGGR_MUL, ext = p.aggr == NGPDE_AGGR_MAX || p.aggr == NGPDE_AGGR_MIN, want_max = p.aggr == NGPDE_AGGR_MAX;

  TileMeta<Shape> meta;
  int jt = tr.wg_in_xcd;
  if (jt < tr.range_len) fetch_meta(p, tr.range_lo + jt, grp, q, meta);

  for (; jt < tr.range_len; jt += tr.wgs_per_xcd) {
    const int4 sc = meta.sc;
    // ---- stage the tile: Q halo rows, P rows, gradient rows (the loads of a tile are issued here; the next tile's metadata
    // is prefetched below)
    {
      const int node = max(sc.x, 0);
      TileRows<Shape> rows;
      fetch_rows<true>(p.P, p.Q, h1, p.halo_rows, meta, grp, q, rows);
      float4 grow = (sc.x >= 0 && 4 * q < dw) ? *reinterpret_cast<const float4 *>(p.dout + (size_t)node * dw + 4 * q) : f4_zero();
      if (p.aggr == NGPDE_AGGR_MEAN) grow = sc.z > 0 ? f4_scale(1.0f / (float)sc.z, grow) : f4_zero();
      stage_rows(rows, p.halo_rows, grp, q, ldsQ, ldsP);
      *reinterpret_cast<float4 *>(&ldsG[grp * kTS + 4 * q]) = grow;
    }
    stage_tile_degrees<true>(meta, grp, q, ldsOff, ldsSlots, ldsRs);
    const int jn = jt + tr.wgs_per_xcd;
    if (jn < tr.range_len) fetch_meta(p, tr.range_lo + jn, grp, q, meta);
    __syncthreads();
    scan_tile_degrees(ldsOff, tid);
    __syncthreads();
    int total, my_lo, my_hi;
    expand_tile_edges(ldsOff, ldsRowOf, grp, q, total, my_lo, my_hi);
    float4 racc = f4_zero();
    __syncthreads();

    if (mul || ext) {
      // ---- aggr = *: a first pass over the tile's edges recomputes the messages and leaves, per target and feature, the product of the
      // nonzero ones (folded into the gradient row) and the number of zeros; max / min: the target's extremum (the second pass gives the
      // gradient to every message equal to it, as NNlib's pullback of scatter(max) does)
      float4 pacc = make_float4(1.f, 1.f, 1.f, 1.f), zacc = f4_zero();
      const float e0 = want_max ? -INFINITY : INFINITY;
      float4 eacc = make_float4(e0, e0, e0, e0);
      for (int c0 = 0; c0 < total; c0 += kChunk) {
        const bool wave_on = c0 + wave * 16 < total;   // wave-uniform
        const int k = c0 + wave * 16 + ei;
        const bool valid = k < total;
        int r, slot;
        size_t pe;
        lane_edge(ldsRowOf, ldsOff, ldsSlots, ldsRs, k, valid, zero_slot, r, slot, pe);
        float *mine = ldsS + (size_t)(wave * 16) * kTS;
        float4 m[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
        if (wave_on) {
          float4 z1[4], a1[4];
          first_layer(ldsP, ldsQ, p.Eterm, h1, p.act1, r, slot, pe, valid, kq, z1, a1);   // the per-edge forward, recomputed
          if (NTAIL) {
            dense_transposed<true>(ldsWf, ldsBias, h1, dw, ei, kq, a1, m);
            f4n_act<4>(p.act2, m);
          } else {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) m[ct] = a1[ct];
          }
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<float4 *>(&mine[ei * kTS + 16 * mt + 4 * kq]) = m[mt];
        __syncthreads();
        {
          const int lo = max(my_lo, c0), hi = min(my_hi, c0 + kChunk);
          for (int kk = lo; kk < hi; ++kk) {
            const float4 v = *reinterpret_cast<const float4 *>(&ldsS[(kk - c0) * kTS + 4 * q]);
            pacc = make_float4(pacc.x * (v.x != 0.f ? v.x : 1.f), pacc.y * (v.y != 0.f ? v.y : 1.f), pacc.z * (v.z != 0.f ? v.z : 1.f),
                               pacc.w * (v.w != 0.f ? v.w : 1.f));
            zacc = make_float4(zacc.x + (v.x == 0.f ? 1.f : 0.f), zacc.y + (v.y == 0.f ? 1.f : 0.f), zacc.z + (v.z == 0.f ? 1.f : 0.f),
                               zacc.w + (v.w == 0.f ? 1.f : 0.f));
            eacc = want_max ? make_float4(fmaxf(eacc.x, v.x), fmaxf(eacc.y, v.y), fmaxf(eacc.z, v.z), fmaxf(eacc.w, v.w))
                            : make_float4(fminf(eacc.x, v.x), fminf(eacc.y, v.y), fminf(eacc.z, v.z), fminf(eacc.w, v.w));
          }
        }
        __syncthreads();
      }
      if (mul) {
        float4 *gr = reinterpret_cast<float4 *>(&ldsG[grp * kTS + 4 * q]);
        *gr = f4_mul(*gr, pacc);
      }
      *reinterpret_cast<float4 *>(&ldsZc[grp * kTS + 4 * q]) = mul ? zacc : eacc;
      __syncthreads();
    }

    for (int c0 = 0; c0 < total; c0 += kChunk) {
      const bool wave_on = c0 + wave * 16 < total;   // wave-uniform
      const int k = c0 + wave * 16 + ei;
      const bool valid = k < total;
      int r, slot;
      size_t pe;
      lane_edge(ldsRowOf, ldsOff, ldsSlots, ldsRs, k, valid, zero_slot, r, slot, pe);
      float *mine = ldsS + (size_t)(wave * 16) * kTS;          // this wave's 16 rows of the staging tile
      float4 dz1[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
      if (wave_on) {
        float4 z1[4], a1[4];
        first_layer(ldsP, ldsQ, p.Eterm, h1, p.act1, r, slot, pe, valid, kq, z1, a1);   // the per-edge forward, recomputed
        f4n_dact<4>(p.act1, z1);                       // z1 <- act1'(z1): only the derivative is needed from here on
        float4 gz[4];                                          // NTAIL = 0: g itself; NTAIL = 1: dz2 = g * act2'(z2)
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const int f = 16 * mt + 4 * kq;
          gz[mt] = (valid && f < dw) ? *reinterpret_cast<const float4 *>(&ldsG[r * kTS + f]) : f4_zero();
        }
        // aggr = *: dL/dm_e = g_i . (product of the target's OTHER messages) = (g_i . product of its nonzero messages) / m_e where
        // none of them is zero; the one zero message of a row gets the product of the others; two zeros leave nothing
        auto others = [&](float4 (&gv)[4], const float4 (&m)[4]) {
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) {
            const int f = 16 * mt + 4 * kq;
            const float4 zc = (valid && f < dw) ? *reinterpret_cast<const float4 *>(&ldsZc[r * kTS + f]) : make_float4(2.f, 2.f, 2.f, 2.f);
            if (ext) {   // (zc holds the extremum; invalid edges / padded features carry a zero gradient already)
              gv[mt] = make_float4(m[mt].x == zc.x ? gv[mt].x : 0.f, m[mt].y == zc.y ? gv[mt].y : 0.f, m[mt].z == zc.z ? gv[mt].z : 0.f,
                                   m[mt].w == zc.w ? gv[mt].w : 0.f);
              continue;
            }
            auto one = [](float g, float mm, float z) { return mm != 0.f ? (z == 0.f ? g / mm : 0.f) : (z == 1.f ? g : 0.f); };
            gv[mt] = make_float4(one(gv[mt].x, m[mt].x, zc.x), one(gv[mt].y, m[mt].y, zc.y), one(gv[mt].z, m[mt].z, zc.z), one(gv[mt].w, m[mt].w, zc.w));
          }
        };
        if (!NTAIL && (mul || ext)) others(gz, a1);
        if (NTAIL) {
          // ---- z2 (transposed product), dz2
          float4 z2[4];
          dense_transposed<true>(ldsWf, ldsBias, h1, dw, ei, kq, a1, z2);
          if (mul || ext) {
            float4 m2[4] = {z2[0], z2[1], z2[2], z2[3]};
            f4n_act<4>(p.act2, m2);
            others(gz, m2);
          }
          f4n_dact<4>(p.act2, z2);
#pragma unroll
          for (int mt = 0; mt < 4; ++mt) {
            gz[mt] = f4_mul(gz[mt], z2[mt]);                  // g is zero for invalid edges / padded features
            dbacc[mt] = f4_add(dbacc[mt], gz[mt]);
          }
          weight_grad_products<true>(mine, a1, gz, h1, dw, ei, kq, accW);   // dW2 += a1^T dz2
          // ---- da1 (transposed product with W2), dz1
          float4 da1[4];
          dense_transposed<false>(ldsWb, nullptr, dw, h1, ei, kq, gz, da1);
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) dz1[ct] = f4_mul(da1[ct], z1[ct]);
        } else {
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) dz1[ct] = f4_mul(gz[ct], z1[ct]);
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int f = 16 * ct + 4 * kq;
          if (!(valid && f < h1)) dz1[ct] = f4_zero();
          else if (p.dE) *reinterpret_cast<float4 *>(p.dE + pe * h1 + f) = dz1[ct];
        }
      }
      // ---- dz1 of the chunk -> LDS, lane group g sums the rows of target g in edge order (= dP)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<float4 *>(&mine[ei * kTS + 16 * ct + 4 * kq]) = dz1[ct];
      __syncthreads();
      row_sum_chunk(ldsS, c0, kChunk, my_lo, my_hi, q, racc);
      __syncthreads();
    }
    if (p.dP && sc.x >= 0 && 4 * q < h1) *reinterpret_cast<float4 *>(p.dP + (size_t)sc.x * h1 + 4 * q) = racc;
  }

  // ---- fold the waves' dW2 / db2 accumulators into this workgroup's slab, wave by wave (fixed order), then write it out
  if (NTAIL) {
    float *slab = ldsS;                                            // [(h1 + 1)][dw], needs 65 * 64 floats <= kChunk * kTS
    __syncthreads();
    for (int idx = tid; idx < (h1 + 1) * dw; idx += kT) slab[idx] = 0.f;
    fold_bias_lanes(dbacc);
    __syncthreads();
    for (int w = 0; w < kT / 64; ++w) {
      if (wave == w) fold_slab<true>(slab, h1, dw, accW, dbacc, ei, kq);
      __syncthreads();
    }
    float *dst = p.partial + (size_t)blockIdx.x * (h1 + 1) * dw;
    for (int idx = tid; idx < (h1 + 1) * dw; idx += kT) dst[idx] = slab[idx];
  }
}

__global__ void activation_fwd_kernel(int64_t count, int act, const float *__restrict__ z, float *__restrict__ a) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (int64_t)gridDim.x * blockDim.x)
    a[i] = act_apply(act, z[i]);
}

}  // namespace

int32_t launch_edge_mlp_fused_fwd(const ngpde_graph *g, const EdgeFwd &p, const EdgeMlpArgs &a, hipStream_t stream) {
  NGPDE_REQUIRE(p.supported, NGPDE_ERR_UNSUPPORTED,
                "fused edge-MLP path needs widths <= 64 and multiples of 4, <= 3 layers after the first, and a graph whose "
                "tiles fit the LDS halo (degree <= %d, <= %d distinct sources per 32-row tile)", kSlotWidth, kHaloCap);
  if (p.form == EdgeFwdForm::None) return NGPDE_OK;   // no nodes
  if (p.form == EdgeFwdForm::Edge64) return launch_edge_mlp64_fwd(g, p, a, stream);
  const EdgeMlpDesc &d = a.d;
  EdgeMlpK k;
  fill_tile_args(g, tile_geom(g), k);   // (halo region sized by the largest halo of this graph's tiles)
  k.h1 = d.h1; k.act1 = d.act1; k.aggr = d.aggr;
  k.P = a.P; k.Q = a.Q; k.Eterm = a.Eterm; k.n_tail = d.n_tail;
  for (int l = 0; l < 3; ++l) {
    k.din[l] = l < d.n_tail ? d.din(l) : 0; k.dout[l] = d.dout[l]; k.act[l] = d.act[l]; k.wt[l] = a.wt[l]; k.bias[l] = a.bias[l];
  }
  k.out = a.out;
  for (int l = 0; l < 4; ++l) k.save_z[l] = a.save_z[l];
  NGPDE_STAMP_SET(k, kStampEdge, 0);
  const char *name = "edge_mlp_fused_fwd_kernel";
  switch (p.n_tail) {
    case 0: return launch_with_lds(edge_mlp_fused_fwd_kernel<0>, p.grid, p.threads, p.lds, stream, k, name);
    case 1: return launch_with_lds(edge_mlp_fused_fwd_kernel<1>, p.grid, p.threads, p.lds, stream, k, name);
    case 2: return launch_with_lds(edge_mlp_fused_fwd_kernel<2>, p.grid, p.threads, p.lds, stream, k, name);
    default: return launch_with_lds(edge_mlp_fused_fwd_kernel<3>, p.grid, p.threads, p.lds, stream, k, name);
  }
}

int32_t launch_edge_mlp_fused_bwd(const ngpde_graph *g, const EdgeBwd &p, const EdgeMlpBwdArgs &a, hipStream_t stream) {
  NGPDE_REQUIRE(p.supported, NGPDE_ERR_UNSUPPORTED,
                "fused edge-MLP pullback needs widths <= 64 and multiples of 4, at most one layer after the first and a graph whose tiles fit "
                "the LDS halo");
  if (!p.launch) return NGPDE_OK;   // no nodes
  if (int32_t st = check_workspace("fused edge-MLP pullback", a.workspace, a.workspace_bytes, p.workspace_bytes, 1)) return st;
  NGPDE_REQUIRE(!p.dE_missing, NGPDE_ERR_INVALID_ARGUMENT, "fused edge-MLP pullback: the [E][h1] buffer dE is required");
  if (p.form == EdgeBwdForm::Edge64) return launch_edge_mlp64_bwd(g, p, a, stream);
  const EdgeMlpDesc &d = a.d;
  const TileGeom t = tile_geom(g);
  EdgeMlpBwdK k;
  fill_tile_args(g, t, k);
  k.h1 = d.h1; k.act1 = d.act1; k.aggr = d.aggr; k.n_tail = d.n_tail;
  k.dw = d.n_tail ? d.dout[0] : d.h1; k.act2 = d.act[0];
  k.P = a.P; k.Q = a.Q; k.Eterm = a.Eterm; k.wt = a.wt[0]; k.bias = a.bias[0]; k.dout = a.dout;
  k.dP = a.dP; k.dE = a.dE;
  Workspace w(a.workspace);
  EdgeBwdWs ws;
  edge_mlp_bwd_layout(w, t, d, p.form, ws);
  k.partial = ws.partial[0];
  int32_t st = p.n_tail ? launch_with_lds(edge_mlp_fused_bwd_kernel<1>, p.grid, p.threads, p.lds, stream, k, "edge_mlp_fused_bwd_kernel")
                        : launch_with_lds(edge_mlp_fused_bwd_kernel<0>, p.grid, p.threads, p.lds, stream, k, "edge_mlp_fused_bwd_kernel");
  if (st) return st;
  if (p.n_tail && (st = launch_dense_weight_reduce(p.grid, d.h1, d.dout[0], k.partial, a.dwt[0], a.dbias[0], stream))) return st;
  if (p.by_source && (st = launch_edge_sum_by_source(g, d.h1, a.dE, a.dQ, stream))) return st;
  return NGPDE_OK;
}

int32_t launch_activation_fwd(int64_t count, int act, const float *z, float *a, hipStream_t stream) {
  if (count == 0) return NGPDE_OK;
  const int blocks = (int)std::min<int64_t>((count + 255) / 256, 4096);
  hipLaunchKernelGGL(activation_fwd_kernel, dim3(blocks), dim3(256), 0, stream, count, act, z, a);
  NGPDE_LAUNCH_CHECK("activation_fwd_kernel");
  return NGPDE_OK;
}

}  // namespace ngpde
