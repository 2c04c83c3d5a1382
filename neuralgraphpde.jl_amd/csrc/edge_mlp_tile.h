// edge_mlp_tile.h -- the tile machinery shared by the one-launch message-MLP kernels: edge_mlp_fused.hip (general forward and
// pullback), edge_mlp64.hip (the 64-wide pipelined pair) and edge_mlp_deep_bwd.hip (pullback of three / four Dense layers).
// A workgroup owns one 32-row tile of the locality schedule at a time; 16-lane groups stage rows and sum per target, waves own 16
// edges of a chunk (lane ei = lane & 15 <-> edge, kq = lane >> 4 <-> features 16 ct + 4 kq .. + 3 of four float4).
//
// Everything here is arithmetic and LDS traffic BETWEEN barriers: no function contains a __syncthreads(), a hand-issued ds_read,
// an s_waitcnt or a scheduling pin.  The kernels keep those, and they decide when the next tile's metadata and rows are fetched.
// Internal (anonymous namespace: every translation unit gets its own copy).
#pragma once

#include <algorithm>

#include "common.h"
#include "device_utils.h"

namespace ngpde {
namespace {

using namespace edge_mlp;   // kW, kTS, kRows, thread counts and chunk sizes: edge_mlp_forms.h

// Thread shapes: how the 16-lane groups of a workgroup map to the tile's 32 rows and to its halo list.
struct RowPerGroup {       // 512 threads: group g <-> row g, halo rows g + 32 k
  static constexpr int kThreads = 512, kGroups = 32, kRowsPerGroup = 1, kHalo = 3;
};
struct TwoRowsPerGroup {   // 256 threads: group g <-> rows g and g + 16, halo rows g + 16 k
  static constexpr int kThreads = 256, kGroups = 16, kRowsPerGroup = 2, kHalo = 6;
};

// ---- argument block and host side -------------------------------------------------------------------------------------------
// what every kernel of the family reads of the graph (the kernels' argument blocks derive from it)
struct EdgeTileArgs {
  const int4 *sched;
  const int2 *halo;
  const uint8_t *slots;
  int n_tiles, halo_rows;   // halo_rows: LDS rows of the halo region = the largest halo of this graph's tiles
};

inline void fill_tile_args(const ngpde_graph *g, const TileGeom &t, EdgeTileArgs &k) {
  k.sched = g->by_t.sched; k.halo = g->by_t.halo; k.slots = g->by_t.slots;
  k.n_tiles = t.n_tiles;
  k.halo_rows = edge_halo_rows(t);
}

// more than 64 KB of dynamic LDS has to be requested explicitly
template <class KERNEL, class ARGS>
int32_t launch_with_lds(KERNEL kernel, int grid, int block, size_t lds, hipStream_t stream, const ARGS &k, const char *name) {
  const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail(NGPDE_ERR_HIP, "%s: LDS request of %zu bytes refused: %s", name, lds, hipGetErrorString(e));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds, stream, k);
  NGPDE_LAUNCH_CHECK(name);
  return NGPDE_OK;
}

// ---- tile range of a workgroup ----------------------------------------------------------------------------------------------
// XCD x = blockIdx % 8 owns a contiguous range of tiles; its workgroups stride through it: tile range_lo + jt for
// jt = wg_in_xcd, wg_in_xcd + wgs_per_xcd, ... < range_len
struct EdgeTileRange {
  int wg_in_xcd, wgs_per_xcd, range_len, range_lo;
  __device__ __forceinline__ explicit EdgeTileRange(int n_tiles) {
    const int xcd = blockIdx.x & 7;
    wg_in_xcd = blockIdx.x >> 3;
    wgs_per_xcd = gridDim.x >> 3;
    range_len = n_tiles / 8 + (xcd < n_tiles % 8 ? 1 : 0);
    range_lo = xcd * (n_tiles / 8) + min(xcd, n_tiles % 8);
  }
};

// ---- tile metadata and rows, held in registers between the moment they are fetched (under the previous tile's arithmetic) and
// the moment they are staged into LDS ------------------------------------------------------------------------------------------
template <class SHAPE>
struct TileMeta;
template <>
struct TileMeta<RowPerGroup> {
  int4 sc;        // schedule row g: {node or -1, first edge in p order, degree, .}
  uint4 s0, s1;   // its 32 slot bytes
  int2 he[3];     // halo entries g + 32 k
};
template <>
struct TileMeta<TwoRowsPerGroup> {
  int4 sc0, sc1;       // schedule rows g and g + 16
  unsigned sw0, sw1;   // slot word (q & 7) of those rows
  int he[6];           // node ids of halo rows g + 16 k
};
template <class SHAPE>
struct TileRows {
  float4 prow[SHAPE::kRowsPerGroup], hv[SHAPE::kHalo];
};

__device__ __forceinline__ void fetch_meta(const EdgeTileArgs &p, int tile, int g, int q, TileMeta<RowPerGroup> &m) {
  m.sc = p.sched[(size_t)tile * kTileRows + g];
  m.s0 = reinterpret_cast<const uint4 *>(p.slots)[((size_t)tile * kTileRows + g) * 2];
  m.s1 = reinterpret_cast<const uint4 *>(p.slots)[((size_t)tile * kTileRows + g) * 2 + 1];
#pragma unroll
  for (int k = 0; k < 3; ++k) m.he[k] = p.halo[(size_t)tile * kHaloCap + min(g + k * 32, kHaloCap - 1)];
}
__device__ __forceinline__ void fetch_meta(const EdgeTileArgs &p, int tile, int g, int q, TileMeta<TwoRowsPerGroup> &m) {
  const size_t row = (size_t)tile * kTileRows + g;
  m.sc0 = p.sched[row];
  m.sc1 = p.sched[row + 16];
  m.sw0 = reinterpret_cast<const unsigned *>(p.slots)[row * 8 + (q & 7)];
  m.sw1 = reinterpret_cast<const unsigned *>(p.slots)[(row + 16) * 8 + (q & 7)];
#pragma unroll
  for (int k = 0; k < 6; ++k) m.he[k] = p.halo[(size_t)tile * kHaloCap + min(g + 16 * k, kHaloCap - 1)].x;
}

__device__ __forceinline__ int meta_node(const TileMeta<RowPerGroup> &m, int) { return m.sc.x; }
__device__ __forceinline__ int meta_node(const TileMeta<TwoRowsPerGroup> &m, int i) { return i ? m.sc1.x : m.sc0.x; }
__device__ __forceinline__ int meta_halo(const TileMeta<RowPerGroup> &m, int k) { return m.he[k].x; }
__device__ __forceinline__ int meta_halo(const TileMeta<TwoRowsPerGroup> &m, int k) { return m.he[k]; }

// the tile's P rows (of its targets) and the distinct Q rows it references, features 4q .. 4q + 3.  GUARDED: width h1 <= 64, P / Q
// nullable; otherwise both present and 64 wide.
template <bool GUARDED, class SHAPE>
__device__ __forceinline__ void fetch_rows(const float *P, const float *Q, int h1, int halo_rows, const TileMeta<SHAPE> &m, int g, int q,
                                           TileRows<SHAPE> &r) {
  const int w = GUARDED ? h1 : kW;
  const bool on = !GUARDED || 4 * q < h1;
#pragma unroll
  for (int i = 0; i < SHAPE::kRowsPerGroup; ++i)
    r.prow[i] = ((!GUARDED || P) && on) ? *reinterpret_cast<const float4 *>(P + (size_t)max(meta_node(m, i), 0) * w + 4 * q) : f4_zero();
#pragma unroll
  for (int k = 0; k < SHAPE::kHalo; ++k)
    r.hv[k] = ((!GUARDED || Q) && g + k * SHAPE::kGroups < halo_rows && on) ? *reinterpret_cast<const float4 *>(Q + (size_t)meta_halo(m, k) * w + 4 * q)
                                                                            : f4_zero();
}
template <class SHAPE>
__device__ __forceinline__ void stage_rows(const TileRows<SHAPE> &r, int halo_rows, int g, int q, float *ldsQ, float *ldsP) {
#pragma unroll
  for (int k = 0; k < SHAPE::kHalo; ++k) {
    const int hh = g + k * SHAPE::kGroups;
    if (hh < halo_rows) *reinterpret_cast<float4 *>(&ldsQ[hh * kTS + 4 * q]) = r.hv[k];
  }
#pragma unroll
  for (int i = 0; i < SHAPE::kRowsPerGroup; ++i) *reinterpret_cast<float4 *>(&ldsP[(g + 16 * i) * kTS + 4 * q]) = r.prow[i];
}
// the all-zero halo row that padding slot bytes and edges beyond the tile name, written by the first 16-lane group
__device__ __forceinline__ void zero_halo_row(float *ldsQ, int zero_slot, int g, int q) {
  if (g == 0) *reinterpret_cast<float4 *>(&ldsQ[zero_slot * kTS + 4 * q]) = f4_zero();
}

// ---- tile index: offsets of the rows' edges in the tile, and the map tile edge -> row --------------------------------------------
// Three steps with a barrier of the KERNEL between them (the kernels fetch the next tile's metadata in front of the first):
//   stage_tile_degrees   degrees into off[1..32] (off[0] = 0), the slot words, and on request the rows' first edge (RS) and
//                        node / 1 / deg (NODE)                                                     -- barrier --
//   scan_tile_degrees    wave 0 turns the degrees into offsets                                     -- barrier --
//   expand_tile_edges    every group reads its rows' ranges and writes the edge map                -- barrier before its readers --
template <bool RS>
__device__ __forceinline__ void stage_tile_degrees(const TileMeta<RowPerGroup> &m, int g, int q, int *off, unsigned *slots, int *rs) {
  if (q == 0) {
    off[g + 1] = m.sc.x >= 0 ? m.sc.z : 0;
    if (RS) rs[g] = m.sc.y;
    if (g == 0) off[0] = 0;
  }
  if (q < 8) {
    const unsigned w[8] = {m.s0.x, m.s0.y, m.s0.z, m.s0.w, m.s1.x, m.s1.y, m.s1.z, m.s1.w};
    unsigned v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) v = (q == j) ? w[j] : v;
    slots[g * 8 + q] = v;
  }
}
template <bool RS, bool NODE>
__device__ __forceinline__ void stage_tile_degrees(const TileMeta<TwoRowsPerGroup> &m, int g, int q, bool mean, int *off, unsigned *slots, int *rs,
                                                   int *node, float *inv) {
  if (q == 0) {
    const int d0 = m.sc0.x >= 0 ? m.sc0.z : 0, d1 = m.sc1.x >= 0 ? m.sc1.z : 0;
    off[g + 1] = d0;
    off[g + 17] = d1;
    if (RS) {
      rs[g] = m.sc0.y;
      rs[g + 16] = m.sc1.y;
    }
    if (NODE) {
      node[g] = max(m.sc0.x, 0);
      node[g + 16] = max(m.sc1.x, 0);
      inv[g] = mean ? (d0 > 0 ? 1.0f / (float)d0 : 0.f) : 1.0f;
      inv[g + 16] = mean ? (d1 > 0 ? 1.0f / (float)d1 : 0.f) : 1.0f;
    }
    if (g == 0) off[0] = 0;
  }
  if (q < 8) {
    slots[g * 8 + q] = m.sw0;
    slots[(g + 16) * 8 + q] = m.sw1;
  }
}
// inclusive scan of the 32 degrees inside wave 0 (DPP shuffles, no LDS round trips)
__device__ __forceinline__ void scan_tile_degrees(int *off, int tid) {
  if (tid < kRows) {
    int v = off[tid + 1];
#pragma unroll
    for (int o = 1; o < kRows; o <<= 1) {
      const int u = __shfl_up(v, o);
      if (tid >= o) v += u;
    }
    off[tid + 1] = v;
  }
}
__device__ __forceinline__ unsigned slot_byte(const unsigned *slots, int row, int j) { return (slots[row * 8 + (j >> 2)] >> (8 * (j & 3))) & 0xff; }
// one row per group: tile edge k -> row of the tile (deg <= kSlotWidth: total <= 1024)
__device__ __forceinline__ void expand_tile_edges(const int *off, uint8_t *row_of, int g, int q, int &total, int &lo, int &hi) {
  total = off[kRows];
  lo = off[g];
  hi = off[g + 1];
  for (int k = lo + q; k < hi; k += 16) row_of[k] = (uint8_t)g;
}
// two rows per group: tile edge k -> {row of the tile, halo slot << 8}
__device__ __forceinline__ void expand_tile_edges(const int *off, const unsigned *slots, uint16_t *edge, int g, int q, int &total, int &lo0, int &hi0,
                                                  int &lo1, int &hi1) {
  total = off[kRows];
  lo0 = off[g], hi0 = off[g + 1], lo1 = off[g + 16], hi1 = off[g + 17];
  for (int k = lo0 + q; k < hi0; k += 16) edge[k] = (uint16_t)(g | (slot_byte(slots, g, k - lo0) << 8));
  for (int k = lo1 + q; k < hi1; k += 16) edge[k] = (uint16_t)((g + 16) | (slot_byte(slots, g + 16, k - lo1) << 8));
}

// the lane's edge k of the tile: row, halo slot, position in p order (an edge beyond the tile: row 0, the all-zero slot)
__device__ __forceinline__ void lane_edge(const uint8_t *row_of, const int *off, const unsigned *slots, const int *rs, int k, bool valid, int zero_slot,
                                          int &r, int &slot, size_t &pe) {
  r = 0, slot = zero_slot, pe = 0;
  if (valid) {
    r = row_of[k];
    const int j = k - off[r];
    slot = slot_byte(slots, r, j);
    pe = (size_t)(rs[r] + j);
  }
}
__device__ __forceinline__ void lane_edge(const uint16_t *edge, const int *off, const int *rs, int k, bool valid, int zero_slot, int &r, int &slot,
                                          size_t &pe) {
  const unsigned ew = edge[valid ? k : 0];
  r = ew & 0xff;
  slot = valid ? (int)(ew >> 8) : zero_slot;
  pe = (size_t)(rs[r] + (k - off[r]));
}

// ---- weights of one Dense layer into LDS, once per workgroup: W^T rows (output j, contiguous inputs) and, BOTH, W rows (input j,
// contiguous outputs), [64][kTS] each; GUARDED: din x dw zero-padded to 64 x 64 and a nullable bias, otherwise 64 x 64 ---------------
template <int THREADS, bool GUARDED, bool BOTH>
__device__ __forceinline__ void stage_weights(const float *w, const float *bias, int din, int dw, int tid, float *ldsWf, float *ldsWb, float *ldsBias) {
  constexpr int KG = THREADS / kW;          // input quads per pass
  const int j = tid % kW, kg0 = tid / kW;   // column j, quads kg0 + KG ps
#pragma unroll
  for (int ps = 0; ps < 16 / KG; ++ps) {
    const int k = 4 * (kg0 + KG * ps);
    if (GUARDED) {
      float t[4], u[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        t[r] = (k + r < din && j < dw) ? w[(size_t)(k + r) * dw + j] : 0.f;                 // W^T row j (output), inputs k..k+3
        if (BOTH) u[r] = (j < din && k + r < dw) ? w[(size_t)j * dw + k + r] : 0.f;         // W row j (input), outputs k..k+3
      }
      *reinterpret_cast<float4 *>(&ldsWf[j * kTS + k]) = make_float4(t[0], t[1], t[2], t[3]);
      if (BOTH) *reinterpret_cast<float4 *>(&ldsWb[j * kTS + k]) = make_float4(u[0], u[1], u[2], u[3]);
    } else {
      *reinterpret_cast<float4 *>(&ldsWf[j * kTS + k]) =
          make_float4(w[(size_t)k * kW + j], w[(size_t)(k + 1) * kW + j], w[(size_t)(k + 2) * kW + j], w[(size_t)(k + 3) * kW + j]);
      if (BOTH) *reinterpret_cast<float4 *>(&ldsWb[j * kTS + k]) = *reinterpret_cast<const float4 *>(w + (size_t)j * kW + k);
    }
  }
  if (tid < kW) ldsBias[tid] = (bias && (!GUARDED || tid < dw)) ? bias[tid] : 0.f;
}

// ---- the chain the pullbacks recompute --------------------------------------------------------------------------------------
// z1 = P[r] + Q[slot] + E[pe], a1 = act1(z1) zeroed on padded features and on edges beyond the tile
__device__ __forceinline__ void first_layer(const float *ldsP, const float *ldsQ, const float *Eterm, int h1, int act1, int r, int slot, size_t pe,
                                            bool valid, int kq, float4 (&z1)[4], float4 (&a1)[4]) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    const int f = 16 * ct + 4 * kq;
    float4 z = f4_add(*reinterpret_cast<const float4 *>(&ldsP[r * kTS + f]), *reinterpret_cast<const float4 *>(&ldsQ[slot * kTS + f]));
    if (Eterm && valid && f < h1) z = f4_add(z, *reinterpret_cast<const float4 *>(Eterm + pe * h1 + f));
    z1[ct] = z;
    a1[ct] = z;
  }
  f4n_act<4>(act1, a1);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
    if (!(valid && 16 * ct + 4 * kq < h1)) a1[ct] = f4_zero();
}
// z^T = M a^T (+ b) on the matrix pipe, M = [64 rows][kTS] in LDS, zero-padded: the W^T image gives a layer's pre-activations, the
// W image (BIAS = false, din / dout swapped) the gradient of its input.  The D layout of the product is the operand layout of the
// next one, so products chain in registers.  Row tiles beyond dout stay zero.
template <bool BIAS>
__device__ __forceinline__ void dense_transposed(const float *ldsM, const float *ldsBias, int din, int dout, int ei, int kq, const float4 (&a)[4],
                                                 float4 (&z)[4]) {
  const int n_ct = (din + 15) >> 4, n_mt = (dout + 15) >> 4;   // uniform
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    z[mt] = f4_zero();
    if (mt < n_mt) {
      f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
      const float *wl = ldsM + (mt * 16 + ei) * kTS + 4 * kq;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (ct < n_ct) {
          const float4 w4 = *reinterpret_cast<const float4 *>(wl + 16 * ct);
          acc = mfma16(w4.x, a[ct].x, acc);
          acc = mfma16(w4.y, a[ct].y, acc);
          acc = mfma16(w4.z, a[ct].z, acc);
          acc = mfma16(w4.w, a[ct].w, acc);
        }
      }
      if (BIAS) {
        const float4 b4 = *reinterpret_cast<const float4 *>(&ldsBias[16 * mt + 4 * kq]);
        z[mt] = make_float4(acc[0] + b4.x, acc[1] + b4.y, acc[2] + b4.z, acc[3] + b4.w);
      } else {
        z[mt] = make_float4(acc[0], acc[1], acc[2], acc[3]);
      }
    }
  }
}
// dW += a^T dz over the wave's 16 edges (accW[ct][mt] <-> inputs 16 ct .. + 15 x outputs 16 mt .. + 15): both operands transposed
// through the wave's own 16 rows of LDS (`mine`; wave-private, so no barrier)
template <bool GUARDED>
__device__ __forceinline__ void weight_grad_products(float *mine, const float4 (&a)[4], const float4 (&dz)[4], int din, int dw, int ei, int kq,
                                                     f32x4 (&accW)[4][4]) {
  const int n_ct = (din + 15) >> 4, n_mt = (dw + 15) >> 4;   // uniform
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<float4 *>(&mine[ei * kTS + 16 * ct + 4 * kq]) = a[ct];
  float aT[4][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int sI = 0; sI < 4; ++sI) aT[ct][sI] = mine[(4 * sI + kq) * kTS + 16 * ct + ei];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) *reinterpret_cast<float4 *>(&mine[ei * kTS + 16 * mt + 4 * kq]) = dz[mt];
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    if (!GUARDED || mt < n_mt) {
      float dzT[4];
#pragma unroll
      for (int sI = 0; sI < 4; ++sI) dzT[sI] = mine[(4 * sI + kq) * kTS + 16 * mt + ei];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        if (!GUARDED || ct < n_ct) {
#pragma unroll
          for (int sI = 0; sI < 4; ++sI) accW[ct][mt] = mfma16(aT[ct][sI], dzT[sI], accW[ct][mt]);
        }
      }
    }
  }
}

// ---- per-target fold over a chunk in LDS: the rows lo .. hi of a target that lie in the chunk [c0, c0 + len), in edge order
// (chunk = row c0's address).  U = 4: four independent LDS reads in flight, folded in the same order.
template <int U = 1, class OP>
__device__ __forceinline__ void row_fold_chunk(const float *chunk, int c0, int len, int lo, int hi, int q, float4 &racc, OP op) {
  const float *base = chunk + 4 * q - c0 * kTS;
  int kk = max(lo, c0);
  const int end = min(hi, c0 + len);
  if (U == 4) {
    for (; kk + 4 <= end; kk += 4) {
      const float4 m0 = *reinterpret_cast<const float4 *>(base + kk * kTS), m1 = *reinterpret_cast<const float4 *>(base + (kk + 1) * kTS);
      const float4 m2 = *reinterpret_cast<const float4 *>(base + (kk + 2) * kTS), m3 = *reinterpret_cast<const float4 *>(base + (kk + 3) * kTS);
      racc = op(op(op(op(racc, m0), m1), m2), m3);
    }
  }
  for (; kk < end; ++kk) racc = op(racc, *reinterpret_cast<const float4 *>(base + kk * kTS));
}
template <int U = 1>
__device__ __forceinline__ void row_sum_chunk(const float *chunk, int c0, int len, int lo, int hi, int q, float4 &racc) {
  row_fold_chunk<U>(chunk, c0, len, lo, hi, q, racc, [](float4 a, float4 b) { return f4_add(a, b); });
}

// ---- weight-gradient slab of a workgroup: [(din + 1)][dw] floats in LDS (row din = bias gradient).  The kernel clears it, calls
// fold_bias_lanes, and after a barrier lets wave 0, 1, ... call fold_slab one after the other (fixed order) with a barrier each ----
__device__ __forceinline__ void fold_bias_lanes(float4 (&db)[4]) {   // sum the 16 edge lanes of each k-quarter inside the wave
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    float v[4] = {db[mt].x, db[mt].y, db[mt].z, db[mt].w};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) v[c] += __shfl_xor(v[c], o);
    }
    db[mt] = make_float4(v[0], v[1], v[2], v[3]);
  }
}
template <bool GUARDED>
__device__ __forceinline__ void fold_slab(float *slab, int din, int dw, const f32x4 (&accW)[4][4], const float4 (&db)[4], int ei, int kq) {
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kin = 16 * ct + 4 * kq + r, o = 16 * mt + ei;
        if (!GUARDED || (kin < din && o < dw)) slab[kin * dw + o] += accW[ct][mt][r];
      }
  if (ei == 0) {
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const int o = 16 * mt + 4 * kq;
      if (!GUARDED || o < dw) {
        slab[din * dw + o] += db[mt].x; slab[din * dw + o + 1] += db[mt].y;
        slab[din * dw + o + 2] += db[mt].z; slab[din * dw + o + 3] += db[mt].w;
      }
    }
  }
}

}  // namespace
}  // namespace ngpde
