// edge_mlp64.hip -- the message path of the edge-function layers for the 64-wide two-layer message MLP
//   m_i = aggr_{e: t_e = i}  act2( W2^T act1( P[t_e] + Q[s_e] ) + b2 )      (/root/reference/src/layers.jl:409-416, :316-326,
//                                                                            :103-111 with the first Dense split at node level)
// in the shape BASELINE's config 4 runs (MPPDEConv, h = 64, phi = Dense(. => 64) -> Dense(64 => 64)), as a software-pipelined
// specialisation of edge_mlp_fused.hip: widths and activations are compile-time constants, so the steady state of the edge loop is
// ONE basic block in which a wave's 64 v_mfma_f32_16x16x4_f32 of slice s run beside the bias + activation + LDS store of slice
// s - 1 and the gather + first activation of slice s + 1.  The general kernel walks the same phases one after the other with every
// wave of the SIMD in the same phase (identical waves stay in step), so its matrix pipe idles during the activations and its
// VALU during the products (matrix pipe 39 % busy at config 4); and its 128-edge chunks pad a 192-edge tile to 256.
//
// A workgroup = 4 waves owns a 32-row tile of the locality schedule and walks the tile's edges 64 (4 x 16) at a time; tile
// metadata, P rows and the distinct Q rows (halo) of the NEXT tile are in flight in registers under the current tile's arithmetic
// (edge_mlp_fused.hip's scheme).  Register layout of a slice, transposed products and the in-tile segmented reduction in edge
// (= COO) order are those of edge_mlp_fused.hip: no atomics, bitwise reproducible, and bitwise equal to the general kernel.
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "device_utils.h"
#include "edge_mlp_tile.h"
#include "stamps.h"
#include "switches.h"

namespace ngpde {

namespace {

template <int S, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  if constexpr (S < N) {
    f(std::integral_constant<int, S>{});
    static_for<S + 1, N>(f);
  }
}

// Pins a value to this point of the instruction stream: the (empty) volatile asm is ordered against the other pins and the
// sched_barriers of the pipelined block, so what computes the value stays before it and what uses it after it.  Without the pins
// instruction selection places pure arithmetic next to its use -- the whole activation of the next slice behind the last MFMA.
#define PIN(x) asm volatile("" : "+v"(x))
// nothing moves across this point in instruction scheduling
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
// LDS reads issued by hand (the compiler does not track them: the consumer waits with an explicit s_waitcnt that takes the
// destination registers as operands, so nothing that uses them can move above it)
__device__ __forceinline__ unsigned lds_addr(const void *ptr) { return (unsigned)(uintptr_t)ptr; }   // low half of a generic LDS pointer
#define lds_read4(dst, addr) asm volatile("ds_read_b128 %0, %1" : "=v"(dst) : "v"(addr))
#define lds_read_u16(dst, addr) asm volatile("ds_read_u16 %0, %1" : "=v"(dst) : "v"(addr))

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kSlice = 16;   // edges of a wave's slice (kT4, kChunk4, kW, kTS, kRows: edge_mlp_forms.h)
using Shape = TwoRowsPerGroup;

struct EdgeMlp64K : EdgeTileArgs {
  int aggr;
  const float *P, *Q, *wt, *bias;
  float *out;
  NGPDE_STAMP_FIELD
};

template <int ACT1, int ACT2>
__global__ __launch_bounds__(kT4, 2) void edge_mlp64_fwd_kernel(const EdgeMlp64K p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float *ldsQ = dyn;                                              // [halo_rows + 1][kTS]
  float *ldsP = ldsQ + (size_t)(p.halo_rows + 1) * kTS;           // [32][kTS]
  float *ldsWt = ldsP + kRows * kTS;                              // [64 out][kTS]   W2^T
  float *ldsMsg0 = ldsWt + kW * kTS;                              // [2][64 edges][kTS]: the messages of chunk c go to buffer c & 1, so
                                                                  // that one barrier per chunk orders them against the reduction
  __shared__ int ldsOff[kRows + 1];
  __shared__ __attribute__((aligned(16))) unsigned ldsSlots[kRows * 8];
  __shared__ uint16_t ldsEdge[kRows * kSlotWidth];   // tile edge k -> {row of the tile, halo slot << 8}
  __shared__ __attribute__((aligned(16))) float ldsBias[kW];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g16 = tid >> 4, q = tid & 15;           // staging / reduction role: rows g16 and g16 + 16, features 4q .. 4q + 3
  const int ei = lane & 15, kq = lane >> 4;         // MFMA role
  const int zero_slot = p.halo_rows;

  const EdgeTileRange tr(p.n_tiles);

  // ---- once per workgroup: W2^T rows (output j, contiguous inputs), bias, the all-zero halo row
  stage_weights<kT4, false, false>(p.wt, p.bias, kW, kW, tid, ldsWt, nullptr, ldsBias);
  zero_halo_row(ldsQ, zero_slot, g16, q);

  // ---- the activation in stages: y = fin(x, tr2(mid(tr1(pre(x))))) with the two quarter-rate transcendentals (tr1, tr2) as
  // separate steps, so that the pipelined block below can put exactly one of them behind every MFMA; pre / mid / fin on pairs of
  // values (packed instructions).  Same operations in the same order as act_apply (device_utils.h): bitwise the same values.
  auto tr1 = [](auto act, float t) -> float {
    constexpr int A = decltype(act)::value;
    return (A == NGPDE_ACT_SWISH || A == NGPDE_ACT_TANH) ? __builtin_amdgcn_exp2f(t) : t;
  };
  auto tr2 = [](auto act, float d) -> float {
    constexpr int A = decltype(act)::value;
    return (A == NGPDE_ACT_SWISH || A == NGPDE_ACT_TANH) ? __builtin_amdgcn_rcpf(d) : d;
  };
  // the packed (two-value) forms of the non-transcendental steps: the same operations on both halves
  auto pre2 = [](auto act, f32x2 x) -> f32x2 {
    constexpr int A = decltype(act)::value;
    if (A == NGPDE_ACT_SWISH) return (-x) * 1.4426950408889634f;
    if (A == NGPDE_ACT_TANH) return (2.0f * x) * 1.4426950408889634f;
    return x;
  };
  auto mid2 = [](auto act, f32x2 e) -> f32x2 {
    constexpr int A = decltype(act)::value;
    return (A == NGPDE_ACT_SWISH || A == NGPDE_ACT_TANH) ? 1.0f + e : e;
  };
  auto fin2 = [](auto act, f32x2 x, f32x2 r) -> f32x2 {
    constexpr int A = decltype(act)::value;
    if (A == NGPDE_ACT_SWISH) return x * r;
    if (A == NGPDE_ACT_TANH) return 1.0f - 2.0f * r;
    if (A == NGPDE_ACT_RELU) return (f32x2){fmaxf(x[0], 0.0f), fmaxf(x[1], 0.0f)};
    return x;
  };
  const std::integral_constant<int, ACT1> act1_c{};
  const std::integral_constant<int, ACT2> act2_c{};

  // permanent registers: the bias of the lane's 16 output features, the W2^T fragments of the first 16 input features
  f32x2 bias2[8];   // bias2[2 mt + h] = bias of features 16 mt + 4 kq + 2 h, + 1
  f32x4 w0[4];
  {
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const float4 b4 = *reinterpret_cast<const float4 *>(&ldsBias[16 * mt + 4 * kq]);
      bias2[2 * mt] = (f32x2){b4.x, b4.y}; bias2[2 * mt + 1] = (f32x2){b4.z, b4.w};
      const float4 w4 = *reinterpret_cast<const float4 *>(&ldsWt[(mt * 16 + ei) * kTS + 4 * kq]);
      w0[mt] = (f32x4){w4.x, w4.y, w4.z, w4.w};
    }
  }
  auto comp = [](const f32x4 &v, int r) -> float { return v[r]; };
  const unsigned wt_addr = lds_addr(ldsWt + ei * kTS + 4 * kq);   // W2^T fragment (mt, ct) at + (mt * 16 * kTS + 16 * ct) floats

  // ---- one pipelined block = 64 slots.  Slot s: MFMA s of the current slice (ct = s / 16, r = (s / 4) % 4, mt = s % 4: four
  // independent accumulator chains) and one stage of the activation of a pair of values -- pairs 0..7 (slots 0..31) are the
  // messages of the PREVIOUS slice (bias + act2, stored to LDS as each float4 completes), pairs 8..15 (slots 32..63) the first
  // activation of the NEXT slice (P[row] + Q[slot]).  LDS reads are issued by hand in fixed slots and collected by three waits
  // that each sit several slots behind the last issue: slot 0 the lane's edge word, 1..4 the W2^T fragments of input block 1,
  // wait at 7; 17..20 fragments of block 2, 21..24 the P / Q rows of feature blocks 0 and 1, wait at 31; 33..36 the rows of
  // feature blocks 2 and 3, 37..40 the fragments of block 3, wait at 47.  A sched_barrier after every slot and the pins keep
  // this order through instruction selection and scheduling.
  //   MF: the products run; PUB: there is a previous slice to publish; ASM: assemble the slice `it_next`.
  auto block = [&](auto mf_c, auto pub_c, auto asm_c, int it_next, int total, float *ldsMsg, f32x4 (&a)[4], f32x4 (&accp)[4]) __attribute__((always_inline)) {
    constexpr bool MF = decltype(mf_c)::value, PUB = decltype(pub_c)::value, ASM = decltype(asm_c)::value;
    f32x4 acc[4];
    f32x4 wf[4][4];
    f32x2 xs2[16], ts2[16];
    f32x4 pr[4], qr[4];
    unsigned eword = 0, p_addr = 0, q_addr = 0;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) wf[0][mt] = w0[mt];
    static_for<0, 64>([&](auto s_c) __attribute__((always_inline)) {
      constexpr int s = decltype(s_c)::value;
      constexpr int ct = s >> 4, rr = (s >> 2) & 3, mt = s & 3;
      if (MF) {
        const f32x4 c0 = (ct == 0 && rr == 0) ? (f32x4){0.f, 0.f, 0.f, 0.f} : acc[mt];
        acc[mt] = mfma16(comp(wf[ct][mt], rr), comp(a[ct], rr), c0);
        PIN(acc[mt]);
        if (s >= 1 && s <= 4) lds_read4(wf[1][s - 1], wt_addr + ((s - 1) * 16 * kTS + 16) * 4);
        if (s >= 17 && s <= 20) lds_read4(wf[2][s - 17], wt_addr + ((s - 17) * 16 * kTS + 32) * 4);
        if (s >= 37 && s <= 40) lds_read4(wf[3][s - 37], wt_addr + ((s - 37) * 16 * kTS + 48) * 4);
      }
      if (ASM) {   // the next slice's edge word {row of the tile, halo slot}, then its P / Q rows
        if (s == 0) {
          const int k = min(it_next * kChunk4 + wave * kSlice + ei, total - 1);
          lds_read_u16(eword, lds_addr(ldsEdge) + 2 * k);
        }
        if (s == 8) {
          p_addr = lds_addr(ldsP) + ((eword & 0xff) * kTS + 4 * kq) * 4;
          q_addr = lds_addr(ldsQ) + ((eword >> 8) * kTS + 4 * kq) * 4;
          PIN(p_addr);
          PIN(q_addr);
        }
        if (s == 21) lds_read4(pr[0], p_addr);
        if (s == 22) lds_read4(qr[0], q_addr);
        if (s == 23) lds_read4(pr[1], p_addr + 64);
        if (s == 24) lds_read4(qr[1], q_addr + 64);
        if (s == 33) lds_read4(pr[2], p_addr + 128);
        if (s == 34) lds_read4(qr[2], q_addr + 128);
        if (s == 35) lds_read4(pr[3], p_addr + 192);
        if (s == 36) lds_read4(qr[3], q_addr + 192);
      }
      // the three collection points
      if (s == 7) {
        if (MF && ASM) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wf[1][0]), "+v"(wf[1][1]), "+v"(wf[1][2]), "+v"(wf[1][3]), "+v"(eword));
        else if (MF) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wf[1][0]), "+v"(wf[1][1]), "+v"(wf[1][2]), "+v"(wf[1][3]));
        else if (ASM) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(eword));
      }
      if (s == 31) {
        if (MF) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wf[2][0]), "+v"(wf[2][1]), "+v"(wf[2][2]), "+v"(wf[2][3]));
        if (ASM) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pr[0]), "+v"(qr[0]), "+v"(pr[1]), "+v"(qr[1]));
      }
      if (s == 47) {
        if (MF) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wf[3][0]), "+v"(wf[3][1]), "+v"(wf[3][2]), "+v"(wf[3][3]));
        if (ASM) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pr[2]), "+v"(qr[2]), "+v"(pr[3]), "+v"(qr[3]));
      }
      {
        // values travel in PAIRS (two consecutive features of the lane): the non-transcendental steps are one packed instruction
        // per pair (v_pk_add_f32 / v_pk_mul_f32) -- with the matrix instruction unable to run beside the VALU every such
        // instruction is a matrix-pipe bubble.  Pair pp, slots 4 pp .. 4 pp + 3: {source + pre-scale, tr1(e0)} {tr1(e1)}
        // {mid, tr2(e0)} {tr2(e1)}; its last step (fin) opens the next pair's first slot.
        constexpr int pp = s >> 2, ph = s & 3;
        constexpr bool pub_pair = pp < 8;
        if constexpr (ph == 0 && pp > 0) {
          constexpr bool prev_pub = (pp - 1) < 8;
          if (prev_pub ? PUB : ASM) {
            xs2[pp - 1] = prev_pub ? fin2(act2_c, xs2[pp - 1], ts2[pp - 1]) : fin2(act1_c, xs2[pp - 1], ts2[pp - 1]);
            PIN(xs2[pp - 1]);
          }
        }
        if constexpr (PUB && pub_pair && ph == 1 && (pp & 1) == 0 && pp > 0) {   // float4 mt = pp / 2 - 1 of the messages is complete
          constexpr int m = pp / 2 - 1;
          *reinterpret_cast<float4 *>(&ldsMsg[(wave * kSlice + ei) * kTS + 16 * m + 4 * kq]) =
              make_float4(xs2[2 * m][0], xs2[2 * m][1], xs2[2 * m + 1][0], xs2[2 * m + 1][1]);
        }
        if (PUB && s == 33)
          *reinterpret_cast<float4 *>(&ldsMsg[(wave * kSlice + ei) * kTS + 48 + 4 * kq]) = make_float4(xs2[6][0], xs2[6][1], xs2[7][0], xs2[7][1]);
        if constexpr (pub_pair ? PUB : ASM) {
          if constexpr (ph == 0) {
            if constexpr (pub_pair) {
              constexpr int mt_ = pp >> 1, h_ = 2 * (pp & 1);
              xs2[pp] = (f32x2){accp[mt_][h_], accp[mt_][h_ + 1]} + bias2[pp];
              ts2[pp] = pre2(act2_c, xs2[pp]);
              ts2[pp][0] = tr1(act2_c, ts2[pp][0]);
            } else {
              constexpr int c_ = (pp - 8) >> 1, h_ = 2 * (pp & 1);
              xs2[pp] = (f32x2){pr[c_][h_], pr[c_][h_ + 1]} + (f32x2){qr[c_][h_], qr[c_][h_ + 1]};
              ts2[pp] = pre2(act1_c, xs2[pp]);
              ts2[pp][0] = tr1(act1_c, ts2[pp][0]);
            }
            PIN(xs2[pp]);
            PIN(ts2[pp]);
          } else if constexpr (ph == 1) {
            ts2[pp][1] = pub_pair ? tr1(act2_c, ts2[pp][1]) : tr1(act1_c, ts2[pp][1]);
            PIN(ts2[pp]);
          } else if constexpr (ph == 2) {
            ts2[pp] = pub_pair ? mid2(act2_c, ts2[pp]) : mid2(act1_c, ts2[pp]);
            ts2[pp][0] = pub_pair ? tr2(act2_c, ts2[pp][0]) : tr2(act1_c, ts2[pp][0]);
            PIN(ts2[pp]);
          } else {
            ts2[pp][1] = pub_pair ? tr2(act2_c, ts2[pp][1]) : tr2(act1_c, ts2[pp][1]);
            PIN(ts2[pp]);
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    if (ASM) {
      xs2[15] = fin2(act1_c, xs2[15], ts2[15]);
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) a[ct] = (f32x4){xs2[8 + 2 * ct][0], xs2[8 + 2 * ct][1], xs2[9 + 2 * ct][0], xs2[9 + 2 * ct][1]};
    }
    if (MF) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) accp[mt] = acc[mt];
    }
  };
  const std::true_type yes{};
  const std::false_type no{};

  TileMeta<Shape> meta;
  TileRows<Shape> rows;
  int jt = tr.wg_in_xcd;
  if (jt < tr.range_len) {
    fetch_meta(p, tr.range_lo + jt, g16, q, meta);
    fetch_rows<false>(p.P, p.Q, kW, p.halo_rows, meta, g16, q, rows);
  }

  for (; jt < tr.range_len; jt += tr.wgs_per_xcd) {
    const bool stamp_tile = (jt == tr.wg_in_xcd + 4 * tr.wgs_per_xcd);   // a tile in steady state (the fifth of the workgroup)
    if (stamp_tile) { NGPDE_STAMP(p.stamps, 16, 0, memtime); NGPDE_STAMP(p.stamps, 16, 14, memrealtime); }
    // ---- stage this tile (fetched under the previous tile's arithmetic)
    const int4 sc0 = meta.sc0, sc1 = meta.sc1;
    stage_rows(rows, p.halo_rows, g16, q, ldsQ, ldsP);
    stage_tile_degrees<false, false>(meta, g16, q, false, ldsOff, ldsSlots, nullptr, nullptr, nullptr);
    const int jn = jt + tr.wgs_per_xcd;
    const bool has_next = jn < tr.range_len;       // workgroup-uniform
    if (has_next) fetch_meta(p, tr.range_lo + jn, g16, q, meta);
    __syncthreads();
    scan_tile_degrees(ldsOff, tid);
    __syncthreads();
    int total, lo0, hi0, lo1, hi1;
    expand_tile_edges(ldsOff, ldsSlots, ldsEdge, g16, q, total, lo0, hi0, lo1, hi1);
    float4 racc0 = f4_zero(), racc1 = f4_zero();
    __syncthreads();

    if (stamp_tile) NGPDE_STAMP(p.stamps, 16, 1, memtime);
    const int n_it = (total + kChunk4 - 1) / kChunk4;
    auto reduce = [&](int it) {   // lane group g16 sums the messages of rows g16 and g16 + 16 that lie in chunk `it`, edge order
      const float *chunk = ldsMsg0 + (it & 1) * (kChunk4 * kTS);
      row_sum_chunk<4>(chunk, it * kChunk4, kChunk4, lo0, hi0, q, racc0);
      row_sum_chunk<4>(chunk, it * kChunk4, kChunk4, lo1, hi1, q, racc1);
    };
    if (n_it > 0) {
      f32x4 a[4], accp[4];
      block(no, no, yes, 0, total, ldsMsg0, a, accp);          // a1 of slice 0
      if (stamp_tile) NGPDE_STAMP(p.stamps, 16, 2, memtime);
      block(yes, no, yes, 1, total, ldsMsg0, a, accp);         // products of slice 0 | a1 of slice 1
      if (stamp_tile) NGPDE_STAMP(p.stamps, 16, 3, memtime);
      if (has_next) fetch_rows<false>(p.P, p.Q, kW, p.halo_rows, meta, g16, q, rows);   // the next tile's rows: in flight across this tile's remaining arithmetic
      if (stamp_tile) NGPDE_STAMP(p.stamps, 16, 4, memtime);
      for (int it = 1; it < n_it; ++it) {
        // products of slice it | messages of slice it - 1 (-> buffer (it - 1) & 1) | a1 of slice it + 1
        block(yes, yes, yes, it + 1, total, ldsMsg0 + ((it - 1) & 1) * (kChunk4 * kTS), a, accp);
        if (it == 1 && stamp_tile) NGPDE_STAMP(p.stamps, 16, 5, memtime);
        __syncthreads();
        if (it == 1 && stamp_tile) NGPDE_STAMP(p.stamps, 16, 6, memtime);
        reduce(it - 1);   // (no second barrier: the next block writes the other buffer)
        if (it == 1 && stamp_tile) NGPDE_STAMP(p.stamps, 16, 7, memtime);
        if (it == 1 && stamp_tile) NGPDE_STAMP(p.stamps, 16, 8, memtime);
        if (it == 2 && stamp_tile) NGPDE_STAMP(p.stamps, 16, 9, memtime);
      }
      if (stamp_tile) NGPDE_STAMP(p.stamps, 16, 10, memtime);
      block(no, yes, no, 0, total, ldsMsg0 + ((n_it - 1) & 1) * (kChunk4 * kTS), a, accp);   // messages of the last slice
      if (stamp_tile) NGPDE_STAMP(p.stamps, 16, 11, memtime);
      __syncthreads();
      reduce(n_it - 1);
      __syncthreads();
      if (stamp_tile) NGPDE_STAMP(p.stamps, 16, 12, memtime);
    } else if (has_next) {
      fetch_rows<false>(p.P, p.Q, kW, p.halo_rows, meta, g16, q, rows);
    }
    if (sc0.x >= 0) {
      const int deg = hi0 - lo0;
      if (p.aggr == NGPDE_AGGR_MEAN) racc0 = deg > 0 ? f4_scale(1.0f / (float)deg, racc0) : f4_zero();
      *reinterpret_cast<float4 *>(p.out + (size_t)sc0.x * kW + 4 * q) = racc0;
    }
    if (sc1.x >= 0) {
      const int deg = hi1 - lo1;
      if (p.aggr == NGPDE_AGGR_MEAN) racc1 = deg > 0 ? f4_scale(1.0f / (float)deg, racc1) : f4_zero();
      *reinterpret_cast<float4 *>(p.out + (size_t)sc1.x * kW + 4 * q) = racc1;
    }
    if (stamp_tile) { NGPDE_STAMP(p.stamps, 16, 13, memtime); NGPDE_STAMP(p.stamps, 16, 15, memrealtime); }
  }
}

// ---- pullback of the same message path (edge_mlp_fused_bwd_kernel's algorithm, specialised) -------------------------------------
// Per 16-edge wave slice, all in registers: z1 = P[t] + Q[s], s1 = sigma(z1) once for a1 = act1(z1) AND act1'(z1); z2^T = W2^T
// a1^T + b2 (MFMA); dz2 = g[t] . act2'(z2); dW2 += a1^T dz2 (MFMA over the slice's edges, operands transposed through the wave's
// 4 KB of LDS); da1^T = W2 dz2^T (MFMA); dz1 = da1 . act1'(z1) -> dE (memory, once) and through LDS into the per-target sum dP.
// What differs from the general kernel: 4 waves per workgroup and 64-edge chunks (a 192-edge tile is three full chunks; the
// general kernel's 128-edge chunks leave half of its waves idle in every second one), TWO workgroups per CU whose phases drift
// apart (one's tile loads and reductions under the other's products), the incoming gradient rows read where they are used
// instead of staged (that is what lets two workgroups fit the LDS), compile-time widths and activations, and one sigmoid per
// value where activation and derivative both need it.
struct EdgeMlp64BwdK : EdgeTileArgs {
  int aggr;
  const float *P, *Q, *wt, *bias, *dout;
  float *dP, *dE, *partial;   // partial: [n_workgroups][65][64]  (row 64 = bias gradient)
  float *dqpart;              // DQ: [n_tiles][kDqStride][64] per-tile sums of dz1 by FOREIGN halo slot (the by-source sum, first half)
  float *dQ;                  // DQ: the sums of a tile's OWN slots (= its own rows) go straight to the node's row
};
// kDqSlots halo slots per 16-lane group stay in registers (DQ); kDqStride = 16 kDqSlots rows: edge_mlp_forms.h

// a = act(z), d = act'(z) with the shared transcendental evaluated once (same operations as act_apply / act_deriv)
template <int ACT>
__device__ __forceinline__ void act_both(float z, float &a, float &d) {
  if (ACT == NGPDE_ACT_SWISH) {
    const float s = sigmoidf_(z);
    a = z * s;
    d = s * (1.0f + z * (1.0f - s));
  } else if (ACT == NGPDE_ACT_TANH) {
    const float t = tanhf_(z);
    a = t;
    d = 1.0f - t * t;
  } else if (ACT == NGPDE_ACT_RELU) {
    a = fmaxf(z, 0.0f);
    d = z > 0.f ? 1.0f : 0.0f;
  } else {
    a = z;
    d = 1.0f;
  }
}

// DQ (no per-edge first-layer term, halos of at most kDqStride rows: meshes such as BASELINE config 4's): the [E][64] array dz1
// is NOT written.  Its only reader would be the by-source sum dQ; instead each 16-lane group keeps the sums of dz1 over the edges of
// "its" halo slots (slot = the edge's source row in the tile's halo list) in registers -- the edges of a chunk that carry a slot
// are found by ballots over the chunk's slot ids and added in edge order, so the result is reproducible.  The sums of the tile's OWN
// slots (slot k < 32 = its k-th row: most of a mesh's edges stay inside their tile) are the node's row of dQ up to what other tiles
// add: they are stored there; the sums of FOREIGN slots go to one row per (tile, slot), and edge64_dq_combine_kernel adds them to
// the few nodes that other tiles reference (graph handle: halo_inverse), ascending by tile.  (Round 4 wrote every slot's row and
// summed all of them per node: 452 MB of traffic for the 134 MB result; now 134 + 3 x 25 MB.)
template <int ACT1, int ACT2, bool DQ>
__global__ __launch_bounds__(kT4, 2) void edge_mlp64_bwd_kernel(const EdgeMlp64BwdK p) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  float *ldsQ = dyn;                                              // [halo_rows + 1][kTS]
  float *ldsP = ldsQ + (size_t)(p.halo_rows + 1) * kTS;           // [32][kTS]
  float *ldsS = ldsP + kRows * kTS;                               // [64][kTS]  wave-private transposes, then dz1 of the chunk
  float *ldsWf = ldsS + kChunk4 * kTS;                            // [64 out][kTS]  W2^T   (an unpadded XOR-swizzled image of both was measured in
  float *ldsWb = ldsWf + kW * kTS;                                // [64 in][kTS]   W2     round 5: conflict share 0.375 -> 0.231, launch 932 -> 958 us)
  __shared__ int ldsOff[kRows + 1], ldsRs[kRows], ldsNode[kRows];
  __shared__ float ldsInv[kRows];
  __shared__ __attribute__((aligned(16))) unsigned ldsSlots[kRows * 8];
  __shared__ uint16_t ldsEdge[kRows * kSlotWidth];
  __shared__ __attribute__((aligned(16))) float ldsBias[kW];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g16 = tid >> 4, q = tid & 15;
  const int ei = lane & 15, kq = lane >> 4;
  const int zero_slot = p.halo_rows;

  const EdgeTileRange tr(p.n_tiles);

  stage_weights<kT4, false, true>(p.wt, p.bias, kW, kW, tid, ldsWf, ldsWb, ldsBias);   // W2^T and W2 rows, bias
  zero_halo_row(ldsQ, zero_slot, g16, q);

  // dW2 accumulators of this wave: tile (ct, mt) <-> rows 16 ct .. + 15 (inputs) x columns 16 mt .. + 15 (outputs)
  f32x4 accW[4][4];
  float4 dbacc[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    dbacc[a] = f4_zero();
#pragma unroll
    for (int b = 0; b < 4; ++b) accW[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }

  TileMeta<Shape> meta;
  int jt = tr.wg_in_xcd;
  if (jt < tr.range_len) fetch_meta(p, tr.range_lo + jt, g16, q, meta);

  for (; jt < tr.range_len; jt += tr.wgs_per_xcd) {
    const int4 sc0 = meta.sc0, sc1 = meta.sc1;
    {   // stage the tile: P rows and the distinct Q rows (the other workgroup of the CU computes meanwhile)
      TileRows<Shape> rows;
      fetch_rows<false>(p.P, p.Q, kW, p.halo_rows, meta, g16, q, rows);
      // (stored here, not through stage_rows: with the call the swish / swish instantiations spill a register)
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        const int hh = g16 + 16 * k;
        if (hh < p.halo_rows) *reinterpret_cast<float4 *>(&ldsQ[hh * kTS + 4 * q]) = rows.hv[k];
      }
      *reinterpret_cast<float4 *>(&ldsP[g16 * kTS + 4 * q]) = rows.prow[0];
      *reinterpret_cast<float4 *>(&ldsP[(g16 + 16) * kTS + 4 * q]) = rows.prow[1];
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
    float4 qacc[kDqSlots];
#pragma unroll
    for (int j = 0; j < kDqSlots; ++j) qacc[j] = f4_zero();
    __syncthreads();

    for (int c0 = 0; c0 < total; c0 += kChunk4) {
      const bool wave_on = c0 + wave * kSlice < total;   // wave-uniform
      const int k = c0 + wave * kSlice + ei;
      const bool valid = k < total;
      float *mine = ldsS + (size_t)(wave * kSlice) * kTS;          // this wave's 16 rows of the staging tile
      float4 dz1[4] = {f4_zero(), f4_zero(), f4_zero(), f4_zero()};
      if (wave_on) {
        int r, slot;
        size_t pe;
        lane_edge(ldsEdge, ldsOff, ldsRs, k, valid, zero_slot, r, slot, pe);
        // incoming gradient rows of the edge's target (g = dout / deg for mean): issued now, used behind the first product
        // (kept raw until then: scaled at the load, the compiler loads them one after the other into one register
        // quad, each waited for before the next is issued -- three exposed round trips per slice)
        float4 gz[4];
        const float *grow = p.dout + (size_t)ldsNode[r] * kW + 4 * kq;
        const float inv = valid ? ldsInv[r] : 0.f;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) gz[mt] = *reinterpret_cast<const float4 *>(grow + 16 * mt);
        float4 a1[4], d1[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const int f = 16 * ct + 4 * kq;
          const float4 z = f4_add(*reinterpret_cast<const float4 *>(&ldsP[r * kTS + f]), *reinterpret_cast<const float4 *>(&ldsQ[slot * kTS + f]));
          act_both<ACT1>(z.x, a1[ct].x, d1[ct].x);
          act_both<ACT1>(z.y, a1[ct].y, d1[ct].y);
          act_both<ACT1>(z.z, a1[ct].z, d1[ct].z);
          act_both<ACT1>(z.w, a1[ct].w, d1[ct].w);
          if (!valid) a1[ct] = f4_zero();
        }
        // ---- z2 (transposed product), dz2 = g . act2'(z2).  The W2^T fragment of group (mt, ct) + 1 is asked for in front of the
        // four products of group (mt, ct): left to itself the compiler puts every ds_read right before its use and waits for it
        // (16 exposed LDS latencies per product; `SCHED_FENCE` keeps the order through scheduling)
        {
          const float *wl0 = ldsWf + ei * kTS + 4 * kq;
          float4 wq[2];
          float4 bq[2];
          wq[0] = *reinterpret_cast<const float4 *>(wl0);
          bq[0] = *reinterpret_cast<const float4 *>(&ldsBias[4 * kq]);
          f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int mt = g >> 2, ct = g & 3;
            if (g + 1 < 16) wq[(g + 1) & 1] = *reinterpret_cast<const float4 *>(wl0 + ((g + 1) >> 2) * 16 * kTS + 16 * ((g + 1) & 3));
            if (ct == 0 && mt + 1 < 4) bq[(mt + 1) & 1] = *reinterpret_cast<const float4 *>(&ldsBias[16 * (mt + 1) + 4 * kq]);
            SCHED_FENCE();
            const float4 w4 = wq[g & 1];
            acc = mfma16(w4.x, a1[ct].x, acc);
            acc = mfma16(w4.y, a1[ct].y, acc);
            acc = mfma16(w4.z, a1[ct].z, acc);
            acc = mfma16(w4.w, a1[ct].w, acc);
            SCHED_FENCE();
            if (ct == 3) {
              const float4 b4 = bq[mt & 1];
              const float4 z2 = make_float4(acc[0] + b4.x, acc[1] + b4.y, acc[2] + b4.z, acc[3] + b4.w);
              gz[mt] = f4_mul(f4_scale(inv, gz[mt]), make_float4(dact_c<ACT2>(z2.x), dact_c<ACT2>(z2.y), dact_c<ACT2>(z2.z), dact_c<ACT2>(z2.w)));
              dbacc[mt] = f4_add(dbacc[mt], gz[mt]);
              acc = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
          }
        }
        weight_grad_products<false>(mine, a1, gz, kW, kW, ei, kq, accW);   // dW2 += a1^T dz2
        // ---- da1 (transposed product with W2), dz1 = da1 . act1'(z1); fragments one group ahead as above
        {
          const float *wl0 = ldsWb + ei * kTS + 4 * kq;
          float4 wq[2];
          wq[0] = *reinterpret_cast<const float4 *>(wl0);
          f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            const int ct = g >> 2, mt = g & 3;
            if (g + 1 < 16) wq[(g + 1) & 1] = *reinterpret_cast<const float4 *>(wl0 + ((g + 1) >> 2) * 16 * kTS + 16 * ((g + 1) & 3));
            SCHED_FENCE();
            const float4 w4 = wq[g & 1];
            acc = mfma16(w4.x, gz[mt].x, acc);
            acc = mfma16(w4.y, gz[mt].y, acc);
            acc = mfma16(w4.z, gz[mt].z, acc);
            acc = mfma16(w4.w, gz[mt].w, acc);
            SCHED_FENCE();
            if (mt == 3) {
              dz1[ct] = f4_mul(make_float4(acc[0], acc[1], acc[2], acc[3]), d1[ct]);
              if (!DQ && valid) *reinterpret_cast<float4 *>(p.dE + pe * kW + 16 * ct + 4 * kq) = dz1[ct];   // (a non-temporal store here: +3 %)
              acc = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
          }
        }
      }
      // ---- dz1 of the chunk -> LDS, lane group g16 sums the rows of targets g16 and g16 + 16 in edge order (= dP)
      {
        float *mine2 = ldsS + (size_t)(wave * kSlice) * kTS;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) *reinterpret_cast<float4 *>(&mine2[ei * kTS + 16 * ct + 4 * kq]) = dz1[ct];
      }
      __syncthreads();
      row_sum_chunk(ldsS, c0, kChunk4, lo0, hi0, q, racc0);
      row_sum_chunk(ldsS, c0, kChunk4, lo1, hi1, q, racc1);
      if constexpr (DQ) {
        // lane q of a group looks at the slot ids of edges c0 + 16 i + q of the chunk; a ballot per i gives every group the 16 match
        // bits of its own slot; the set bits, lowest first, are the chunk's edges with that source in edge order
        unsigned sl4[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int kk = c0 + 16 * i + q;
          sl4[i] = kk < total ? (unsigned)(ldsEdge[kk] >> 8) : 0xffffu;
        }
        const int gsh = 16 * (g16 & 3);
#pragma unroll
        for (int j = 0; j < kDqSlots; ++j) {
          const unsigned s = (unsigned)(g16 + 16 * j);
          unsigned long long m = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) m |= ((__ballot(sl4[i] == s) >> gsh) & 0xffffull) << (16 * i);
          float4 acc = qacc[j];
          while (m) {   // (a two-edges-per-slot, three-slots-at-once form of this loop was measured: 1 075 against 988 us for the launch)
            const int kk = __builtin_ctzll(m);
            m &= m - 1;
            acc = f4_add(acc, *reinterpret_cast<const float4 *>(ldsS + kk * kTS + 4 * q));
          }
          qacc[j] = acc;
        }
      }
      __syncthreads();
    }
    if constexpr (DQ) {
#pragma unroll
      for (int j = 0; j < kDqSlots; ++j) {
        const int sl = g16 + 16 * j;
        if (j < 2) {   // own rows g16 / g16 + 16 of the tile
          const int node = j == 0 ? sc0.x : sc1.x;
          if (node >= 0) *reinterpret_cast<float4 *>(p.dQ + (size_t)node * kW + 4 * q) = qacc[j];
        } else if (sl < p.halo_rows) {
          *reinterpret_cast<float4 *>(p.dqpart + ((size_t)(tr.range_lo + jt) * kDqStride + sl) * kW + 4 * q) = qacc[j];
        }
      }
    }
    if (p.dP) {
      if (sc0.x >= 0) *reinterpret_cast<float4 *>(p.dP + (size_t)sc0.x * kW + 4 * q) = racc0;
      if (sc1.x >= 0) *reinterpret_cast<float4 *>(p.dP + (size_t)sc1.x * kW + 4 * q) = racc1;
    }
  }

  // ---- fold the waves' dW2 / db2 accumulators into this workgroup's slab, wave by wave (fixed order), then write it out
  {
    float *slab = ldsS;                                            // [65][64] <= [64][kTS]
    __syncthreads();
    for (int idx = tid; idx < (kW + 1) * kW; idx += kT4) slab[idx] = 0.f;
    fold_bias_lanes(dbacc);
    __syncthreads();
#pragma unroll   // (as the compiler did on its own while the body was written out here)
    for (int w = 0; w < kT4 / 64; ++w) {
      if (wave == w) fold_slab<false>(slab, kW, kW, accW, dbacc, ei, kq);
      __syncthreads();
    }
    float *dst = p.partial + (size_t)blockIdx.x * (kW + 1) * kW;
    for (int idx = tid; idx < (kW + 1) * kW; idx += kT4) dst[idx] = slab[idx];
  }
}

// the instantiation of an activation pair edge_mlp_forms.h admits (edge64_shape): f(A1, A2) with both as integral constants
template <class F>
int32_t edge64_pair(int act1, int act2, F f) {
  auto second = [&](auto a1) { return act2 == act1 ? f(a1, a1) : f(a1, std::integral_constant<int, NGPDE_ACT_IDENTITY>{}); };
  switch (act1) {
    case NGPDE_ACT_SWISH: return second(std::integral_constant<int, NGPDE_ACT_SWISH>{});
    case NGPDE_ACT_RELU: return second(std::integral_constant<int, NGPDE_ACT_RELU>{});
    default: return second(std::integral_constant<int, NGPDE_ACT_TANH>{});
  }
}

}  // namespace

int32_t launch_edge_mlp64_fwd(const ngpde_graph *g, const EdgeFwd &p, const EdgeMlpArgs &a, hipStream_t stream) {
  EdgeMlp64K k;
  fill_tile_args(g, tile_geom(g), k);
  k.aggr = a.d.aggr;
  k.P = a.P; k.Q = a.Q; k.wt = a.wt[0]; k.bias = a.bias[0]; k.out = a.out;
  NGPDE_STAMP_SET(k, kStampEdge64, 0);
  return edge64_pair(p.act1, p.act2, [&](auto a1, auto a2) {
    return launch_with_lds(edge_mlp64_fwd_kernel<decltype(a1)::value, decltype(a2)::value>, p.grid, p.threads, p.lds, stream, k, "edge_mlp64_fwd_kernel");
  });
}

// dQ[node] += the partial rows of the OTHER tiles whose halo list holds the node (entries ascending by tile: fixed order); the node's
// own tile has stored its share.  One 16-lane group per listed node (the nodes no other tile references are not touched).
__global__ __launch_bounds__(256) void edge64_dq_combine_kernel(int n_listed, const int *__restrict__ nodes, const int *__restrict__ ptr,
                                                                const int *__restrict__ ent, const float *__restrict__ part, float *__restrict__ dQ) {
  const int k = (int)((blockIdx.x * (size_t)blockDim.x + threadIdx.x) >> 4), q = threadIdx.x & 15;
  if (k >= n_listed) return;
  const int lo = ptr[k], hi = ptr[k + 1];
  float4 *dst = reinterpret_cast<float4 *>(dQ + (size_t)nodes[k] * kW + 4 * q);
  float4 a = *dst;
  for (int e = lo; e < hi; ++e) a = f4_add(a, *reinterpret_cast<const float4 *>(part + (size_t)ent[e] * kW + 4 * q));
  *dst = a;
}

// ---- pullback launch (launch_edge_mlp_fused_bwd has checked the workspace and the dE rule)
int32_t launch_edge_mlp64_bwd(const ngpde_graph *g, const EdgeBwd &p, const EdgeMlpBwdArgs &a, hipStream_t stream) {
  const TileGeom t = tile_geom(g);
  EdgeMlp64BwdK k;
  fill_tile_args(g, t, k);
  k.aggr = a.d.aggr;
  k.P = a.P; k.Q = a.Q; k.wt = a.wt[0]; k.bias = a.bias[0]; k.dout = a.dout;
  k.dP = a.dP; k.dE = a.dE;
  Workspace w(a.workspace);
  EdgeBwdWs ws;
  edge_mlp_bwd_layout(w, t, a.d, p.form, ws);
  k.partial = ws.partial[0];
  const HaloInverse *hinv = nullptr;
  if (p.dq) {
    int32_t sti = graph_halo_inverse(g, kDqStride, &hinv);
    if (sti) return sti;
  }
  k.dqpart = p.dq ? ws.dqpart : nullptr;
  k.dQ = p.dq ? a.dQ : nullptr;
  int32_t st = edge64_pair(p.act1, p.act2, [&](auto a1, auto a2) {
    return p.dq ? launch_with_lds(edge_mlp64_bwd_kernel<decltype(a1)::value, decltype(a2)::value, true>, p.grid, p.threads, p.lds, stream, k, "edge_mlp64_bwd_kernel")
                : launch_with_lds(edge_mlp64_bwd_kernel<decltype(a1)::value, decltype(a2)::value, false>, p.grid, p.threads, p.lds, stream, k, "edge_mlp64_bwd_kernel");
  });
  if (st) return st;
  if ((st = launch_dense_weight_reduce(p.grid, kW, kW, k.partial, a.dwt[0], a.dbias[0], stream))) return st;
  if (p.dq && hinv->n_listed > 0) {
    const int64_t threads = (int64_t)hinv->n_listed * 16;
    hipLaunchKernelGGL(edge64_dq_combine_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, hinv->n_listed, hinv->node, hinv->ptr,
                       hinv->ent, k.dqpart, a.dQ);
    NGPDE_LAUNCH_CHECK("edge64_dq_combine_kernel");
  }
  if (p.by_source && (st = launch_edge_sum_by_source(g, kW, a.dE, a.dQ, stream))) return st;
  return NGPDE_OK;
}

}  // namespace ngpde
