// node_persistent.hip -- the fixed-step neural graph ODE over Chain(GCNConv(64 => 64, relu), GCNConv(64 => 64, relu)) as TWO
// persistent launches (forward solve, discrete adjoint) instead of 1205 kernel launches replayed from HIP graphs.
// [caller of the hot path in the reference: docs/src/tutorials/graph_node.md:44-66, :78; layer: src/layers.jl:200-239]
//
// Why: at the BASELINE size (16 384 nodes = 512 tiles of 32 rows) every launch of the replayed plan is exactly one wave of
// co-resident workgroups, the tile -> workgroup map never changes, and each launch pays the platform's dependent-launch floor
// (1.87 us, tools/launch_floor.hip) plus a cold start in which halo lists, slot bytes, schedule entries and W are fetched again
// -- 1205 times.  Here a workgroup keeps its tile for the whole solve:
//   * in registers: the tile's own rows of u and of the six stage derivatives k_j (forward) / of lambda and the stage adjoints
//     U-bar_j (adjoint), the dW / db accumulators of both layers for the whole adjoint (no slab read-modify-write), slot bytes,
//     halo node ids, c;
//   * in LDS: both W^T, the biases, the tile's own rows of the array being exchanged (halo slots 0..31);
//   * exchanged through memory: only the 32 rows a tile produces per phase (sc1 = write-through stores) and the <= 64 rows of
//     OTHER tiles its halo references (sc1 loads straight into LDS by LDS-DMA).
// A grid-wide barrier costs 9.2 us per phase on this chip (tools/persistent_floor.hip, mode 3); the dependency is local, so a
// tile waits only for the tiles its halo references: one flag word per tile holding the last finished phase, written by one
// lane after every wave has drained its stores (s_waitcnt vmcnt(0)) and the workgroup has met at a barrier, polled relaxed by
// one wave of the consumer.  Measured floor of that hand-off with this geometry: 2.3-2.5 us per phase, every payload word
// checked (mode 1 of the same tool; the launch-boundary form is 1.87 us + the cold start).  The wait list is the symmetric
// closure of "my halo references a row of yours" over BOTH directions of the graph: a tile that waits for its readers of the
// previous phase also may overwrite the array they read (the two exchanged arrays ping-pong).
// Every spin is bounded (abort word + ~2 s timeout); an aborted solve poisons its outputs with NaN and raises the plan's
// fault flag (ngpde_node_fault).  All workgroups must be co-resident: the host checks the grid against the occupancy of the
// kernels and otherwise keeps the replayed plan (node.hip).  Two persistent solves in flight on one device (two processes or
// two streams) can starve each other of residency: one solve at a time per device, NGPDE_NO_PERSISTENT=1 for anything else.
//
// Arithmetic is that of the pre-scaled replayed plan (gcn_fused.hip, PRE = true) operation for operation: same aggregation
// order (slot bytes, then the own row), same fp32 MFMA products, same stage combinations in the same order.

#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <type_traits>
#include <vector>

#include "common.h"
#include "persistent_gcn_tile.h"
#include "stamps.h"
#include "switches.h"

namespace ngpde {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// forward solve
// ---------------------------------------------------------------------------------------------------------------------

// WGT (edge weights, src/layers.jl:206-231): the 4 KB of slot weights of the tile need LDS that two resident W^T do not leave, so layer 1's
// W^T is B fragments in registers for the whole launch (16 per lane; the forward kernel has them to spare) and only W2^T is in LDS
// HUB: the hub geometry (256-row halo, variable-length slot lists, long rows shared by the 32 lane groups, one workgroup per CU)
template <int ACT, bool TAPE, bool WGT = false, bool HUB = false>
__global__ __launch_bounds__(kThreads, HUB ? 2 : 4) void node_fwd_persistent_kernel(const PFwdK p) {
  static_assert(!(HUB && WGT), "hub geometry: its own weight lists (HubCtx::hw), not the WGT form");
  constexpr int XH = HUB ? kHubXhF : kXhF, MF = HUB ? kHubMetaF : kMetaF;
  __shared__ __attribute__((aligned(16))) float lds[XH + 2 * kTileF + (WGT ? kWF + kSlotWF : 2 * kWF) + 2 * PD + MF + 48 + 4];
  static_assert(!HUB || sizeof(lds) <= 160 * 1024 - 64, "one workgroup per CU");
  float *ldsXh = lds, *ldsT = lds + XH, *ldsZ = ldsT + kTileF, *ldsW1 = ldsZ + kTileF, *ldsW2 = WGT ? ldsW1 : ldsW1 + kWF;
  float *ldsSW = ldsW2 + kWF, *ldsB = WGT ? ldsSW + kSlotWF : ldsSW;
  float *ldsMeta = ldsB + 2 * PD, *ldsC = ldsMeta + MF;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48);
  typename std::conditional<HUB, HubCtx, TileCtx>::type c;
  if constexpr (HUB) hub_ctx_init(p.m, c, ldsMeta);
  else tile_ctx_init(p.m, c, ldsMeta);
  coef_to_lds(ldsC, p.cf, 42, c.tid);
  const int act = ACT >= 0 ? ACT : p.act;
  float4 *Xh4 = reinterpret_cast<float4 *>(ldsXh);
  float bw1[16];
  if constexpr (WGT) {
    reinterpret_cast<float2 *>(ldsSW)[c.tid] = reinterpret_cast<const float2 *>(p.m.slot_w + (size_t)c.tile * kSlotWF)[c.tid];   // [32][32]
    c.lds_w = ldsSW;
    const int i16 = c.lane & 15, kq = c.lane >> 4, ct = c.wave_u / PG::RT;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) bw1[4 * kb + r] = p.w1[(16 * kb + 4 * kq + r) * PD + 16 * ct + i16];
  } else {
    load_weight_lds(p.w1, ldsW1, c.tid, true);
  }
  load_weight_lds(p.w2, ldsW2, c.tid, true);
  biases_to_lds(ldsB, p.b1, p.b2, c.tid);
  if (!HUB) zero_halo_row(ldsXh, c.grp == 0, c.q);
  if (c.tid == 0) *s_ok = 1;
  const unsigned own = own_row_offset(c);   // byte offset of this thread's 16 bytes in a [N][64] array
  __syncthreads();
  // own rounds of this wave's rows (the plan's own-first tables; 0: everything is summed behind the gather, as without them)
  int of_pre = 0;
  if constexpr (!HUB && !WGT) {
    if (p.m.of_pre) of_pre = __builtin_amdgcn_readfirstlane((int)p.m.of_pre[(size_t)c.tile * 8 + c.wave_u]);
  }
  const float4 bias1 = reinterpret_cast<const float4 *>(ldsB)[c.q], bias2 = reinterpret_cast<const float4 *>(ldsB + PD)[c.q];
  bool ok = true;
  int ph = 0;   // phases count on across the members: a tile starts the next trajectory while its neighbours finish this one
  for (int mb = 0; mb < p.n_members; ++mb) {
  const float *u_in = p.u_in + (size_t)mb * p.row_elems;
  const size_t ev0 = (size_t)mb * p.n_steps * p.S * 2;
  float4 u = f4_sel(c.valid && ok, ld4_g(u_in, own), f4_zero());
  // six named values written through component-wise selects (f4_sel): an array written as `k[j] = (j == i) ? yv : k[j]` ends
  // up in scratch memory
  float4 k0 = f4_zero(), k1 = f4_zero(), k2 = f4_zero(), k3 = f4_zero(), k4 = f4_zero(), k5 = f4_zero();
  Xh4[c.grp * PG::LPR + c.q] = u;   // (nobody reads the halo slots between a publish and the next gather's barrier ...
  if constexpr (!HUB && !WGT) __syncthreads();   // ... except the own rounds of a member's first phase, summed ahead of any barrier)
  for (int n = 0; n < p.n_steps && ok; ++n) {
    for (int i = 0; i < p.S && ok; ++i) {
#pragma unroll
      for (int layer = 0; layer < 2; ++layer) {
        ++ph;
        const float *X = layer == 0 ? ((n == 0 && i == 0) ? u_in : p.bufA) : p.bufB;
        NGPDE_PHASE_STAMP(p.m.stamps, ph, 0);
        float4 agg;
        if constexpr (HUB) {
          unsigned sw[8];
          hub_slot_words(c, sw);
          if (!hub_wait(p.m, c, ph, s_ok)) { ok = false; break; }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
          hub_gather_foreign(c, X, ldsXh);
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          agg = hub_aggregate(c, sw, ldsXh, ldsZ);   // (the product's output tile is free until this phase's product)
        } else if constexpr (!WGT) {
          unsigned sw[8], swf[8];
          tile_slot_words(c, sw);
          tile_slot_words_from(c, of_pre, swf);
          unsigned goff[2];
          tile_gather_offsets(c, goff);
          const float4 self = Xh4[c.grp * PG::LPR + c.q];   // (this thread's own store of the last epilogue)
          float4 a = tile_aggregate_rounds(c, sw, ldsXh, f4_zero(), of_pre);   // own rows: under the wait
          tile_wait_arrive(p.m, c, ph, s_ok, p.m.flags);
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
          if (!tile_gather_foreign_checked(c, X, ldsXh, goff, s_ok)) { ok = false; break; }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          a = tile_aggregate_rounds(c, swf, ldsXh, a, ((c.wmax + 3) >> 2) - of_pre);
          agg = f4_add(a, self);
        } else {
          unsigned sw[8];
          tile_slot_words(c, sw);
          if (!tile_wait(p.m, c, ph, s_ok)) { ok = false; break; }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
          tile_gather_foreign(c, X, ldsXh);
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          agg = tile_aggregate_weighted(c, ldsXh);
        }
        float4 acc = f4_scale(c.ci, agg);   // a_i = c_i * sum of the stored (pre-scaled) rows
        tile_row_store(ldsT, c, acc);
        const size_t ev = ev0 + (size_t)(n * p.S + i) * 2 + layer;
        __syncthreads();
        NGPDE_PHASE_STAMP(p.m.stamps, ph, 3);
        if (WGT && layer == 0) mfma_rows_times_bfrag64(ldsT, bw1, ldsZ, c.wave_u, c.lane);
        else mfma_rows_times_bt<PD>(ldsT, layer == 0 ? ldsW1 : ldsW2, ldsZ, c.wave_u, c.lane);
        __syncthreads();
        NGPDE_PHASE_STAMP(p.m.stamps, ph, 4);
        const float4 z = fwd_preact(ldsZ, c, layer == 0 ? bias1 : bias2);
        const uint8_t sign_bits = relu_sign_bits(z);
        float4 yv = fwd_output(c, act, z);
        if (layer == 0) {
          if (c.valid) store_sc1(p.bufB, own, yv);
          Xh4[c.grp * PG::LPR + c.q] = yv;
        } else {
          // k_i = yv, kept in its register; then the next stage input (or the step update)
          k0 = f4_sel(i == 0, yv, k0); k1 = f4_sel(i == 1, yv, k1); k2 = f4_sel(i == 2, yv, k2);
          k3 = f4_sel(i == 3, yv, k3); k4 = f4_sel(i == 4, yv, k4); k5 = f4_sel(i == 5, yv, k5);
          const float4 v = rk_combine<false>(RkCoefInPlace{ldsC, i}, i, yv, u, k0, k1, k2, k3, k4);
          if (i == p.S - 1) u = v;
          if (c.valid) store_sc1(p.bufA, own, v);
          Xh4[c.grp * PG::LPR + c.q] = v;
        }
        NGPDE_PHASE_STAMP(p.m.stamps, ph, 5);
        tile_publish(p.m, c, ph);
        NGPDE_PHASE_STAMP(p.m.stamps, ph, 6);
        // relu' for the adjoint (any other activation: the pre-activation itself): only the adjoint launch reads it, so it leaves
        // after the rows are published
        if constexpr (TAPE && ACT == NGPDE_ACT_RELU) stu8_g(p.masks + ev * p.mask_bytes + (size_t)c.tile * kThreads, (unsigned)c.tid, sign_bits);
        else if (TAPE && c.valid) st4_stream_g(p.ztape + ev * p.row_elems, own, z);
        // the tape row likewise: the aggregated row stays in ldsT until this thread overwrites it in the next phase, so its 64-bit address
        // arithmetic, its issue and its share of the publish's drain are out of the chain between "flags seen" and "flag published"
        if (TAPE && c.valid) st4_stream_g(p.tape + ev * p.row_elems, own, tile_row(ldsT, c));
      }
    }
  }
  // (a tile writes its rows of u(T) only after all readers of its u0 rows are past that member's first phase)
  if (c.valid) st4_g(p.u_out + (size_t)mb * p.row_elems, own, f4_sel(ok, u, f4_nan()));
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// forward solve, K tiles per workgroup taking turns ("tile rounds"): graphs of more tiles than two per co-resident workgroup
// ---------------------------------------------------------------------------------------------------------------------
// Workgroup b holds tiles t, t + W, ..., t + (K - 1) W (W = the grid) and walks them in that order in EVERY phase.  Nothing of a
// tile lives in registers across its turns: u and the stage derivatives are own rows of p.state (the same thread writes and
// reads them), the slot / halo tables are re-read per turn, and ONE layer's W^T is in LDS at a time (staged once per phase for
// all K tiles).  No gather-ahead pipeline is needed: by the time a tile's turn comes again the workgroup has spent K - 1 turns on
// its other tiles, and the neighbours' rows and flags of the previous phase have long arrived (what the GAT solver's batch kernels
// showed, gat_fused.hip).  A workgroup's own tiles may even be neighbours: turn s of phase ph needs the others' phase ph - 1 only.
// Arithmetic per tile is node_fwd_persistent_kernel's, operation for operation.  Weighted graphs only: each tile's slot weights
// take the LDS of the pipelined kernel below, which runs the unweighted ones.
template <int ACT, bool TAPE>
__global__ __launch_bounds__(kThreads, 4) void node_fwd_persistentK_kernel(const PFwdK p) {
  constexpr int kMS = meta_stride<true>(), kMT = meta_tiles<true>();
  __shared__ __attribute__((aligned(16))) float lds[kXhF + 2 * kTileF + kWF + 2 * PD + kMT * kMS + 48 + 4];
  static_assert(sizeof(lds) <= 80 * 1024 - 64, "two workgroups per CU");
  float *ldsXh = lds, *ldsT = lds + kXhF, *ldsZ = ldsT + kTileF, *ldsW = ldsZ + kTileF, *ldsB = ldsW + kWF;
  float *ldsMeta = ldsB + 2 * PD, *ldsC = ldsMeta + kMT * kMS;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48);
  const int tid = threadIdx.x, q = tid & 15;
  coef_to_lds(ldsC, p.cf, 42, tid);
  const int act = ACT >= 0 ? ACT : p.act;
  biases_to_lds(ldsB, p.b1, p.b2, tid);
  zero_halo_row(ldsXh, tid < PG::LPR, tid & 15);
  if (tid == 0) *s_ok = 1;
  const int W = p.pair_wgs, K = min(p.k_tiles, kMT);
  const int t0 = xcd_tile(blockIdx.x, W);
  const unsigned rowb = (unsigned)(p.row_elems * sizeof(float));
  tile_round_tables<true>(p.m, t0, W, K, ldsMeta);
  const int KT = tile_round_count(p.m, t0, W, K);   // tiles this workgroup really holds
  __syncthreads();
  const float4 bias1 = reinterpret_cast<const float4 *>(ldsB)[q], bias2 = reinterpret_cast<const float4 *>(ldsB + PD)[q];
  bool ok = true;
  int ph = 0;
  for (int n = 0; n < p.n_steps && ok; ++n) {
    for (int i = 0; i < p.S && ok; ++i) {
#pragma unroll 1
      for (int layer = 0; layer < 2 && ok; ++layer) {
        ++ph;
        const float *X = layer == 0 ? ((n == 0 && i == 0) ? p.u_in : p.bufA) : p.bufB;
        const size_t ev = (size_t)(n * p.S + i) * 2 + layer;
        const bool last_phase = (n == p.n_steps - 1 && i == p.S - 1 && layer == 1);
        load_weight_lds(layer == 0 ? p.w1 : p.w2, ldsW, tid, true);   // (every wave is past the previous phase's products: its last publish)
        for (int s = 0; s < K; ++s) {
          const int tile = t0 + s * W;
          if (tile >= p.m.n_tiles) break;   // uniform
          TileCtx c;
          tile_ctx_from_lds<true>(c, tile, ldsMeta + s * kMS);
          const unsigned own = own_row_offset(c);
          if (!tile_wait(p.m, c, ph, s_ok)) { ok = false; break; }
          halo_fill_all(c, X, ldsXh);
          // own rows of the state, in flight under the gather and the product: 0 = u, 1 + j = k_j (zero at launch, like the
          // registers of the one-tile kernel)
          float4 su = f4_zero(), sk0 = f4_zero(), sk1 = f4_zero(), sk2 = f4_zero(), sk3 = f4_zero(), sk4 = f4_zero();
          if (layer == 1) {
            su = (n == 0) ? f4_sel(c.valid, ld4_g(p.u_in, own), f4_zero()) : ld4_g(p.state, own);
            // (only the stage derivatives this stage combines, k_j with j < i: the others meet a zero coefficient)
            sk0 = i > 0 ? ld4_g(p.state, own + rowb) : f4_zero(); sk1 = i > 1 ? ld4_g(p.state, own + 2 * rowb) : f4_zero();
            sk2 = i > 2 ? ld4_g(p.state, own + 3 * rowb) : f4_zero(); sk3 = i > 3 ? ld4_g(p.state, own + 4 * rowb) : f4_zero();
            sk4 = i > 4 ? ld4_g(p.state, own + 5 * rowb) : f4_zero();
          }
          wait_vmcnt0();
          __syncthreads();   // halo rows landed (and the phase's W is in LDS)
          float4 acc = f4_scale(c.ci, tile_aggregate_weighted(c, ldsXh));
          tile_row_store(ldsT, c, acc);
          if (TAPE && c.valid) st4_stream_g(p.tape + ev * p.row_elems, own, acc);
          __syncthreads();
          mfma_rows_times_bt<PD>(ldsT, ldsW, ldsZ, c.wave_u, c.lane);
          __syncthreads();
          const float4 z = fwd_preact(ldsZ, c, layer == 0 ? bias1 : bias2);
          const uint8_t sign_bits = relu_sign_bits(z);
          const float4 yv = fwd_output(c, act, z);
          if (layer == 0) {
            if (c.valid) store_sc1(p.bufB, own, yv);
          } else {
            const float4 k0 = i == 0 ? yv : sk0, k1 = i == 1 ? yv : sk1, k2 = i == 2 ? yv : sk2, k3 = i == 3 ? yv : sk3, k4 = i == 4 ? yv : sk4;   // k_i is yv itself
            const float4 v = rk_combine<false>(RkCoefInPlace{ldsC, i}, i, yv, su, k0, k1, k2, k3, k4);
            if (c.valid) {
              if (i < p.S - 1) st4_g(p.state, own + (unsigned)(1 + i) * rowb, yv);   // (the last stage's derivative is combined here and never read again)
              if (i == p.S - 1) st4_g(p.state, own, v);
              if (last_phase) st4_g(p.u_out, own, v);
              store_sc1(p.bufA, own, v);
            }
          }
          tile_publish(p.m, c, ph);
          if constexpr (TAPE && ACT == NGPDE_ACT_RELU) stu8_g(p.masks + ev * p.mask_bytes + (size_t)c.tile * kThreads, (unsigned)c.tid, sign_bits);
          else if (TAPE && c.valid) st4_stream_g(p.ztape + ev * p.row_elems, own, z);
        }
      }
    }
  }
  if (!ok) {   // a wait was aborted: poison every row this workgroup owns
    __syncthreads();
    poison_tile_rounds(p.m, p.u_out, t0, W, KT, tid);
  }
}


// ---------------------------------------------------------------------------------------------------------------------
// forward solve, tile rounds with the NEXT turn's hand-off taken off the current turn's instruction stream
// ---------------------------------------------------------------------------------------------------------------------
// node_fwd_persistentK_kernel runs poll -> gather -> aggregate -> product -> epilogue -> drain -> flag one after the other for every
// turn (4.8 us), with only the CU's other workgroup to fill the three fabric round trips.  But a workgroup's NEXT turn depends on
// nothing this turn produces (turn s + 1 of a phase needs the neighbours' previous phase; turn 0 of the next phase needs what they
// finished K - 1 turns ago), so, as in the two-slot kernels (fwd_slot_phase):
//   T0  s_waitcnt vmcnt(0) + barrier: this turn's halo rows (gathered during the previous turn) have landed and the previous turn's
//       row stores are drained -> ITS flag goes out here (deferred publish); wave 0 issues the flag loads of the NEXT turn's wait
//       list (not waited for)
//   T1  LDS aggregation, operand tile, tape row; wave 0 looks at the flags; barrier (the halo region is free from here)
//   T2  if they were all there: the next turn's rows go out by LDS-DMA and travel under the product and the epilogue; product; barrier
//   T5  bias, activation, stage combination, row / state stores (not drained); then the next turn's state rows are fetched into the
//       registers this turn has just finished with
// A next turn whose flags were not there takes the blocking path at its T0.  Arithmetic per tile is node_fwd_persistent_kernel's.
template <int ACT, bool TAPE>
__global__ __launch_bounds__(kThreads, 4) void node_fwd_persistentKP_kernel(const PFwdK p) {
  constexpr int kMS = meta_stride<false>(), kMT = meta_tiles<false>();
  __shared__ __attribute__((aligned(16))) float lds[kXhF + 2 * kTileF + kWF + 2 * PD + kMT * kMS + 48 + 4];
  static_assert(sizeof(lds) <= 80 * 1024 - 64, "two workgroups per CU");
  float *ldsXh = lds, *ldsT = lds + kXhF, *ldsZ = ldsT + kTileF, *ldsW = ldsZ + kTileF, *ldsB = ldsW + kWF;
  float *ldsMeta = ldsB + 2 * PD, *ldsC = ldsMeta + kMT * kMS;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48), *s_pre = s_ok + 1;
  const int tid = threadIdx.x, q = tid & 15;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  coef_to_lds(ldsC, p.cf, 42, tid);
  const int act = ACT >= 0 ? ACT : p.act;
  biases_to_lds(ldsB, p.b1, p.b2, tid);
  zero_halo_row(ldsXh, tid < PG::LPR, tid & 15);
  if (tid == 0) *s_ok = 1, *s_pre = 0;
  const int W = p.pair_wgs, K = min(p.k_tiles, kMT);
  const int t0 = xcd_tile(blockIdx.x, W);
  const unsigned rowb = (unsigned)(p.row_elems * sizeof(float));
  tile_round_tables<false>(p.m, t0, W, K, ldsMeta);
  const int KT = tile_round_count(p.m, t0, W, K);   // tiles this workgroup really holds
  __syncthreads();
  const float4 bias1 = reinterpret_cast<const float4 *>(ldsB)[q], bias2 = reinterpret_cast<const float4 *>(ldsB + PD)[q];
  // no weight reload per phase (the tile-round kernel stages the phase's W^T in LDS every phase: ~1.2 k cycles per turn at four
  // tiles per workgroup): W2^T stays in LDS, W1^T is B fragments in registers for the whole launch (gcn_tile.h)
  float bw1[16];
  {
    const int i16 = lane & 15, kq = lane >> 4, ct = wave_u / PG::RT;
#pragma unroll
    for (int kb = 0; kb < 4; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) bw1[4 * kb + r] = p.w1[(16 * kb + 4 * kq + r) * PD + 16 * ct + i16];
  }
  load_weight_lds(p.w2, ldsW, tid, true);
  bool ok = true, pre = false;
  unsigned *pend_flags = nullptr;
  int pend_ph = 0, n_ahead = 0;
  // this turn's state rows (layer-2 turns): fetched at the end of the previous turn when its gather went out ahead, else at T0
  float4 su = f4_zero(), sk0 = f4_zero(), sk1 = f4_zero(), sk2 = f4_zero(), sk3 = f4_zero(), sk4 = f4_zero();
  auto load_state = [&](const TileCtx &c, unsigned own, int n, int si) {   // si: the stage whose layer-2 turn reads them
    su = (n == 0) ? f4_sel(c.valid, ld4_g(p.u_in, own), f4_zero()) : ld4_g(p.state, own);
    // (only the stage derivatives that stage combines, k_j with j < si: the others meet a zero coefficient)
    sk0 = si > 0 ? ld4_g(p.state, own + rowb) : f4_zero(); sk1 = si > 1 ? ld4_g(p.state, own + 2 * rowb) : f4_zero();
    sk2 = si > 2 ? ld4_g(p.state, own + 3 * rowb) : f4_zero(); sk3 = si > 3 ? ld4_g(p.state, own + 4 * rowb) : f4_zero();
    sk4 = si > 4 ? ld4_g(p.state, own + 5 * rowb) : f4_zero();
  };
  int ph = 0;
  for (int n = 0; n < p.n_steps && ok; ++n) {
    for (int i = 0; i < p.S && ok; ++i) {
#pragma unroll 1
      for (int layer = 0; layer < 2 && ok; ++layer) {
        ++ph;
        const float *X = layer == 0 ? ((n == 0 && i == 0) ? p.u_in : p.bufA) : p.bufB;
        const size_t ev = (size_t)(n * p.S + i) * 2 + layer;
        const bool last_phase = (n == p.n_steps - 1 && i == p.S - 1 && layer == 1);
        for (int s = 0; s < KT; ++s) {
          const int tile = t0 + s * W;
          TileCtx c;
          tile_ctx_from_lds<false>(c, tile, ldsMeta + s * kMS);
          const unsigned own = own_row_offset(c);
          // ---- T0
          [[maybe_unused]] const int turn = (ph - 1) * KT + s + 1;   // (stamps: one record per turn)
          NGPDE_PHASE_STAMP(p.m.stamps, turn, 0);
          wait_vmcnt0();
          __syncthreads();
          NGPDE_PHASE_STAMP(p.m.stamps, turn, 1);
          n_ahead += pre ? 1 : 0;
          if (pend_flags && tid == 0) __hip_atomic_store(pend_flags, (unsigned)pend_ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          pend_flags = nullptr;
          if (!pre) {
            if (!tile_wait(p.m, c, ph, s_ok)) { ok = false; break; }
            halo_fill_all(c, X, ldsXh);
            if (layer == 1) load_state(c, own, n, i);
            wait_vmcnt0();
            __syncthreads();
          }
          NGPDE_PHASE_STAMP(p.m.stamps, turn, 2);
          // ---- the turn after this one: the next tile of this phase, or this workgroup's first tile in the next phase
          const bool same_phase = s + 1 < KT;
          const int ns = same_phase ? s + 1 : 0, nph = same_phase ? ph : ph + 1, nlayer = same_phase ? layer : 1 - layer;
          const int nn = (same_phase || layer == 0) ? n : ((i == p.S - 1) ? n + 1 : n);
          const bool nexists = (same_phase || !last_phase) && KT > 1;   // (one tile: its own rows of the next phase are stored in THIS turn)
          const float *nX = same_phase ? X : (nlayer == 0 ? p.bufA : p.bufB);   // (only the launch's very first phase reads u_in)
          const float *nmeta = ldsMeta + ns * kMS;
          // its flags: fetched now, looked at behind the aggregation (they were published K - 1 turns ago: one look is enough).
          // (kFlagLine spelled out here and at pend_flags below: with flag_line this kernel's instructions move)
          unsigned f1 = 0;
          if (nexists && wave_u == 0) {
            const int nb = reinterpret_cast<const int *>(nmeta + kMetaF + kTM * 4)[lane];
            const unsigned *addr = (lane == 63) ? p.m.abort_word : (nb >= 0 ? p.m.flags + kFlagLine * nb : nullptr);
            f1 = (lane == 63) ? 0u : 0xffffffffu;
            if (addr) f1 = __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          // ---- T1
          float4 acc = f4_scale(c.ci, tile_aggregate_lean(c, ldsXh));
          tile_row_store(ldsT, c, acc);
          if (TAPE && c.valid) st4_stream_g(p.tape + ev * p.row_elems, own, acc);
          if (wave_u == 0) {
            const unsigned need = (unsigned)(nph - 1);
            const bool hit = nexists && __all((int)(lane == 63 ? f1 == 0u : f1 >= need)) != 0;
            if (lane == 0) *s_pre = hit ? 1 : 0;
          }
          __syncthreads();
          // ---- T2: the halo region is free; the next turn's rows travel under the product and the epilogue
          NGPDE_PHASE_STAMP(p.m.stamps, turn, 3);
          pre = *s_pre != 0;
          TileCtx cn;
          unsigned ownn = 0;
          if (pre) {
            tile_ctx_from_lds<false>(cn, t0 + ns * W, nmeta);
            ownn = own_row_offset(cn);
            halo_fill_all(cn, nX, ldsXh);
          }
          NGPDE_PHASE_STAMP(p.m.stamps, turn, 4);
          if (layer == 0) mfma_rows_times_bfrag64(ldsT, bw1, ldsZ, wave_u, lane);
          else mfma_rows_times_bt<PD>(ldsT, ldsW, ldsZ, wave_u, lane);
          __syncthreads();
          NGPDE_PHASE_STAMP(p.m.stamps, turn, 5);
          // ---- T5
          const float4 z = fwd_preact(ldsZ, c, layer == 0 ? bias1 : bias2);
          const RkCoef cf = rk_coef(ldsC, i);   // (read here: every LDS read of the epilogue in front of a DMA that may go out)
          const uint8_t sign_bits = relu_sign_bits(z);
          const float4 yv = fwd_output(c, act, z);
          if (layer == 0) {
            if (c.valid) store_sc1(p.bufB, own, yv);
          } else {
            const float4 k0 = i == 0 ? yv : sk0, k1 = i == 1 ? yv : sk1, k2 = i == 2 ? yv : sk2, k3 = i == 3 ? yv : sk3, k4 = i == 4 ? yv : sk4;
            const float4 v = rk_combine<false>(cf, i, yv, su, k0, k1, k2, k3, k4);
            if (c.valid) {
              if (i < p.S - 1) st4_g(p.state, own + (unsigned)(1 + i) * rowb, yv);   // (the last stage's derivative is combined here and never read again)
              if (i == p.S - 1) st4_g(p.state, own, v);
              if (last_phase) st4_g(p.u_out, own, v);
              store_sc1(p.bufA, own, v);
            }
          }
          if (pre && nlayer == 1) load_state(cn, ownn, nn, i);   // (this turn's state rows are dead from here; a layer-2 turn that follows this one belongs to stage i)
          pend_flags = p.m.flags + kFlagLine * tile;
          pend_ph = ph;
          if constexpr (TAPE && ACT == NGPDE_ACT_RELU) stu8_g(p.masks + ev * p.mask_bytes + (size_t)tile * kThreads, (unsigned)tid, sign_bits);
          else if (TAPE && c.valid) st4_stream_g(p.ztape + ev * p.row_elems, own, z);
          NGPDE_PHASE_STAMP(p.m.stamps, turn, 6);
        }
      }
    }
  }
  wait_vmcnt0();
  __syncthreads();
  if (ok && pend_flags && tid == 0) __hip_atomic_store(pend_flags, (unsigned)pend_ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!ok) {   // a wait was aborted: poison every row this workgroup owns
    __syncthreads();
    poison_tile_rounds(p.m, p.u_out, t0, W, KT, tid);
  }
  if (tid == 0 && p.m.stats) p.m.stats[2 * t0] = n_ahead;
}


// ---------------------------------------------------------------------------------------------------------------------
// forward solve, TWO trajectories of a batch interleaved in one workgroup
// ---------------------------------------------------------------------------------------------------------------------
// A block-diagonal batch of identical structures (test/runtests.jl:89-102, src/layers.jl:359-361) solved member after member
// pays the exposed hand-off (drain -> flag -> detect -> gather, ~2.4 us of a 4.1 us phase) once per member and phase: the CU idles
// while the rows travel.  Here a workgroup keeps the SAME tile of two members ("slots") and alternates between them phase by
// phase: while slot 0's rows and flag cross the fabric the workgroup aggregates, multiplies and stores slot 1's phase, and vice
// versa.  Each slot has its own exchanged arrays (bufA / bufB + slot * row_elems) and its own flag line per tile
// (flags + slot * flag_stride); wait lists, halo lists, slot bytes and W are shared.  The members are taken in pairs (0, 1),
// (2, 3), ...; an odd last member runs alone in slot 0.  Per-slot state in registers: u, k_0..k_5 and the slot's own row of the
// array it last published (the LDS halo region is shared by the slots, so the own rows are re-written at every phase start).
// Arithmetic per member is that of node_fwd_persistent_kernel operation for operation: u(T) is bitwise equal.
struct FSlot {
  float4 u, k0, k1, k2, k3, k4, k5, xown;
};

// What the fabric costs a slot-phase when its steps are simply run one after the other: the poll (a load that must reach memory),
// the gather of the foreign rows, the drain of the row stores in front of the flag -- three dependent round trips, ~2 us of a
// 3.8 us slot-phase, and alternating the slots alone hides none of them (measured: 18.3 ms for 8 members against 19.2 one by
// one).  So the round trips of the NEXT slot-phase are taken off the instruction stream of the current one:
//   T0  s_waitcnt vmcnt(0) + barrier: this slot-phase's halo rows have landed (gathered during the previous slot-phase) and the
//       previous slot-phase's row stores are drained -> ITS flag is published here (deferred publish: no wait of its own)
//   T1  LDS aggregation, operand tile, tape row
//   T2  barrier; wave 0 issues the flag loads of the NEXT slot-phase's wait list (not waited for)
//   T3  MFMA
//   T4  wave 0 looks at the flags it fetched; barrier
//   T5  if they were all there: the next slot-phase's own rows and the LDS-DMA of its foreign rows go out now (the halo region has
//       been free since T2) and fly during the epilogue; then bias, activation, stage combination, row stores (not drained)
// A next slot-phase whose flags were not there yet (or that does not exist: the last one, a single slot) takes the blocking
// path at its T0: publish what is pending, poll, gather -- the round-2 sequence.
struct FNext {          // the slot-phase after this one
  bool exists;
  int ph;               // its phase number
  const float *X;       // the array its halo rows come from
  const unsigned *flags;
};

// PAIR = false: the slots are the SAME tile of two members of a batch (c and cn are one context).  PAIR = true: the slots are two
// TILES of one member -- a graph of more tiles than co-resident workgroups (up to twice as many) -- with their own contexts; the
// exchanged arrays and the flag array are then common to both slots.
template <int ACT, bool TAPE, bool PAIR>
__device__ __forceinline__ bool fwd_slot_phase(const PFwdK &p, const TileCtx &c, const TileCtx &cn, FSlot &S, FSlot &Snext, const int sl, const int ph, const int n,
                                               const int i, const int layer, const float *X, const size_t ev0, const int act,
                                               const unsigned own, bool &pre, int &n_ahead, unsigned *&pend_flags, int &pend_ph, const FNext nx,
                                               float *ldsXh, float *ldsT, float *ldsZ, const float *ldsW, const float *ldsBias,
                                               const float *ldsC, int *s_ok, int *s_pre) {
  float4 *Xh4 = reinterpret_cast<float4 *>(ldsXh);
  float *bufA = p.bufA + (PAIR ? 0 : (size_t)sl * p.row_elems), *bufB = p.bufB + (PAIR ? 0 : (size_t)sl * p.row_elems);
  unsigned *flags = p.m.flags + (PAIR ? 0 : (size_t)sl * p.flag_stride);
  NGPDE_PHASE_STAMP(p.m.stamps, ph, 0);
  // T0
  wait_vmcnt0();
  __syncthreads();
  unsigned sw[8];
  tile_slot_words(c, sw);
  n_ahead += pre ? 1 : 0;
  if (pend_flags && c.tid == 0) __hip_atomic_store(pend_flags, (unsigned)pend_ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  pend_flags = nullptr;
  if (!pre) {
    Xh4[c.grp * PG::LPR + c.q] = S.xown;   // (behind the barrier: nobody is still aggregating from the halo region)
    if (!tile_wait(p.m, c, ph, s_ok, flags)) return false;
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
    tile_gather_foreign(c, X, ldsXh);
  }
  NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
  // T1
  float4 acc = f4_scale(c.ci, tile_aggregate(c, sw, ldsXh));
  tile_row_store(ldsT, c, acc);
  const size_t ev = ev0 + (size_t)(n * p.S + i) * 2 + layer;
  if (TAPE && c.valid) st4_stream_g(p.tape + ev * p.row_elems, own, acc);
  // T2
  __syncthreads();
  unsigned f1 = 0;
  if (nx.exists && c.wave_u == 0) f1 = poll_issue(p.m, cn, nx.flags);
  NGPDE_PHASE_STAMP(p.m.stamps, ph, 3);
  // T3
  mfma_rows_times_bt<PD>(ldsT, ldsW, ldsZ, c.wave_u, c.lane);
  // T4.  (A workgroup that runs AHEAD of its neighbours looks too early -- their flags of the phase before are published at the
  // top of their current slot-phase -- and takes the blocking path at its next T0, after which it is behind and finds them; a
  // second look behind the epilogue's arithmetic was measured: the barrier and the wait for the second load cost what the saved
  // blocking paths gave, 14.9 against 14.1 ms for 8 members.)
  if (c.wave_u == 0) {
    const bool hit = nx.exists && poll_ready(c, f1, nx.ph);
    if (c.lane == 0) *s_pre = hit ? 1 : 0;
  }
  __syncthreads();
  NGPDE_PHASE_STAMP(p.m.stamps, ph, 4);
  // T5.  Every LDS read of the epilogue comes BEFORE a DMA is issued (see halo_fill_ahead)
  pre = *s_pre != 0;
  const float4 z = f4_add(tile_row(ldsZ, c), reinterpret_cast<const float4 *>(ldsBias)[c.q]);   // (fwd_preact with the bias row read from LDS, behind the product's)
  const RkCoef cf = rk_coef(ldsC, i);
  if (pre) halo_fill_ahead(cn, nx.X, ldsXh, Snext.xown);
  const uint8_t sign_bits = relu_sign_bits(z);
  const float4 yv = fwd_output(c, act, z);
  float4 v = f4_zero();
  // (k_i = yv enters with the zero weight cf[i][i], as in node_fwd_persistent_kernel, where it is assigned first)
  if (layer != 0) v = rk_combine<true>(cf, i, yv, S.u, S.k0, S.k1, S.k2, S.k3, S.k4);
  if (layer == 0) {
    if (c.valid) store_sc1(bufB, own, yv);
    S.xown = yv;
  } else {
    S.k0 = f4_sel(i == 0, yv, S.k0); S.k1 = f4_sel(i == 1, yv, S.k1); S.k2 = f4_sel(i == 2, yv, S.k2);
    S.k3 = f4_sel(i == 3, yv, S.k3); S.k4 = f4_sel(i == 4, yv, S.k4); S.k5 = f4_sel(i == 5, yv, S.k5);
    if (i == p.S - 1) S.u = v;
    if (c.valid) store_sc1(bufA, own, v);
    S.xown = v;
  }
  NGPDE_PHASE_STAMP(p.m.stamps, ph, 5);
  pend_flags = flag_line(flags, c.tile);     // published at the next T0 (or behind the loops)
  pend_ph = ph;
  if (TAPE) stu8_g(p.masks + ev * p.mask_bytes + (size_t)c.tile * kThreads, (unsigned)c.tid, sign_bits);
  NGPDE_PHASE_STAMP(p.m.stamps, ph, 6);
  return true;
}

template <int ACT, bool TAPE, bool PAIR>
__global__ __launch_bounds__(kThreads, 4) void node_fwd_persistent2_kernel(const PFwdK p) {
  __shared__ __attribute__((aligned(16))) float lds[kXhF + 2 * kTileF + 2 * kWF + 2 * PD + (PAIR ? 2 : 1) * kMetaF + 48 + 4];
  float *ldsXh = lds, *ldsT = lds + kXhF, *ldsZ = ldsT + kTileF, *ldsW1 = ldsZ + kTileF, *ldsW2 = ldsW1 + kWF, *ldsB = ldsW2 + kWF;
  float *ldsMeta = ldsB + 2 * PD, *ldsC = ldsMeta + (PAIR ? 2 : 1) * kMetaF;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48), *s_pre = s_ok + 1;
  TileCtx c, c1s;
  tile_ctx_init(p.m, c, ldsMeta, PAIR ? xcd_tile(blockIdx.x, p.pair_wgs) : -1);
  const bool has1 = !PAIR || c.tile + p.pair_wgs < p.m.n_tiles;   // (PAIR: an odd tile count leaves the last workgroups one tile)
  if (PAIR) tile_ctx_init(p.m, c1s, ldsMeta + kMetaF, has1 ? c.tile + p.pair_wgs : c.tile);
  const TileCtx &c1 = PAIR ? c1s : c;
  coef_to_lds(ldsC, p.cf, 42, c.tid);
  const int act = ACT >= 0 ? ACT : p.act;
  load_weight_lds(p.w1, ldsW1, c.tid, true);
  load_weight_lds(p.w2, ldsW2, c.tid, true);
  biases_to_lds(ldsB, p.b1, p.b2, c.tid);
  zero_halo_row(ldsXh, c.grp == 0, c.q);
  if (c.tid == 0) *s_ok = 1, *s_pre = 0;
  const unsigned own = own_row_offset(c);
  const unsigned own1 = row_offset(c1.node, c.q);
  __syncthreads();
  bool ok = true;
  int ph = 0;   // both slots run the same phase numbers; the count runs on across the pairs
  bool pre = false;
  int n_ahead = 0;
  unsigned *pend_flags = nullptr;
  int pend_ph = 0;
  const int NP = p.n_steps * p.S * 2;   // phases of one member
  for (int mb = 0; mb < p.n_members && ok; mb += 2) {
    const bool two = PAIR ? has1 : mb + 1 < p.n_members;
    const float *u_in0 = p.u_in + (size_t)mb * p.row_elems, *u_in1 = u_in0 + ((two && !PAIR) ? p.row_elems : 0);
    const size_t ev00 = (size_t)mb * NP, ev01 = PAIR ? ev00 : ev00 + NP;
    const size_t boff1 = PAIR ? 0 : p.row_elems;            // slot 1's offset in the exchanged arrays
    unsigned *flags1 = p.m.flags + (PAIR ? 0 : p.flag_stride);
    FSlot s0, s1;
    s0.u = f4_sel(c.valid, ld4_g(u_in0, own), f4_zero());
    s1.u = f4_sel(c1.valid && two, ld4_g(u_in1, own1), f4_zero());
    s0.k0 = s0.k1 = s0.k2 = s0.k3 = s0.k4 = s0.k5 = f4_zero();
    s1.k0 = s1.k1 = s1.k2 = s1.k3 = s1.k4 = s1.k5 = f4_zero();
    s0.xown = s0.u;
    s1.xown = s1.u;
    int n = 0, i = 0;
    for (int P = 0; P < NP && ok; P += 2) {   // P: layer-1 phase of stage evaluation (n, i); P + 1: its layer-2 phase
#pragma unroll
      for (int layer = 0; layer < 2; ++layer) {
        ++ph;
        const float *ldsW = layer == 0 ? ldsW1 : ldsW2, *ldsBias = layer == 0 ? ldsB : ldsB + PD;
        // the arrays the halo rows of this phase / of the next phase come from, per slot
        const float *X0 = layer == 0 ? (P == 0 ? u_in0 : p.bufA) : p.bufB;
        const float *X1 = layer == 0 ? (P == 0 ? u_in1 : p.bufA + boff1) : p.bufB + boff1;
        FNext nx0, nx1;   // after (phase, slot 0): (phase, slot 1) if there are two slots; after (phase, slot 1): (phase + 1, slot 0)
        nx0.exists = two; nx0.ph = ph; nx0.X = X1; nx0.flags = flags1;
        nx1.exists = P + layer + 1 < NP; nx1.ph = ph + 1; nx1.X = layer == 0 ? p.bufB : p.bufA; nx1.flags = p.m.flags;
        if (!fwd_slot_phase<ACT, TAPE, PAIR>(p, c, c1, s0, s1, 0, ph, n, i, layer, X0, ev00, act, own, pre, n_ahead, pend_flags, pend_ph, nx0, ldsXh,
                                             ldsT, ldsZ, ldsW, ldsBias, ldsC, s_ok, s_pre)) { ok = false; break; }
        if (two && !fwd_slot_phase<ACT, TAPE, PAIR>(p, c1, c, s1, s0, 1, ph, n, i, layer, X1, ev01, act, own1, pre, n_ahead, pend_flags, pend_ph, nx1,
                                                    ldsXh, ldsT, ldsZ, ldsW, ldsBias, ldsC, s_ok, s_pre)) { ok = false; break; }
      }
      if (++i == p.S) i = 0, ++n;
    }
    // the last slot-phase's flag (the next pair's first phases wait for it; nothing was gathered ahead: pre is false here)
    wait_vmcnt0();
    __syncthreads();
    if (ok && pend_flags && c.tid == 0) __hip_atomic_store(pend_flags, (unsigned)pend_ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pend_flags = nullptr;
    // (a tile writes its rows of u(T) only after all readers of its u0 rows are past that member's first phase)
    if (c.valid) st4_g(p.u_out + (size_t)mb * p.row_elems, own, f4_sel(ok, s0.u, f4_nan()));
    if (two && c1.valid) st4_g(p.u_out + (PAIR ? 0 : (size_t)(mb + 1) * p.row_elems), own1, f4_sel(ok, s1.u, f4_nan()));
    if (PAIR) break;   // one member
  }
  if (!ok) {   // an aborted solve poisons every member's output
    poison_members(p.u_out, p.n_members, p.row_elems, c.valid, own);
    poison_members(p.u_out, p.n_members, p.row_elems, PAIR && has1 && c1.valid, own1);
  }
  if (c.tid == 0 && p.m.stats) p.m.stats[2 * c.tile] = n_ahead;
}

// ---------------------------------------------------------------------------------------------------------------------
// discrete adjoint
// ---------------------------------------------------------------------------------------------------------------------

// ACT = NGPDE_ACT_RELU: relu' from the forward launch's sign bits; ACT = -1: any activation (p.act), act'(z) from the saved
// pre-activations (one more tape row per phase)
// WGT: the tile's slot weights need 4 KB of LDS that two padded W do not leave (and the adjoint has no 16 registers to park
// fragments in: fetched per phase they spill).  W1 is kept UNPADDED and XOR-swizzled instead (16 KB, conflict-free fragment reads:
// gcn_tile.h, mfma_rows_times_bswz64), which makes exactly the room.
template <int ACT, bool WGT = false, bool HUB = false>
__global__ __launch_bounds__(kThreads, HUB ? 2 : 4) void node_bwd_persistent_kernel(const PBwdK p) {
  static_assert(!(HUB && WGT), "hub geometry: its own weight lists (HubCtx::hw), not the WGT form");
  constexpr bool RELU = (ACT == NGPDE_ACT_RELU);
  using Aux = typename std::conditional<RELU, unsigned, float4>::type;   // what act' is formed from: 4 sign bits / the row of z
  constexpr int XH = HUB ? kHubXhF : kXhF, MF = HUB ? kHubMetaF : kMetaF;
  __shared__ __attribute__((aligned(16))) float lds[XH + 2 * kTileF + (WGT ? PD * PD + kWF + kSlotWF : 2 * kWF) + MF + 48 + 4];
  static_assert(sizeof(lds) <= (HUB ? 160 : 80) * 1024 - 64, "two workgroups per CU (hub geometry: one)");
  float *ldsXh = lds, *ldsG = lds, *ldsDZ = lds + XH, *ldsX = ldsDZ + kTileF, *ldsW1 = ldsX + kTileF, *ldsW2 = ldsW1 + (WGT ? PD * PD : kWF);
  float *ldsSW = ldsW2 + kWF;
  float *ldsMeta = WGT ? ldsSW + kSlotWF : ldsSW, *ldsC = ldsMeta + MF;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48);
  typename std::conditional<HUB, HubCtx, TileCtx>::type c;
  if constexpr (HUB) hub_ctx_init(p.m, c, ldsMeta);
  else tile_ctx_init(p.m, c, ldsMeta);
  coef_to_lds(ldsC, p.cb, 48, c.tid);
  float4 *Xh4 = reinterpret_cast<float4 *>(ldsXh);
  if constexpr (WGT) {
    reinterpret_cast<float2 *>(ldsSW)[c.tid] = reinterpret_cast<const float2 *>(p.m.slot_w + (size_t)c.tile * kSlotWF)[c.tid];
    c.lds_w = ldsSW;
#pragma unroll
    for (int k = 0; k < PG::W4; ++k) {   // W1 straight (B^T[j = in][k = out] = W1[j][k]), quad k4 of row j at quad k4 ^ (j & 15)
      const int idx = c.tid + k * kThreads;
      if (idx < PD * PD / 4) {
        const int wi = (idx * 4) / PD, w4 = ((idx * 4) % PD) / 4;
        *reinterpret_cast<float4 *>(&ldsW1[wi * PD + 4 * (w4 ^ (wi & 15))]) = reinterpret_cast<const float4 *>(p.w1)[idx];
      }
    }
  } else {
    load_weight_lds(p.w1, ldsW1, c.tid, false);
  }
  load_weight_lds(p.w2, ldsW2, c.tid, false);
  if (!HUB) zero_halo_row(ldsXh, c.grp == 0, c.q);
  if (c.tid == 0) *s_ok = 1;
  const unsigned own = own_row_offset(c);
  f32x4 dw1[PG::DWT], dw2[PG::DWT];
#pragma unroll
  for (int mm = 0; mm < PG::DWT; ++mm) dw1[mm] = dw2[mm] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f;
  const int dbc = c.tid / PG::DBP, dbpart = c.tid % PG::DBP;
  const int S = p.S;
  __syncthreads();

  // the dense half of a phase: dL/dy = c .* K-bar, relu' by the sign bits, G = dZ W^T -> c .* G stored for the next gather,
  // dW += A^T dZ, db += column sums; then publish and keep the own rows of G in the halo slots
  auto tape_row = [&](size_t ev) { return ld4_stream_g(p.tape + ev * p.row_elems, own); };
  auto mask_of = [&](size_t ev) -> Aux {
    if constexpr (RELU) return ldu8_g(p.masks + ev * p.mask_bytes + (size_t)c.tile * kThreads, (unsigned)c.tid);
    else return ld4_stream_g(p.ztape + ev * p.row_elems, own);
  };
  // The tape row and the sign bits of the NEXT phase (mk_n / xrow_n) are asked for between the publish and the parameter-gradient
  // products: cold rows from HBM, ~4.6 k cycles away.  Asked for at the head of their own phase -- in front of the poll, as rounds
  // 2 - 3 had it -- they hold the poll up, because a wave's loads return in order: the first look at the flags came back only behind
  // the tape row (wait 4.6 k cycles against the forward kernel's 3.0 k for the same hand-off).
  Aux mk_n{};
  float4 xrow_n = f4_zero();
  // The first look at the NEXT phase's flags is asked for right behind the publish, in front of the tape prefetch and the
  // parameter-gradient products (poll_issue), and read when the next phase begins (tile_wait_primed): a tile whose neighbours have all
  // published before it no longer pays a poll round trip at the top of the phase.  Measured (round 6, same box, alternating): adjoint
  // launch 2.81 -> 2.78 ms.  (Also measured there and NOT kept: wave 0's tape rows fetched memory -> LDS by DMA a phase early, or by
  // four helper waves, so that nothing of wave 0's is in flight in front of its polls -- the hypothesis being that a wave's loads return
  // in order and the cold tape lines hold the polls up: adjoint 2.93 - 2.95 ms, the wait unchanged at 2.6 - 2.8 k cycles; and every
  // added register spills here -- 123 of 128 are taken -- a spilled dW accumulator is reloaded with s_waitcnt vmcnt(0) in front of the
  // products, which then waits for the tape rows.)
  unsigned f_next = 0;
  auto dense = [&](int ph, const float *ldsW, f32x4 (&dwl)[PG::DWT], float &dbl, float4 kbar, Aux mk, float4 xrow, float *gout, bool pf, size_t ev_n) {
    const float4 dz = adjoint_dz<RELU>(c, p.act, kbar, mk);
    tile_row_store(ldsDZ, c, dz);
    __syncthreads();
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 3);
    if (WGT && ldsW == ldsW1) mfma_rows_times_bswz64(ldsDZ, ldsW, ldsG, c.wave_u, c.lane);   // (layer 1 of a weighted graph: the unpadded, swizzled W1)
    else mfma_rows_times_bt<PD>(ldsDZ, ldsW, ldsG, c.wave_u, c.lane);
    __syncthreads();
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 4);
    const float4 gv = adjoint_g_row(ldsG, c);
    if (c.valid) store_sc1(gout, own, gv);
    // the tape row for the parameter-gradient products, which run behind the publish: written under the drain of the row stores, in
    // front of the publish's barrier (its readers of the phase before are two barriers back)
    adjoint_x_store(ldsX, c, xrow);
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 5);
    tile_publish(p.m, c, ph);
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 6);
    Xh4[c.grp * PG::LPR + c.q] = gv;   // behind the barrier: every thread has read its row of G (same LDS region)
    if constexpr (!HUB) {
      if (c.wave_u == 0) f_next = poll_issue(p.m, c, p.m.flags);
    }
    if (pf) {
      mk_n = mask_of(ev_n);
      xrow_n = tape_row(ev_n);
    }
    // behind the publish (the operand tiles stay intact until the next phase's dense half, two barriers away)
    param_grad_products(ldsX, ldsDZ, c.wave_u, c.lane, dbc, dbpart, dwl, dbl);
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 7);
  };

  bool ok = true;
  int ph = 0;   // phases count on across the members (the parameter-gradient accumulators too: the gradient of a batch is the sum)
  for (int mb = 0; mb < p.n_members; ++mb) {
  float *lam_g = p.lam + (size_t)mb * p.row_elems;
  const size_t ev0 = (size_t)mb * p.n_steps * S * 2;
  float4 lam = f4_sel(c.valid && ok, ld4_g(lam_g, own), f4_zero());
  float4 ub1 = f4_zero(), ub2 = f4_zero(), ub3 = f4_zero(), ub4 = f4_zero(), ub5 = f4_zero();   // named, not an array (see the forward kernel)
  if (ok) {   // first phase of a member: K-bar of the last stage of the last step = dt b_S lambda, layer 2's dense half (no gather:
              // g2 was last read two phases ago, so no wait either)
    ++ph;
    const size_t ev = ev0 + (size_t)((p.n_steps - 1) * S + (S - 1)) * 2 + 1;
    dense(ph, ldsW2, dw2, db2, adjoint_kbar_last(ldsC, S, lam), mask_of(ev), tape_row(ev), p.g2, true,
          ev0 + (size_t)((p.n_steps - 1) * S + (S - 1)) * 2);   // (next: layer 1 of the last stage of the last step)
  }
  for (int n = p.n_steps - 1; n >= 0 && ok; --n) {
    for (int i = S - 1; i >= 0 && ok; --i) {
      {   // layer 1 of stage i: dL/dy1 = A^T g2
        ++ph;
        NGPDE_PHASE_STAMP(p.m.stamps, ph, 0);
        const Aux mk = mk_n;                      // asked for behind the publish of the phase before
        const float4 xrow = xrow_n;
        // next: layer 2 of the stage evaluated before this one (none in the very last phase of the member)
        const bool last_next = (i == 0 && n == 0);
        const size_t ev_next = ev0 + ((i >= 1) ? (size_t)(n * S + i - 1) * 2 + 1 : (size_t)((max(n, 1) - 1) * S + (S - 1)) * 2 + 1);
        float4 t;
        if constexpr (HUB) {
          unsigned sw[8];
          hub_slot_words(c, sw);
          if (!hub_wait(p.m, c, ph, s_ok)) { ok = false; break; }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
          hub_gather_foreign(c, p.g2, ldsXh);
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          t = hub_aggregate(c, sw, ldsXh, ldsDZ);   // (the operand tiles of the previous phase's products are dead: that phase ended at this wait's barrier)
        } else if constexpr (WGT) {
          if (!tile_wait_primed(p.m, c, ph, s_ok, p.m.flags, f_next)) { ok = false; break; }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
          tile_gather_foreign(c, p.g2, ldsXh);
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          t = tile_aggregate_weighted(c, ldsXh);
        } else {
          unsigned sw[8], goff[2];
          tile_slot_words(c, sw);
          if constexpr (RELU) tile_gather_offsets(c, goff);   // (with a row of pre-activations in flight as well, the two offsets spill)
          if constexpr (RELU) {
            tile_wait_primed_arrive(p.m, c, ph, s_ok, p.m.flags, f_next);
            NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
            if (!tile_gather_foreign_checked(c, p.g2, ldsXh, goff, s_ok)) { ok = false; break; }
          } else {
            if (!tile_wait_primed(p.m, c, ph, s_ok, p.m.flags, f_next)) { ok = false; break; }
            NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
            tile_gather_foreign(c, p.g2, ldsXh);
          }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          float4 self;
          if constexpr (RELU) self = Xh4[c.grp * PG::LPR + c.q];   // asked for in front of the rounds: LDS reads return in order
          t = tile_aggregate_rounds_rolling(c, sw, ldsXh, f4_zero(), (c.wmax + 3) >> 2);
          if constexpr (!RELU) self = Xh4[c.grp * PG::LPR + c.q];
          t = f4_add(t, self);
        }
        dense(ph, ldsW1, dw1, db1, t, mk, xrow, p.g1, !last_next, ev_next);
      }
      {   // U-bar_i = A^T g1; K-bar of the stage evaluated before it (or the lambda update), layer 2's dense half
        ++ph;
        const bool last = (i == 0 && n == 0);
        NGPDE_PHASE_STAMP(p.m.stamps, ph, 0);
        const Aux mk = mk_n;                      // (the last phase of a member runs no dense half: nothing was asked for)
        const float4 xrow = xrow_n;
        // next: layer 1 of stage i - 1, or of the last stage of the step before
        const size_t ev_next = ev0 + (size_t)(i >= 1 ? n * S + i - 1 : (max(n, 1) - 1) * S + (S - 1)) * 2;
        float4 t;
        if constexpr (HUB) {
          unsigned sw[8];
          hub_slot_words(c, sw);
          if (!hub_wait(p.m, c, ph, s_ok)) { ok = false; break; }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
          hub_gather_foreign(c, p.g1, ldsXh);
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          t = hub_aggregate(c, sw, ldsXh, ldsDZ);   // (the operand tiles of the previous phase's products are dead: that phase ended at this wait's barrier)
        } else if constexpr (WGT) {
          if (!tile_wait_primed(p.m, c, ph, s_ok, p.m.flags, f_next)) { ok = false; break; }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
          tile_gather_foreign(c, p.g1, ldsXh);
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          t = tile_aggregate_weighted(c, ldsXh);
        } else {
          unsigned sw[8], goff[2];
          tile_slot_words(c, sw);
          if constexpr (RELU) tile_gather_offsets(c, goff);   // (with a row of pre-activations in flight as well, the two offsets spill)
          if constexpr (RELU) {
            tile_wait_primed_arrive(p.m, c, ph, s_ok, p.m.flags, f_next);
            NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
            if (!tile_gather_foreign_checked(c, p.g1, ldsXh, goff, s_ok)) { ok = false; break; }
          } else {
            if (!tile_wait_primed(p.m, c, ph, s_ok, p.m.flags, f_next)) { ok = false; break; }
            NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
            tile_gather_foreign(c, p.g1, ldsXh);
          }
          NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
          float4 self;
          if constexpr (RELU) self = Xh4[c.grp * PG::LPR + c.q];   // asked for in front of the rounds: LDS reads return in order
          t = tile_aggregate_rounds_rolling(c, sw, ldsXh, f4_zero(), (c.wmax + 3) >> 2);
          if constexpr (!RELU) self = Xh4[c.grp * PG::LPR + c.q];
          t = f4_add(t, self);
        }
        float4 kbar;
        if (i >= 1) {
          ub1 = f4_sel(i == 1, t, ub1); ub2 = f4_sel(i == 2, t, ub2); ub3 = f4_sel(i == 3, t, ub3);
          ub4 = f4_sel(i == 4, t, ub4); ub5 = f4_sel(i == 5, t, ub5);
          kbar = adjoint_kbar_stage(ldsC, i, t, lam, ub2, ub3, ub4, ub5);
        } else {
          const float4 v = adjoint_lambda_update(t, lam, ub1, ub2, ub3, ub4, ub5);
          lam = v;
          kbar = adjoint_kbar_last(ldsC, S, v);
        }
        if (last) break;   // (this phase writes nothing other tiles read: no flag; the next member's first phase publishes ph + 1)
        dense(ph, ldsW2, dw2, db2, kbar, mk, xrow, p.g2, true, ev_next);
      }
    }
  }
  if (c.valid) st4_g(lam_g, own, f4_sel(ok, lam, f4_nan()));
  }
  // the tile's contribution to the parameter gradients: one slab per tile, summed by reduce_slabs_kernel
  write_slab(dw1, db1, p.slab_dw1, p.slab_db1, c.wave_u, c.lane, dbc, dbpart, ok);
  write_slab(dw2, db2, p.slab_dw2, p.slab_db2, c.wave_u, c.lane, dbc, dbpart, ok);
}


// ---------------------------------------------------------------------------------------------------------------------
// discrete adjoint, TWO trajectories of a batch interleaved in one workgroup (see node_fwd_persistent2_kernel)
// ---------------------------------------------------------------------------------------------------------------------
// Registers are what this kernel is short of (128 per thread at two workgroups per CU; the parameter-gradient accumulators of
// both layers take 16, the matrix products ~40), so NO per-slot state stays in them between slot-phases:
//   * lambda lives in p.lam (its own array, [member][N][64]) and the stage adjoints U-bar_1..5 in a scratch array (p.ubar:
//     [slot][5][N][64]) -- rows private to the thread that owns them, written when formed, fetched at the top of the slot-phase
//     that combines them and dead again before the matrix products;
//   * a slot's own rows of the exchanged array come back by the same LDS-DMA as the foreign ones (they were stored write-through
//     a slot-phase earlier and are drained by then).
// Same products, same order of additions per member as node_bwd_persistent_kernel: du0 is bitwise equal; the parameter gradients
// are summed over the members in interleaved order (equal to rounding).
struct BNext {          // the slot-phase after this one (see fwd_slot_phase): what can be fetched for it ahead of time
  bool gather;          // it gathers halo rows (from X, after the flags of its wait list show ph - 1)
  int ph;
  const float *X;
  const unsigned *flags;
  bool tape;            // it reads a tape row and sign bits (event ev)
  size_t ev;
};

// PAIR: the slots are two TILES of one member (see fwd_slot_phase); a look at the next slot-phase's flags then never blocks -- with
// cross-slot neighbours a workgroup spinning for a flag that its neighbour publishes only behind ITS spin would be a cycle -- and
// a miss takes the blocking path at the next T0, which publishes what is pending first.
template <bool PAIR>
__global__ __launch_bounds__(kThreads, 4) void node_bwd_persistent2_kernel(const PBwdK p) {
  __shared__ __attribute__((aligned(16))) float lds[kXhF + 2 * kTileF + 2 * kWF + (PAIR ? 2 : 1) * kMetaF + 48 + 4];
  float *ldsXh = lds, *ldsG = lds, *ldsDZ = lds + kXhF, *ldsX = ldsDZ + kTileF, *ldsW1 = ldsX + kTileF, *ldsW2 = ldsW1 + kWF;
  float *ldsMeta = ldsW2 + kWF, *ldsC = ldsMeta + (PAIR ? 2 : 1) * kMetaF;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48), *s_pre = s_ok + 1;
  TileCtx c, c1s;
  tile_ctx_init(p.m, c, ldsMeta, PAIR ? xcd_tile(blockIdx.x, p.pair_wgs) : -1);
  const bool has1 = !PAIR || c.tile + p.pair_wgs < p.m.n_tiles;
  if (PAIR) tile_ctx_init(p.m, c1s, ldsMeta + kMetaF, has1 ? c.tile + p.pair_wgs : c.tile);
  const TileCtx &c1 = PAIR ? c1s : c;
  coef_to_lds(ldsC, p.cb, 48, c.tid);
  load_weight_lds(p.w1, ldsW1, c.tid, false);
  load_weight_lds(p.w2, ldsW2, c.tid, false);
  zero_halo_row(ldsXh, c.grp == 0, c.q);
  if (c.tid == 0) *s_ok = 1, *s_pre = 0;
  const unsigned own = own_row_offset(c);
  const unsigned own1 = row_offset(c1.node, c.q);
  f32x4 dw1[PG::DWT], dw2[PG::DWT];
#pragma unroll
  for (int mm = 0; mm < PG::DWT; ++mm) dw1[mm] = dw2[mm] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f;
  const int dbc = c.tid / PG::DBP, dbpart = c.tid % PG::DBP;
  const int S = p.S;
  __syncthreads();

  // state of the software pipeline (uniform): was the coming slot-phase's halo gathered ahead; the flag still to be published;
  // the tape row and sign bits fetched ahead for the coming slot-phase
  bool pre = false, dead = false;   // dead: a wait inside a dense half was aborted
  int n_ahead = 0;
  unsigned *pend_flags = nullptr;
  int pend_ph = 0;
  unsigned pf_mk = 0;
  float4 pf_x = f4_zero();

  // T0 of a slot-phase: everything this wave has in flight lands (halo rows gathered ahead, the previous slot-phase's row
  // stores), the workgroup meets, the previous slot-phase's flag goes out
  auto t0_publish = [&]() {
    wait_vmcnt0();
    __syncthreads();
    if (pend_flags && c.tid == 0) __hip_atomic_store(pend_flags, (unsigned)pend_ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pend_flags = nullptr;
  };

  // the operand tiles are __restrict__ so that the products' LDS reads do not wait for a DMA issued just before them into the halo
  // region (halo_fill_ahead); wave and lane are the kernel's own, whichever slot's context the dense half runs with
  auto dw_products = [&](const float *__restrict__ tX, const float *__restrict__ tDZ, f32x4 (&dwl)[PG::DWT], float &dbl) {
    param_grad_products(tX, tDZ, c.wave_u, c.lane, dbc, dbpart, dwl, dbl);
  };

  // the dense half of a slot-phase (T1's tail .. T5): dL/dy = c .* K-bar, relu' by the sign bits, G = dZ W^T -> c .* G stored for the
  // next gather (not drained: the flag goes out at the next T0), dW += A^T dZ, db += column sums; the next slot-phase's flags are
  // looked at under the matrix products and, if they are all there, its halo rows go out before the row stores
  // (c, own: this slot's tile; cn, ownn: the next slot-phase's)
  auto dense = [&](const TileCtx &c, const TileCtx &cn, unsigned own, unsigned ownn, unsigned *flags, int ph, const float *ldsW,
                   f32x4 (&dwl)[PG::DWT], float &dbl, float4 kbar, unsigned mk, float4 xrow, float *gout, const BNext &nx) {
    const float4 dz = adjoint_dz<true>(c, NGPDE_ACT_RELU, kbar, mk);
    tile_row_store(ldsDZ, c, dz);
    adjoint_x_store(ldsX, c, xrow);
    __syncthreads();   // T2
    if (nx.tape) {     // the next slot-phase's tape row and sign bits: a slot-phase ahead, so that they are there at its T0
      pf_mk = ldu8_g(p.masks + nx.ev * p.mask_bytes + (size_t)cn.tile * kThreads, (unsigned)c.tid);
      pf_x = ld4_stream_g(p.tape + nx.ev * p.row_elems, ownn);
    }
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 3);
    // T3: both matrix products of the phase back to back (no barrier between them: they read the same operand tiles and write
    // different things): G = dZ W^T into the halo region (free since T2), then dW += A^T dZ, db.  Wave 0 fetches the next
    // slot-phase's flags between the two -- as late as it can be done with the answer still there when the products end
    mfma_rows_times_bt<PD>(ldsDZ, ldsW, ldsG, c.wave_u, c.lane);
    unsigned f1 = 0;
    if (nx.gather && c.wave_u == 0) f1 = poll_issue(p.m, cn, nx.flags);
    dw_products(ldsX, ldsDZ, dwl, dbl);
    // T4: the next slot-phase's flags (members: wave 0 spins if this workgroup leads its neighbours, see tile_wait_primed; tile
    // pairs: one look, see the kernel's head), the barrier
    if (nx.gather && !PAIR) {   // uniform
      if (!tile_wait_primed(p.m, cn, nx.ph, s_ok, nx.flags, f1)) { dead = true; return; }
      pre = true;
    } else if (nx.gather) {
      if (c.wave_u == 0) {
        const bool hit = poll_ready(cn, f1, nx.ph);
        if (c.lane == 0) *s_pre = hit ? 1 : 0;
      }
      __syncthreads();
      pre = *s_pre != 0;
    } else {
      __syncthreads();
      pre = false;
    }
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 4);
    const float4 gv = adjoint_g_row(ldsG, c);
    if (pre) {   // uniform
      __syncthreads();   // every thread has read its row of G: the region is the halo again
      halo_fill_all(cn, nx.X, ldsXh);
    }
    if (c.valid) store_sc1(gout, own, gv);
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 5);
    pend_flags = flag_line(flags, c.tile);
    pend_ph = ph;
  };

  // the gathering half: T0, then (unless the rows were gathered ahead) own rows + blocking wait + gather
  auto top = [&](const TileCtx &c, const unsigned *flags, int ph, const float *X) -> bool {
    t0_publish();
    n_ahead += pre ? 1 : 0;
    if (!pre) {
      if (!tile_wait(p.m, c, ph, s_ok, flags)) return false;
      NGPDE_PHASE_STAMP(p.m.stamps, ph, 1);
      halo_fill_all(c, X, ldsXh);
      wait_vmcnt0();
      __syncthreads();
    }
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 2);
    return true;
  };

  // layer 1 of stage i of one slot: dL/dy1 = A^T g2
  auto phase_l1 = [&](const TileCtx &c, const TileCtx &cn, unsigned own, unsigned ownn, int sl, int ph, const BNext &nx) -> bool {
    float *g1 = p.g1 + (PAIR ? 0 : (size_t)sl * p.row_elems), *g2 = p.g2 + (PAIR ? 0 : (size_t)sl * p.row_elems);
    unsigned *flags = p.m.flags + (PAIR ? 0 : (size_t)sl * p.flag_stride);
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 0);
    const unsigned mk = pf_mk;
    const float4 xrow = pf_x;
    if (!top(c, flags, ph, g2)) return false;
    const float4 t = tile_aggregate_lean(c, ldsXh);   // (the unrolled form with the slot words in registers: 24 spilled dwords)
    dense(c, cn, own, ownn, flags, ph, ldsW1, dw1, db1, t, mk, xrow, g1, nx);
    return !dead;
  };

  // U-bar_i = A^T g1; K-bar of the stage evaluated before it (or the lambda update), layer 2's dense half.  `last`: the member's
  // final phase (no dense half, nothing published)
  auto phase_l2 = [&](const TileCtx &c, const TileCtx &cn, unsigned own, unsigned ownn, int sl, float *lam_g, int ph, int i, bool last,
                      const BNext &nx) -> bool {
    float *g1 = p.g1 + (PAIR ? 0 : (size_t)sl * p.row_elems), *g2 = p.g2 + (PAIR ? 0 : (size_t)sl * p.row_elems);
    float *ubar = p.ubar + (PAIR ? 0 : (size_t)sl * 5 * p.row_elems);   // (tile pairs: the rows of one member)
    unsigned *flags = p.m.flags + (PAIR ? 0 : (size_t)sl * p.flag_stride);
    NGPDE_PHASE_STAMP(p.m.stamps, ph, 0);
    const unsigned mk = pf_mk;
    const float4 xrow = pf_x;
    if (!top(c, flags, ph, g1)) return false;
    // the stage adjoints this combination needs: U-bar_j, j > i, of THIS step (j < S); everything else enters as an exact zero
    // (node_bwd_persistent_kernel keeps zeros / finished values with zero weights in those places).  ONE scalar base + 32-bit
    // offsets the optimiser cannot see through: five bases per slot ended up as 64-bit vector addresses hoisted out of the loops
    // and spilled
    float4 ub1 = f4_zero(), ub2 = f4_zero(), ub3 = f4_zero(), ub4 = f4_zero(), ub5 = f4_zero();
    const unsigned rowb = (unsigned)(p.row_elems * sizeof(float));
    unsigned uo = own;
    asm volatile("" : "+v"(uo));
    const float4 lam = f4_sel(c.valid, ld4_g(lam_g, uo), f4_zero());
    if (i < 1 && 1 < S) ub1 = ld4_g(ubar, uo);
    if (i < 2 && 2 < S) ub2 = ld4_g(ubar, uo + rowb);
    if (i < 3 && 3 < S) ub3 = ld4_g(ubar, uo + 2 * rowb);
    if (i < 4 && 4 < S) ub4 = ld4_g(ubar, uo + 3 * rowb);
    if (i < 5 && 5 < S) ub5 = ld4_g(ubar, uo + 4 * rowb);
    const float4 t = tile_aggregate_lean(c, ldsXh);   // (the unrolled form with the slot words in registers: 24 spilled dwords)
    float4 kbar;
    if (i >= 1) {
      if (c.valid) st4_g(ubar, uo + (unsigned)(i - 1) * rowb, t);   // U-bar_i
      kbar = adjoint_kbar_stage(ldsC, i, t, lam, ub2, ub3, ub4, ub5);
    } else {
      const float4 v = adjoint_lambda_update(t, lam, ub1, ub2, ub3, ub4, ub5);
      if (c.valid) st4_g(lam_g, uo, v);   // lambda of the step before (the member's dL/du~0 at the end)
      kbar = adjoint_kbar_last(ldsC, S, v);
    }
    if (!last) dense(c, cn, own, ownn, flags, ph, ldsW2, dw2, db2, kbar, mk, xrow, g2, nx);
    else pre = false;
    return !dead;
  };

  bool ok = true;
  int ph = 0;
  const size_t per = (size_t)p.n_steps * S * 2;   // tape events of one member
  for (int mb = 0; mb < p.n_members && ok; mb += 2) {
    const bool two = PAIR ? has1 : mb + 1 < p.n_members;
    float *lam_g0 = p.lam + (size_t)mb * p.row_elems, *lam_g1 = lam_g0 + ((two && !PAIR) ? p.row_elems : 0);
    const size_t ev00 = (size_t)mb * per, ev01 = PAIR ? ev00 : ev00 + per;
    const size_t goff1 = PAIR ? 0 : p.row_elems;            // slot 1's offset in the exchanged arrays
    unsigned *flags0 = p.m.flags, *flags1 = p.m.flags + (PAIR ? 0 : p.flag_stride);
    const size_t e1_first = (size_t)((p.n_steps - 1) * S + (S - 1)) * 2;   // layer-1 event of the first stage the adjoint visits
    {   // first phase of a member: K-bar of the last stage of the last step = dt b_S lambda, layer 2's dense half (no gather, no wait)
      ++ph;
      const size_t e = e1_first + 1;
      BNext nx;
      {
        t0_publish();
        const unsigned mk = ldu8_g(p.masks + (ev00 + e) * p.mask_bytes + (size_t)c.tile * kThreads, (unsigned)c.tid);
        const float4 xrow = ld4_stream_g(p.tape + (ev00 + e) * p.row_elems, own);
        // next: the same phase of slot 1 (nothing to gather; its tape row is read there), or layer 1 of slot 0
        // (one slot: nothing is gathered ahead -- the next slot-phase is this slot's own next phase, whose flags cannot be there
        // before this one's is published -- only its tape row is fetched)
        nx.gather = false; nx.ph = ph + 1; nx.X = p.g2; nx.flags = flags0; nx.tape = !two; nx.ev = ev00 + e1_first;
        const float4 lam = f4_sel(c.valid, ld4_g(lam_g0, own), f4_zero());
        dense(c, two ? c1 : c, own, two ? own1 : own, flags0, ph, ldsW2, dw2, db2, adjoint_kbar_last(ldsC, S, lam), mk, xrow, p.g2, nx);
        if (dead) ok = false;
      }
      if (two && ok) {
        t0_publish();
        const unsigned mk = ldu8_g(p.masks + (ev01 + e) * p.mask_bytes + (size_t)c1.tile * kThreads, (unsigned)c.tid);
        const float4 xrow = ld4_stream_g(p.tape + (ev01 + e) * p.row_elems, own1);
        nx.gather = true; nx.ph = ph + 1; nx.X = p.g2; nx.flags = flags0; nx.tape = true; nx.ev = ev00 + e1_first;
        const float4 lam = f4_sel(c1.valid, ld4_g(lam_g1, own1), f4_zero());
        dense(c1, c, own1, own, flags1, ph, ldsW2, dw2, db2, adjoint_kbar_last(ldsC, S, lam), mk, xrow, p.g2 + goff1, nx);
        if (dead) ok = false;
      }
    }
    for (int n = p.n_steps - 1; n >= 0 && ok; --n) {
      for (int i = S - 1; i >= 0 && ok; --i) {
        const bool last = (i == 0 && n == 0);
        const size_t e1 = (size_t)(n * S + i) * 2;
        const size_t e2 = (i >= 1) ? (size_t)(n * S + i - 1) * 2 + 1 : (size_t)((max(n, 1) - 1) * S + (S - 1)) * 2 + 1;
        const size_t e1n = (i >= 1) ? (size_t)(n * S + i - 1) * 2 : (size_t)((max(n, 1) - 1) * S + (S - 1)) * 2;   // layer-1 event of the stage after this one
        BNext nx;
        ++ph;   // layer 1
        // after (L1, slot 0): (L1, slot 1) or, with one slot, (L2, slot 0); after (L1, slot 1): (L2, slot 0)
        nx.gather = two; nx.ph = two ? ph : ph + 1; nx.X = two ? p.g2 + goff1 : p.g1; nx.flags = two ? flags1 : flags0;
        nx.tape = two ? true : !last; nx.ev = two ? ev01 + e1 : ev00 + e2;
        if (!phase_l1(c, two ? c1 : c, own, two ? own1 : own, 0, ph, nx)) { ok = false; break; }
        if (two) {
          nx.gather = true; nx.ph = ph + 1; nx.X = p.g1; nx.flags = flags0; nx.tape = !last; nx.ev = ev00 + e2;
          if (!phase_l1(c1, c, own1, own, 1, ph, nx)) { ok = false; break; }
        }
        ++ph;   // layer 2
        // after (L2, slot 0): (L2, slot 1) or, with one slot, the next stage's (L1, slot 0); after (L2, slot 1): the next (L1, slot 0)
        nx.gather = two; nx.ph = two ? ph : ph + 1; nx.X = two ? p.g1 + goff1 : p.g2; nx.flags = two ? flags1 : flags0;
        nx.tape = two ? !last : !last; nx.ev = two ? ev01 + e2 : ev00 + e1n;
        if (!phase_l2(c, two ? c1 : c, own, two ? own1 : own, 0, lam_g0, ph, i, last, nx)) { ok = false; break; }
        if (two) {
          nx.gather = !last; nx.ph = ph + 1; nx.X = p.g2; nx.flags = flags0; nx.tape = !last; nx.ev = ev00 + e1n;
          if (!phase_l2(c1, c, own1, own, 1, lam_g1, ph, i, last, nx)) { ok = false; break; }
        }
      }
    }
    // the last published slot-phase's flag (the final phase of a member publishes nothing; the next pair's first phase publishes
    // ph + 1 and waits for nothing)
    t0_publish();
    if (PAIR) break;   // one member
  }
  if (!ok) {
    poison_members(p.lam, p.n_members, p.row_elems, c.valid, own);
    poison_members(p.lam, p.n_members, p.row_elems, PAIR && has1 && c1.valid, own1);
  }
  write_slab(dw1, db1, p.slab_dw1, p.slab_db1, c.wave_u, c.lane, dbc, dbpart, ok);
  write_slab(dw2, db2, p.slab_dw2, p.slab_db2, c.wave_u, c.lane, dbc, dbpart, ok);
  if (c.tid == 0 && p.m.stats) p.m.stats[2 * c.tile + 1] = n_ahead;
}

// ---------------------------------------------------------------------------------------------------------------------
// adjoint, K tiles per workgroup taking turns (see node_fwd_persistentK_kernel): lambda and the stage adjoints are own rows of
// p.lam / p.ubar (zero at launch where the one-tile kernel starts from zero registers), one layer's W in LDS at a time, the
// parameter-gradient accumulators in registers over all tiles and phases (one slab per WORKGROUP at the end).  Weighted graphs
// only, as in the forward (unweighted: node_bwd_persistentKP_kernel).
// ---------------------------------------------------------------------------------------------------------------------
template <int ACT>
__global__ __launch_bounds__(kThreads, 4) void node_bwd_persistentK_kernel(const PBwdK p) {
  constexpr bool RELU = (ACT == NGPDE_ACT_RELU);
  using Aux = typename std::conditional<RELU, unsigned, float4>::type;
  constexpr int kMS = meta_stride<true>(), kMT = meta_tiles<true>();
  __shared__ __attribute__((aligned(16))) float lds[kXhF + 2 * kTileF + kWF + kMT * kMS + 48 + 4];
  static_assert(sizeof(lds) <= 80 * 1024 - 64, "two workgroups per CU");
  float *ldsXh = lds, *ldsG = lds, *ldsDZ = lds + kXhF, *ldsX = ldsDZ + kTileF, *ldsW = ldsX + kTileF;
  float *ldsMeta = ldsW + kWF, *ldsC = ldsMeta + kMT * kMS;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  coef_to_lds(ldsC, p.cb, 48, tid);
  zero_halo_row(ldsXh, tid < PG::LPR, tid & 15);
  if (tid == 0) *s_ok = 1;
  f32x4 dw1[PG::DWT], dw2[PG::DWT];
#pragma unroll
  for (int mm = 0; mm < PG::DWT; ++mm) dw1[mm] = dw2[mm] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f;
  const int dbc = tid / PG::DBP, dbpart = tid % PG::DBP;
  const int S = p.S, W = p.pair_wgs, K = min(p.k_tiles, kMT);
  const int t0 = xcd_tile(blockIdx.x, W);
  const unsigned rowb = (unsigned)(p.row_elems * sizeof(float));
  tile_round_tables<true>(p.m, t0, W, K, ldsMeta);
  const int Kv = tile_round_count(p.m, t0, W, K);   // tiles this workgroup really holds
  __syncthreads();

  // the dense half of a turn (node_bwd_persistent_kernel's, with the tile context as an argument)
  // The tape row and sign bits of the NEXT turn (mk_n / xrow_n: the workgroup's next tile in this phase, or its first tile in the next
  // phase) are asked for at the head of this turn's dense half, when this turn's own have just gone to LDS: cold rows, ~4.5 k cycles
  // away, with the product, the stores, the drain and the parameter-gradient products to arrive in.  (The drain in front of the flag
  // waits for them, which costs the publish ~1.5 k cycles -- nobody reads a tile's rows before the workgroup's other turns are through.
  // Asked for at the head of their own turn, in front of the poll, they held every turn's first look at the flags up by their
  // latency: a wave's loads return in order.)
  Aux mk_n{};
  float4 xrow_n = f4_zero();
  auto fetch = [&](size_t ev, int s) {
    const int node = max(reinterpret_cast<const int4 *>(ldsMeta + s * kMS + kMetaF)[tid >> 4].x, 0);
    const unsigned own = row_offset(node, tid & 15);
    if constexpr (RELU) mk_n = ldu8_g(p.masks + ev * p.mask_bytes + (size_t)(t0 + s * W) * kThreads, (unsigned)tid);
    else mk_n = ld4_stream_g(p.ztape + ev * p.row_elems, own);
    xrow_n = ld4_stream_g(p.tape + ev * p.row_elems, own);
  };
  auto dense = [&](const TileCtx &c, unsigned own, int ph, f32x4 (&dwl)[PG::DWT], float &dbl, float4 kbar, Aux mk, float4 xrow, float *gout,
                   bool pf, size_t ev_n, int s_n) {
    const float4 dz = adjoint_dz<RELU>(c, p.act, kbar, mk);
    tile_row_store(ldsDZ, c, dz);
    adjoint_x_store(ldsX, c, xrow);
    if (pf) fetch(ev_n, s_n);
    __syncthreads();
    mfma_rows_times_bt<PD>(ldsDZ, ldsW, ldsG, c.wave_u, c.lane);
    __syncthreads();
    const float4 gv = adjoint_g_row(ldsG, c);
    if (c.valid) store_sc1(gout, own, gv);
    tile_publish(p.m, c, ph);
    param_grad_products(ldsX, ldsDZ, c.wave_u, c.lane, dbc, dbpart, dwl, dbl);
  };

  bool ok = true;
  int ph = 0;
  {   // first phase: K-bar of the last stage of the last step = dt b_S lambda, layer 2's dense half (no gather, no wait)
    ++ph;
    const size_t ev = (size_t)((p.n_steps - 1) * S + (S - 1)) * 2 + 1;
    load_weight_lds(p.w2, ldsW, tid, false);
    if (Kv > 0) fetch(ev, 0);
    for (int s = 0; s < K; ++s) {
      const int tile = t0 + s * W;
      if (tile >= p.m.n_tiles) break;
      TileCtx c;
      tile_ctx_from_lds<true>(c, tile, ldsMeta + s * kMS);
      const unsigned own = own_row_offset(c);
      __syncthreads();   // (the phase's W is in LDS; the previous turn's products are done with the operand tiles)
      const float4 lam = f4_sel(c.valid, ld4_g(p.lam, own), f4_zero());
      const Aux mk = mk_n;
      const float4 xrow = xrow_n;
      const bool more = s + 1 < Kv;   // next: the workgroup's next tile, or layer 1 of the last stage of the last step on its first one
      dense(c, own, ph, dw2, db2, adjoint_kbar_last(ldsC, S, lam), mk, xrow, p.g2, true,
            more ? ev : (size_t)((p.n_steps - 1) * S + (S - 1)) * 2, more ? s + 1 : 0);
    }
  }
  for (int n = p.n_steps - 1; n >= 0 && ok; --n) {
    for (int i = S - 1; i >= 0 && ok; --i) {
      {   // layer 1 of stage i: dL/dy1 = A^T g2
        ++ph;
        const size_t ev = (size_t)(n * S + i) * 2;
        __syncthreads();
        load_weight_lds(p.w1, ldsW, tid, false);
        for (int s = 0; s < K; ++s) {
          const int tile = t0 + s * W;
          if (tile >= p.m.n_tiles) break;
          TileCtx c;
          tile_ctx_from_lds<true>(c, tile, ldsMeta + s * kMS);
          const unsigned own = own_row_offset(c);
          const Aux mk = mk_n;
          const float4 xrow = xrow_n;
          if (!tile_wait(p.m, c, ph, s_ok)) { ok = false; break; }
          halo_fill_all(c, p.g2, ldsXh);
          wait_vmcnt0();
          __syncthreads();
          const float4 t = tile_aggregate_weighted(c, ldsXh);
          __syncthreads();   // every thread has its sum: the region becomes the product's result tile
          // next: the workgroup's next tile, or layer 2 of the stage evaluated before this one (the very last phase asks for nothing)
          const bool more = s + 1 < Kv;
          const size_t ev_b = (i >= 1) ? (size_t)(n * S + i - 1) * 2 + 1 : (size_t)((max(n, 1) - 1) * S + (S - 1)) * 2 + 1;
          dense(c, own, ph, dw1, db1, t, mk, xrow, p.g1, more || !(i == 0 && n == 0), more ? ev : ev_b, more ? s + 1 : 0);
        }
        if (!ok) break;
      }
      {   // U-bar_i = A^T g1; K-bar of the stage evaluated before it (or the lambda update), layer 2's dense half
        ++ph;
        const bool last = (i == 0 && n == 0);
        const size_t ev = (i >= 1) ? (size_t)(n * S + i - 1) * 2 + 1 : (size_t)((max(n, 1) - 1) * S + (S - 1)) * 2 + 1;
        __syncthreads();
        load_weight_lds(p.w2, ldsW, tid, false);
        for (int s = 0; s < K; ++s) {
          const int tile = t0 + s * W;
          if (tile >= p.m.n_tiles) break;
          TileCtx c;
          tile_ctx_from_lds<true>(c, tile, ldsMeta + s * kMS);
          const unsigned own = own_row_offset(c);
          const Aux mk = mk_n;        // (the last phase runs no dense half: nothing was asked for)
          const float4 xrow = xrow_n;
          if (!tile_wait(p.m, c, ph, s_ok)) { ok = false; break; }
          halo_fill_all(c, p.g1, ldsXh);
          // lambda and the stage adjoints of this step from memory (rows 0..4 of ubar = U-bar_1..5), in flight under the gather
          const float4 lam = f4_sel(c.valid, ld4_g(p.lam, own), f4_zero());
          // (only the stage adjoints this stage combines, U-bar_j with i < j < S: the others meet a zero coefficient or are zero)
          const float4 lb1 = (i < 1 && S > 1) ? ld4_g(p.ubar, own) : f4_zero(), lb2 = (i < 2 && S > 2) ? ld4_g(p.ubar, own + rowb) : f4_zero(),
                       lb3 = (i < 3 && S > 3) ? ld4_g(p.ubar, own + 2 * rowb) : f4_zero(), lb4 = (i < 4 && S > 4) ? ld4_g(p.ubar, own + 3 * rowb) : f4_zero(),
                       lb5 = (i < 5 && S > 5) ? ld4_g(p.ubar, own + 4 * rowb) : f4_zero();
          wait_vmcnt0();
          __syncthreads();
          const float4 t = tile_aggregate_weighted(c, ldsXh);
          __syncthreads();
          const float4 ub1 = i == 1 ? t : lb1, ub2 = i == 2 ? t : lb2, ub3 = i == 3 ? t : lb3, ub4 = i == 4 ? t : lb4,
                       ub5 = i == 5 ? t : lb5;   // U-bar_i is t itself
          float4 kbar;
          if (i >= 1) {
            if (c.valid) st4_g(p.ubar, own + (unsigned)(i - 1) * rowb, t);
            kbar = adjoint_kbar_stage(ldsC, i, t, lam, ub2, ub3, ub4, ub5);
          } else {
            const float4 v = adjoint_lambda_update(t, lam, ub1, ub2, ub3, ub4, ub5);
            if (c.valid) st4_g(p.lam, own, v);
            kbar = adjoint_kbar_last(ldsC, S, v);
          }
          if (!last) {   // next: the workgroup's next tile, or layer 1 of stage i - 1 / of the last stage of the step before
            const bool more = s + 1 < Kv;
            const size_t ev_a = (size_t)(i >= 1 ? n * S + i - 1 : (max(n, 1) - 1) * S + (S - 1)) * 2;
            dense(c, own, ph, dw2, db2, kbar, mk, xrow, p.g2, true, more ? ev : ev_a, more ? s + 1 : 0);
          } else {
            __syncthreads();
          }
        }
        if (!ok) break;
      }
    }
  }
  if (!ok) {
    __syncthreads();
    poison_tile_rounds(p.m, p.lam, t0, W, Kv, tid);
  }
  write_slab(dw1, db1, p.slab_dw1, p.slab_db1, wave_u, lane, dbc, dbpart, ok);
  write_slab(dw2, db2, p.slab_dw2, p.slab_db2, wave_u, lane, dbc, dbpart, ok);
}


// ---------------------------------------------------------------------------------------------------------------------
// adjoint, tile rounds with the NEXT turn's hand-off taken off the current turn's instruction stream (round 5)
// ---------------------------------------------------------------------------------------------------------------------
// node_bwd_persistentK_kernel runs poll -> gather -> aggregate -> product -> store -> drain -> flag -> parameter-gradient products one
// after the other for every turn.  But a workgroup's NEXT turn (its next tile in this phase, or its first tile in the next phase)
// depends on nothing this turn produces, so -- the tile-pair kernel's pipeline (node_bwd_persistent2_kernel<true>), for K tiles:
//   T0  s_waitcnt vmcnt(0) + barrier: this turn's halo rows (gathered during the previous turn's parameter-gradient products) have
//       landed, the previous turn's row stores are drained -> ITS flag goes out here (deferred publish)
//   T1  LDS aggregation, K-bar, operand tiles; the next turn's tape row and sign bits are asked for; barrier; G = dZ W^T
//   T2  wave 0 asks for the flags of the next turn's wait list, not waited for; dW += A^T dZ, db (the longest stretch of the turn)
//   T3  one look at the flags; if they were all there, the next turn's rows go out by LDS-DMA behind this turn's read of G (the halo
//       region is the product's result tile); row stores (not drained)
// A next turn whose flags were not there (the first tile of the next phase, mostly: its neighbours are in THIS phase) takes the
// blocking path at its T0, which publishes what is pending first -- so a workgroup never spins in front of its own publish.
// Arithmetic per tile is node_bwd_persistent_kernel's, operation for operation: du0 bitwise equal to the replayed plan's.
template <int ACT>
__global__ __launch_bounds__(kThreads, 4) void node_bwd_persistentKP_kernel(const PBwdK p) {
  constexpr bool RELU = (ACT == NGPDE_ACT_RELU);
  using Aux = typename std::conditional<RELU, unsigned, float4>::type;
  constexpr int kMS = meta_stride<false>(), kMT = meta_tiles<false>();
  __shared__ __attribute__((aligned(16))) float lds[kXhF + 2 * kTileF + kWF + kMT * kMS + 48 + 4];
  static_assert(sizeof(lds) <= 80 * 1024 - 64, "two workgroups per CU");
  float *ldsXh = lds, *ldsG = lds, *ldsDZ = lds + kXhF, *ldsX = ldsDZ + kTileF, *ldsW = ldsX + kTileF;
  float *ldsMeta = ldsW + kWF, *ldsC = ldsMeta + kMT * kMS;
  int *s_ok = reinterpret_cast<int *>(ldsC + 48), *s_pre = s_ok + 1;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave_u = __builtin_amdgcn_readfirstlane(tid >> 6);
  coef_to_lds(ldsC, p.cb, 48, tid);
  zero_halo_row(ldsXh, tid < PG::LPR, tid & 15);
  if (tid == 0) *s_ok = 1, *s_pre = 0;
  f32x4 dw1[PG::DWT], dw2[PG::DWT];
#pragma unroll
  for (int mm = 0; mm < PG::DWT; ++mm) dw1[mm] = dw2[mm] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float db1 = 0.f, db2 = 0.f;
  const int dbc = tid / PG::DBP, dbpart = tid % PG::DBP;
  const int S = p.S, W = p.pair_wgs, K = min(p.k_tiles, kMT);
  const int t0 = xcd_tile(blockIdx.x, W);
  const unsigned rowb = (unsigned)(p.row_elems * sizeof(float));
  tile_round_tables<false>(p.m, t0, W, K, ldsMeta);
  const int Kv = tile_round_count(p.m, t0, W, K);   // tiles this workgroup really holds
  __syncthreads();

  bool pre = false, ok = true;
  unsigned *pend_flags = nullptr;
  int pend_ph = 0, n_ahead = 0;
  Aux mk_n{};
  float4 xrow_n = f4_zero();
  struct Next {          // the turn after this one
    bool gather;         // it gathers halo rows from X once the flags of its wait list show ph - 1
    int ph, s;
    const float *X;
    bool tape;           // it runs a dense half: tape row and sign bits of event ev
    size_t ev;
  };
  auto fetch = [&](size_t ev, int s) {
    const int node = max(reinterpret_cast<const int4 *>(ldsMeta + s * kMS + kMetaF)[tid >> 4].x, 0);
    const unsigned own = row_offset(node, tid & 15);
    if constexpr (RELU) mk_n = ldu8_g(p.masks + ev * p.mask_bytes + (size_t)(t0 + s * W) * kThreads, (unsigned)tid);
    else mk_n = ld4_stream_g(p.ztape + ev * p.row_elems, own);
    xrow_n = ld4_stream_g(p.tape + ev * p.row_elems, own);
  };
  auto t0_publish = [&]() {
    wait_vmcnt0();
    __syncthreads();
    if (pend_flags && tid == 0) __hip_atomic_store(pend_flags, (unsigned)pend_ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    pend_flags = nullptr;
  };
  // T0, then (unless the rows were gathered ahead) blocking wait + gather
  auto top = [&](const TileCtx &c, int ph, const float *X) -> bool {
    t0_publish();
    n_ahead += pre ? 1 : 0;
    if (!pre) {
      if (!tile_wait(p.m, c, ph, s_ok)) return false;
      halo_fill_all(c, X, ldsXh);
      wait_vmcnt0();
      __syncthreads();
    }
    return true;
  };
  auto dense = [&](const TileCtx &c, unsigned own, int ph, f32x4 (&dwl)[PG::DWT], float &dbl, float4 kbar, Aux mk, float4 xrow, float *gout,
                   const Next &nx) {
    const float4 dz = adjoint_dz<RELU>(c, p.act, kbar, mk);
    tile_row_store(ldsDZ, c, dz);
    adjoint_x_store(ldsX, c, xrow);
    if (nx.tape) fetch(nx.ev, nx.s);
    __syncthreads();
    mfma_rows_times_bt<PD>(ldsDZ, ldsW, ldsG, wave_u, lane);
    TileCtx cn;
    unsigned f1 = 0;
    if (nx.gather) {   // uniform
      tile_ctx_from_lds<false>(cn, t0 + nx.s * W, ldsMeta + nx.s * kMS);
      if (wave_u == 0) f1 = poll_issue(p.m, cn, p.m.flags);
    }
    param_grad_products_beside_dma(ldsX, ldsDZ, wave_u, lane, dbc, dbpart, dwl, dbl);
    if (nx.gather) {
      if (wave_u == 0) {
        const bool hit = poll_ready(cn, f1, nx.ph);
        if (lane == 0) *s_pre = hit ? 1 : 0;
      }
      __syncthreads();
      pre = *s_pre != 0;
    } else {
      __syncthreads();
      pre = false;
    }
    const float4 gv = adjoint_g_row(ldsG, c);
    if (pre) {   // uniform
      __syncthreads();   // every thread has read its row of G: the region is the halo again
      halo_fill_all(cn, nx.X, ldsXh);
    }
    if (c.valid) store_sc1(gout, own, gv);
    pend_flags = flag_line(p.m.flags, c.tile);
    pend_ph = ph;
  };

  const bool multi = Kv > 1;   // (one tile: the next turn is this tile's own next phase, whose rows are stored in THIS turn)
  int ph = 0;
  {   // first phase: K-bar of the last stage of the last step = dt b_S lambda, layer 2's dense half (no gather, no wait)
    ++ph;
    const size_t ev = (size_t)((p.n_steps - 1) * S + (S - 1)) * 2 + 1;
    load_weight_lds(p.w2, ldsW, tid, false);
    if (Kv > 0) fetch(ev, 0);
    for (int s = 0; s < Kv; ++s) {
      TileCtx c;
      tile_ctx_from_lds<false>(c, t0 + s * W, ldsMeta + s * kMS);
      const unsigned own = own_row_offset(c);
      t0_publish();   // (the phase's W is in LDS; the previous turn's products are done with the operand tiles)
      const float4 lam = f4_sel(c.valid, ld4_g(p.lam, own), f4_zero());
      const Aux mk = mk_n;
      const float4 xrow = xrow_n;
      const bool more = s + 1 < Kv;   // next: the workgroup's next tile, or layer 1 of the last stage of the last step on its first one
      Next nx;
      nx.gather = !more && multi; nx.ph = ph + 1; nx.s = more ? s + 1 : 0; nx.X = p.g2; nx.tape = true;
      nx.ev = more ? ev : (size_t)((p.n_steps - 1) * S + (S - 1)) * 2;
      dense(c, own, ph, dw2, db2, adjoint_kbar_last(ldsC, S, lam), mk, xrow, p.g2, nx);
    }
  }
  for (int n = p.n_steps - 1; n >= 0 && ok; --n) {
    for (int i = S - 1; i >= 0 && ok; --i) {
      const bool last = (i == 0 && n == 0);
      const size_t ev_b = (i >= 1) ? (size_t)(n * S + i - 1) * 2 + 1 : (size_t)((max(n, 1) - 1) * S + (S - 1)) * 2 + 1;   // layer-2 event behind this stage's layer 1
      {   // layer 1 of stage i: dL/dy1 = A^T g2
        ++ph;
        const size_t ev = (size_t)(n * S + i) * 2;
        __syncthreads();
        load_weight_lds(p.w1, ldsW, tid, false);
        for (int s = 0; s < Kv; ++s) {
          TileCtx c;
          tile_ctx_from_lds<false>(c, t0 + s * W, ldsMeta + s * kMS);
          const unsigned own = own_row_offset(c);
          const Aux mk = mk_n;
          const float4 xrow = xrow_n;
          if (!top(c, ph, p.g2)) { ok = false; break; }
          const float4 t = tile_aggregate_lean(c, ldsXh);
          const bool more = s + 1 < Kv;
          Next nx;
          nx.gather = multi; nx.ph = more ? ph : ph + 1; nx.s = more ? s + 1 : 0; nx.X = more ? p.g2 : p.g1;
          nx.tape = more || !last; nx.ev = more ? ev : ev_b;
          dense(c, own, ph, dw1, db1, t, mk, xrow, p.g1, nx);
        }
        if (!ok) break;
      }
      {   // U-bar_i = A^T g1; K-bar of the stage evaluated before it (or the lambda update), layer 2's dense half
        ++ph;
        const size_t ev = ev_b;
        __syncthreads();
        load_weight_lds(p.w2, ldsW, tid, false);
        for (int s = 0; s < Kv; ++s) {
          TileCtx c;
          tile_ctx_from_lds<false>(c, t0 + s * W, ldsMeta + s * kMS);
          const unsigned own = own_row_offset(c);
          const Aux mk = mk_n;        // (the last phase runs no dense half: nothing was asked for)
          const float4 xrow = xrow_n;
          if (!top(c, ph, p.g1)) { ok = false; break; }
          // lambda and the stage adjoints of this step from memory (rows 0..4 of ubar = U-bar_1..5): in flight under the aggregation
          const float4 lam = f4_sel(c.valid, ld4_g(p.lam, own), f4_zero());
          // (only the stage adjoints this stage combines, U-bar_j with i < j < S: the others meet a zero coefficient or are zero)
          const float4 lb1 = (i < 1 && S > 1) ? ld4_g(p.ubar, own) : f4_zero(), lb2 = (i < 2 && S > 2) ? ld4_g(p.ubar, own + rowb) : f4_zero(),
                       lb3 = (i < 3 && S > 3) ? ld4_g(p.ubar, own + 2 * rowb) : f4_zero(), lb4 = (i < 4 && S > 4) ? ld4_g(p.ubar, own + 3 * rowb) : f4_zero(),
                       lb5 = (i < 5 && S > 5) ? ld4_g(p.ubar, own + 4 * rowb) : f4_zero();
          const float4 t = tile_aggregate_lean(c, ldsXh);
          const float4 ub1 = i == 1 ? t : lb1, ub2 = i == 2 ? t : lb2, ub3 = i == 3 ? t : lb3, ub4 = i == 4 ? t : lb4,
                       ub5 = i == 5 ? t : lb5;   // U-bar_i is t itself
          float4 kbar;
          if (i >= 1) {
            if (c.valid) st4_g(p.ubar, own + (unsigned)(i - 1) * rowb, t);
            kbar = adjoint_kbar_stage(ldsC, i, t, lam, ub2, ub3, ub4, ub5);
          } else {
            const float4 v = adjoint_lambda_update(t, lam, ub1, ub2, ub3, ub4, ub5);
            if (c.valid) st4_g(p.lam, own, v);
            kbar = adjoint_kbar_last(ldsC, S, v);
          }
          if (!last) {   // next: the workgroup's next tile, or layer 1 of stage i - 1 / of the last stage of the step before
            const bool more = s + 1 < Kv;
            const size_t ev_a = (size_t)(i >= 1 ? n * S + i - 1 : (max(n, 1) - 1) * S + (S - 1)) * 2;
            Next nx;
            nx.gather = multi; nx.ph = more ? ph : ph + 1; nx.s = more ? s + 1 : 0; nx.X = more ? p.g1 : p.g2;
            nx.tape = true; nx.ev = more ? ev : ev_a;
            dense(c, own, ph, dw2, db2, kbar, mk, xrow, p.g2, nx);
          } else {
            pre = false;     // (the final phase: every turn takes the blocking path; nothing is published)
            __syncthreads();
          }
        }
        if (!ok) break;
      }
    }
  }
  if (!ok) {
    __syncthreads();
    poison_tile_rounds(p.m, p.lam, t0, W, Kv, tid);
  }
  // (as a captured lambda the call leaves this kernel's register allocation, and with it its scratch size, as it was)
  auto slab = [&](const f32x4 (&dwl)[PG::DWT], float dbl, float *slab_dw, float *slab_db) { write_slab(dwl, dbl, slab_dw, slab_db, wave_u, lane, dbc, dbpart, ok); };
  slab(dw1, db1, p.slab_dw1, p.slab_db1);
  slab(dw2, db2, p.slab_dw2, p.slab_db2);
  if (tid == 0 && p.m.stats && Kv > 0) p.m.stats[2 * t0 + 1] = n_ahead;
}

}  // namespace

// ---- host side (wait lists, setup, launch bracket: persistent_plan.hip) ------------------------------------------------------

// The kernel table: every instantiation a plan can launch, by family.  The residency queries below and the two launchers read the
// same entries, so the grid a query admits is measured on the kernels the launch will pick from.
namespace {
enum class Family { OneTile, OneTileW, Hub, Pair, Interleaved, Rounds, RoundsW };   // Rounds: pipelined (KP); RoundsW: plain (K), weighted graphs
using FwdKernel = void (*)(const PFwdK);
using BwdKernel = void (*)(const PBwdK);

template <int ACT, bool TAPE>
FwdKernel fwd_kernel_of(Family f) {
  constexpr bool kSlots2 = !(TAPE && ACT != NGPDE_ACT_RELU);   // the two-slot kernels keep no pre-activation tape
  switch (f) {
    case Family::OneTile: return node_fwd_persistent_kernel<ACT, TAPE>;
    case Family::OneTileW: return node_fwd_persistent_kernel<ACT, TAPE, true>;
    case Family::Hub: return node_fwd_persistent_kernel<ACT, TAPE, false, true>;
    case Family::Pair: if constexpr (kSlots2) return node_fwd_persistent2_kernel<ACT, TAPE, true>; else return nullptr;
    case Family::Interleaved: if constexpr (kSlots2) return node_fwd_persistent2_kernel<ACT, TAPE, false>; else return nullptr;
    case Family::Rounds: return node_fwd_persistentKP_kernel<ACT, TAPE>;
    case Family::RoundsW: return node_fwd_persistentK_kernel<ACT, TAPE>;
  }
  return nullptr;
}
template <int ACT>
BwdKernel bwd_kernel_of(Family f) {
  switch (f) {
    case Family::OneTile: return node_bwd_persistent_kernel<ACT>;
    case Family::OneTileW: return node_bwd_persistent_kernel<ACT, true>;
    case Family::Hub: return node_bwd_persistent_kernel<ACT, false, true>;
    case Family::Pair: return ACT == NGPDE_ACT_RELU ? node_bwd_persistent2_kernel<true> : nullptr;
    case Family::Interleaved: return node_bwd_persistent2_kernel<false>;   // (one kernel, the activation a launch argument)
    case Family::Rounds: return node_bwd_persistentKP_kernel<ACT>;
    case Family::RoundsW: return node_bwd_persistentK_kernel<ACT>;
  }
  return nullptr;
}
// null: the family has no such kernel
FwdKernel fwd_kernel(Family f, bool relu, bool tape) {
  if (relu) return tape ? fwd_kernel_of<NGPDE_ACT_RELU, true>(f) : fwd_kernel_of<NGPDE_ACT_RELU, false>(f);
  return tape ? fwd_kernel_of<-1, true>(f) : fwd_kernel_of<-1, false>(f);
}
BwdKernel bwd_kernel(Family f, bool relu) { return relu ? bwd_kernel_of<NGPDE_ACT_RELU>(f) : bwd_kernel_of<-1>(f); }

// co-residency of the spin-waiting workgroups: over EVERY kernel of the families a plan of this kind can launch
int resident_tiles(std::initializer_list<Family> families) {
  std::vector<const void *> kernels;
  const auto add = [&](auto kernel) {
    const void *k = reinterpret_cast<const void *>(kernel);
    if (k && std::find(kernels.begin(), kernels.end(), k) == kernels.end()) kernels.push_back(k);
  };
  for (Family f : families)
    for (int relu = 0; relu < 2; ++relu) {
      add(fwd_kernel(f, relu, true));
      add(fwd_kernel(f, relu, false));
      add(bwd_kernel(f, relu));
    }
  return resident_workgroups(kernels, kThreads, 0);
}
}  // namespace

// Can the plan run as two persistent launches?  (same conditions as the pre-scaled replayed plan, plus: d = 64, unweighted, ALL
// workgroups co-resident.)  0: no.  1: one tile per workgroup (graphs of at most CUs x occupancy tiles).  2: two tiles per
// workgroup through the two-slot kernels (up to twice as many tiles; relu when a backward is asked for).
int node_persistent_mode(const ngpde_graph *g, int d, int act, bool with_bwd) {
  if (switch_on(Switch::NoPersistent)) return 0;
  if (!g || d != PD || !fused_prescaled_supported(g, d)) return 0;
  const bool weighted = g->by_t.slot_w || g->by_s.slot_w;
  if (weighted && !(g->by_t.slot_w && g->by_s.slot_w)) return 0;
  const int nt = g->n_sched / kTileRows, resident = resident_tiles({Family::OneTile, Family::Interleaved, Family::Pair});
  if (nt < 1) return 0;
  if (weighted) {
    // edge weights: one tile per workgroup on the WGT one-tile kernels (slot weights in the LDS of one W; W1 as register fragments)
    // where the graph is one wave of workgroups, else the tile-round kernels (they keep one W in LDS anyway)
    if (nt <= resident_tiles({Family::OneTileW}) && !switch_on(Switch::WeightedTileRounds)) return 1;
    return nt <= kMaxTileRoundsW * resident ? 3 : 0;
  }
  if (nt <= resident) return 1;
  if (switch_on(Switch::NoTilePairs)) return 0;
  if (nt <= 2 * resident && (!with_bwd || act == NGPDE_ACT_RELU) && !switch_on(Switch::TileRounds)) return 2;
  if (nt <= kMaxTileRounds * resident) return 3;   // K tiles per workgroup taking turns (node_*_persistentK_kernel)
  return 0;
}
int node_persistent_rounds(const ngpde_graph *g) {   // K of mode 3: tiles per workgroup
  // (weighted graphs: the K kernels as well)
  const int resident = g->by_t.slot_w ? resident_tiles({Family::Rounds, Family::RoundsW}) : resident_tiles({Family::Rounds});
  const int nt = g->n_sched / kTileRows;
  if (resident < 1) return 0;
  const int k = (nt + resident - 1) / resident;
  // (the K kernels' occupancy can be lower than what node_persistent_mode assumed from the one-tile kernels: a k beyond what the
  // kernels' LDS tables hold would leave tiles unprocessed -- their neighbours would spin into the timeout -- so it is refused here
  // and node_create keeps the replayed plan)
  if (k > (g->by_t.slot_w ? kMaxTileRoundsW : kMaxTileRounds)) return 0;
  return k;
}

bool node_persistent_hub_possible(const ngpde_graph *g, int d) {
  if (switch_on(Switch::NoHalo) || switch_on(Switch::NoPersistent)) return false;   // (NO_HALO asks for the per-row global gather everywhere)
  if (!g || d != PD || !g->has_norm || !g->self_loops || ((g->by_t.slot_w || g->by_s.slot_w) && !g->w_coo)) return false;
  if (g->by_t.halo_ok && g->by_s.halo_ok) return false;   // the 96-row geometry takes it
  const int nt = g->n_sched / kTileRows;
  return nt >= 1 && nt <= resident_tiles({Family::Hub});
}

// ---- a plan's own-first slot tables (OwnFirst, common.h) ----------------------------------------------------------------------------
namespace {
// one 64-thread workgroup per tile, thread r < 32 = row r: the row's slot bytes with the own-tile slots (< 32) first, padded with the
// all-zero row (kHaloCap) to 4 x the own rounds of the row's group of four (= a wave of the 64-wide kernels), then the foreign slots;
// weights travel with their slots; a group in which some row would not fit its 32 bytes keeps the handle's order (pre = 0)
__global__ __launch_bounds__(64) void own_first_tables_kernel(int n_tiles, const uint8_t *__restrict__ slots, const int4 *__restrict__ sched,
                                                              const float *__restrict__ slot_w, uint8_t *__restrict__ o_slots,
                                                              int4 *__restrict__ o_sched, float *__restrict__ o_w, uint8_t *__restrict__ o_pre) {
  const int tile = blockIdx.x, r = threadIdx.x;
  const bool row = r < kTileRows;
  const size_t pos = (size_t)tile * kTileRows + (row ? r : 0);
  int4 sc = sched[pos];
  const int deg = (row && sc.x >= 0) ? min(sc.z, kSlotWidth) : 0;
  uint8_t b[kSlotWidth];
  {
    const uint4 lo = reinterpret_cast<const uint4 *>(slots + pos * kSlotWidth)[0], hi = reinterpret_cast<const uint4 *>(slots + pos * kSlotWidth)[1];
    const unsigned w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int j = 0; j < kSlotWidth; ++j) b[j] = (uint8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xff);
  }
  int no = 0, nf = 0;
#pragma unroll
  for (int j = 0; j < kSlotWidth; ++j) {
    if (j < deg) {
      if (b[j] < kTileRows) ++no;
      else ++nf;
    }
  }
  int pre = (no + 3) >> 2;
  pre = max(pre, __shfl_xor(pre, 1));
  pre = max(pre, __shfl_xor(pre, 2));
  int fits = (4 * pre + nf <= kSlotWidth) ? 1 : 0;
  fits = min(fits, __shfl_xor(fits, 1));
  fits = min(fits, __shfl_xor(fits, 2));
  if (!fits) pre = 0;
  if (row) {
    uint8_t *ob = o_slots + pos * kSlotWidth;
    float *ow = o_w ? o_w + pos * kSlotWidth : nullptr;
    const float *iw = slot_w ? slot_w + pos * kSlotWidth : nullptr;
    if (fits) {
      int k = 0;
      for (int j = 0; j < deg; ++j)
        if (b[j] < kTileRows) { ob[k] = b[j]; if (ow) ow[k] = iw[j]; ++k; }
      for (; k < 4 * pre; ++k) { ob[k] = (uint8_t)kHaloCap; if (ow) ow[k] = 0.f; }
      for (int j = 0; j < deg; ++j)
        if (b[j] >= kTileRows) { ob[k] = b[j]; if (ow) ow[k] = iw[j]; ++k; }
      const int len = k;
      for (; k < kSlotWidth; ++k) { ob[k] = (uint8_t)kHaloCap; if (ow) ow[k] = 0.f; }
      if (sc.x >= 0) sc.z = len;
    } else {
      for (int j = 0; j < kSlotWidth; ++j) { ob[j] = b[j]; if (ow) ow[j] = iw[j]; }
    }
    o_sched[pos] = sc;
    if ((r & 3) == 0) o_pre[(size_t)tile * 8 + (r >> 2)] = (uint8_t)pre;
  }
}
}  // namespace

int32_t own_first_tables_build(const ngpde_graph *g, OwnFirst *of, hipStream_t stream) {
  const int nt = g->n_sched / kTileRows;
  // the by-target lists only: the adjoint's tiles reach their wait with the flags already set (its parameter-gradient products sit
  // between publish and wait), so there the padding rounds cost more than the early sums win (measured with by-source tables too:
  // 2.913 -> 2.925 ms, profiles/r06_l_own_first.txt)
  const Csr &c = g->by_t;
  if (c.halo_ok && c.slots && c.sched) {
    NGPDE_HIP_CHECK(hipMalloc((void **)&of->slots, (size_t)g->n_sched * kSlotWidth));
    NGPDE_HIP_CHECK(hipMalloc((void **)&of->sched, (size_t)g->n_sched * sizeof(int4)));
    NGPDE_HIP_CHECK(hipMalloc((void **)&of->pre, (size_t)nt * 8));
    if (c.slot_w) NGPDE_HIP_CHECK(hipMalloc((void **)&of->slot_w, (size_t)g->n_sched * kSlotWidth * sizeof(float)));
    hipLaunchKernelGGL(own_first_tables_kernel, dim3(nt), dim3(64), 0, stream, nt, c.slots, c.sched, c.slot_w, of->slots, of->sched,
                       of->slot_w, of->pre);
    NGPDE_LAUNCH_CHECK("own_first_tables_kernel");
  }
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  return NGPDE_OK;
}

void own_first_tables_free(OwnFirst *of) {
  if (of->slots) (void)hipFree(of->slots);
  if (of->sched) (void)hipFree(of->sched);
  if (of->slot_w) (void)hipFree(of->slot_w);
  if (of->pre) (void)hipFree(of->pre);
  *of = OwnFirst();
}

namespace {
// of: the plan's own-first tables (forward only, dir 0), or NULL
TileMeta make_meta(const Csr &c, const NodePersist &ps, int dir, const OwnFirst *of = nullptr) {
  TileMeta m;
  m.halo = c.halo; m.slots = c.slots; m.sched = c.sched; m.tile_info = c.tile_info; m.nbr = ps.nbr; m.slot_w = c.slot_w;
  m.of_pre = nullptr;
  if (of && of->slots && !ps.hub) {   // the plan's own-first tables: the same rows in another order, padded lengths in the schedule
    m.slots = of->slots; m.sched = of->sched; m.of_pre = of->pre;
    if (m.slot_w) m.slot_w = of->slot_w;
  }
  const NodePersist::HubLists &L = ps.hub_lists[dir];
  m.hub_halo = L.halo; m.hub_slots = L.slots; m.hub_rows = L.rows; m.hub_info = L.info; m.hub_long = L.longs; m.hub_sched = L.sched;
  m.hub_w = L.w;
  if (ps.hub) m.slot_w = nullptr;   // (the hub geometry reads its own weight lists)
  m.flags = ps.sync; m.abort_word = sync_abort_word(ps.sync, ps.n_tiles); m.n_tiles = ps.n_tiles;
  m.stats = ps.stats;
  NGPDE_STAMP_SET(m, kStampPersistent, 0);
  return m;
}
// the family a launch belongs to (m: its make_meta, whose slot_w says "weighted" for every geometry but the hub's)
Family family_of(int k_tiles, const TileMeta &m, bool hub, bool pair, bool interleave) {
  if (k_tiles > 0) return m.slot_w ? Family::RoundsW : Family::Rounds;
  if (hub) return Family::Hub;
  if (m.slot_w) return Family::OneTileW;
  return pair ? Family::Pair : interleave ? Family::Interleaved : Family::OneTile;
}
}  // namespace

int32_t launch_node_fwd_persistent(const NodePersistFwd &a, hipStream_t stream) {
  const ngpde_graph *g = a.g;
  const NodePersist &ps = *a.ps;
  int32_t st;
  PersistentTurn turn;
  if ((st = turn.enter(ps, stream))) return st;
  PFwdK k;
  k.m = make_meta(g->by_t, ps, 0, a.of);
  k.n_steps = a.n_steps; k.S = a.S; k.act = a.act; k.n_members = a.n_members;
  k.u_in = a.u_in; k.u_out = a.u_out; k.bufA = a.bufA; k.bufB = a.bufB;
  k.w1 = a.w1; k.b1 = a.b1; k.w2 = a.w2; k.b2 = a.b2;
  k.tape = a.tape; k.masks = a.masks; k.row_elems = a.row_elems; k.mask_bytes = a.mask_bytes;
  k.flag_stride = sync_slot_stride(ps.n_tiles);
  k.pair_wgs = a.pair ? ps.pair_wgs : 0;
  k.cf = ps.coef;
  NGPDE_REQUIRE(!a.pair || (ps.pair_wgs > 0 && !a.interleave && a.n_members == 1), NGPDE_ERR_STATE, "tile-pair launch without its setup");
  k.k_tiles = a.k_tiles; k.state = a.state; k.ztape = a.ztape;
  const Family family = family_of(a.k_tiles, k.m, ps.hub, a.pair, a.interleave);
  const bool relu = a.act == NGPDE_ACT_RELU;
  dim3 grid(a.pair ? ps.pair_wgs : ps.n_tiles);
  const char *name = "node_fwd_persistent_kernel";
  if (a.k_tiles > 0) {   // tile rounds: K tiles per workgroup, state in memory
    // unweighted: the pipelined kernel; weighted: the plain tile-round kernel (the slot weights leave no LDS for the pipeline)
    NGPDE_REQUIRE(ps.pair_wgs > 0 && a.n_members == 1 && a.state, NGPDE_ERR_STATE, "tile-round launch without its setup");
    NGPDE_REQUIRE(a.k_tiles <= kMaxTileRounds, NGPDE_ERR_STATE, "tile rounds: at most %d tiles per workgroup", kMaxTileRounds);
    k.pair_wgs = ps.pair_wgs;
    if ((st = launch_zero(a.state + a.row_elems, 6 * a.row_elems * sizeof(float), stream))) return st;   // k_0 .. k_5 start from zero
    grid = dim3(ps.pair_wgs);
    NGPDE_REQUIRE(!k.m.slot_w || a.k_tiles <= kMaxTileRoundsW, NGPDE_ERR_STATE, "weighted tile rounds: at most %d tiles per workgroup", kMaxTileRoundsW);
    name = "node_fwd_persistentK_kernel";
  } else {
    NGPDE_REQUIRE(!k.m.slot_w || (!a.pair && !a.interleave && a.n_members == 1), NGPDE_ERR_STATE,
                  "weighted graphs: one tile per workgroup or tile rounds, one member");
    if (family == Family::Hub) {   // hub geometry: one tile per workgroup and CU
      NGPDE_REQUIRE(!a.pair && !a.interleave, NGPDE_ERR_STATE, "hub geometry: one tile per workgroup, the members of a batch one after the other");
      NGPDE_REQUIRE(!a.tape || (relu ? a.masks != nullptr : a.ztape != nullptr), NGPDE_ERR_INVALID_ARGUMENT,
                    "persistent forward with a tape needs the sign-bit masks (relu) or the pre-activation tape");
      name = "node_fwd_persistent_kernel (hub geometry)";
    } else if (a.tape && relu) {
      NGPDE_REQUIRE(a.masks != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "persistent forward with a relu tape needs the sign-bit masks");
    } else if (a.tape) {
      NGPDE_REQUIRE(a.ztape != nullptr && !a.interleave && !a.pair, NGPDE_ERR_INVALID_ARGUMENT,
                    "persistent forward with a tape: activations other than relu keep the pre-activations (one member at a time)");
    }
  }
  const FwdKernel kernel = fwd_kernel(family, relu, a.tape != nullptr);
  NGPDE_REQUIRE(kernel, NGPDE_ERR_STATE, "persistent forward: no kernel of this form");
  launch_timed(kernel, grid, dim3(kThreads), 0, stream, a.ev_start, a.ev_stop, k);
  NGPDE_LAUNCH_CHECK(name);
  if (!a.no_latch && (st = turn.latch())) return st;
  return turn.leave();
}

int32_t launch_node_bwd_persistent(const NodePersistBwd &a, hipStream_t stream) {
  const ngpde_graph *g = a.g;
  const NodePersist &ps = *a.ps;
  int32_t st;
  PersistentTurn turn;
  if ((st = turn.enter(ps, stream))) return st;
  PBwdK k;
  k.m = make_meta(g->by_s, ps, 1);
  k.n_steps = a.n_steps; k.S = a.S; k.n_members = a.n_members; k.act = a.act; k.ztape = a.ztape;
  k.lam = a.lam; k.g1 = a.g1; k.g2 = a.g2; k.w1 = a.w1; k.w2 = a.w2;
  k.tape = a.tape; k.masks = a.masks; k.row_elems = a.row_elems; k.mask_bytes = a.mask_bytes;
  k.slab_dw1 = a.slab_dw1; k.slab_db1 = a.slab_db1; k.slab_dw2 = a.slab_dw2; k.slab_db2 = a.slab_db2;
  k.cb = ps.coef + 42;
  k.flag_stride = sync_slot_stride(ps.n_tiles);
  k.pair_wgs = a.pair ? ps.pair_wgs : 0;
  k.ubar = a.ubar;
  NGPDE_REQUIRE(!a.pair || (ps.pair_wgs > 0 && !a.interleave && a.n_members == 1 && a.act == NGPDE_ACT_RELU), NGPDE_ERR_STATE,
                "tile-pair launch without its setup");
  k.k_tiles = a.k_tiles;
  const Family family = family_of(a.k_tiles, k.m, ps.hub, a.pair, a.interleave);
  const bool relu = a.act == NGPDE_ACT_RELU;
  dim3 grid(a.pair ? ps.pair_wgs : ps.n_tiles);
  const char *name = "node_bwd_persistent_kernel";
  const char *const need_ztape = "persistent adjoint: activations other than relu need the saved pre-activations";
  if (a.k_tiles > 0) {   // tile rounds
    NGPDE_REQUIRE(ps.pair_wgs > 0 && a.n_members == 1 && a.ubar, NGPDE_ERR_STATE, "tile-round launch without its setup");
    NGPDE_REQUIRE(a.k_tiles <= kMaxTileRounds, NGPDE_ERR_STATE, "tile rounds: at most %d tiles per workgroup", kMaxTileRounds);
    NGPDE_REQUIRE(relu || a.ztape, NGPDE_ERR_INVALID_ARGUMENT, "%s", need_ztape);
    k.pair_wgs = ps.pair_wgs;
    if ((st = launch_zero(a.ubar, 5 * a.row_elems * sizeof(float), stream))) return st;   // the stage adjoints start from zero
    grid = dim3(ps.pair_wgs);
    NGPDE_REQUIRE(!k.m.slot_w || a.k_tiles <= kMaxTileRoundsW, NGPDE_ERR_STATE, "weighted tile rounds: at most %d tiles per workgroup", kMaxTileRoundsW);
    name = "node_bwd_persistentK_kernel";
  } else {
    NGPDE_REQUIRE(!k.m.slot_w || (!a.pair && !a.interleave && a.n_members == 1), NGPDE_ERR_STATE,
                  "weighted graphs: one tile per workgroup or tile rounds, one member");
    if (family == Family::Hub)
      NGPDE_REQUIRE(!a.pair && !a.interleave, NGPDE_ERR_STATE, "hub geometry: one tile per workgroup, the members of a batch one after the other");
    if (family == Family::Pair) NGPDE_REQUIRE(a.ubar != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "tile-pair persistent adjoint without its stage-adjoint scratch");
    else if (family == Family::Interleaved)
      NGPDE_REQUIRE(a.ubar != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "interleaved persistent adjoint without its stage-adjoint scratch");
    else NGPDE_REQUIRE(relu || a.ztape, NGPDE_ERR_INVALID_ARGUMENT, "%s", need_ztape);
  }
  const BwdKernel kernel = bwd_kernel(family, relu);
  NGPDE_REQUIRE(kernel, NGPDE_ERR_STATE, "persistent adjoint: no kernel of this form");
  launch_timed(kernel, grid, dim3(kThreads), 0, stream, a.ev_start, a.ev_stop, k);
  NGPDE_LAUNCH_CHECK(name);
  if (!a.no_latch && (st = turn.latch())) return st;
  return turn.leave();
}

}  // namespace ngpde
