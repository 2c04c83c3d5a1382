// persistent_gcn_tile.h -- device pieces of the persistent GCN solver (node_persistent.hip): the tile context and its tables, the flag
// waits and the publish, the halo gathers, the neighbour sums of the three geometries (96-row halo, weighted rows, hub), and -- written
// once for the eight kernels -- arithmetic of a phase: the forward's pre-activation, output row and Runge-Kutta stage combination, the
// adjoint's operand rows, parameter-gradient products and stage-adjoint combination.  The kernels themselves, their LDS layouts and their
// schedules are in node_persistent.hip.
#pragma once

#include "common.h"
#include "device_utils.h"
#include "gcn_tile.h"
#include "persistent_mem.h"
#include "persistent_sync.h"
#include "stamps.h"

namespace ngpde {

namespace {

constexpr int PD = 64;
using PG = Geo<PD>;
static_assert(PG::R == 1 && PG::GROUPS == kTM && PG::LPR == 16, "one 16-lane group per tile row");
constexpr int kXhF = (kHaloCap + 1) * PD;   // halo region (floats), +1: the all-zero row
constexpr int kTileF = kTM * PG::TS;        // one 32-row MFMA operand / result tile
constexpr int kWF = PD * PG::TS;            // one transposed weight matrix
constexpr int kMaxTileRounds = 8;            // tile rounds: at most this many tiles per workgroup

struct TileCtx {
  int tid, lane, wave_u, grp, q, tile, node, hcount, wmax, my_nbr;
  bool valid;
  float ci;
  // kept in LDS, not in registers (the 16 lanes of a group would each hold the same 8 words): the 32 slot bytes of every row
  // [32][8] and the node ids of the 64 foreign halo slots
  const unsigned *lds_slots;
  const int *lds_hnode;
  const float *lds_w;   // weighted graphs (tile rounds only): the tile's slot weights [32][32], else unused
};
constexpr int kMetaF = kTM * 8 + 2 * kTM;   // floats of LDS the two tables take

struct TileMeta {
  const int2 *halo;
  const uint8_t *slots;
  const int4 *sched;
  const int2 *tile_info;
  const int *nbr;
  const float *slot_w;   // [n_sched][kSlotWidth] edge weights in slot order, or NULL (unweighted)
  unsigned *flags, *abort_word;
  int n_tiles;
  const uint8_t *of_pre;   // [n_tiles][8] own rounds per wave when slots / sched are a plan's own-first tables, else NULL
  int *stats;   // [n_tiles][2] (forward, adjoint): slot-phases of the last launch whose halo rows were gathered ahead of time
  // hub geometry (HUB kernels only; then `nbr` is [n_tiles][kHubNbr])
  const int *hub_halo;        // [n_tiles][kHubHalo] node ids, own rows first
  const uint8_t *hub_slots;   // [n_tiles][kHubList]
  const int2 *hub_rows;       // [n_sched] {start, length} of the row's list inside its tile's slot bytes
  const int4 *hub_info;       // [n_tiles] {halo count, list bytes, long rows, 0}
  const int4 *hub_sched;      // [n_sched] {node or -1, 0, 0, bits of c[node]}: the hub geometry's OWN tile partition (see hub_partition)
  const uint8_t *hub_long;    // [n_tiles][kTileRows] rows (0 .. 31) with more than kSlotWidth entries
  const float *hub_w;         // [n_tiles][kHubList] edge weights of the entries, or NULL (unweighted)
  NGPDE_STAMP_FIELD
};

__device__ __forceinline__ void tile_ctx_init(const TileMeta &m, TileCtx &c, float *lds_meta, int tile = -1) {
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  c.wave_u = __builtin_amdgcn_readfirstlane(c.tid >> 6);
  c.grp = c.tid >> 4;
  c.q = c.tid & 15;
  c.tile = tile >= 0 ? tile : xcd_tile(blockIdx.x, m.n_tiles);
  const size_t pos = (size_t)c.tile * kTM + c.grp;
  const int4 sc = m.sched[pos];
  c.valid = sc.x >= 0;
  c.node = max(sc.x, 0);
  c.ci = c.valid ? __int_as_float(sc.w) : 0.f;
  unsigned *ls = reinterpret_cast<unsigned *>(lds_meta);
  int *lh = reinterpret_cast<int *>(lds_meta + kTM * 8);
  if (c.q < 8) ls[c.grp * 8 + c.q] = reinterpret_cast<const unsigned *>(m.slots)[pos * 8 + c.q];
  if (c.q >= 8 && c.q < 10) lh[c.grp + 32 * (c.q - 8)] = m.halo[(size_t)c.tile * kHaloCap + c.grp + 32 * (c.q - 7)].x;
  c.lds_slots = ls;
  c.lds_hnode = lh;
  c.hcount = __builtin_amdgcn_readfirstlane(m.tile_info[c.tile].x);
  int wm = c.valid ? sc.z : 0;
  wm = max(wm, __shfl_xor(wm, 16));
  wm = max(wm, __shfl_xor(wm, 32));
  c.wmax = __builtin_amdgcn_readfirstlane(wm);
  c.my_nbr = m.nbr[(size_t)c.tile * kNbrStride + c.lane];
}

// Tile rounds (node_*_persistentK_kernel): the tables of ALL the workgroup's tiles stay in LDS for the whole launch -- slot words,
// halo node ids, schedule entries, wait list, halo count per tile -- so that a turn sets its context up from LDS instead of
// re-reading five arrays from memory (one round trip and a barrier per turn).
constexpr int kMetaKF = kMetaF + kTM * 4 + kNbrStride + 4;   // floats per tile
// Weighted graphs (GCNConv's edge_weight, src/layers.jl:206-231) run on the tile-round kernels only: those keep ONE layer's W in LDS,
// which leaves room for the 4 KB of slot weights per tile behind the tile's tables -- for at most kMaxTileRoundsW tiles per workgroup.
constexpr int kMaxTileRoundsW = 3;
constexpr int kSlotWF = kTM * kSlotWidth;
template <bool WGT> constexpr int meta_stride() { return kMetaKF + (WGT ? kSlotWF : 0); }
template <bool WGT> constexpr int meta_tiles() { return WGT ? kMaxTileRoundsW : kMaxTileRounds; }
template <bool WGT = false>
__device__ __forceinline__ void tile_tables_to_lds(const TileMeta &m, int tile, float *base) {
  const int tid = threadIdx.x, grp = tid >> 4, q = tid & 15;
  const size_t pos = (size_t)tile * kTM + grp;
  unsigned *ls = reinterpret_cast<unsigned *>(base);
  int *lh = reinterpret_cast<int *>(base + kTM * 8);
  int4 *lsc = reinterpret_cast<int4 *>(base + kMetaF);
  int *ln = reinterpret_cast<int *>(base + kMetaF + kTM * 4);
  if (q < 8) ls[grp * 8 + q] = reinterpret_cast<const unsigned *>(m.slots)[pos * 8 + q];
  if (q >= 8 && q < 10) lh[grp + 32 * (q - 8)] = m.halo[(size_t)tile * kHaloCap + grp + 32 * (q - 7)].x;
  if (q == 10) lsc[grp] = m.sched[pos];
  if (tid < kNbrStride) ln[tid] = m.nbr[(size_t)tile * kNbrStride + tid];
  if (tid == kNbrStride) ln[kNbrStride] = m.tile_info[tile].x;
  if constexpr (WGT) {
    float2 *lw = reinterpret_cast<float2 *>(base + kMetaKF);
    lw[tid] = reinterpret_cast<const float2 *>(m.slot_w + (size_t)tile * kSlotWF)[tid];   // 512 threads x 2 floats = [32][32]
  }
}
template <bool WGT = false>
__device__ __forceinline__ void tile_ctx_from_lds(TileCtx &c, int tile, const float *base) {
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  c.wave_u = __builtin_amdgcn_readfirstlane(c.tid >> 6);
  c.grp = c.tid >> 4;
  c.q = c.tid & 15;
  c.tile = tile;
  const int4 sc = reinterpret_cast<const int4 *>(base + kMetaF)[c.grp];
  const int *ln = reinterpret_cast<const int *>(base + kMetaF + kTM * 4);
  c.valid = sc.x >= 0;
  c.node = max(sc.x, 0);
  c.ci = c.valid ? __int_as_float(sc.w) : 0.f;
  c.lds_slots = reinterpret_cast<const unsigned *>(base);
  c.lds_hnode = reinterpret_cast<const int *>(base + kTM * 8);
  c.hcount = __builtin_amdgcn_readfirstlane(ln[kNbrStride]);
  int wm = c.valid ? sc.z : 0;
  wm = max(wm, __shfl_xor(wm, 16));
  wm = max(wm, __shfl_xor(wm, 32));
  c.wmax = __builtin_amdgcn_readfirstlane(wm);
  c.my_nbr = ln[c.lane];
  c.lds_w = WGT ? base + kMetaKF : nullptr;
}

// Wait until every tile of the wait list has finished phase ph - 1: wave 0 polls (flag_poll, persistent_sync.h), one flag per lane
// (lanes 0..62) and the abort word on lane 63; everybody meets at the barrier.  Returns false when the solve was aborted.
// (tile_wait_arrive: the wait without the look at its verdict -- *s_ok, valid behind the barrier -- for callers that read it later, see
// tile_gather_foreign_checked)
__device__ __forceinline__ void tile_wait_arrive(const TileMeta &m, const TileCtx &c, int ph, int *s_ok, const unsigned *flags) {
  if (ph <= 1) return;
  if (c.wave_u == 0) {
    const unsigned *const a[1] = {watch_first(m.abort_word, flags, c.lane, c.my_nbr)};
    flag_poll<1>(a, m.abort_word, c.lane, (unsigned)(ph - 1), s_ok);
  }
  __syncthreads();
}
__device__ __forceinline__ bool tile_wait(const TileMeta &m, const TileCtx &c, int ph, int *s_ok, const unsigned *flags) {
  if (ph <= 1) return true;
  tile_wait_arrive(m, c, ph, s_ok, flags);
  return *s_ok != 0;
}
__device__ __forceinline__ bool tile_wait(const TileMeta &m, const TileCtx &c, int ph, int *s_ok) { return tile_wait(m, c, ph, s_ok, m.flags); }
// The same wait with its first round of flag loads issued earlier by the caller (poll_issue: `f` holds wave 0's samples, in flight
// under whatever the workgroup did in between).  A workgroup that is level with its neighbours finds the flags in that sample
// and only meets at the barrier; one that runs ahead spins here exactly as long as it leads.  (Used by the interleaved adjoint,
// whose slot-phase is long enough for the flags to be there.)
__device__ __forceinline__ void tile_wait_primed_arrive(const TileMeta &m, const TileCtx &c, int ph, int *s_ok, const unsigned *flags, unsigned f) {
  if (c.wave_u == 0) {
    const unsigned need = (unsigned)(ph - 1);
    const unsigned *addr = watch_first(m.abort_word, flags, c.lane, c.my_nbr);
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool ok = true;
    for (unsigned it = 1;; ++it) {
      if (__any((int)(c.lane == 63 && f != 0))) { ok = false; break; }
      if (__all((int)(c.lane == 63 || f >= need))) break;
      if ((it & 1023u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) {
        if (c.lane == 0) __hip_atomic_store(m.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = false;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      f = (c.lane == 63) ? 0u : need;
      if (addr) f = __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (c.lane == 0) *s_ok = ok ? 1 : 0;
  }
  __syncthreads();
}
__device__ __forceinline__ bool tile_wait_primed(const TileMeta &m, const TileCtx &c, int ph, int *s_ok, const unsigned *flags, unsigned f) {
  tile_wait_primed_arrive(m, c, ph, s_ok, flags, f);
  return *s_ok != 0;
}

__device__ __forceinline__ void tile_publish(const TileCtx &c, int ph, unsigned *flags) { flag_publish(flags, c.tid, (unsigned)ph, c.tile); }
__device__ __forceinline__ void tile_publish(const TileMeta &m, const TileCtx &c, int ph) { tile_publish(c, ph, m.flags); }

// the rows of OTHER tiles this tile's halo references: memory -> LDS slots 32.., sc1 (the producers stored them write-through
// in the previous phase; sc1 loads bypass this CU's L1, which may hold the same addresses from two phases ago)
__device__ __forceinline__ void tile_gather_foreign(const TileCtx &c, const float *X, float *ldsXh) {
  float4 *Xh4 = reinterpret_cast<float4 *>(ldsXh);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (4 * c.wave_u + 32 * (k + 1) < c.hcount) {   // wave-uniform: a wave's four groups stage four consecutive slots
      const unsigned off = (unsigned)c.lds_hnode[c.grp + 32 * k] * (unsigned)(PD * 4) + (unsigned)(c.q * 16);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const char *>(X) + off),
                                       (__attribute__((address_space(3))) void *)(Xh4 + (c.grp + 32 * (k + 1)) * PG::LPR + c.q), 16, 0, 16);
    }
  }
  wait_vmcnt0();
  __syncthreads();
}

// The same gather with the byte offsets of the foreign rows formed by the caller BEFORE the wait (tile_gather_offsets): read behind the
// wait, every halo index is an LDS round trip between "the flags were seen" and the DMA it addresses, paid by all waves in step.
__device__ __forceinline__ void tile_gather_offsets(const TileCtx &c, unsigned (&off)[2]) {
#pragma unroll
  for (int k = 0; k < 2; ++k) off[k] = (unsigned)c.lds_hnode[c.grp + 32 * k] * (unsigned)(PD * 4) + (unsigned)(c.q * 16);
}
// ... and with the wait's verdict (*s_ok, written in front of the wait's barrier) read under the DMAs instead of between the wait and the
// gather, where it is one more LDS round trip in everybody's way.  A gather that an aborted solve issues reads valid rows and is drained
// here before anybody leaves.  Returns false when the solve was aborted.
__device__ __forceinline__ bool tile_gather_foreign_checked(const TileCtx &c, const float *X, float *ldsXh, const unsigned (&off)[2], const int *s_ok) {
  float4 *Xh4 = reinterpret_cast<float4 *>(ldsXh);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (4 * c.wave_u + 32 * (k + 1) < c.hcount) {   // wave-uniform: a wave's four groups stage four consecutive slots
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const char *>(X) + off[k]),
                                       (__attribute__((address_space(3))) void *)(Xh4 + (c.grp + 32 * (k + 1)) * PG::LPR + c.q), 16, 0, 16);
    }
  }
  const int verdict = *s_ok;
  wait_vmcnt0();
  __syncthreads();
  return verdict != 0;
}

// sum of the row's neighbours (slot bytes, in CSR order) + its own row (self loop), all from LDS
// (plain adds on purpose: this file is built without SLP packing, and written as v_pk_add_f32 -- f4_add_pk -- these sums cost the
// headline 2 %: they run beside the CU's other workgroup's MFMAs, where packed f32 VALU is slow; profiles/r05_x_ab_slp.txt)
// the row's 32 slot bytes, fetched from LDS BEFORE the wait (one address per 16-lane group: broadcast reads): they are live
// only across the wait and the gather, where registers are plentiful, and the aggregation does not start with a dependent read
__device__ __forceinline__ void tile_slot_words(const TileCtx &c, unsigned (&w)[8]) {
  const uint4 a = reinterpret_cast<const uint4 *>(c.lds_slots)[c.grp * 2], b = reinterpret_cast<const uint4 *>(c.lds_slots)[c.grp * 2 + 1];
  w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}

// the four rows a slot word names (one ds_read_b128 each)
__device__ __forceinline__ void tile_round_rows(const float4 *Xh4, unsigned w, int q, float4 (&v)[4]) {
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) v[jb] = Xh4[((w >> (8 * jb)) & 0xff) * PG::LPR + q];
}
// Rounds 0 .. n - 1 (n wave-uniform, 0 .. 8) of the slot words w added to a: a + ((v0 + v1) + (v2 + v3)) per round, rounds in order.
// Software-pipelined: the four rows of round r + 1 are asked for BEFORE round r is summed, so a round costs the issue of its reads and
// adds and not an LDS round trip of its own (one basic block per round behind a wave-uniform `if`, as this sum was written before,
// exposes the full latency in every round of a wave).  The exit test sits in front of the prefetch, never between a round's prefetch
// and the adds it covers; the last round is a peeled epilogue (adds only).  Worth <= 1 % of the headline: the tile's other waves already
// covered most of that latency, the sums are bound by VALU issue (profiles/r07_a_pipelined_sums.txt).
__device__ __forceinline__ float4 tile_aggregate_rounds(const TileCtx &c, const unsigned (&w)[8], const float *ldsXh, float4 a, int n) {
  const float4 *Xh4 = reinterpret_cast<const float4 *>(ldsXh);
  if (n <= 0) return a;   // wave-uniform
  float4 v[4];
  tile_round_rows(Xh4, w[0], c.q, v);
#pragma unroll
  for (int jw = 0; jw < 8; ++jw) {
    if (jw == 7 || jw + 1 >= n) {   // wave-uniform
      a = f4_add(a, f4_add(f4_add(v[0], v[1]), f4_add(v[2], v[3])));
      break;
    }
    float4 nx[4];
    tile_round_rows(Xh4, w[jw + 1], c.q, nx);
    __builtin_amdgcn_sched_barrier(0);   // the reads first: left alone, the scheduler starts every other round with the adds that wait
    a = f4_add(a, f4_add(f4_add(v[0], v[1]), f4_add(v[2], v[3])));
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) v[jb] = nx[jb];
  }
  return a;
}
// The same sum without the second buffer of rows, for the adjoint (16 more registers across its sums spill there): the two halves of
// a round roll through their own registers -- rows 0, 1 of round r + 1 are asked for as soon as v0 + v1 of round r is formed, rows
// 2, 3 as soon as v2 + v3 is -- so half a round's reads are always in flight under the other half's adds.  Same additions, same order.
__device__ __forceinline__ float4 tile_aggregate_rounds_rolling(const TileCtx &c, const unsigned (&w)[8], const float *ldsXh, float4 a, int n) {
  const float4 *Xh4 = reinterpret_cast<const float4 *>(ldsXh);
  if (n <= 0) return a;   // wave-uniform
  auto row = [&](unsigned wd, int jb) { return Xh4[((wd >> (8 * jb)) & 0xff) * PG::LPR + c.q]; };
  float4 v0 = row(w[0], 0), v1 = row(w[0], 1), v2 = row(w[0], 2), v3 = row(w[0], 3);
#pragma unroll
  for (int jw = 0; jw < 8; ++jw) {
    if (jw == 7 || jw + 1 >= n) {   // wave-uniform
      a = f4_add(a, f4_add(f4_add(v0, v1), f4_add(v2, v3)));
      break;
    }
    const float4 p = f4_add(v0, v1);
    __builtin_amdgcn_sched_barrier(0);
    v0 = row(w[jw + 1], 0); v1 = row(w[jw + 1], 1);
    __builtin_amdgcn_sched_barrier(0);
    const float4 s2 = f4_add(v2, v3);
    __builtin_amdgcn_sched_barrier(0);
    v2 = row(w[jw + 1], 2); v3 = row(w[jw + 1], 3);
    __builtin_amdgcn_sched_barrier(0);
    a = f4_add(a, f4_add(p, s2));
  }
  return a;
}

// (the two-slot kernels' form, one basic block per round: the tile-pair kernels have no 16 registers for a second buffer of rows)
__device__ __forceinline__ float4 tile_aggregate(const TileCtx &c, const unsigned (&sw)[8], const float *ldsXh) {
  const float4 *Xh4 = reinterpret_cast<const float4 *>(ldsXh);
  float4 a = f4_zero();
#pragma unroll
  for (int jw = 0; jw < 8; ++jw) {
    if (jw * 4 < c.wmax) {   // wave-uniform
      const unsigned w = sw[jw];
      float4 v[4];
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) v[jb] = Xh4[((w >> (8 * jb)) & 0xff) * PG::LPR + c.q];
      a = f4_add(a, f4_add(f4_add(v[0], v[1]), f4_add(v[2], v[3])));
    }
  }
  return f4_add(a, Xh4[c.grp * PG::LPR + c.q]);
}
// the same sums in the same order with the slot words read from LDS round by round (8 fewer registers across the rounds; for the
// interleaved adjoint, which is at the 128-register edge)
__device__ __forceinline__ float4 tile_aggregate_lean(const TileCtx &c, const float *ldsXh) {
  const float4 *Xh4 = reinterpret_cast<const float4 *>(ldsXh);
  float4 a = f4_zero();
#pragma unroll 1
  for (int jw = 0; jw * 4 < c.wmax; ++jw) {   // wave-uniform
    const unsigned w = c.lds_slots[c.grp * 8 + jw];
    float4 v[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) v[jb] = Xh4[((w >> (8 * jb)) & 0xff) * PG::LPR + c.q];
    a = f4_add(a, f4_add(f4_add(v[0], v[1]), f4_add(v[2], v[3])));
  }
  return f4_add(a, Xh4[c.grp * PG::LPR + c.q]);
}

// weighted rows: the replayed plan's order of operations (halo_finish, gcn_fused.hip: one fma per slot, in slot order); the four
// weights of a round are one 16-byte LDS read that the row's 16 lanes share
__device__ __forceinline__ float4 tile_aggregate_weighted(const TileCtx &c, const float *ldsXh) {
  const float4 *Xh4 = reinterpret_cast<const float4 *>(ldsXh);
  float4 a = f4_zero();
#pragma unroll 1
  for (int jw = 0; jw * 4 < c.wmax; ++jw) {   // wave-uniform
    const unsigned w = c.lds_slots[c.grp * 8 + jw];
    const float4 wv = *reinterpret_cast<const float4 *>(c.lds_w + c.grp * kSlotWidth + 4 * jw);
    float4 v[4];
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) v[jb] = Xh4[((w >> (8 * jb)) & 0xff) * PG::LPR + c.q];
    a = f4_fma(wv.x, v[0], a); a = f4_fma(wv.y, v[1], a); a = f4_fma(wv.z, v[2], a); a = f4_fma(wv.w, v[3], a);
  }
  return f4_add(a, Xh4[c.grp * PG::LPR + c.q]);
}


// ---- own-first aggregation (round 6; the plan's OwnFirst tables, common.h) ------------------------------------------------------------
// The slot bytes a plan's forward kernels read list every row's own-tile slots first (padded to the wave's number of own rounds), then the
// foreign ones; TileMeta::of_pre names the own rounds per wave.  The one-tile forward kernels sum those rounds BEFORE they wait for their
// neighbours' flags -- a tile's own rows are in LDS since its last epilogue -- and only the foreign rounds behind the gather.  Measured
// with an in-kernel re-ordering of the same kind (profiles/r06_a_own_first.txt): forward launch 2.301 -> 2.234 ms.
// The foreign rounds start at a wave-uniform round r0 = of_pre: their slot words are fetched a second time, shifted, so that the pipelined
// sum (tile_aggregate_rounds) indexes its words from 0 with constants: w[k] = the row's word min(r0 + k, 7).  Fetched with the own
// rounds' words BEFORE the wait; the own rounds' words are dead by then, so no more registers cross the wait than before.
__device__ __forceinline__ void tile_slot_words_from(const TileCtx &c, int r0, unsigned (&w)[8]) {
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = c.lds_slots[c.grp * 8 + min(r0 + k, 7)];
}
// ---- hub geometry (graphs whose tiles do not fit the 96-row halo / 32-entry rows: BASELINE config 1's Cora-shaped graph) --------
// One workgroup per CU and tile; per tile and direction (lists built by node_persistent_setup, not part of the graph handle):
//   * a halo of up to kHubHalo = 256 distinct rows (own rows first), 64 KB of LDS -- the reach of an LDS-DMA destination;
//   * per row a VARIABLE-length list of slot bytes in CSR order (start aligned to 4, {start, length} per row), at most kHubList bytes
//     per tile; no zero row: the tail of a list is masked, not padded;
//   * rows longer than kSlotWidth entries ("long rows", the hubs) are summed by all 32 lane groups together: group g takes entries
//     g, g + 32, ..., the 32 partial rows meet in LDS and the row's own group adds them in group order;
//   * a wait list of up to 255 tiles: four flags per lane of the polling wave (position 63 of the list is the abort word's lane).
// Arithmetic per row otherwise as in the 96-row geometry (groups of four slots, then the own row).
constexpr int kHubHalo = 256;
constexpr int kHubList = 4096;
constexpr int kHubNbr = 256;
constexpr int kHubXhF = kHubHalo * PD;
constexpr int kHubMetaF = kHubList / 4 + (kHubHalo - kTM) + 2 * kTM + kTM / 4 + kHubList;   // slot bytes, foreign node ids, {start, length} per row, long-row indices, entry weights

struct HubCtx : TileCtx {
  const uint8_t *hs;         // LDS: the tile's slot bytes
  const int2 *hrows;         // LDS: {start, length} of every row's list
  const uint8_t *hlong;      // LDS: rows with more than kSlotWidth entries
  const float *hw;           // LDS: the entries' edge weights (same positions as the slot bytes), or NULL: unweighted graph
  int start, len;            // this row's list (len = 0 for a long row: it is summed cooperatively)
  int n_long;
  int nb1, nb2, nb3;         // wave 0: wait-list entries lane + 64, + 128, + 192 (my_nbr = entry lane)
};

__device__ __forceinline__ void hub_ctx_init(const TileMeta &m, HubCtx &c, float *lds_meta) {
  c.tid = threadIdx.x;
  c.lane = c.tid & 63;
  c.wave_u = __builtin_amdgcn_readfirstlane(c.tid >> 6);
  c.grp = c.tid >> 4;
  c.q = c.tid & 15;
  c.tile = xcd_tile(blockIdx.x, m.n_tiles);
  const size_t pos = (size_t)c.tile * kTM + c.grp;
  const int4 sc = m.hub_sched[pos];
  c.valid = sc.x >= 0;
  c.node = max(sc.x, 0);
  c.ci = c.valid ? __int_as_float(sc.w) : 0.f;
  const int4 info = m.hub_info[c.tile];   // {halo count, list bytes (multiple of 16), long rows, -}
  uint4 *ls = reinterpret_cast<uint4 *>(lds_meta);
  int *lh = reinterpret_cast<int *>(lds_meta + kHubList / 4);
  int2 *lr = reinterpret_cast<int2 *>(lds_meta + kHubList / 4 + (kHubHalo - kTM));
  unsigned *ll = reinterpret_cast<unsigned *>(lds_meta + kHubList / 4 + (kHubHalo - kTM) + 2 * kTM);
  if (c.tid * 16 < info.y) ls[c.tid] = reinterpret_cast<const uint4 *>(m.hub_slots + (size_t)c.tile * kHubList)[c.tid];
  if (c.tid < kHubHalo - kTM) lh[c.tid] = m.hub_halo[(size_t)c.tile * kHubHalo + kTM + c.tid];
  if (c.tid >= 256 && c.tid < 256 + kTM) lr[c.tid - 256] = m.hub_rows[(size_t)c.tile * kTM + (c.tid - 256)];
  if (c.tid >= 320 && c.tid < 320 + kTM / 4) ll[c.tid - 320] = reinterpret_cast<const unsigned *>(m.hub_long + (size_t)c.tile * kTM)[c.tid - 320];
  c.hs = reinterpret_cast<const uint8_t *>(ls);
  c.lds_hnode = lh;
  c.lds_slots = nullptr;
  c.lds_w = nullptr;
  c.hrows = lr;
  c.hlong = reinterpret_cast<const uint8_t *>(ll);
  c.hw = nullptr;
  if (m.hub_w) {   // (uniform) edge weights (src/layers.jl:206-231): one float beside every slot byte
    float4 *lw = reinterpret_cast<float4 *>(lds_meta + kHubList / 4 + (kHubHalo - kTM) + 2 * kTM + kTM / 4);
    const float4 *gw = reinterpret_cast<const float4 *>(m.hub_w + (size_t)c.tile * kHubList);
#pragma unroll
    for (int k = 0; k < kHubList / 4 / kThreads; ++k)
      if ((c.tid + k * kThreads) * 4 < info.y) lw[c.tid + k * kThreads] = gw[c.tid + k * kThreads];
    c.hw = reinterpret_cast<const float *>(lw);
  }
  c.hcount = __builtin_amdgcn_readfirstlane(info.x);
  c.n_long = __builtin_amdgcn_readfirstlane(info.z);
  const int2 mine = m.hub_rows[pos];
  c.start = mine.x;
  c.len = (c.valid && mine.y <= kSlotWidth) ? mine.y : 0;
  int wm = c.len;
  wm = max(wm, __shfl_xor(wm, 16));
  wm = max(wm, __shfl_xor(wm, 32));
  c.wmax = __builtin_amdgcn_readfirstlane(wm);
  const int *nb = m.nbr + (size_t)c.tile * kHubNbr;
  c.my_nbr = nb[c.lane]; c.nb1 = nb[c.lane + 64]; c.nb2 = nb[c.lane + 128]; c.nb3 = nb[c.lane + 192];
}

// tile_wait for a wait list of up to 255 tiles: four independent flag loads per lane and round.  (Its own copy of flag_poll's loop,
// with the stride spelled out: through flag_poll<4>, or with flag_line here, the hub kernels come out different and measured slower.)
__device__ __forceinline__ bool hub_wait(const TileMeta &m, const HubCtx &c, int ph, int *s_ok) {
  if (ph <= 1) return true;
  if (c.wave_u == 0) {
    const unsigned need = (unsigned)(ph - 1);
    const unsigned *a0 = (c.lane == 63) ? m.abort_word : (c.my_nbr >= 0 ? m.flags + kFlagLine * c.my_nbr : nullptr);
    const unsigned *a1 = c.nb1 >= 0 ? m.flags + kFlagLine * c.nb1 : nullptr, *a2 = c.nb2 >= 0 ? m.flags + kFlagLine * c.nb2 : nullptr,
                   *a3 = c.nb3 >= 0 ? m.flags + kFlagLine * c.nb3 : nullptr;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool ok = true;
    for (unsigned it = 1;; ++it) {
      unsigned f0 = need, f1 = need, f2 = need, f3 = need;
      if (a0) f0 = __hip_atomic_load(a0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a1) f1 = __hip_atomic_load(a1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a2) f2 = __hip_atomic_load(a2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (a3) f3 = __hip_atomic_load(a3, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__any((int)(c.lane == 63 && f0 != 0))) { ok = false; break; }              // somebody gave up
      if (__all((int)((c.lane == 63 || f0 >= need) && f1 >= need && f2 >= need && f3 >= need))) break;
      if ((it & 1023u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) {
        if (c.lane == 0) __hip_atomic_store(m.abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ok = false;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (c.lane == 0) *s_ok = ok ? 1 : 0;
  }
  __syncthreads();
  return *s_ok != 0;
}

// tile_gather_foreign for up to 224 foreign rows (halo slots 32 .. 255)
__device__ __forceinline__ void hub_gather_foreign(const HubCtx &c, const float *X, float *ldsXh) {
  float4 *Xh4 = reinterpret_cast<float4 *>(ldsXh);
#pragma unroll
  for (int k = 0; k < (kHubHalo - kTM) / kTM; ++k) {
    if (4 * c.wave_u + 32 * (k + 1) < c.hcount) {   // wave-uniform: a wave's four groups stage four consecutive slots
      const unsigned off = (unsigned)c.lds_hnode[c.grp + 32 * k] * (unsigned)(PD * 4) + (unsigned)(c.q * 16);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const char *>(X) + off),
                                       (__attribute__((address_space(3))) void *)(Xh4 + (c.grp + 32 * (k + 1)) * PG::LPR + c.q), 16, 0, 16);
    }
  }
  wait_vmcnt0();
  __syncthreads();
}

// the row's first 32 slot bytes, fetched from LDS BEFORE the wait (as tile_slot_words; words beyond the row's list hold other rows'
// bytes or table words -- valid LDS, masked at use)
__device__ __forceinline__ void hub_slot_words(const HubCtx &c, unsigned (&w)[8]) {
  const unsigned *s4 = reinterpret_cast<const unsigned *>(c.hs + c.start);
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = s4[k];
}

// sum of the row's neighbours + its own row; `part` = 32 x 64 floats of LDS that nobody else uses during the aggregation.
// (Measured and not kept: the long row's partial rows formed first, eight masked entries per group unrolled with their slot bytes
// fetched together -- 8 + 8 LDS reads per lane whatever the row's length: the hub tile's aggregation 3.8 k -> 4.7 k cycles.)
// Weighted graphs (c.hw): one fma per entry in list order, as the 96-row geometry's weighted rows (tile_aggregate_weighted); a long
// row's groups fold weight * row into their partial sums.
__device__ __forceinline__ float4 hub_aggregate(const HubCtx &c, const unsigned (&sw)[8], const float *ldsXh, float *part) {
  const float4 *Xh4 = reinterpret_cast<const float4 *>(ldsXh);
  float4 a = f4_zero();
  if (c.hw) {   // (uniform)
#pragma unroll 1
    for (int jw = 0; jw * 4 < c.wmax; ++jw) {   // wave-uniform
      const unsigned w = sw[jw];
      const float4 wv = *reinterpret_cast<const float4 *>(c.hw + c.start + 4 * jw);   // (list starts are multiples of four: 16-byte aligned)
      const float ww[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
      for (int jb = 0; jb < 4; ++jb) {
        const float4 v = f4_sel(4 * jw + jb < c.len, Xh4[((w >> (8 * jb)) & 0xff) * PG::LPR + c.q], f4_zero());
        a = f4_fma(4 * jw + jb < c.len ? ww[jb] : 0.f, v, a);
      }
    }
  } else {
#pragma unroll
    for (int jw = 0; jw < 8; ++jw) {
      if (jw * 4 < c.wmax) {   // wave-uniform
        const unsigned w = sw[jw];
        float4 v[4];
#pragma unroll
        for (int jb = 0; jb < 4; ++jb) v[jb] = f4_sel(4 * jw + jb < c.len, Xh4[((w >> (8 * jb)) & 0xff) * PG::LPR + c.q], f4_zero());
        a = f4_add_pk(a, f4_add_pk(f4_add_pk(v[0], v[1]), f4_add_pk(v[2], v[3])));
      }
    }
  }
  for (int li = 0; li < c.n_long; ++li) {   // uniform
    const int r = c.hlong[li];
    const int2 rl = c.hrows[r];
    float4 p = f4_zero();
    if (c.hw) {
      for (int j = c.grp; j < rl.y; j += kTM) p = f4_fma(c.hw[rl.x + j], Xh4[(unsigned)c.hs[rl.x + j] * PG::LPR + c.q], p);
    } else {
      for (int j = c.grp; j < rl.y; j += kTM) p = f4_add_pk(p, Xh4[(unsigned)c.hs[rl.x + j] * PG::LPR + c.q]);
    }
    reinterpret_cast<float4 *>(part)[c.grp * PG::LPR + c.q] = p;
    __syncthreads();
    if (c.wave_u == (r >> 2)) {   // the wave of the row's group: each of its four groups adds eight partial rows, two exchanges fold them
      const int g4 = c.grp & 3;
      float4 t = reinterpret_cast<const float4 *>(part)[g4 * PG::LPR + c.q];
#pragma unroll
      for (int k = 1; k < kTM / 4; ++k) t = f4_add_pk(t, reinterpret_cast<const float4 *>(part)[(g4 + 4 * k) * PG::LPR + c.q]);
      t.x += __shfl_xor(t.x, 16); t.y += __shfl_xor(t.y, 16); t.z += __shfl_xor(t.z, 16); t.w += __shfl_xor(t.w, 16);
      t.x += __shfl_xor(t.x, 32); t.y += __shfl_xor(t.y, 32); t.z += __shfl_xor(t.z, 32); t.w += __shfl_xor(t.w, 32);
      if (c.grp == r) a = f4_add_pk(a, t);
    }
    __syncthreads();   // (the buffer is written again: by the next long row, or by the caller -- the adjoint's dz tile)
  }
  return f4_add_pk(a, Xh4[c.grp * PG::LPR + c.q]);
}

// W (row-major [in][out]) -> LDS, transposed (forward: B[k = in][j = out], stored Bt[j][k]) or straight (pullback: Bt[j = in][k = out])
__device__ __forceinline__ void load_weight_lds(const float *wt, float *ldsBt, int tid, bool transpose) {
  if (transpose) {
    const int j = tid % PD, kg0 = tid / PD;
#pragma unroll
    for (int ps = 0; ps < PG::NPASS; ++ps) {
      const int kg = kg0 + ps * PG::KGP;
      if (kg < PD / 4) {
        const float *w = wt + (size_t)(4 * kg) * PD + j;
        *reinterpret_cast<float4 *>(&ldsBt[j * PG::TS + 4 * kg]) = make_float4(w[0], w[PD], w[2 * PD], w[3 * PD]);
      }
    }
  } else {
#pragma unroll
    for (int k = 0; k < PG::W4; ++k) {
      const int idx = tid + k * kThreads;
      if (idx < PD * PD / 4) {
        const int wi = (idx * 4) / PD, wo = (idx * 4) % PD;
        *reinterpret_cast<float4 *>(&ldsBt[wi * PG::TS + wo]) = reinterpret_cast<const float4 *>(wt)[idx];
      }
    }
  }
}

// ---- pieces of the interleaved kernels' software pipeline -------------------------------------------------------------------
// wave 0: one flag load per lane of the wait list (lane 63: the abort word), NOT waited for
__device__ __forceinline__ unsigned poll_issue(const TileMeta &m, const TileCtx &c, const unsigned *flags) {
  const unsigned *addr = (c.lane == 63) ? m.abort_word : (c.my_nbr >= 0 ? flag_line(flags, c.my_nbr) : nullptr);
  unsigned f = (c.lane == 63) ? 0u : 0xffffffffu;
  if (addr) f = __hip_atomic_load(addr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return f;
}
// wave 0: did every tile of the wait list show phase ph - 1 (and nobody give up)?
__device__ __forceinline__ bool poll_ready(const TileCtx &c, unsigned f, int ph) {
  const unsigned need = (unsigned)(ph - 1);
  return __all((int)(c.lane == 63 ? f == 0u : f >= need)) != 0;
}
// a slot's own rows into halo slots 0..31 and the LDS-DMA of the foreign rows (tile_gather_foreign without its wait).  `halo`
// is __restrict__ so that LDS reads of OTHER regions issued behind it are not made to wait for the DMA (see dense_mfma.hip,
// products_beside_dma: behind a global_load_lds the wait-count pass otherwise drains vmcnt in front of every LDS access)
__device__ __forceinline__ void halo_fill_ahead(const TileCtx &c, const float *X, float *__restrict__ halo, float4 xown) {
  float4 *Xh4 = reinterpret_cast<float4 *>(halo);
  Xh4[c.grp * PG::LPR + c.q] = xown;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (4 * c.wave_u + 32 * (k + 1) < c.hcount) {   // wave-uniform
      const unsigned off = (unsigned)c.lds_hnode[c.grp + 32 * k] * (unsigned)(PD * 4) + (unsigned)(c.q * 16);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const char *>(X) + off),
                                       (__attribute__((address_space(3))) void *)(Xh4 + (c.grp + 32 * (k + 1)) * PG::LPR + c.q), 16, 0, 16);
    }
  }
}
// the same with the slot's OWN rows fetched as well (halo slots 0..31 = the tile's rows: one more DMA per wave; they were stored
// write-through at least a slot-phase earlier).  For kernels that keep no copy of them in registers.
__device__ __forceinline__ void halo_fill_all(const TileCtx &c, const float *X, float *__restrict__ halo) {
  float4 *Xh4 = reinterpret_cast<float4 *>(halo);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (k == 0 || 4 * c.wave_u + 32 * k < c.hcount) {   // wave-uniform
      const unsigned row = k == 0 ? (unsigned)c.node : (unsigned)c.lds_hnode[c.grp + 32 * (k - 1)];
      const unsigned off = row * (unsigned)(PD * 4) + (unsigned)(c.q * 16);
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(reinterpret_cast<const char *>(X) + off),
                                       (__attribute__((address_space(3))) void *)(Xh4 + (c.grp + 32 * k) * PG::LPR + c.q), 16, 0, 16);
    }
  }
}

// ---- the kernels' argument blocks --------------------------------------------------------------------------------------------
// forward solve
struct PFwdK {
  TileMeta m;          // lists by TARGET
  int n_steps, S, act;
  int n_members;       // trajectories solved one after the other on the same structure (a block-diagonal batch of identical graphs)
  const float *u_in;   // [n_members][N][64]  c .* u0
  float *u_out;        // [n_members][N][64]  c .* u(T)
  float *bufA, *bufB;  // exchanged arrays: stage input (A), layer-1 output (B)
  const float *w1, *b1, *w2, *b2;
  float *tape;         // [n_members][n_steps][S][2][N][64] aggregated layer inputs, or null (forward-only plan)
  uint8_t *masks;      // [n_members][n_steps][S][2][mask_bytes] relu sign bits
  float *ztape;        // same shape as tape: the pre-activations, kept instead of the sign bits when the activation is not relu
  size_t row_elems, mask_bytes;
  size_t flag_stride;  // two-slot kernels: slot s uses bufA / bufB + s * row_elems and the flag words m.flags + s * flag_stride
  int pair_wgs;        // tile-pair mode of the two-slot kernels (PAIR): the grid; workgroup b holds tiles t and t + pair_wgs of ONE member
  int k_tiles;         // tile-round mode (node_fwd_persistentK_kernel): workgroup b holds tiles t, t + pair_wgs, ..., k_tiles of them
  float *state;        // ... and keeps their state in memory: [7][N][64] own rows -- u, k_0 .. k_5 (k rows zero at launch)
  const float *cf;     // device table [36 + 6]: cf[i * 6 + j], j < i: coefficient of k_j in the array written after stage i (next
                       // stage input / step update), 0 elsewhere; cf[36 + i]: coefficient of k_i itself.  Copied to LDS.
};

// discrete adjoint
struct PBwdK {
  TileMeta m;          // lists by SOURCE
  int n_steps, S, n_members, act;
  const float *ztape;  // pre-activations (activations other than relu), or null
  float *lam;          // [n_members][N][64] in: dL/du~(T) (adjoint seed ./ c); out: dL/du~0
  float *g1, *g2;      // exchanged arrays: c .* (dZ1 W1^T), c .* (dZ2 W2^T)
  const float *w1, *w2;
  const float *tape;
  const uint8_t *masks;
  size_t row_elems, mask_bytes;
  float *slab_dw1, *slab_db1, *slab_dw2, *slab_db2;   // [n_tiles][...] written ONCE, at the end
  int pair_wgs;        // tile-pair mode (PAIR): the grid; workgroup b holds tiles t and t + pair_wgs of ONE member
  int k_tiles;         // tile-round mode (node_bwd_persistentK_kernel): k_tiles tiles per workgroup, state in lam / ubar (zero at launch)
  size_t flag_stride;  // two-slot kernel: slot s uses g1 / g2 + s * row_elems, the flag words m.flags + s * flag_stride and
  float *ubar;         // the stage-adjoint scratch ubar + s * 5 * row_elems ([slot][5][N][64])
  const float *cb;     // device table [6 + 36 + 6], copied to LDS: cb[j] = dt * b[j]; cb[6 + i * 6 + j], j > i >= 1: dt * a[j][i-1], the
                       // weight of U-bar_j in K-bar_{i-1}, 0 elsewhere; cb[42 + i] = dt * a[i][i-1], the weight of U-bar_i itself
};

// =====================================================================================================================
// The solver's arithmetic, written once.  The eight kernels of node_persistent.hip differ in SCHEDULE only -- where the waits, the
// gathers, the publishes and the prefetches sit -- and every one of them is held bitwise to the replayed plan (u(T), du0).  What
// follows is the order of operations those tests pin; a kernel body calls these pieces and keeps its schedule.  No piece holds a
// barrier, a wait for memory, a poll, a publish or a phase stamp.  Rows and coefficients travel by value, so that a kernel decides
// where they come from (registers, memory rows fetched turns ago, LDS); a pointer is __restrict__ only in the form that says why.
// profiles/r08_a_persistent_shared_arithmetic.txt compares every kernel's instruction stream with the pasted form's.
// =====================================================================================================================

// this thread's 16 bytes of a 32-row MFMA operand / result tile in LDS
__device__ __forceinline__ float4 tile_row(const float *tile, const TileCtx &c) { return *reinterpret_cast<const float4 *>(&tile[c.grp * PG::TS + 4 * c.q]); }
__device__ __forceinline__ void tile_row_store(float *tile, const TileCtx &c, float4 v) { *reinterpret_cast<float4 *>(&tile[c.grp * PG::TS + 4 * c.q]) = v; }

// byte offset of a thread's 16 bytes (lane q of the row's 16) of row `node` in a [N][64] array; of its own row
__device__ __forceinline__ unsigned row_offset(int node, int q) { return (unsigned)node * (unsigned)(PD * 4) + (unsigned)(q * 16); }
__device__ __forceinline__ unsigned own_row_offset(const TileCtx c) { return row_offset(c.node, c.q); }

// ---- launch prologue -------------------------------------------------------------------------------------------------
// the Runge-Kutta coefficient table (PFwdK::cf, 42 words / PBwdK::cb, 48 words) -> LDS
__device__ __forceinline__ void coef_to_lds(float *ldsC, const float *table, int n, int tid) {
  if (tid < n) ldsC[tid] = table[tid];
}
// both layers' biases -> LDS (a layer without a bias adds zero)
__device__ __forceinline__ void biases_to_lds(float *ldsB, const float *b1, const float *b2, int tid) {
  if (tid < PD) ldsB[tid] = b1 ? b1[tid] : 0.f;
  else if (tid < 2 * PD) ldsB[tid] = b2 ? b2[tid - PD] : 0.f;
}
// halo slot kHaloCap: the all-zero row that padding slot bytes name, written by the first 16-lane group; q = the lane within the row
__device__ __forceinline__ void zero_halo_row(float *ldsXh, bool first_group, int q) {
  if (first_group) reinterpret_cast<float4 *>(ldsXh)[kHaloCap * PG::LPR + q] = f4_zero();
}
// tile rounds: workgroup b holds tiles t0, t0 + W, ..., at most K of them, within the graph (the last workgroups of a ragged grid hold
// one fewer).  Their tables -> LDS; how many it really holds
template <bool WEIGHTED>
__device__ __forceinline__ void tile_round_tables(const TileMeta &m, int t0, int W, int K, float *ldsMeta) {
  for (int s = 0; s < K && t0 + s * W < m.n_tiles; ++s) tile_tables_to_lds<WEIGHTED>(m, t0 + s * W, ldsMeta + s * meta_stride<WEIGHTED>());
}
__device__ __forceinline__ int tile_round_count(const TileMeta &m, int t0, int W, int K) {
  int n = 0;
  for (int s = 0; s < K && t0 + s * W < m.n_tiles; ++s) n = s + 1;
  return n;
}

// ---- a wait was aborted: NaN into every output row this workgroup owns -------------------------------------------------------
// tile rounds: the rows of its n tiles t0, t0 + W, ...
__device__ __forceinline__ void poison_tile_rounds(const TileMeta &m, float *out, int t0, int W, int n, int tid) {
  for (int s = 0; s < n; ++s) {
    const int4 sc = m.sched[(size_t)(t0 + s * W) * kTM + (tid >> 4)];
    if (sc.x >= 0) st4_g(out, row_offset(sc.x, tid & 15), f4_nan());
  }
}
// two-slot kernels: one row in every member's array
__device__ __forceinline__ void poison_members(float *out, int n_members, size_t row_elems, bool valid, unsigned own) {
  for (int mb = 0; mb < n_members; ++mb)
    if (valid) st4_g(out + (size_t)mb * row_elems, own, f4_nan());
}

// ---------------------------------------------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------------------------------------------
// pre-activation of this thread's 16 bytes: product tile + bias
__device__ __forceinline__ float4 fwd_preact(const float *ldsZ, const TileCtx &c, float4 bias) { return f4_add(tile_row(ldsZ, c), bias); }
// relu'(z) of this thread's four columns as four bits, the forward's tape for the adjoint (adjoint_dz)
__device__ __forceinline__ uint8_t relu_sign_bits(float4 z) {
  return (uint8_t)((z.x > 0.f ? 1 : 0) | (z.y > 0.f ? 2 : 0) | (z.z > 0.f ? 4 : 0) | (z.w > 0.f ? 8 : 0));
}
// the layer's output row, stored as c .* y (pre-scaled for the next aggregation); padding rows are zero
__device__ __forceinline__ float4 fwd_output(const TileCtx &c, int act, float4 z) { return f4_sel(c.valid, f4_scale(c.ci, f4_act(act, z)), f4_zero()); }

// The six coefficients of stage i (PFwdK::cf in LDS): of k_i itself and of k_0 .. k_4 in the array written after the stage.
// RkCoef: read at once -- for kernels whose epilogue issues an LDS-DMA, in front of which every LDS read must sit.
// RkCoefInPlace: read where the sum uses them.
struct RkCoef {
  float s, c0, c1, c2, c3, c4;
  __device__ __forceinline__ float self() const { return s; }
  __device__ __forceinline__ float k0() const { return c0; }
  __device__ __forceinline__ float k1() const { return c1; }
  __device__ __forceinline__ float k2() const { return c2; }
  __device__ __forceinline__ float k3() const { return c3; }
  __device__ __forceinline__ float k4() const { return c4; }
};
__device__ __forceinline__ RkCoef rk_coef(const float *ldsC, int i) {
  return RkCoef{ldsC[36 + i], ldsC[i * 6 + 0], ldsC[i * 6 + 1], ldsC[i * 6 + 2], ldsC[i * 6 + 3], ldsC[i * 6 + 4]};
}
struct RkCoefInPlace {
  const float *ldsC;
  int i;
  __device__ __forceinline__ float self() const { return ldsC[36 + i]; }
  __device__ __forceinline__ float k0() const { return ldsC[i * 6 + 0]; }
  __device__ __forceinline__ float k1() const { return ldsC[i * 6 + 1]; }
  __device__ __forceinline__ float k2() const { return ldsC[i * 6 + 2]; }
  __device__ __forceinline__ float k3() const { return ldsC[i * 6 + 3]; }
  __device__ __forceinline__ float k4() const { return ldsC[i * 6 + 4]; }
};
// The array written after stage i (next stage input, or the step update) = u + sum_j cf[i][j] k_j, in the order of the replayed plan:
// coef_self * k_i first, then u, then k_0 .. k_4.  Terms with a zero coefficient add an exact zero (k_j is finite, stale values of later
// stages included), so a caller may pass a stale k_j or a zero row in the places stage i does not combine.  k_i = yv: passed in its
// place by the caller, or (KI_IS_YV) put there here, where the caller's k_i still holds the previous step's.
template <bool KI_IS_YV>
__device__ __forceinline__ float4 rk_stage_row(int i, int j, float4 yv, float4 kj) {
  if constexpr (KI_IS_YV) return f4_sel(i == j, yv, kj);
  else return kj;
}
template <bool KI_IS_YV, class Coef>
__device__ __forceinline__ float4 rk_combine(Coef cf, int i, float4 yv, float4 u, float4 k0, float4 k1, float4 k2, float4 k3, float4 k4) {
  float4 v = f4_scale(cf.self(), yv);
  v = f4_fma(1.0f, u, v);
  v = f4_fma(cf.k0(), rk_stage_row<KI_IS_YV>(i, 0, yv, k0), v); v = f4_fma(cf.k1(), rk_stage_row<KI_IS_YV>(i, 1, yv, k1), v);
  v = f4_fma(cf.k2(), rk_stage_row<KI_IS_YV>(i, 2, yv, k2), v); v = f4_fma(cf.k3(), rk_stage_row<KI_IS_YV>(i, 3, yv, k3), v);
  v = f4_fma(cf.k4(), rk_stage_row<KI_IS_YV>(i, 4, yv, k4), v);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------------
// adjoint
// ---------------------------------------------------------------------------------------------------------------------
// dZ of this thread's 16 bytes: dL/dy = c .* K-bar times act'(z) -- relu' from the forward's sign bits (RELU, Aux = unsigned), any
// other activation from the saved pre-activations (Aux = float4); padding rows are zero
template <bool RELU, class Aux>
__device__ __forceinline__ float4 adjoint_dz(const TileCtx &c, int act, float4 kbar, Aux mk) {
  kbar = f4_scale(c.ci, kbar);
  if constexpr (RELU) {
    return c.valid ? make_float4((mk & 1u) ? kbar.x : 0.f, (mk & 2u) ? kbar.y : 0.f, (mk & 4u) ? kbar.z : 0.f, (mk & 8u) ? kbar.w : 0.f)
                   : f4_zero();
  } else {
    return f4_sel(c.valid, f4_mul(kbar, f4_dact(act, mk)), f4_zero());
  }
}
// K-bar of a step's last stage: dt b_S times lambda (PBwdK::cb in LDS)
__device__ __forceinline__ float4 adjoint_kbar_last(const float *ldsC, int S, float4 lam) { return f4_scale(ldsC[S - 1], lam); }
// the tape row as the parameter-gradient products' other operand; padding rows are zero
__device__ __forceinline__ void adjoint_x_store(float *ldsX, const TileCtx &c, float4 xrow) { tile_row_store(ldsX, c, f4_sel(c.valid, xrow, f4_zero())); }
// the row of G = dZ W^T, stored as c .* G for the next gather
__device__ __forceinline__ float4 adjoint_g_row(const float *ldsG, const TileCtx &c) { return f4_sel(c.valid, f4_scale(c.ci, tile_row(ldsG, c)), f4_zero()); }

// Parameter gradients of a tile: dWt[i][o] += sum_n A[n][i] dZ[n][o] over the tile's 32 rows (tX = the tape rows, tDZ = dZ, both
// MFMA operand tiles in LDS), db += column sums of dZ.  Nobody waits for them, so the kernels run them behind the publish (or behind
// the product of a turn whose flag goes out later): they fill the time the neighbours need to see the flag and this tile needs to
// see theirs.  dbc / dbpart: the column and the row-partial this thread sums (tid / DBP, tid % DBP).
__device__ __forceinline__ void param_grad_products(const float *tX, const float *tDZ, int wave_u, int lane, int dbc, int dbpart,
                                                    f32x4 (&dwl)[PG::DWT], float &dbl) {
  constexpr int NT = PG::CT * PG::CT;
  const int i16 = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int mm = 0; mm < PG::DWT; ++mm) {
    const int tt = wave_u + PG::WAVES * mm;
    if (tt < NT) {   // wave-uniform
      const int mt = tt / PG::CT, nt = tt % PG::CT;
#pragma unroll
      for (int kh = 0; kh < 2; ++kh) {   // two halves of the 32-row contraction: 8 operand registers live instead of 16
        float a[kTM / 8], b[kTM / 8];
#pragma unroll
        for (int ks = 0; ks < kTM / 8; ++ks) {
          a[ks] = tX[(4 * (ks + 4 * kh) + kq) * PG::TS + mt * 16 + i16];
          b[ks] = tDZ[(4 * (ks + 4 * kh) + kq) * PG::TS + nt * 16 + i16];
        }
#pragma unroll
        for (int ks = 0; ks < kTM / 8; ++ks) dwl[mm] = mfma16(a[ks], b[ks], dwl[mm]);
      }
    }
  }
  float sdb = 0.f;
#pragma unroll
  for (int nn = dbpart; nn < kTM; nn += PG::DBP) sdb += tDZ[nn * PG::TS + dbc];
#pragma unroll
  for (int o = 1; o < PG::DBP; o <<= 1) sdb += __shfl_xor(sdb, o);
  dbl += sdb;
}
// The same for a kernel that issues the next turn's LDS-DMA into the halo region just before: the operand tiles are __restrict__ so that
// these LDS reads do not wait for that DMA (halo_fill_ahead).  The qualifier reaches the loads through inlining only (the body above
// is not restrict): check the products' s_waitcnt in the assembly after a compiler change.
__device__ __forceinline__ void param_grad_products_beside_dma(const float *__restrict__ tX, const float *__restrict__ tDZ, int wave_u, int lane, int dbc,
                                                               int dbpart, f32x4 (&dwl)[PG::DWT], float &dbl) {
  param_grad_products(tX, tDZ, wave_u, lane, dbc, dbpart, dwl, dbl);
}

// The adjoint of the stage combination, t = U-bar_i = A^T g1 of this phase, in the order of the replayed plan: coef_self * t first, then
// lambda, then the later stages' U-bar (PBwdK::cb in LDS).  Zero weights add an exact zero -- cb[6 + i * 6 + j] is zero for j <= i, and
// stage adjoints beyond S stay zero -- so U-bar_i itself may be passed as t, as a stale value or as zero.
// stage i >= 1: K-bar of the stage evaluated before it
__device__ __forceinline__ float4 adjoint_kbar_stage(const float *ldsC, int i, float4 t, float4 lam, float4 ub2, float4 ub3, float4 ub4, float4 ub5) {
  float4 v = f4_scale(ldsC[42 + i], t);
  v = f4_fma(ldsC[i - 1], lam, v);
  v = f4_fma(ldsC[6 + i * 6 + 2], ub2, v); v = f4_fma(ldsC[6 + i * 6 + 3], ub3, v);
  v = f4_fma(ldsC[6 + i * 6 + 4], ub4, v); v = f4_fma(ldsC[6 + i * 6 + 5], ub5, v);
  return v;
}
// stage 0: lambda of the step before (the member's dL/du~0 at the end); K-bar of that step's last stage is dt b_S times it
__device__ __forceinline__ float4 adjoint_lambda_update(float4 t, float4 lam, float4 ub1, float4 ub2, float4 ub3, float4 ub4, float4 ub5) {
  float4 v = f4_scale(1.0f, t);
  v = f4_fma(1.0f, lam, v);
  v = f4_fma(1.0f, ub1, v); v = f4_fma(1.0f, ub2, v); v = f4_fma(1.0f, ub3, v);
  v = f4_fma(1.0f, ub4, v); v = f4_fma(1.0f, ub5, v);
  return v;
}

// A workgroup's contribution to a layer's parameter gradients: its accumulators -> its slab (summed by reduce_slabs_kernel), written
// once, at the end; NaN when a wait was aborted.
__device__ __forceinline__ void write_slab(const f32x4 (&dwl)[PG::DWT], float dbl, float *slab_dw, float *slab_db, int wave_u, int lane,
                                           int dbc, int dbpart, bool ok) {
  float4 *slab4 = reinterpret_cast<float4 *>(slab_dw + (size_t)blockIdx.x * PD * PD);
#pragma unroll
  for (int mm = 0; mm < PG::DWT; ++mm) {
    const int tt = wave_u + PG::WAVES * mm;
    if (tt < PG::CT * PG::CT) slab4[tt * 64 + lane] = f4_sel(ok, make_float4(dwl[mm][0], dwl[mm][1], dwl[mm][2], dwl[mm][3]), f4_nan());
  }
  if (dbpart == 0) slab_db[(size_t)blockIdx.x * PD + dbc] = ok ? dbl : __int_as_float(0x7fc00000);
}

}  // namespace

}  // namespace ngpde
