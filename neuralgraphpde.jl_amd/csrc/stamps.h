// stamps.h -- in-kernel phase timestamps of the diagnostic build (`make diag`, -DNGPDE_STAMPS; read by tools/stamps.py).  The only
// place that tests NGPDE_STAMPS: in the product build every macro below expands to nothing, and no kernel, parameter struct or
// export changes.
//
// A family's kernels carry a StampSink in their parameter struct (NGPDE_STAMP_FIELD).  Thread 0 of a workgroup writes word k of
// its row: [gridDim.x][w] (NGPDE_STAMP), or [gridDim.x][phases][8] for the persistent solvers (NGPDE_PHASE_STAMP).  A word at or
// past the sink's capacity, or a phase past its count, is not written.
#pragma once

#include <cstddef>
#include <cstdint>

#include "common.h"

namespace ngpde {

// the first argument of ngpde_debug_set_stamps; tools/stamps.py keeps the same numbering
enum StampFamily : int32_t {
  kStampGcn,          // gcn_fused.hip: [launch][block][16], clock / wall pairs at 2k, 2k + 1, halo sub-phases at 10 ..
  kStampPersistent,   // node_persistent.hip: [block][phase][8]
  kStampVmh,          // node_vmh.hip: [block][phase][8]
  kStampGat,          // gat_fused.hip: [block][16], wall clock at 11 / 12
  kStampPair,         // dense_mfma.hip, dense_pair_fwd_kernel: [block][16], the workgroup's 4th tile
  kStampPairBwd,      // dense_stream_bwd.hip, dense_pair64_bwd_kernel: [block][16], the 4th tile, hardware ids at 10 / 11
  kStampSmallDense,   // dense_small_bwd.hip: [block][8], wall clock
  kStampEdge,         // edge_mlp_fused.hip: [block][16], one steady-state tile, wall clock at 8 / 9
  kStampEdge64,       // edge_mlp64.hip: [block][16], one steady-state tile, wall clock at 14 / 15
  kStampFamilies
};

struct StampSink {
  unsigned long long *buf;   // NULL: not recorded
  int64_t words;             // capacity
  int32_t phases;            // per-phase families: phases recorded per workgroup
};

}  // namespace ngpde

#ifdef NGPDE_STAMPS

namespace ngpde {

#define NGPDE_STAMP_FIELD ::ngpde::StampSink stamps;
// what: memtime (shader clock), memrealtime (100 MHz wall clock), hw_id or xcc_id (where the workgroup runs)
#define NGPDE_STAMP(sink, w, k, what) ::ngpde::stamp_word((sink), (size_t)blockIdx.x * (w) + (k), ::ngpde::stamp_##what())
// ph = 1, 2, ...
#define NGPDE_PHASE_STAMP(sink, ph, k)                                                                                          \
  ::ngpde::stamp_word((sink), (ph) >= 1 && (ph) <= (sink).phases ? ((size_t)blockIdx.x * (sink).phases + ((ph) - 1)) * 8 + (k) \
                                                                 : SIZE_MAX,                                                    \
                      ::ngpde::stamp_memtime())
// a device function's sink (NULL in the product build)
#define NGPDE_STAMP_SINK(p) (&(p).stamps)
// the next stamp waits for v to arrive
#define NGPDE_STAMP_AFTER(v) asm volatile("" ::"v"(v))
// host: the next launch's sink (slice: the words a GCN launch writes, else 0)
#define NGPDE_STAMP_SET(kk, family, slice) (kk).stamps = ::ngpde::stamp_sink(family, slice)

__device__ __forceinline__ unsigned long long stamp_memtime() { return __builtin_amdgcn_s_memtime(); }
__device__ __forceinline__ unsigned long long stamp_memrealtime() { return __builtin_amdgcn_s_memrealtime(); }
__device__ __forceinline__ unsigned long long stamp_hw_id() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}
__device__ __forceinline__ unsigned long long stamp_xcc_id() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
  return v;
}
__device__ __forceinline__ void stamp_word(const StampSink &s, size_t idx, unsigned long long t) {
  if (threadIdx.x == 0 && s.buf && idx < (size_t)s.words) s.buf[idx] = t;
}
__device__ __forceinline__ void stamp_word(const StampSink *s, size_t idx, unsigned long long t) {
  if (s) stamp_word(*s, idx, t);
}

// host registry: what ngpde_debug_set_stamps set, per family
struct StampReg {
  unsigned long long *buf;
  int64_t words;
  int32_t n;      // launches to record (GCN), or phases per workgroup (persistent solvers)
  int32_t next;   // slices handed out
};
inline StampReg g_stamp_reg[kStampFamilies] = {};

// The GCN family hands its launches successive slices of `slice` words, one per launch, until n are handed out or the buffer is
// full; later launches are not recorded.  Every other family (slice 0) hands each launch the whole buffer.
inline StampSink stamp_sink(StampFamily f, int64_t slice) {
  StampReg &r = g_stamp_reg[f];
  if (!r.buf) return StampSink{nullptr, 0, 0};
  if (slice == 0) return StampSink{r.buf, r.words, r.n};
  if (r.next >= r.n || (r.next + 1) * slice > r.words) return StampSink{nullptr, 0, 0};
  return StampSink{r.buf + r.next++ * slice, slice, 0};
}

}  // namespace ngpde

// buf: device memory of `words` 64-bit words, or NULL to stop recording.  slots_or_phases: launches to record, each in a slice of
// its own (kStampGcn), or phases per workgroup (kStampPersistent, kStampVmh); the other families ignore it.  Weak: every stamped
// object defines it, and the diagnostic library links any subset of the sources built with the stamps.
extern "C" __attribute__((weak, visibility("default"))) int32_t ngpde_debug_set_stamps(int32_t family, unsigned long long *buf,
                                                                                        int64_t words, int32_t slots_or_phases) {
  if (family < 0 || family >= ngpde::kStampFamilies || words < 0 || slots_or_phases < 0) return NGPDE_ERR_INVALID_ARGUMENT;
  ngpde::g_stamp_reg[family] = ngpde::StampReg{buf, words, slots_or_phases, 0};
  return NGPDE_OK;
}

#else

#define NGPDE_STAMP_FIELD
#define NGPDE_STAMP(sink, w, k, what)
#define NGPDE_PHASE_STAMP(sink, ph, k)
#define NGPDE_STAMP_SINK(p) nullptr
#define NGPDE_STAMP_AFTER(v)
#define NGPDE_STAMP_SET(kk, family, slice)

#endif
