// persistent_sync.h -- the tile hand-off protocol the device-resident solvers share (node_persistent.hip, node_vmh.hip, gat_fused.hip).
// Host half: the sync arena's layout, the timed launch and the residency of a set of kernels (the launch bracket is PersistentTurn,
// common.h; the wait lists and the rest of the shared host side: persistent_plan.hip).  Device half: the bounded
// flag poll and the publish; tile_wait_arrive, vmh_wait, gat_wait and the three *_publish build their addresses and call these.
#pragma once

#include <algorithm>

#include <hip/hip_ext.h>

#include "common.h"
#include "device_utils.h"

namespace ngpde {
namespace {

// wait lists (node_persistent_setup): [n_tiles][kNbrStride] tile ids, -1 padded; at most 63 entries (one lane of the polling wave
// each, lane 63 watches the abort word)
constexpr int kNbrStride = 64;

// The sync arena (NodePersist::sync): 2 n_tiles 128-byte flag lines -- slot 0's line of every tile, then slot 1's (the two-slot
// kernels: flags + slot * sync_slot_stride; VMH: one line per half tile, 2 t and 2 t + 1) -- then one line that holds the abort word.
// A flag line holds the last phase its owner published (the kernels address line t as flag_line(flags, t)); the arena is zeroed
// before every launch (PersistentTurn::enter).
constexpr int kFlagLine = 32;   // words per line
template <typename W> __host__ __device__ __forceinline__ W *flag_line(W *flags, int line) { return flags + kFlagLine * line; }
__host__ __device__ __forceinline__ size_t sync_slot_stride(int n_tiles) { return (size_t)n_tiles * kFlagLine; }
__host__ __device__ __forceinline__ unsigned *sync_abort_word(unsigned *sync, int n_tiles) { return sync + 2 * sync_slot_stride(n_tiles); }

// a launch timed between ev_start and ev_stop when ev_start is set (the benchmark's kernel times)
template <typename... P, typename... A>
void launch_timed(void (*kernel)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop,
                  A... args) {
  if (ev_start) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, ev_start, ev_stop, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

// Workgroups of `block` threads and `lds` dynamic LDS bytes the current device keeps resident at once whichever of `kernels` they
// run: CUs x the least occupancy over the list.  Every workgroup of a persistent launch spin-waits on its neighbours, so a plan's
// grid must fit this number taken over EVERY kernel the plan can later launch: a solver's "does it fit" query and its launcher read
// the same kernel table.  0: a query failed.
inline int resident_workgroups(const std::vector<const void *> &kernels, int block, size_t lds) {
  int dev = 0, cus = 0, occ = kernels.empty() ? 0 : 1 << 30;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
  for (const void *kernel : kernels) {
    int o = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, kernel, block, lds) != hipSuccess) o = 0;
    occ = std::min(occ, o);
  }
  return cus * occ;
}

// ---- device half ----------------------------------------------------------------------------------------------------------
// What wave 0's lane watches first: lane 63 the abort word, another lane the flag line `line` of its wait-list entry (none: line < 0).
__device__ __forceinline__ const unsigned *watch_line(const unsigned *flags, int line) { return line >= 0 ? flag_line(flags, line) : nullptr; }
__device__ __forceinline__ const unsigned *watch_first(const unsigned *abort_word, const unsigned *flags, int lane, int line) {
  return lane == 63 ? abort_word : watch_line(flags, line);
}

// A waiting wave gives up after ~2 s of the 100 MHz counter (a whole solve takes milliseconds) and raises the abort word itself.
constexpr unsigned long long kWaitTicks = 200000000ull;

// The poll, run by ONE wave: until every watched flag line shows a phase >= need.  Each lane watches NA lines, a[0] .. a[NA - 1]
// (null: nothing to watch, counts as reached); lane 63's a[0] is the abort word, and a non-zero abort word ends the poll with the
// verdict "aborted".  The verdict goes to *s_ok (lane 0); the caller's barrier makes it visible to the workgroup.
// Two waits of the GCN solver keep a loop of their own (persistent_gcn_tile.h), the same statements: tile_wait_primed_arrive, whose
// first sample is the caller's (poll_issue) and whose loads therefore sit behind the sleep, and hub_wait (four lines per lane).  Through
// this loop their kernels -- the headline's adjoint among them -- measured 0.3 - 1.5 % slower (profiles/r11_a_handoff_once.txt).
//  - All of a round's loads are issued before the first test, and there is ONE round of loads per poll: a second dependent load
//    per round would double the polling period, which is the granularity a published flag is seen with.
//  - s_sleep(1): 2 / 4 / 8 measured, no difference beyond run-to-run noise; the polling period is not what a phase waits for.
//  - What the stamps of tools/stamps.py interleaved say about the hand-off: a flag store is seen by a poll from another XCD
//    ~3-4 k cycles (1.2-1.5 us) after it was issued, a poll or a gather is a ~1.5 k-cycle round trip, the drain in front of the
//    flag ~1 k: with only two slots the ~2.4 us of hand-off exceed the ~1.7 us of work the other slot offers in the forward
//    kernel -- wherever the look is put, the difference is waited for.
template <int NA>
__device__ __forceinline__ void flag_poll(const unsigned *const (&a)[NA], unsigned *abort_word, int lane, unsigned need, int *s_ok) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  bool ok = true;
  for (unsigned it = 1;; ++it) {
    unsigned f[NA];
#pragma unroll
    for (int k = 0; k < NA; ++k) {
      f[k] = need;
      if (a[k]) f[k] = __hip_atomic_load(a[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    bool reached = lane == 63 || f[0] >= need;
#pragma unroll
    for (int k = 1; k < NA; ++k) reached = reached && f[k] >= need;
    if (__any((int)(lane == 63 && f[0] != 0))) { ok = false; break; }   // somebody gave up
    if (__all((int)reached)) break;
    if ((it & 1023u) == 0 && __builtin_amdgcn_s_memrealtime() - t0 > kWaitTicks) {
      if (lane == 0) __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      ok = false;
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  if (lane == 0) *s_ok = ok ? 1 : 0;
}

// The publish: every storing wave drains, the workgroup meets, ONE lane stores the phase to flag line `line` (Guideline 16, R1);
// a workgroup that owns two lines (VMH's whole tile) stores the second from the next lane.
__device__ __forceinline__ void flag_publish(unsigned *flags, int tid, unsigned ph, int line, int line2 = -1) {
  wait_vmcnt0();
  __syncthreads();
  if (tid == 0) __hip_atomic_store(flag_line(flags, line), ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (line2 >= 0 && tid == 1) __hip_atomic_store(flag_line(flags, line2), ph, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace
}  // namespace ngpde
