// persistent_sync.h -- host-side pieces of the tile hand-off protocol the device-resident solvers share (node_persistent.hip,
// node_vmh.hip, gat_fused.hip): the sync arena's layout and the timed launch.  The launch bracket is PersistentTurn (common.h).
#pragma once

#include <hip/hip_ext.h>

#include "common.h"

namespace ngpde {
namespace {

// wait lists (node_persistent_setup): [n_tiles][kNbrStride] tile ids, -1 padded; at most 63 entries (one lane of the polling wave
// each, lane 63 watches the abort word)
constexpr int kNbrStride = 64;

// The sync arena (NodePersist::sync): 2 n_tiles 128-byte flag lines -- slot 0's line of every tile, then slot 1's (the two-slot
// kernels: flags + slot * sync_slot_stride; VMH: one line per half tile, 2 t and 2 t + 1) -- then one line that holds the abort word.
// A flag line holds the last phase its owner published (the kernels address line t as flags + 32 * t); the arena is zeroed before
// every launch (PersistentTurn::enter).
constexpr int kFlagLine = 32;   // words per line
__host__ __device__ __forceinline__ size_t sync_slot_stride(int n_tiles) { return (size_t)n_tiles * kFlagLine; }
__host__ __device__ __forceinline__ unsigned *sync_abort_word(unsigned *sync, int n_tiles) { return sync + 2 * sync_slot_stride(n_tiles); }

// a launch timed between ev_start and ev_stop when ev_start is set (the benchmark's kernel times)
template <typename... P, typename... A>
void launch_timed(void (*kernel)(P...), dim3 grid, dim3 block, unsigned lds, hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop,
                  A... args) {
  if (ev_start) hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, ev_start, ev_stop, 0, args...);
  else hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

}  // namespace
}  // namespace ngpde
