// coo_compact.h -- the stable compaction that the files that rewrite a device COO list share (graph_ops.hip, graph_edit.hip,
// graph_query.hip, graph_matrix.hip):
//   flags -> exclusive scan -> scatter: kept edges stay in COO order
// so that ngpde_coo_compact, ngpde_coo_remove_edges and ngpde_coo_intersect run one definition of it.  The temporaries and the rest of
// the host-side kit are device_scratch.h's.  Everything here has internal linkage.
#pragma once

#include <cstdint>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "device_scratch.h"

namespace ngpde {

namespace {

template <class T>
int32_t scan_i32(bool inclusive, const int32_t *in, T *out, size_t count, Scratch &sc, hipStream_t stream) {
  return with_temp(sc, [&](void *tmp, size_t &bytes) {
    return inclusive ? rocprim::inclusive_scan(tmp, bytes, in, out, count, rocprim::plus<int32_t>(), stream)
                     : rocprim::exclusive_scan(tmp, bytes, in, out, 0, count, rocprim::plus<int32_t>(), stream);
  });
}

// edge e with keep[e] != 0 goes to slot pos[e] (pos = the exclusive scan of keep), renumbered through `relabel` if given; *count =
// the number of kept edges
__global__ void compact_kernel(int64_t m, int base, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                               const int32_t *__restrict__ relabel, const int32_t *__restrict__ keep, const int32_t *__restrict__ pos,
                               int32_t *__restrict__ s_out, int32_t *__restrict__ t_out, int64_t *__restrict__ kept,
                               int32_t *__restrict__ count) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int32_t p = pos[e];
  if (keep[e]) {   // (a kept edge has both ends in range)
    const int32_t a = s[e] - base, b = t[e] - base;
    s_out[p] = (relabel ? relabel[a] : a) + base;
    t_out[p] = (relabel ? relabel[b] : b) + base;
    kept[p] = e;
  }
  if (e == m - 1) *count = p + keep[e];
}

// the scan and the scatter over m > 0 edges whose keep flags (0 / 1) are written; `pos` is a temporary of m words
int32_t compact_flagged(int64_t m, int base, const int32_t *s, const int32_t *t, const int32_t *relabel, const int32_t *keep, int32_t *pos,
                        int32_t *s_out, int32_t *t_out, int64_t *kept, int32_t *count, Scratch &sc, hipStream_t stream) {
  if (int32_t st = scan_i32(false, keep, pos, (size_t)m, sc, stream)) return st;
  hipLaunchKernelGGL(compact_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, base, s, t, relabel, keep, pos, s_out, t_out, kept, count);
  NGPDE_LAUNCH_CHECK("compact_kernel");
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde
