// coo_rows.h -- the by-node rows of a device COO list, shared by the files that walk a node's edges in COO order (sampling.hip:
// sample_neighbors; graph_query.hip: adjacency_list), so that both read one definition of a ROW: the COO positions grouped stably by
// target (NGPDE_DIR_IN) or source (NGPDE_DIR_OUT) with rocPRIM's LSD radix sort, as ngpde_coo_degree groups them, and a row pointer
// found by bisection.  Everything here has internal linkage; the temporaries, the launch sizing and the bisection are
// device_scratch.h's.
#pragma once

#include <algorithm>
#include <cstdint>

#include <rocprim/rocprim.hpp>

#include "common.h"
#include "device_scratch.h"

namespace ngpde {

namespace {

// the sort key of edge e: the node whose row it lies in.  Both ends are checked; a bad edge sets *bad and goes to row 0.
__global__ void row_keys_kernel(int64_t m, int64_t n, int base, int dir, const int32_t *__restrict__ s, const int32_t *__restrict__ t,
                                uint32_t *__restrict__ key, int32_t *__restrict__ iota, int32_t *__restrict__ bad) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= m) return;
  const int64_t a = (int64_t)s[e] - base, b = (int64_t)t[e] - base;
  int64_t v = dir == NGPDE_DIR_IN ? b : a;
  if (a < 0 || a >= n || b < 0 || b >= n) {
    atomicOr(bad, 1);
    v = 0;
  }
  key[e] = (uint32_t)v;
  iota[e] = (int32_t)e;
}

// rowptr[v] = the first position of the sorted row keys that is >= v, v = 0 .. n
__global__ void rowptr_kernel(int64_t n, int64_t m, const uint32_t *__restrict__ key, int32_t *__restrict__ rowptr) {
  const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v > n) return;
  rowptr[v] = (int32_t)lower_bound_dev(key, m, (uint32_t)v);
}

struct Rows {
  uint32_t *row_of = nullptr;   // [E] the node of every sorted position
  int32_t *eid = nullptr;       // [E] the COO position of every sorted position
  int32_t *rowptr = nullptr;    // [N + 1]
};

// A member of *rows that is not NULL on entry is the caller's buffer and is written in place; the others are temporaries of `sc`.
// bad: the device word an edge end outside the node range sets.
int32_t build_rows(int64_t n, int64_t m, const int32_t *s, const int32_t *t, int base, int dir, Rows *rows, int32_t *bad, Scratch &sc,
                   hipStream_t stream) {
  uint32_t *key = nullptr;
  int32_t *iota = nullptr;
  int32_t st;
  if ((st = sc.get(&key, (size_t)m)) || (!rows->row_of && (st = sc.get(&rows->row_of, (size_t)m))) || (st = sc.get(&iota, (size_t)m)) ||
      (!rows->eid && (st = sc.get(&rows->eid, (size_t)m))) || (!rows->rowptr && (st = sc.get(&rows->rowptr, (size_t)n + 1))))
    return st;
  hipLaunchKernelGGL(row_keys_kernel, dim3(blocks_for(m)), dim3(kB), 0, stream, m, n, base, dir, s, t, key, iota, bad);
  NGPDE_LAUNCH_CHECK("row_keys_kernel");
  const unsigned end_bit = bits_for(std::max<int64_t>(n, 2));
  auto sort = [&](void *tmp, size_t &bytes) {
    return rocprim::radix_sort_pairs(tmp, bytes, key, rows->row_of, iota, rows->eid, (size_t)m, 0u, end_bit, stream);
  };
  if ((st = with_temp(sc, sort))) return st;
  hipLaunchKernelGGL(rowptr_kernel, dim3(blocks_for(n + 1)), dim3(kB), 0, stream, n, m, rows->row_of, rows->rowptr);
  NGPDE_LAUNCH_CHECK("rowptr_kernel");
  return NGPDE_OK;
}

}  // namespace

}  // namespace ngpde
