// device_scratch.h -- the host-side kit of the files that work on device lists (graph_device.hip, graph_ops.hip, graph_edit.hip,
// graph_query.hip, graph_traverse.hip, graph_matrix.hip, sampling.hip, neighbors.hip, readout.hip; coo_compact.h and coo_rows.h stand on it): the
// temporaries of one call, the launch sizing, the rocPRIM size-query-then-run call, the eight flag words of a call with their one
// read-back, the word that names the smallest offending id, the argument checks of a COO list, and the bisection the kernels share.  Everything here has internal linkage.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include <hip/hip_runtime.h>

#include "common.h"

namespace ngpde {

namespace {

constexpr int kB = 256;
inline unsigned blocks_for(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + kB - 1) / kB); }

inline unsigned bits_for(unsigned long long n) {   // bits that hold every value below n
  unsigned b = 1;
  while (b < 64 && (1ull << b) < n) ++b;
  return b;
}

// max(count, 1) elements the caller owns; *p is NULL after a failure
template <class T>
int32_t dev_alloc(T **p, size_t count) {
  *p = nullptr;
  NGPDE_HIP_CHECK(hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T)));
  return NGPDE_OK;
}

struct Scratch {   // device temporaries of one call; freed on scope exit
  std::vector<void *> ptrs;
  ~Scratch() {
    for (void *p : ptrs) (void)hipFree(p);
  }
  template <class T>
  int32_t get(T **p, size_t count) {
    const int32_t st = dev_alloc(p, count);
    if (!st) ptrs.push_back(*p);
    return st;
  }
};

// A rocPRIM call in its two phases: call(nullptr, bytes) asks for the size of the temporary, call(tmp, bytes) runs.  temp_bytes and
// the second call by hand where one temporary serves the rounds of a loop.
template <class F>
int32_t temp_bytes(size_t *bytes, F &&call) {
  *bytes = 0;
  NGPDE_HIP_CHECK(call((void *)nullptr, *bytes));
  return NGPDE_OK;
}

template <class F>
int32_t with_temp(Scratch &sc, F &&call) {
  size_t bytes = 0;
  void *tmp = nullptr;
  int32_t st;
  if ((st = temp_bytes(&bytes, call)) || (st = sc.get((char **)&tmp, bytes))) return st;
  NGPDE_HIP_CHECK(call(tmp, bytes));
  return NGPDE_OK;
}

// ---- the device flag words of one call: each file names its own (an enum below kFlagWords) ---------------------------------------
constexpr int kFlagWords = 8;

int32_t new_flags(Scratch &sc, int32_t **flags, hipStream_t stream) {
  unsigned long long *words = nullptr;   // (allocated as 64-bit words: graph_query.hip reads words 0 and 1 as one)
  if (int32_t st = sc.get(&words, kFlagWords / 2)) return st;
  *flags = reinterpret_cast<int32_t *>(words);
  NGPDE_HIP_CHECK(hipMemsetAsync(*flags, 0, kFlagWords * sizeof(int32_t), stream));
  return NGPDE_OK;
}

int32_t read_flags(const int32_t *flags, int32_t *h, hipStream_t stream) {   // (synchronises: the temporaries may be freed after it)
  NGPDE_HIP_CHECK(hipMemcpyAsync(h, flags, kFlagWords * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
  return NGPDE_OK;
}

// `copies`: how many copies of every edge the call sorts (2 when it symmetrises)
int32_t check_coo(const char *fn, int64_t n_nodes, int64_t n_edges, const int32_t *s, const int32_t *t, int64_t copies = 1) {
  NGPDE_REQUIRE(n_nodes >= 0 && n_edges >= 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: negative size (n_nodes %lld, n_edges %lld)", fn,
                (long long)n_nodes, (long long)n_edges);
  NGPDE_REQUIRE(n_nodes <= 0x7fffffffLL, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld nodes, at most 2^31 - 1", fn, (long long)n_nodes);
  NGPDE_REQUIRE(n_edges <= 0x7fffffffLL / copies, NGPDE_ERR_INVALID_ARGUMENT, "%s: %lld edges%s, at most 2^31 - 1", fn,
                (long long)(n_edges * copies), copies > 1 ? " after symmetrising" : "");
  NGPDE_REQUIRE(n_edges == 0 || (s && t), NGPDE_ERR_INVALID_ARGUMENT, "%s: s / t is NULL", fn);
  NGPDE_REQUIRE(n_edges == 0 || n_nodes > 0, NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %lld edges on a graph without nodes", fn,
                (long long)n_edges);
  return NGPDE_OK;
}

// The smallest id reported wins: the word holds the complement of the order-preserving map of the signed id to unsigned, so that
// atomicMax keeps the smallest id and 0 means "none".
__device__ __forceinline__ void report_offender(unsigned long long *word, int64_t v) {
  unsigned long long enc = (unsigned long long)v ^ (1ull << 63);
  if (enc == ~0ull) enc = ~0ull - 1;
  atomicMax(word, ~enc);
}
inline int64_t decode_offender(unsigned long long w) { return (int64_t)((~w) ^ (1ull << 63)); }

// first position of the ascending list that is >= v
template <class T>
__device__ __forceinline__ int64_t lower_bound_dev(const T *__restrict__ a, int64_t m, T v) {
  int64_t lo = 0, hi = m;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

}  // namespace

}  // namespace ngpde
