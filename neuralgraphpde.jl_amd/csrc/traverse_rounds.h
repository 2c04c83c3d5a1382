// traverse_rounds.h -- what the round-synchronous traversals share (graph_traverse.hip: components, hop distances; graph_paths.hip:
// weighted shortest paths; included by these two only).  A call enqueues ROUNDS, kernel boundaries are the only synchronisation,
// and nothing here but the source check's report_offender reads and writes a word in one step: every flag is a plain store of a
// value all its writers agree on.  The control block is the last 256 bytes of a call's workspace; the host reads its first 16 words.
//
// THE ROTATION: how a launch learns without a read-back that the round before it changed nothing.  Three words at `base` serve the
// rounds 1, 2, ...; round r owns word r % 3.  Its launch READS the word of round r - 1 (0: that round changed nothing, the answer
// is final, the whole grid exits at once and so does every launch after it), CLEARS the word of round r + 1 from one lane (no launch
// in flight reads or sets that one; with two words a lane of round r that sets its own could run before the clearing lane) and SETS
// its own where a lane changed something.  Word 0 starts at 1, "round 0 changed something", so that round 1 runs.
//
// THE HUB-ROW WALK: a lane per node walks its row entry by entry, but the rows of a wave that have the kernel's threshold of entries
// or more are taken one after the other by the WHOLE wave: a ballot names them, the owner's bounds are shuffled to every lane, lane l
// takes entries l, l + 64, ... and the kernel reduces across the wave for the owner, so a hub row does not serialise on one lane.
#pragma once

#include <algorithm>
#include <cstdint>

#include "device_scratch.h"

namespace ngpde {

namespace {

typedef unsigned long long u64;

constexpr int kWave = 64;
constexpr int kPassSources = 64;                     // the sources of one pass of a separate = 1 call
constexpr size_t kCtlBytes = 256;                    // the control block
constexpr int64_t kMaxUncheckedLaunches = 1 << 20;   // what a call with check_every 0 may enqueue at most (rounds, levels)

// the control words (words 0 - 1 and 2 - 3 are ONE 64-bit word each: the smallest offending node / COO position).  cTurn: the
// rotating words of the rounds (hooked / found a new bit / lowered a distance); cMore: those of a round's compress launches
enum { cOffender = 0, cWeight = 2, cCsr = 4, cTurn = 5, cRounds = 8, cState = 9, cMore = 10, kCtlRead = 16 };

inline u64 word_of(const int32_t *h, int at) { return (u64)(uint32_t)h[at] | (u64)(uint32_t)h[at + 1] << 32; }
inline int32_t *take_ctl(Workspace &w) { return w.take<int32_t>(kCtlBytes / sizeof(int32_t)); }   // taken LAST: the block ends the workspace

__host__ __device__ __forceinline__ int round_word(int base, int r) { return base + r % 3; }
__device__ __forceinline__ void rounds_arm(int32_t *ctl, int base, int64_t i) {   // lane i of the launch that starts a sequence of rounds
  if (i < 3) ctl[base + i] = i == 0 ? 1 : 0;
}
__device__ __forceinline__ void round_mark(int32_t *ctl, int base, int r) { ctl[round_word(base, r)] = 1; }
inline bool round_marked(const int32_t *h, int base, int64_t r) { return h[round_word(base, (int)r)] != 0; }   // of the host's copy
// does round r run?  One lane of the launch also clears the word of round r + 1
__device__ __forceinline__ int round_go(int32_t *ctl, int base, int r, bool first_lane) {
  const int go = ctl[round_word(base, r + 2)];
  if (first_lane) ctl[round_word(base, r + 1)] = 0;
  return go;
}

struct HopRows {   // the rows of one direction: row v = positions ptr[v] .. ptr[v + 1] - 1 of other; ptr NULL: no such set
  const int32_t *ptr;
  const int32_t *other;
  int64_t nnz;
};

// b .. e - 1: the positions of row v; empty for a lane that is not `live`, and for pointers outside the list, which raise cCsr
__device__ __forceinline__ void row_span(const HopRows &rows, int64_t v, bool live, int64_t &b, int64_t &e, int32_t *ctl) {
  b = e = 0;
  if (!live) return;
  b = rows.ptr[v], e = rows.ptr[v + 1];
  if (b < 0 || e > rows.nnz || b > e) ctl[cCsr] = 1, b = e = 0;
}

// body(owner, wb, we), in every lane, for each lane `owner` of the wave whose row wb .. we - 1 is `wide`, in lane order.  Every lane
// of the wave must get here, those without a node included
template <class Body>
__device__ __forceinline__ void for_wide_rows(bool wide, int64_t b, int64_t e, Body body) {
  u64 todo = __ballot(wide);
  while (todo) {
    const int owner = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    body(owner, __shfl(b, owner, kWave), __shfl(e, owner, kWave));
  }
}

// dist = fill, the parents = -1; every listed source is checked here, whichever pass it belongs to (the smallest bad one is named)
template <class T>
__global__ void fill_sources_kernel(int64_t total, T fill, T *__restrict__ dist, int32_t *__restrict__ parent_eid, int32_t *__restrict__ parent,
                                    int64_t n_sources, const int64_t *__restrict__ sources, int base, int64_t n, int32_t *__restrict__ ctl) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < total) {
    dist[i] = fill;
    if (parent_eid) parent_eid[i] = -1;
    if (parent) parent[i] = -1;
  }
  if (i < n_sources) {
    const int64_t v = sources[i] - base;
    if (v < 0 || v >= n) report_offender(reinterpret_cast<u64 *>(ctl + cOffender), v);
  }
}

// where source i of the pass that starts at row `row0` keeps node v in the caller's dist (row 0 when one distance to the NEAREST is asked)
__device__ __forceinline__ size_t source_cell(int separate, int64_t row0, int64_t i, int64_t n, int64_t v) {
  return (size_t)(separate ? row0 + i : 0) * (size_t)n + (size_t)v;
}

// the sources of a pass: kPassSources with separate, else all of them.  Pass k takes min(per, n_sources - k * per) sources from k * per
inline int64_t pass_sources(int64_t n_sources, int separate) { return separate ? kPassSources : std::max<int64_t>(n_sources, 1); }

// *total = the cells of dist_out: one row of n, or a row per source
inline int32_t check_result(const char *fn, int64_t n, int64_t n_sources, int separate, const void *dist_out, int64_t *total) {
  const int64_t n_rows = separate ? n_sources : 1;
  *total = n_rows * n;
  NGPDE_REQUIRE(*total <= ((int64_t)1 << 40), NGPDE_ERR_UNSUPPORTED, "%s: %lld sources x %lld nodes: the result is too large", fn, (long long)n_rows,
                (long long)n);
  NGPDE_REQUIRE(dist_out || *total == 0, NGPDE_ERR_INVALID_ARGUMENT, "%s: dist_out is NULL", fn);
  return NGPDE_OK;
}

// what a control block read back after distance rounds reports, in the order include/ngpde.h lists the errors; `places`: what lies
// outside the lists when cCsr is raised.  (cWeight stays 0 in a call without weights, cCsr where no round ran.)
inline int32_t named_errors(const char *fn, const int32_t *h, int64_t n, const char *places) {
  NGPDE_REQUIRE(!word_of(h, cOffender), NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: sources lists node %lld, outside the %lld nodes", fn,
                (long long)decode_offender(word_of(h, cOffender)), (long long)n);
  NGPDE_REQUIRE(!h[cCsr], NGPDE_ERR_DIMENSION_MISMATCH, "%s: DimensionMismatch: %s lies outside the lists", fn, places);
  NGPDE_REQUIRE(!word_of(h, cWeight), NGPDE_ERR_INVALID_ARGUMENT,
                "%s: ArgumentError: the weight at COO position %lld is negative or NaN (weights must be >= 0; +inf and 0 are valid)", fn,
                (long long)decode_offender(word_of(h, cWeight)));
  return NGPDE_OK;
}

// The round loop of a call.  run() enqueues rounds 1 .. max_rounds of the cTurn words through launch(r), in groups of check_every with
// one read-back -- a stream synchronisation -- per group: errors(h) names what the block reports, and a round that left its word 0
// was the confirming one.  check_every 0 enqueues exactly max_rounds rounds and reads nothing back, which lets a call be captured.
// launch and errors return a status, which ends the run.
struct Rounds {
  int32_t check_every;
  const int32_t *ctl;
  hipStream_t stream;
  int64_t last = 0;       // the last round the latest run() enqueued
  bool done = false;      // ... and whether a read-back found it to confirm
  bool checked = false;   // did a read-back take place, in any run()?
  int32_t h[kCtlRead] = {};
  template <class Errors>
  int32_t read_ctl(Errors errors) {   // (synchronises)
    NGPDE_HIP_CHECK(hipMemcpyAsync(h, ctl, sizeof(h), hipMemcpyDeviceToHost, stream));
    NGPDE_HIP_CHECK(hipStreamSynchronize(stream));
    checked = true;
    return errors(h);
  }
  template <class Launch, class Errors>
  int32_t run(int64_t max_rounds, Launch launch, Errors errors) {
    last = 0, done = false;
    for (int64_t r = 1; r <= max_rounds && !done; ++r) {
      if (int32_t st = launch(r)) return st;
      last = r;
      if (check_every > 0 && (r % check_every == 0 || r == max_rounds)) {
        if (int32_t st = read_ctl(errors)) return st;
        done = !round_marked(h, cTurn, r);
      }
    }
    return NGPDE_OK;
  }
  // no run() read anything back: what the launches before the rounds reported is still to be answered for
  template <class Errors>
  int32_t answer(Errors errors) { return check_every > 0 && !checked ? read_ctl(errors) : NGPDE_OK; }
};

}  // namespace

}  // namespace ngpde
