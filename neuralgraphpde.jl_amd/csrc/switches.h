// switches.h -- every NGPDE_* environment switch the library reads, in one table (host only, plain C++17: no HIP).
//
// One row per switch: X(enumerator, "NAME", read, on, "what it selects").
//   read  Once     read on first use and cached for the life of the process
//         PerCall  read from the environment at every use (the tests flip these inside one process)
//   on    Any      on when the variable is set at all, "0" and "" included
//         One      on when the value starts with '1'
// The two rows that carry a value rather than a yes/no are read with switch_text().  DESIGN.md section 5.8 lists the same rows
// and tests/test_switches_host.py parses this table as text: keep one row per line in this format.
#pragma once

#include <atomic>
#include <cstdlib>

namespace ngpde {

// clang-format off
#define NGPDE_SWITCH_TABLE(X) \
  X(DenseNarrow,        "NGPDE_DENSE_NARROW",         Once,    Any, "Dense forward: no 128-row tiles (neither the streaming nor the wide form)") \
  X(DenseNoGemm128,     "NGPDE_DENSE_NO_GEMM128",     Once,    Any, "Dense: no 128 x 128 GEMM form, forward or backward") \
  X(DenseNoStream,      "NGPDE_DENSE_NO_STREAM",      Once,    Any, "Dense: no streaming forward kernel") \
  X(DenseNoSmallFwd,    "NGPDE_DENSE_NO_SMALL_FWD",   Once,    Any, "Dense: no one-pass forward of the small shapes") \
  X(DenseNoSmallBwd,    "NGPDE_DENSE_NO_SMALL_BWD",   Once,    Any, "Dense: no one-launch backward of the small shapes") \
  X(NoHalo,             "NGPDE_NO_HALO",              Once,    One, "GCN: the per-row global gather everywhere, no LDS-staged halo") \
  X(Roctx,              "NGPDE_ROCTX",                Once,    One, "load the roctx marker library and emit ranges without a profiler") \
  X(NoRoctx,            "NGPDE_NO_ROCTX",             Once,    One, "no roctx ranges even under a profiler") \
  X(NoMask,             "NGPDE_NO_MASK",              PerCall, Any, "solver plan: keep pre-activations instead of ReLU bit masks") \
  X(NoPrescale,         "NGPDE_NO_PRESCALE",          PerCall, Any, "solver plan: no pre-scaled (halo or hub) gather") \
  X(NoFusedGat,         "NGPDE_NO_FUSED_GAT",         PerCall, Any, "GAT attention: the primitive chain instead of the fused kernels") \
  X(NoPersistent,       "NGPDE_NO_PERSISTENT",        PerCall, One, "solvers: per-stage launches instead of the device-resident kernels") \
  X(NoTilePairs,        "NGPDE_NO_TILE_PAIRS",        PerCall, One, "persistent GCN solver: no two-tiles-per-workgroup plan") \
  X(TileRounds,         "NGPDE_TILE_ROUNDS",          PerCall, One, "persistent GCN solver: tile rounds also where tile pairs would do") \
  X(WeightedTileRounds, "NGPDE_WEIGHTED_TILE_ROUNDS", PerCall, One, "persistent GCN solver: tile rounds on weighted graphs of one tile per workgroup") \
  X(NoInterleave,       "NGPDE_NO_INTERLEAVE",        PerCall, One, "persistent GCN solver: batch members one after the other") \
  X(NoWiden,            "NGPDE_NO_WIDEN",             PerCall, One, "solver plan: no widening of a narrow state to the resident width") \
  X(NoOwnFirst,         "NGPDE_NO_OWN_FIRST",         PerCall, One, "solver plan: no own-rows-first halo tables") \
  X(DebugForceAbort,    "NGPDE_DEBUG_FORCE_ABORT",    PerCall, One, "persistent solvers: launch with the abort word set (tests of the abort path)") \
  X(NoVmhNode,          "NGPDE_NO_VMH_NODE",          PerCall, One, "VMH: the generic solver instead of the resident one") \
  X(NoVmhRounds,        "NGPDE_NO_VMH_ROUNDS",        PerCall, One, "VMH: no tile rounds beyond the resident half") \
  X(NoFusedGatLayer,    "NGPDE_NO_FUSED_GAT_LAYER",   PerCall, One, "GAT layer and solver: the composed path instead of the one-launch layer") \
  X(NoGnoMfma,          "NGPDE_NO_GNO_MFMA",          PerCall, One, "GNO: no matrix-pipe apply kernels") \
  X(NoGnoGform,         "NGPDE_NO_GNO_GFORM",         PerCall, One, "GNO: no by-target G form") \
  X(GnoMaterialize,     "NGPDE_GNO_MATERIALIZE",      PerCall, One, "GNO: materialise the per-edge kernel instead of reassociating") \
  X(NoFusedEdge,        "NGPDE_NO_FUSED_EDGE",        PerCall, One, "edge-MLP layers: primitives instead of the fused message launch") \
  X(NoFusedEdgeBwd,     "NGPDE_NO_FUSED_EDGE_BWD",    PerCall, One, "edge-MLP layers: primitives instead of the fused message pullback") \
  X(NoEdge64,           "NGPDE_NO_EDGE64",            PerCall, One, "edge-MLP layers: no 64-wide one-launch kernels") \
  X(Edge64NoDq,         "NGPDE_EDGE64_NO_DQ",         PerCall, One, "edge-MLP layers: the 64-wide pullback without its fused source gradient") \
  X(DenseNoStream2,     "NGPDE_DENSE_NO_STREAM2",     PerCall, One, "Dense: no one-launch pair and two-layer chain forwards") \
  X(DenseNoStreamBwd,   "NGPDE_DENSE_NO_STREAM_BWD",  PerCall, One, "Dense: no streaming backward, single or pair") \
  X(DeepEdgeBwd,        "NGPDE_DEEP_EDGE_BWD",        PerCall, Text, "deep edge-MLP fused pullback: 1 forces, 0 forbids, otherwise by size") \
  X(GnoGformChunk,      "NGPDE_GNO_GFORM_CHUNK",      PerCall, Text, "GNO G form: edges per chunk, 16 or the default 32")
// clang-format on

enum class Switch : int {
#define NGPDE_SWITCH_ENUM(id, name, read, on, what) id,
  NGPDE_SWITCH_TABLE(NGPDE_SWITCH_ENUM)
#undef NGPDE_SWITCH_ENUM
};

enum class SwitchRead : unsigned char { Once, PerCall };
enum class SwitchOn : unsigned char { Any, One, Text };   // Text: a value for switch_text(), not a yes/no

struct SwitchRow {
  const char *name;
  SwitchRead read;
  SwitchOn on;
  const char *what;
};

inline constexpr SwitchRow kSwitchRows[] = {
#define NGPDE_SWITCH_ROW(id, name, read, on, what) {name, SwitchRead::read, SwitchOn::on, what},
    NGPDE_SWITCH_TABLE(NGPDE_SWITCH_ROW)
#undef NGPDE_SWITCH_ROW
};
constexpr int kNumSwitches = (int)(sizeof(kSwitchRows) / sizeof(kSwitchRows[0]));

// The value of a switch as set, or null when it is unset.  Always a fresh read.
inline const char *switch_text(Switch s) { return std::getenv(kSwitchRows[(int)s].name); }

// Whether a switch is on, by its row.  A PerCall row costs one getenv and a character test.  A Once row is latched per switch on
// its first use: 0 = not read yet, 1 = off, 2 = on; two threads that race on the first read both read the environment and store the
// same byte.
inline bool switch_on(Switch s) {
  const SwitchRow &row = kSwitchRows[(int)s];
  auto read = [&row] {
    const char *e = std::getenv(row.name);
    return e && (row.on == SwitchOn::Any || e[0] == '1');
  };
  if (row.read == SwitchRead::PerCall) return read();
  static std::atomic<unsigned char> latched[kNumSwitches];
  std::atomic<unsigned char> &l = latched[(int)s];
  unsigned char v = l.load(std::memory_order_relaxed);
  if (v == 0) {
    v = read() ? 2 : 1;
    l.store(v, std::memory_order_relaxed);
  }
  return v == 2;
}

}  // namespace ngpde
