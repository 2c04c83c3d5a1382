// plan_host.h -- what a device-resident solver plan is on the host: one base (ResidentPlan) that owns the plan's device memory
// (DeviceBlocks) and its hand-off state (NodePersist), the three plans derived from it, and the checks their entries share.
// A create builds its plan in a std::unique_ptr, allocates through p->mem.take, returns at the first failure (the plan's destructor
// frees whatever it holds by then and touches no error text) and releases the pointer into *out at the end.
// A new right-hand side: derive a plan from ResidentPlan here, put its create / forward / backward entries in a file of their own
// beside node_gat_plan.hip, build its tables with rk_tableau.h, and add its case to api_ode.hip.
#pragma once

#include <algorithm>
#include <memory>
#include <new>

#include "common.h"
#include "rk_tableau.h"

namespace ngpde {

#define NGPDE_TRY(expr)                   \
  do {                                    \
    const int32_t _st = (expr);           \
    if (_st != NGPDE_OK) return _st;      \
  } while (0)

// An owning list of device allocations: what take() handed out is freed by the destructor.
class DeviceBlocks {
 public:
  DeviceBlocks() = default;
  DeviceBlocks(const DeviceBlocks &) = delete;
  DeviceBlocks &operator=(const DeviceBlocks &) = delete;
  ~DeviceBlocks() { for (void *b : blocks_) (void)hipFree(b); }
  // *p = `count` elements of T (at least 256 bytes, so an empty array is still a pointer a kernel may be handed), zeroed on request
  template <class T>
  int32_t take(T **p, size_t count, bool zero = false) {
    *p = nullptr;
    const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    void *b = nullptr;
    NGPDE_HIP_CHECK(hipMalloc(&b, bytes));
    blocks_.push_back(b);
    *p = static_cast<T *>(b);
    if (zero) NGPDE_HIP_CHECK(hipMemset(b, 0, bytes));
    return NGPDE_OK;
  }
  // the block leaves the list (the caller frees or parks it); a pointer the list does not hold is left alone
  void give_up(const void *ptr) { blocks_.erase(std::remove(blocks_.begin(), blocks_.end(), ptr), blocks_.end()); }

 private:
  std::vector<void *> blocks_;
};

struct ResidentPlan {
  const ngpde_graph *g = nullptr;
  int S = 0, n_steps = 0;
  int members = 1;       // > 1: a block-diagonal batch of `members` graphs with this structure (arrays are [members][...])
  bool with_bwd = false;
  bool solved = false;   // a forward solve has filled the tape
  NodePersist persist;   // wait lists, flags, abort / fault words (node_persistent_setup)
  size_t tape_bytes = 0;
  DeviceBlocks mem;      // every device array of the plan except what `persist` holds (not copyable, so no plan is)
  virtual ~ResidentPlan() { node_persistent_free(&persist); }
};

// The arguments every create shares (all NGPDE_ERR_INVALID_ARGUMENT); *out is NULL afterwards.  A create without an activation or a
// batch passes NGPDE_ACT_IDENTITY / 1.
template <class Plan>
int32_t plan_check_create(const char *fn, const ngpde_graph *g, Plan **out, int tableau, int n_steps, int act, int members) {
  NGPDE_REQUIRE(g != nullptr && out != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: NULL argument", fn);
  *out = nullptr;
  NGPDE_REQUIRE(members >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: members >= 1 required (got %d)", fn, members);
  NGPDE_REQUIRE(tableau == NGPDE_TABLEAU_EULER || tableau == NGPDE_TABLEAU_TSIT5, NGPDE_ERR_INVALID_ARGUMENT, "%s: unknown tableau %d", fn, tableau);
  NGPDE_REQUIRE(n_steps >= 1, NGPDE_ERR_INVALID_ARGUMENT, "%s: n_steps >= 1 required (got %d)", fn, n_steps);
  NGPDE_REQUIRE(act >= NGPDE_ACT_IDENTITY && act <= NGPDE_ACT_SOFTPLUS, NGPDE_ERR_INVALID_ARGUMENT, "%s: unknown activation code %d", fn, act);
  return NGPDE_OK;
}

// *fault = 1 when a launch of the plan gave up waiting.  A plan without the word (the replayed GCN plan) has nothing to wait for:
// 0, without a synchronisation.
inline int32_t plan_fault(const char *fn, const ResidentPlan *p, ngpde_stream_t stream, int32_t *fault) {
  NGPDE_REQUIRE(p != nullptr && fault != nullptr, NGPDE_ERR_INVALID_ARGUMENT, "%s: NULL argument", fn);
  *fault = 0;
  if (!p->persist.fault_host) return NGPDE_OK;
  NGPDE_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *fault = *p->persist.fault_host ? 1 : 0;
  return NGPDE_OK;
}

// forward / backward entries: a plan whose sticky fault word is set launches nothing more
#define NGPDE_REQUIRE_LIVE(fn, plan)                                                                                             \
  NGPDE_REQUIRE(!((plan)->persist.fault_host && *(plan)->persist.fault_host), NGPDE_ERR_STATE,                                   \
                "%s: an earlier launch of this plan gave up waiting for its neighbours (its outputs are NaN): another kernel "   \
                "held the compute units or another process's solve shared the device; destroy it and create a new plan", fn)

}  // namespace ngpde

/* ---- Chain(GCNConv(d => d), GCNConv(d => d)) (node.hip) ------------------------------------------------------------------------ */
struct ngpde_node : ngpde::ResidentPlan {
  int d = 0, act = 0;
  // du < d: a WIDENED plan -- the caller's state and parameters are du wide (16 or 32) and run zero-padded on the 64-wide persistent
  // kernels (a phase of those is a latency floor, not a byte count, so the padding is free where a native narrow kernel would sit on the
  // same floor); padded columns of u stay decoupled from the real ones because the padded rows AND columns of W are zero
  int du = 0;
  float dt = 0.f;
  bool needs_z = false;
  ngpde::Tableau tb;
  int64_t n = 0;
  size_t row_elems = 0;  // n * d
  size_t all_elems = 0;  // members * row_elems: the persistent launches solve the members one after the other (u0 / uT / du0: [members * n][d])
  int nb = 0;            // workgroups of the fused kernels (= slabs)
  int slots = 0;         // tape slots per stage evaluation

  float *u = nullptr, *ustage = nullptr, *u0keep = nullptr;
  float *w1 = nullptr, *b1 = nullptr, *w2 = nullptr, *b2 = nullptr;
  float *tape = nullptr;
  // relu with backward: the pullback needs only the sign of z, so each evaluation keeps two aggregated inputs on the tape
  // plus two 4-bit-per-value masks; the layer outputs live in 2 S buffers that every step re-uses
  bool mask_mode = false;
  // pre-scaled form: u, the stage inputs, the layer outputs and the adjoint products g1 / g2 are held multiplied by c[row]
  // (u~ = c .* u), so that no kernel scales a row while staging it and the halo rows go to LDS by DMA; lambda and the
  // stage adjoints are derivatives with respect to u~.  u0 is scaled on entry, u(T) and du0 on exit.
  bool pre = false;
  float *ybuf = nullptr;         // [S][2][row_elems]
  uint8_t *masks = nullptr;      // [n_steps][S][2][mask_bytes]
  size_t mask_bytes = 0;
  float *lam = nullptr, *g1 = nullptr, *g2 = nullptr;
  std::vector<float *> ubar;
  float *slabs = nullptr;
  size_t slab_bytes = 0;
  float *slab_dw1 = nullptr, *slab_db1 = nullptr, *slab_dw2 = nullptr, *slab_db2 = nullptr;
  float *dw1 = nullptr, *db1 = nullptr, *dw2 = nullptr, *db2 = nullptr;

  // Persistent form (node_persistent.hip): the whole forward solve / the whole adjoint as ONE launch each, tiles
  // synchronised by per-tile phase flags.  Chosen when the graph is one co-resident wave of tiles (<= 2 per CU), d = 64,
  // relu (adjoint), unweighted, pre-scaled form available; NGPDE_NO_PERSISTENT=1 turns it off.  A plan is persistent in every
  // direction it has, or in none.
  bool persistent = false;
  bool hub = false;          // ... in the hub geometry (graphs whose tiles do not fit the handle's halo lists)
  // persistent adjoint of an activation other than relu: the tape holds the aggregated inputs (first half) and the pre-activations
  // (second half, `ztape`), two rows per stage evaluation each, indexed like the relu plan's tape
  bool ztape_mode = false;
  float *ztape = nullptr;
  ngpde::OwnFirst of;        // the plan's own-first slot tables (common.h): every kernel of the plan, persistent or replayed, reads them
  bool has_of = false;
  float *pbuf = nullptr;     // layer-1 output exchanged between tiles in the persistent forward
  // a batch (members > 1) runs two members at a time per workgroup (node_persistent.hip, "slots"): the exchanged arrays
  // (ustage, pbuf, g1, g2) hold one [N][d] array per slot, pubar is the adjoint's stage-adjoint scratch [2][5][N][d]
  bool interleave = false;
  bool pair = false;         // ONE member, two tiles per workgroup (graphs of up to twice the co-resident tile count)
  int ktiles = 0;            // > 0: tile rounds -- ktiles tiles per workgroup taking turns (larger graphs still); kstate = their u, k_j rows
  float *kstate = nullptr;
  float *pubar = nullptr;

  hipStream_t cap_stream = nullptr;
  hipGraph_t fwd_graph = nullptr, bwd_graph = nullptr;
  hipGraphExec_t fwd_exec = nullptr, bwd_exec = nullptr;
  // The plan owns ONE tape: a second forward overwrites what the first one's backward needs.  Every forward stamps a new
  // generation; a caller that may interleave solves (autograd) records it and has it checked before the backward.
  uint64_t generation = 0;
  bool backward_pending = false;
  int fwd_launches = 0, bwd_launches = 0;

  // tape slot k of (step, stage): 0 = A1 (aggregated input of layer 1), 1 = Y1, 2 = A2, 3 = Y2 = k_i,
  // 4 = Z1, 5 = Z2 (only for activations whose derivative needs the pre-activation)
  float *slot(int step, int stage, int k) const {
    const int s = with_bwd ? step : 0;
    if (mask_mode) {
      if (k == 1 || k == 3) return ybuf + ((size_t)stage * 2 + (k == 3 ? 1 : 0)) * row_elems;
      return tape + ((size_t)(s * tb.S + stage) * 2 + (k == 2 ? 1 : 0)) * row_elems;
    }
    return tape + ((size_t)(s * tb.S + stage) * slots + k) * row_elems;
  }
  uint8_t *mask_slot(int step, int stage, int layer) const {
    return masks + ((size_t)(step * tb.S + stage) * 2 + (layer - 1)) * mask_bytes;
  }
  ~ngpde_node() override;    // the HIP graphs, the capture stream and the own-first tables
};

/* ---- one GAT-style layer (node_gat_plan.hip; kernels: gat_fused.hip) ----------------------------------------------------------- */
struct ngpde_node_gat : ngpde::ResidentPlan {
  int heads = 0, c = 0, act = 0;
  float slope = 0.2f;
  float *cf = nullptr, *cb = nullptr;       // device coefficient tables [(S + 1)][8], [S][8]
  float *xs = nullptr, *yz = nullptr, *alpha = nullptr, *kbuf = nullptr;
  float *ubar = nullptr, *dzbuf = nullptr, *dscore = nullptr, *dal = nullptr, *slabs = nullptr;
  int *xpad = nullptr;
  size_t row_elems = 0, alpha_elems = 0;
};

/* ---- VMHConv(phi, gamma) (node_vmh_plan.hip; kernels: node_vmh.hip) ------------------------------------------------------------- */
struct ngpde_node_vmh : ngpde::ResidentPlan {
  ngpde::VmhShape shape;
  float *pos = nullptr, *cf = nullptr, *cb = nullptr, *x = nullptr;         // x: [2][N] exchanged stage input
  float *state = nullptr;                                                     // [16][N] tile rounds: per-node state between turns
  int *srcpos = nullptr, *srcdeg = nullptr;                                   // schedule-ordered by-source positions (launch_vmh_srcpos)
  float *tape_phi = nullptr, *tape_gam = nullptr, *dz_phi = nullptr, *dz_gam = nullptr, *dsrc = nullptr;
  float *partial = nullptr, *dwpad = nullptr;                                // weight-pullback workspace; [64 x 64 + 64] padded result
  size_t partial_floats = 0;
  size_t tape_cap[4] = {0, 0, 0, 0};   // capacity in floats of tape_phi, tape_gam, dz_phi, dz_gam (a block from the pool may be larger than the need)
  int tape_dev = 0;                    // the device they were allocated on
  ~ngpde_node_vmh() override;          // parks the four tapes (node_vmh_plan.hip: tape_pool_give)
};
