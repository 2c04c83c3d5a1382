"""Who owns a device-resident solver plan's memory (csrc/plan_host.h), seen from outside through the C entries.

One graph for everything: 96 nodes in three 32-row tiles (test_node_gcn_forms_host.tile_count(96): every tile stages all 96 rows by
target, 80 - 86 by source, rows of at most 5 in- and 7 out-edges -- inside every cap of the three persistent plans).

  cycles         create -> forward -> backward -> destroy of the GCN plan (d = 64, relu), the GAT plan (2 heads x 32) and the VMH plan
                 (scalar state, 2 coordinates, 2-layer phi and gamma), each Tsit5 x 2 with backward; the VMH cycle ends with
                 ngpde_release_cached_memory.  After one warm-up cycle the device's free memory (torch.cuda.mem_get_info) is read
                 after each of three further cycles: the three readings are equal.  (The same loop on the commit before plan_host.h,
                 whose destroys listed every pointer by hand, reads three equal values as well: no drift is allowed for.)
  late failure   ngpde_node_gcn2_create_batch(members = 2, d = 128): no persistent plan takes d = 128 (node_persistent_mode and
                 node_persistent_hub_possible return at d != 64), so the create allocates every buffer of the replayed plan and is
                 refused last, for the members: NGPDE_ERR_UNSUPPORTED, *out NULL, ngpde_last_error() that refusal's text and not a
                 later one, free memory as before the call.
  early refusal  GAT heads = 3, VMH hd = 2 (NGPDE_ERR_UNSUPPORTED); tableau 7 for the three creates and ngpde_ode_create
                 (NGPDE_ERR_INVALID_ARGUMENT); *out NULL every time.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from ngpde_amd import _lib
from ngpde_amd.plans import _ode_desc
from test_edge_mlp_forms_gpu import _release_graphs, graph  # noqa: F401
from test_gcn_gpu import needs_persistent_plan
import test_node_gcn_forms_gpu as G
import test_node_gcn_forms_host as H
import test_node_vmh_forms_gpu as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 96
NOT_NULL = 0x1000        # what *out holds before a refused create: the create must overwrite it with NULL


@pytest.fixture(autouse=True)
def _persistent_plan(monkeypatch):
    needs_persistent_plan(monkeypatch)


def gcn_graph():
    g = G.make_handle("N=96", lambda: H.tile_count(N))
    assert g.geo["n_tiles"] == 3 and H.fits(g.geo)
    return g


def tile_graph():
    g = graph(("plan memory", N), lambda: V.VmhGraph(*H.tile_count(N)))
    assert g.n_tiles == 3 and g.fits_both()
    return g


def vmh_model():
    return V.tutorial(2, pd=2, width=16, msg=8)


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


# ---- one cycle per plan ------------------------------------------------------------------------------------------------------------

def gcn_cycle():
    g = gcn_graph()
    params, u0, R = H.draw(N, 64, 11)
    flags, _ = G.run_plan(g, 64, "relu", "tsit5", 2, params, u0, R, solves=1)
    assert flags & G.PFWD and flags & G.PBWD


def gat_cycle():
    g, lib, heads, c = tile_graph(), _lib.load(), 2, 32
    assert lib.ngpde_node_gat_supported(g.ptr, 64, heads, c) == 1
    rng = np.random.default_rng(21)
    dv = lambda a: torch.as_tensor(a.astype(np.float32), device=DEV)
    wt, a, b = dv(rng.normal(size=(64, 64)) * 1.5 / 8), dv(rng.normal(size=(heads, 2 * c)) / np.sqrt(c)), dv(0.1 * rng.normal(size=64))
    u0, ones = dv(rng.normal(size=(N, 64))), torch.ones(N, 64, device=DEV)
    uT, du0, gw, ga, gb = (torch.empty_like(v) for v in (u0, u0, wt, a, b))
    plan, stream, f = C.c_void_p(), _lib.current_stream(), C.c_int32(-1)
    _lib.check(lib.ngpde_node_gat_create(g.ptr, heads, c, 0.2, _lib.ACT["tanh"], _lib.TABLEAU["tsit5"], 2, 0.05, 1, C.byref(plan)))
    try:
        _lib.check(lib.ngpde_node_gat_forward(plan, _lib.ptr(u0), _lib.ptr(wt), _lib.ptr(a), _lib.ptr(b), _lib.ptr(uT), stream))
        _lib.check(lib.ngpde_node_gat_backward(plan, _lib.ptr(wt), _lib.ptr(a), _lib.ptr(ones), _lib.ptr(du0), _lib.ptr(gw), _lib.ptr(ga),
                                               _lib.ptr(gb), stream))
        _lib.check(lib.ngpde_node_gat_fault(plan, stream, C.byref(f)))
        assert f.value == 0 and bool(torch.isfinite(uT).all()) and bool(torch.isfinite(du0).all())
    finally:
        torch.cuda.synchronize()
        _lib.check(lib.ngpde_node_gat_destroy(plan))


def vmh_cycle():
    g, m = tile_graph(), vmh_model()
    u0, R = V.inputs(g, 3)
    V.run_plan(g, m, "mean", "tsit5", 2, u0, R)
    _lib.load().ngpde_release_cached_memory()


@pytest.mark.parametrize("cycle", [gcn_cycle, gat_cycle, vmh_cycle], ids=["gcn", "gat", "vmh"])
def test_cycles_return_every_byte(cycle):
    cycle()                                  # warm-up: torch's allocator, the handle, the library's per-process tables
    readings = []
    for _ in range(3):
        cycle()
        readings.append(free_bytes())
    print(f"\n[plan memory] {cycle.__name__}: free bytes after cycles 2 - 4: {readings}")
    assert readings[0] == readings[1] == readings[2], readings


# ---- refusals ----------------------------------------------------------------------------------------------------------------------

def test_create_refused_after_its_allocations_frees_them():
    g, lib = gcn_graph(), _lib.load()
    args = (2, 128, _lib.ACT["relu"], _lib.TABLEAU["tsit5"], 2, H.DT, 1)
    lib.ngpde_node_gcn2_create_batch(g.ptr, *args, C.byref(C.c_void_p()))        # (warm-up: what the first call of a process sets up)
    before = free_bytes()
    plan = C.c_void_p(NOT_NULL)
    st = lib.ngpde_node_gcn2_create_batch(g.ptr, *args, C.byref(plan))
    msg = lib.ngpde_last_error().decode()
    after = free_bytes()
    print(f"\n[plan memory] late refusal: status {st}, free {before} -> {after}, message: {msg}")
    assert st == _lib.ERR_UNSUPPORTED and plan.value is None
    assert "member-by-member solve exists for the persistent plan only" in msg
    assert after == before


def test_creates_refuse_early_with_todays_codes():
    g, lib, m = tile_graph(), _lib.load(), vmh_model()
    pos = torch.as_tensor(g.positions(m.pd), device=DEV)
    tsit5, relu = _lib.TABLEAU["tsit5"], _lib.ACT["relu"]

    def gat(heads, c, tableau, out):
        return lib.ngpde_node_gat_create(g.ptr, heads, c, 0.2, relu, tableau, 2, 0.05, 1, out)

    def vmh(hd, tableau, out):
        return lib.ngpde_node_vmh_create(g.ptr, hd, m.pd, _lib.ptr(pos), *m.abi_shape(), _lib.AGGR["mean"], tableau, 2, 0.05, 1, out)

    def gcn(tableau, out):
        return lib.ngpde_node_gcn2_create(gcn_graph().ptr, 64, relu, tableau, 2, H.DT, 1, out)

    def ode(tableau, out):
        d = _ode_desc(_lib.RHS_GCN2, "tsit5", 2, H.DT, 1, width=64, act=relu)
        d.tableau = tableau
        return lib.ngpde_ode_create(gcn_graph().ptr, C.byref(d), out, None)

    cases = [("GAT heads = 3", lambda o: gat(3, 16, tsit5, o), _lib.ERR_UNSUPPORTED),
             ("VMH hd = 2", lambda o: vmh(2, tsit5, o), _lib.ERR_UNSUPPORTED),
             ("GCN tableau 7", lambda o: gcn(7, o), _lib.ERR_INVALID_ARGUMENT),
             ("GAT tableau 7", lambda o: gat(2, 32, 7, o), _lib.ERR_INVALID_ARGUMENT),
             ("VMH tableau 7", lambda o: vmh(1, 7, o), _lib.ERR_INVALID_ARGUMENT),
             ("ODE tableau 7", lambda o: ode(7, o), _lib.ERR_INVALID_ARGUMENT)]
    for what, call, code in cases:
        out = C.c_void_p(NOT_NULL)
        assert call(C.byref(out)) == code, what
        assert out.value is None, what
