"""Every entry runs on the stream it is given (include/ngpde.h: "`stream` is a hipStream_t ... explicit stream").

torch's default stream is the legacy NULL stream, and every other GPU test of the suite runs on it: a launch with 0 where `stream` was
meant, a hipMemcpy where hipMemcpyAsync(..., stream) was meant or a read-back that synchronises the wrong stream is ordered with
everything such a test does and cannot fail there.  torch's other streams are created hipStreamNonBlocking, so the NULL stream does
not wait for them.  Here every case runs twice:

  1. expected    on the default stream: the real inputs are drawn (`Draws`, record mode), `want = case(draws)`, the device synchronised;
                 the host wall time of the run is taken with perf_counter and no synchronisation.
  2. stale       the inputs of the second run are separate device buffers of the same shapes and strides holding NaN (floats) or
                 zeros (index lists, graph ids, row pointers: zeros are a valid list for every call here, because all node ids are
                 0-based and every graph has a node 0 -- a kernel that reads them early stays inside its allocations).  The side
                 stream's share of torch's caching allocator is filled with NaN as well (blocks are kept per stream), so that an
                 intermediate the package computes on the side stream -- the packed positions of the VMH plan -- holds NaN until its
                 kernel has run, not what an earlier run left in the block.
  3. side run    under torch.cuda.stream(side): delay(); buffer.copy_(real) for every input; got = case(draws in replay mode).
                 The case builds everything inside: the GNNGraph from device COO buffers (graphops._new_graph, the maker of
                 graphs._graph_from_device_coo), handles, plans, matrices and readouts, so no Python-side cache carries real data
                 across.  A read-back inside the case (a graph build downloads its lists, a handle build synchronises) waits for
                 the delay.  graph_of(), each() and the cases therefore arm again after every read-back they know of, and a draw does
                 when it finds the delay run out: all buffers handed out so far are made stale, delay(), and copied again, all on
                 the side stream.  A well-streamed consumer never notices.
  4. comparison  side.synchronize(), then got == want BITWISE: tensors through an integer view, host values by their bytes.

delay() is torch.cuda._sleep(cycles): bounded GPU work on the current stream, calibrated once per module with two events.  Per case
it lasts the larger of 20 ms and 20 x the host wall time of step 1, at most 250 ms; the test prints it.

The control (`streams`, module scope) comes first and gates everything: ONE deliberately mis-streamed call made by the test itself,
ngpde_transpose with stream = NULL on a NaN buffer that the side stream overwrites behind the delay, must differ from the expected
result, and the same call with side.cuda_stream must match.  A stream that happens to share the NULL stream's hardware queue runs in order
with it; up to 8 of torch's streams are tried for one that does not.  If none differs the module fails: nothing below could fail either.

`Recorder` stands in for the loaded library (as test_workspace_gpu.Guarded does).  For every call made while the side stream is
current it notes the entry, asserts that the argument at the entry's ngpde_stream_t position (from include/ngpde.h) is the side
stream's handle, and notes whether the delay was still pending on entry (an event recorded behind the delay kernel has not
completed).  Every case declares the entries it must reach; tests/test_streams_host.py accounts for all of the header's.  A declared
entry must be entered at least once WHILE THE DELAY IS PENDING -- a read-back between the last draw and the call (a handle built
lazily inside the call expression) would void the case silently -- unless the case names it in `drained` with the read-back that
precedes it.  graph_of() therefore builds the handles a case needs before it arms for the last time.

Every case is bitwise reproducible between the two runs: none is compared with a tolerance.

What it found: the two "VMH plan" cases fail without the synchronisation in plans._OdePlan (the state comes back NaN in 96 of 96
elements: ngpde_ode_create copied the positions on the NULL stream before the side stream had packed them).  They build the handle
first and attach the positions afterwards, because a handle build synchronises the stream and would hide the defect.
"""
import contextlib
import ctypes as C
import os
import re
import time

import numpy as np
import pytest
import torch

import ngpde_amd as ng
from ngpde_amd import _lib, graphops, optim
from ngpde_amd import functional as F
from ngpde_amd.functional import _int_array, _ptr_array
from ngpde_amd.matrices import GraphMatrix
import composed
import test_node_gcn_forms_host as H
import test_node_vmh_forms_gpu as V
import test_workspace_gpu as W
from test_gcn_gpu import needs_persistent_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
MIN_MS, MAX_MS, WALL_FACTOR = 20.0, 250.0, 20.0


# ---- the header: where every entry takes its stream ------------------------------------------------------------------------------

def stream_positions():
    """{entry: index of its ngpde_stream_t argument} of include/ngpde.h, comments stripped as tests/test_abi.py:header_functions does"""
    src = open(os.path.join(ROOT, "include", "ngpde.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(ngpde_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;", src, flags=re.S):
        at = [k for k, a in enumerate(m.group(2).split(",")) if "ngpde_stream_t" in a]
        if at:
            assert len(at) == 1, m.group(1)
            out[m.group(1)] = at[0]
    return out


STREAM_AT = stream_positions()
# the creates that take device pointers and no stream: recorded by name (tests/test_streams_host.py asks for a solver case of each)
CREATES = ("ngpde_node_vmh_create", "ngpde_ode_create")

# entries no case reaches: at most 8, collectives that need a communicator and pure diagnostics only (tests/test_streams_host.py)
ALLOW = {
    "ngpde_grad_allreduce": "collective: needs an ngpde_comm_t of a process group (tests/test_dist_gpu.py)",
    "ngpde_grad_allreduce_adam": "collective: needs an ngpde_comm_t of a process group (tests/test_dist_gpu.py)",
    "ngpde_node_profile": "diagnostic: times a plan's launches and synchronises",
    "ngpde_node_pipeline_stats": "diagnostic: reads a plan's wait counters back",
    "ngpde_node_fault": "diagnostic: the *_fault query of the GCN plan",
    "ngpde_node_gat_fault": "diagnostic: the *_fault query of the GAT plan",
    "ngpde_node_vmh_fault": "diagnostic: the *_fault query of the VMH plan",
    "ngpde_ode_fault": "diagnostic: the *_fault query of the ngpde_ode_* plans",
}


class Recorder:
    """The loaded library, except that every call of an entry that takes a stream (and of the two stream-less creates), made while
    `expect` holds the side stream's handle, is noted in `reached` after its stream argument was compared with that handle."""

    def __init__(self, lib):
        self._lib, self.expect, self.reached, self.replay, self.behind = lib, None, [], None, set()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        at = STREAM_AT.get(name)
        if at is None and name not in CREATES:
            return fn

        def entry(*args):
            if self.expect is not None:
                if at is not None:
                    given = args[at]
                    given = getattr(given, "value", given) or 0
                    assert given == self.expect, f"{name}: stream argument {given:#x}, the current stream is {self.expect:#x}"
                self.reached.append(name)
                if self.replay.pending():          # entered while the delay in front of the inputs had not run out
                    self.behind.add(name)
            return fn(*args)
        return entry


# ---- the delay, the control -------------------------------------------------------------------------------------------------------

class Streams:
    def __init__(self):
        self.side = torch.cuda.Stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)          # (the first launch of the kernel loads it)
        torch.cuda.synchronize()
        cycles = 20_000_000
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        torch.cuda.synchronize()
        self.cycles_per_ms = cycles / a.elapsed_time(b)
        assert 1e3 < self.cycles_per_ms < 1e8, f"torch.cuda._sleep: {self.cycles_per_ms} cycles per ms"

    def delay(self, ms):
        torch.cuda._sleep(int(ms * self.cycles_per_ms))


def bits(t):
    t = t.detach().contiguous()
    if t.is_floating_point() or t.dtype == torch.bool:
        return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])
    return t


def control(st, stream_arg):
    """ngpde_transpose of a NaN buffer that the side stream fills behind a delay, launched from inside the side-stream block with
    `stream_arg`: does the result equal the transpose of the real data?"""
    lib = _lib.load()
    rows, cols = 37, 53
    real = torch.randn(rows, cols, device=DEV)
    want = real.T.contiguous()
    buf = torch.full((rows, cols), float("nan"), device=DEV)
    out = torch.full((cols, rows), -1.0, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(st.side):
        st.delay(50.0)
        buf.copy_(real)
        _lib.check(lib.ngpde_transpose(rows, cols, _lib.ptr(buf), _lib.ptr(out), stream_arg))
        pending = not st.side.query()
    st.side.synchronize()
    torch.cuda.synchronize()
    return torch.equal(bits(out), bits(want)), pending, bool(torch.isnan(out).any())


@pytest.fixture(scope="module")
def streams():
    st = Streams()
    torch.manual_seed(7)
    # The runtime multiplexes its streams onto a few hardware queues, and two streams that share one run in order: late in a long process
    # a new stream can land on the NULL stream's queue.  Such a stream cannot show anything, so up to 8 of torch's streams are tried.
    for attempt in range(8):
        wrong, pending, nan = control(st, None)
        if nan and not wrong:
            break
        print(f"\n[streams] control: side stream {st.side.cuda_stream:#x} runs in order with the NULL stream (attempt {attempt}); trying another")
        st.side = torch.cuda.Stream()
    right, pending2, _ = control(st, st.side.cuda_stream)
    print(f"\n[streams] {st.cycles_per_ms:.0f} sleep cycles per ms; control: NULL stream equal = {wrong} (NaN visible = {nan}, delay still "
          f"pending after the call = {pending}), side stream equal = {right} (pending = {pending2})")
    if wrong or not nan:
        pytest.fail("control: ngpde_transpose launched on the NULL stream saw the data the side stream wrote behind the delay -- the NULL "
                    "stream is ordered with torch's streams on this runtime, or the delay is too short: no case of this module could fail")
    assert right, "control: ngpde_transpose launched on the side stream does not match"
    return st


# ---- the inputs of a case ---------------------------------------------------------------------------------------------------------

def poison(t):
    t.fill_(float("nan")) if t.is_floating_point() else t.zero_()


class Replay:
    """the stale buffers of the side-stream run and what puts the real data into them behind a delay"""

    def __init__(self, real, st, ms):
        self.real, self.st, self.ms, self.armed, self.event = real, st, ms, 0, None
        self.bufs = [torch.empty_strided(r.shape, r.stride(), dtype=r.dtype, device=r.device) for r in real]
        for b in self.bufs:
            poison(b)

    def arm(self, upto):
        with torch.no_grad():
            for b in self.bufs[:upto]:
                poison(b)
            self.st.delay(self.ms)
            self.event = torch.cuda.Event()
            self.event.record()
            for b, r in zip(self.bufs[:upto], self.real):
                b.copy_(r)
        self.armed += 1

    def pending(self):
        return not self.event.query()

    def hand_out(self, k):
        if not self.pending():            # a read-back waited for the delay: everything drawn so far goes behind a new one
            self.arm(k + 1)
        b = self.bufs[k]                  # (an alias with a version counter of its own: arm() writes through `b`, also between a forward and its backward)
        return torch.empty(0, dtype=b.dtype, device=b.device).set_(b.untyped_storage(), b.storage_offset(), b.shape, b.stride())


class Draws:
    """The inputs of one run, in the order the case asks for them.  Record mode (replay None) makes them and keeps them in `real`;
    replay mode hands out the stale buffers in the same order."""

    def __init__(self, seed, monkeypatch, replay=None):
        self.rng, self.mp, self.replay, self.real, self.k = np.random.default_rng(seed), monkeypatch, replay, [], 0

    def tensor(self, make, grad=False):
        v = make()                        # (in both modes: the generator stays in step)
        if self.replay is None:
            r = (v if torch.is_tensor(v) else torch.as_tensor(v)).to(DEV)
            self.real.append(r)
            out = r.clone()
        else:
            out = self.replay.hand_out(self.k)
        self.k += 1
        return out.requires_grad_(True) if grad else out

    def randn(self, *shape, grad=False, scale=1.0):
        return self.tensor(lambda: (self.rng.standard_normal(shape) * scale).astype(np.float32), grad)

    def rand(self, *shape, lo=0.0, hi=1.0, grad=False):
        return self.tensor(lambda: (lo + (hi - lo) * self.rng.random(shape)).astype(np.float32), grad)

    def like(self, t):
        return self.randn(*t.shape)

    def ints(self, values, dtype=torch.int32):
        return self.tensor(lambda: torch.as_tensor(np.asarray(values, dtype=np.int64)).to(dtype))

    def leaves(self, tree):
        """a parameter tree of ng.setup with every leaf drawn (its own values and strides), requiring grad"""
        return {k: (self.leaves(v) if isinstance(v, dict) else self.tensor(lambda v=v: v.detach().clone(), grad=True)) for k, v in tree.items()}

    def rearm(self):
        """everything drawn so far behind a new delay (after a read-back the case knows of)"""
        if self.replay is not None:
            self.replay.arm(self.k)


def leaves_of(tree):
    out = []
    for v in tree.values():
        out += leaves_of(v) if isinstance(v, dict) else [v]
    return out


def pulled(d, y, *leaves):
    """[y, the gradients of the leaves] for a drawn cotangent"""
    y.backward(d.like(y))
    return [y] + [l.grad for l in leaves]


def each(d, *thunks):
    """the results of the calls, each with everything drawn so far behind a new delay (the call before read something back)"""
    out = []
    for f in thunks:
        d.rearm()
        out.append(f())
    return out


def graph_of(d, s, t, n, gi=None, num_graphs=1, order=None, ndata=None, edata=None, gdata=None, edge_weight=None, norms=(None,)):
    """a fresh GNNGraph over device COO lists that come through the draws; gi: 0-based graph ids.  The build downloads the lists,
    which waits for the delay: the buffers are armed again, so that the handle builds wait for them too.  norms: the handles the case
    is going to ask for (None: the plain one) -- a handle build synchronises the stream, so they are built here and everything is
    armed once more: what the case calls next is enqueued behind a pending delay."""
    dev = graphops._device()
    sd, td = d.ints(s), d.ints(t)
    ind = None if gi is None else d.ints(gi).cpu().numpy()
    g = graphops._new_graph(sd, td, n, dev, num_graphs=num_graphs, indicator=ind, ndata=ndata, edata=edata, gdata=gdata, edge_weight=edge_weight,
                            order=None if order is None else np.asarray(order, dtype=np.int32))
    d.rearm()
    for norm in norms:
        g.handle(norm)
    if norms:
        d.rearm()
    return g


# ---- the comparison ---------------------------------------------------------------------------------------------------------------

def flat(o, out, path="out"):
    if o is None or isinstance(o, (bool, int, float, str, np.integer, np.floating, np.ndarray, torch.Tensor)):
        out.append((path, o.detach() if isinstance(o, torch.Tensor) else o))
    elif isinstance(o, ng.GNNGraph):
        dev = graphops._device()
        flat(dict(n=o.num_nodes, e=o.num_edges, graphs=o.num_graphs, s=o._s0, t=o._t0, coo=list(graphops._coo(o, dev)), gi=o.graph_indicator,
                  w=o.edge_weight, ndata=dict(o.ndata), edata=dict(o.edata), gdata=dict(o.gdata)), out, path)
    elif isinstance(o, dict):
        for k in o:
            flat(o[k], out, f"{path}.{k}")
    elif isinstance(o, (list, tuple)):
        for k, v in enumerate(o):
            flat(v, out, f"{path}[{k}]")
    else:                                 # GraphMatrix, AdjacencyList, Components, ShortestPaths, CGInfo, LambdaMaxInfo: their fields
        flat({k: v for k, v in vars(o).items() if not k.startswith("_host") and k != "_graph"}, out, path)


def assert_same(name, got, want):
    a, b = [], []
    flat(got, a)
    flat(want, b)
    assert [p for p, _ in a] == [p for p, _ in b], (name, [p for p, _ in a], [p for p, _ in b])
    assert len(a) > 0, name
    for (path, u), (_, v) in zip(a, b):
        if isinstance(v, torch.Tensor):
            assert isinstance(u, torch.Tensor) and u.shape == v.shape and u.dtype == v.dtype, (name, path, getattr(u, "shape", u), v.shape)
            if not torch.equal(bits(u), bits(v)):
                differ = int((bits(u) != bits(v)).sum())
                nans = int(torch.isnan(u).sum()) if u.is_floating_point() else 0
                raise AssertionError(f"{name}: {path} differs from the default-stream run in {differ} of {v.numel()} elements ({nans} NaN)")
        elif isinstance(v, np.ndarray):
            assert isinstance(u, np.ndarray) and u.shape == v.shape and u.dtype == v.dtype and u.tobytes() == v.tobytes(), (name, path)
        elif isinstance(v, (float, np.floating)):
            assert np.float64(u).tobytes() == np.float64(v).tobytes(), (name, path, u, v)
        else:
            assert type(u) is type(v) and u == v, (name, path, u, v)


# ---- the cases: name -> (function of the draws, the entries it must reach) ---------------------------------------------------------

CASES = {}


def case(name, *entries, drained=()):
    """drained: declared entries the case cannot enter behind a pending delay, because a read-back of the same package call comes
    between its last input and the entry (said where the case is defined); only their stream argument is checked"""
    def add(fn):
        assert name not in CASES and set(drained) <= set(entries)
        CASES[name] = (fn, frozenset(entries), frozenset(drained))
        return fn
    return add


@contextlib.contextmanager
def environ(**kw):
    old = {k: os.environ.get(k) for k in kw}          # (a value of None takes the variable away)
    for k, v in kw.items():
        os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


N = W.N          # 70 nodes: two 64-row tiles, three 32-row ones
_RINGS = W.two_rings()
RING_S, RING_T, RING_GI = _RINGS._s0.copy(), _RINGS._t0.copy(), [0] * 35 + [1] * 35
del _RINGS


def rings(d, **kw):
    """test_workspace_gpu.two_rings: 70 nodes in two graphs, symmetric, in-degree 4"""
    return graph_of(d, RING_S, RING_T, N, gi=RING_GI, num_graphs=2, **kw)


def random_coo(n, e, seed, symmetric=False):
    rng = np.random.default_rng(seed)
    s, t = rng.integers(0, n, e), rng.integers(0, n, e)
    if symmetric:
        s, t = np.concatenate([s, t]), np.concatenate([t, s])
    return s, t


def batch_coo(seed):
    """three members -- (300, 1000), (2, 1) and (40, 90) -- as one block-diagonal list, shuffled: (s, t, n, ids)"""
    ss, tt, gi, off = [], [], [], 0
    for k, (n, e) in enumerate(((300, 1000), (2, 1), (40, 90))):
        s, t = random_coo(n, e, seed + k)
        ss.append(s + off)
        tt.append(t + off)
        gi += [k] * n
        off += n
    s, t = np.concatenate(ss), np.concatenate(tt)
    p = np.random.default_rng(seed).permutation(s.size)
    return s[p], t[p], off, gi


SIZES = ((300, 1000), (2, 1))


# -- layers: the case functions of test_workspace_gpu on a fresh two-rings graph, their inputs through the draws

GCN_NORM = (True, None, False)


def workspace_case(fn, norms=(None,)):
    """fn's inputs AND its cotangent come through the draws; the handle it asks for exists before the last arming"""
    def run(d):
        g = rings(d, norms=norms)
        with d.mp.context() as m:
            m.setattr(W, "randn", lambda *shape, grad=True: d.randn(*shape, grad=grad))
            m.setattr(W, "grads", lambda y, *leaves: pulled(d, y, *leaves))
            return fn(g)
    return run


def gcn_edge_weight(din, dout):
    """test_workspace_gpu.gcn_edge_weight with its weights drawn, so that the weighted handle can be built before the last arming
    (the handle cache is keyed by the weights' address and version: the call below finds it)"""
    def run(d):
        g = rings(d, norms=())
        w = d.rand(g.num_edges, lo=0.5, hi=1.5, grad=True)
        h = g.handle((True, w.detach(), True))
        d.rearm()
        x, wt, b = d.randn(N, din), d.randn(din, dout, grad=True), d.randn(dout, grad=True)
        assert g.handle((True, w.detach(), True)) is h
        return pulled(d, F.gcn_conv(x, wt, b, h, _lib.ACT["tanh"], w), wt, b, w)
    return run


# (ngpde_graph_set_gcn_norm_device: the package calls it right after the build, which has synchronised -- the C-ABI case below arms in between)
HANDLE = ("ngpde_graph_create_device",)
for _name, _fn, _entries in (
        ("gcn fused 64 -> 64", workspace_case(W.gcn(64, 64), [GCN_NORM]), HANDLE + ("ngpde_gcn_forward", "ngpde_gcn_backward")),
        ("gcn any width 12 -> 20", workspace_case(W.gcn(12, 20), [GCN_NORM]), ("ngpde_gcn_forward", "ngpde_gcn_backward")),
        ("gcn any width 20 -> 12", workspace_case(W.gcn(20, 12), [GCN_NORM]), ("ngpde_gcn_forward", "ngpde_gcn_backward")),
        ("gcn edge weights, fused, no dx", gcn_edge_weight(64, 64), HANDLE + ("ngpde_gcn_forward", "ngpde_gcn_backward_ew")),
        ("gcn edge weights 20 -> 12, no dx", gcn_edge_weight(20, 12), ("ngpde_gcn_forward", "ngpde_gcn_backward_ew")),
        ("dense split-K 64 rows x 512", workspace_case(W.dense(64, 48, 512), ()), ("ngpde_dense_forward", "ngpde_dense_backward")),
        ("dense plain", workspace_case(W.dense(N, 48, 40), ()), ("ngpde_dense_forward", "ngpde_dense_backward")),
        ("gat 2 heads x 12", workspace_case(W.gat(2, 12), [GCN_NORM]), ("ngpde_gat_forward", "ngpde_gat_backward")),
        ("gat layer 1 head", workspace_case(W.gat_layer(1), [GCN_NORM]), ("ngpde_gat_layer_forward", "ngpde_gat_layer_backward")),
        ("gat layer 4 heads", workspace_case(W.gat_layer(4), [GCN_NORM]), ("ngpde_gat_layer_forward", "ngpde_gat_layer_backward")),
        ("edge mlp 64 -> 64", workspace_case(W.edge_mlp(64, [64])), ("ngpde_edge_mlp_backward",)),
        ("edge mlp 32 -> 48 -> 24", workspace_case(W.edge_mlp(32, [48, 24])), ("ngpde_edge_mlp_backward",))):
    case("layers: " + _name, *_entries)(_fn)


def _stack(d, dims, acts):
    return [(d.randn(a, b, grad=True, scale=1.0 / np.sqrt(a)), d.randn(b, grad=True, scale=0.3), _lib.ACT[act]) for a, b, act in zip(dims, dims[1:], acts)]


def _stack_leaves(*stacks):
    return [t for st in stacks for wt, b, _ in st for t in (wt, b)]


@case("layers: edge layer (VMH shape), training and no_grad", "ngpde_edge_layer_forward", "ngpde_edge_layer_backward")
def _edge_layer(d):
    g = rings(d)
    x, pos = d.randn(N, 16, grad=True), d.randn(N, 2)
    phi, upd = _stack(d, [34, 64, 64], ["tanh", "tanh"]), _stack(d, [80, 16], ["identity"])
    out = pulled(d, F.edge_layer(g.handle(), _lib.LAYER_VMH, "+", [x], phi, upd, pos=pos), x, *_stack_leaves(phi, upd))
    with torch.no_grad():
        out.append(F.edge_layer(g.handle(), _lib.LAYER_VMH, "+", [x], phi, upd, pos=pos))
    return out


@case("layers: gno layer, training and no_grad", "ngpde_gno_layer_forward", "ngpde_gno_layer_backward")
def _gno_layer(d):
    g = rings(d)
    h, lwt, lb, feat = d.randn(N, 16, grad=True), d.randn(16, 16, grad=True, scale=0.25), d.randn(16, grad=True, scale=0.3), d.randn(N, 2)
    phi = _stack(d, [4, 32, 256], ["relu", "identity"])
    args = (g.handle(), 16, 16, _lib.AGGR["mean"], _lib.ACT["relu"], h, lwt, lb, phi)
    out = pulled(d, F.gno_layer(*args, node_feat=feat), h, lwt, lb, *_stack_leaves(phi))
    with torch.no_grad():
        out.append(F.gno_layer(*args, node_feat=feat))
    return out


def layer_both_ways(d, layer, x, composed_too=True):
    """y and every gradient of `layer` through the package (the layer-level entry) and through tests/composed.py (the primitives)"""
    ps0, st = ng.setup(11, layer)
    out = []
    for call in ((lambda xs, ps: layer(xs, ps, st)),) + ((lambda xs, ps: composed.apply(layer, xs, ps, st),) if composed_too else ()):
        ps = d.leaves(ps0)
        xs = x.detach().clone().requires_grad_(True)
        y, _ = call(xs, ps)
        out += pulled(d, y, xs, *leaves_of(ps))
        with torch.no_grad():
            out.append(call(xs, ps)[0])
    return out


def mlp(dims, acts):
    return ng.Chain(*[ng.Dense(a, b, act) for a, b, act in zip(dims, dims[1:], acts)])


ROW_BLOCKS = ("ngpde_row_blocks_gather", "ngpde_row_blocks_scatter")


@case("layers: ExplicitEdgeConv 6 -> 16 -> 8, mean", "ngpde_edge_layer_forward", "ngpde_edge_layer_backward", "ngpde_dense_pair_forward", *ROW_BLOCKS)
def _edgeconv(d):
    g = rings(d, ndata={"x": d.rand(2, N)})
    layer = ng.ExplicitEdgeConv(mlp([14, 16, 8], ["tanh", "identity"]), initialgraph=g, aggr="mean")
    return layer_both_ways(d, layer, d.randn(6, N))


@case("layers: ExplicitEdgeConv 6 -> 12 -> 20 -> 8, max (the primitives' pullbacks)", "ngpde_edge_layer_forward", "ngpde_edge_layer_backward",
      "ngpde_edge_combine_forward", "ngpde_edge_combine_backward", "ngpde_segment_reduce_forward", "ngpde_segment_reduce_backward")
def _edgeconv_max(d):
    g = rings(d, ndata={"x": d.rand(2, N)})
    layer = ng.ExplicitEdgeConv(mlp([14, 12, 20, 8], ["tanh", "swish", "identity"]), initialgraph=g, aggr="max")
    with environ(NGPDE_NO_FUSED_EDGE="1"):
        return layer_both_ways(d, layer, d.randn(6, N))


@case("layers: VMHConv 1 -> (32, 32, 16) / (24, 1), fused forward with the primitives' pullback", "ngpde_edge_mlp_forward",
      "ngpde_activation_forward", "ngpde_dense_chain2_forward", "ngpde_segment_reduce_backward", "ngpde_edge_combine_backward")
def _vmhconv(d):
    g = rings(d, ndata={"x": d.rand(2, N)})
    layer = ng.VMHConv(mlp([4, 32, 32, 16], ["tanh", "tanh", "identity"]), mlp([17, 24, 1], ["tanh", "identity"]), initialgraph=g)
    return layer_both_ways(d, layer, d.randn(1, N))


@case("layers: MPPDEConv 64 wide on a batch of two meshes", "ngpde_edge_layer_forward", "ngpde_edge_layer_backward", "ngpde_dense_pair_forward",
      "ngpde_dense_chain2_forward", "ngpde_edge_mlp_forward", *ROW_BLOCKS)
def _mppde(d):
    n, traj = 64, 2
    s, t = ng.synth.periodic_mesh_batch(n, traj)
    g = graph_of(d, s, t, n * traj, gi=np.repeat(np.arange(traj), n), num_graphs=traj,
                 ndata={"u": d.rand(1, n * traj), "x": d.rand(1, n * traj)}, gdata={"θ": d.rand(2, traj)})
    layer = ng.MPPDEConv(mlp([2 * 64 + 2 + 2, 64, 64], ["swish", "swish"]), mlp([64 + 64 + 2, 64, 64], ["swish", "identity"]), initialgraph=g)
    return layer_both_ways(d, layer, d.randn(64, n * traj))


@case("layers: MPPDEConv 10 wide, widths outside the fused kernels", "ngpde_edge_layer_forward", "ngpde_edge_layer_backward", "ngpde_rk_stage_combine")
def _mppde_narrow(d):
    n, traj = 35, 2
    s, t = ng.synth.periodic_mesh_batch(n, traj)
    g = graph_of(d, s, t, n * traj, gi=np.repeat(np.arange(traj), n), num_graphs=traj,
                 ndata={"u": d.rand(1, n * traj), "x": d.rand(1, n * traj)}, gdata={"θ": d.rand(2, traj)})
    layer = ng.MPPDEConv(mlp([2 * 10 + 2 + 2, 30], ["swish"]), mlp([10 + 30 + 2, 14, 6], ["swish", "identity"]), initialgraph=g)
    return layer_both_ways(d, layer, d.randn(10, n * traj))


@case("layers: the Dense pair that shares a 64-wide block, 32768 rows (its one-launch pullback)", "ngpde_dense_pair_forward", "ngpde_dense_pair_backward")
def _dense_pair(d):
    n = 32768
    x, pos = d.randn(n, 64, grad=True), d.randn(n, 2)
    wa, wb, ba = d.randn(66, 64, grad=True, scale=0.125), d.randn(66, 64, grad=True, scale=0.125), d.randn(64, grad=True, scale=0.3)
    ya, yb = composed.dense_pair([x, pos], wa, ba, 0, [x, pos], wb, None, 0)
    (ya * d.like(ya) + yb * d.like(yb)).sum().backward()
    return [ya, yb, x.grad, wa.grad, wb.grad, ba.grad]


def gno_graph(d, edge_only=False):
    s, t = random_coo(N, 4 * N, 13)
    return graph_of(d, s, t, N, ndata=None if edge_only else {"x": d.rand(2, N), "f0": d.randn(1, N)}, edata={"e": d.randn(2, s.size)})


GNO = ("ngpde_gno_layer_forward", "ngpde_gno_layer_backward")


@case("layers: GNOConv 16 -> 32, two-layer phi, mean (the message formed in the launch)", *GNO, "ngpde_gno_message_forward",
      "ngpde_gno_message_backward_from_nodes", "ngpde_dense_multi_forward", "ngpde_transpose", "ngpde_rows_scale", "ngpde_bias_act_forward",
      "ngpde_bias_act_backward")
def _gno_two(d):
    g = gno_graph(d)
    g.handle().inv_in_degree(graphops._device())          # (uploaded on first use, by the mean pullback: here, before the inputs)
    d.rearm()
    layer = ng.GNOConv((16, 32), mlp([8, 16, 16 * 32], ["relu", "identity"]), "relu", initialgraph=g, aggr="mean")
    return layer_both_ways(d, layer, d.randn(16, N))


@case("layers: GNOConv 16 -> 32, two-layer phi, max", *GNO, "ngpde_gno_message_forward", "ngpde_gno_apply_backward", "ngpde_edge_combine_backward",
      "ngpde_segment_reduce_forward", "ngpde_segment_reduce_backward")
def _gno_max(d):
    g = gno_graph(d)
    layer = ng.GNOConv((16, 32), mlp([8, 16, 16 * 32], ["relu", "identity"]), "relu", initialgraph=g, aggr="max")
    return layer_both_ways(d, layer, d.randn(16, N))


@case("layers: GNOConv 16 -> 32, three-layer phi (the reassociated message on the primitives)", *GNO, "ngpde_gno_apply_forward",
      "ngpde_gno_apply_backward", "ngpde_edge_combine_forward", "ngpde_edge_combine_backward")
def _gno_three(d):
    g = gno_graph(d)
    layer = ng.GNOConv((16, 32), mlp([8, 24, 16, 16 * 32], ["relu", "swish", "identity"]), "swish", initialgraph=g, aggr="mean")
    return layer_both_ways(d, layer, d.randn(16, N))


@case("layers: GNOConv 16 -> 32, the literal batched product", *GNO, "ngpde_gno_contract_forward", "ngpde_gno_contract_backward")
def _gno_materialized(d):
    g = gno_graph(d)
    layer = ng.GNOConv((16, 32), mlp([8, 16, 16 * 32], ["relu", "identity"]), "relu", initialgraph=g, aggr="mean")
    with environ(NGPDE_GNO_MATERIALIZE="1"):
        return layer_both_ways(d, layer, d.randn(16, N))


@case("layers: GNOConv 32 -> 48 by target (aggregate, then transform), 64 edges per node", *GNO, "ngpde_gno_gform_aggregate",
      "ngpde_gno_gform_transform")
def _gno_gform(d):
    n, deg = 70, 64
    rng = np.random.default_rng(17)
    t, s = np.repeat(np.arange(n), deg), rng.integers(0, n, n * deg)
    p = rng.permutation(n * deg)
    g = graph_of(d, s[p], t[p], n, ndata={"x": d.rand(2, n), "f0": d.randn(1, n)})
    layer = ng.GNOConv((32, 48), mlp([6, 64, 32 * 48], ["relu", "identity"]), "relu", initialgraph=g, aggr="+")
    with environ(NGPDE_NO_GNO_GFORM=None):
        assert composed.gno_gform_preferred(n, n * deg, 32, 48, 64, 1, "+", True)
        return layer_both_ways(d, layer, d.randn(32, n))


@case("layers: SpectralConv(8)", "ngpde_propagate_copy_xj")          # (its weights come from host edge data: ngpde_spectral_weights is in the flat-vector case)
def _spectral(d):
    layer = ng.SpectralConv(8)
    _, st = ng.setup(0, layer)
    st["graph"].handle()          # (the layer's own graph, from host lists; x is drawn after this read-back)
    x = d.randn(3, 8, grad=True)
    y, _ = layer(x, {}, st)
    return pulled(d, y, x)


@case("layers: GATConv 20 -> 2 x 12 (Dense, aggregate, bias and activation)", "ngpde_dense_forward", "ngpde_gat_forward", "ngpde_gat_backward",
      "ngpde_bias_act_forward", "ngpde_bias_act_backward")
def _gatconv(d):
    g = rings(d, norms=())
    layer = ng.GATConv((20, 12), "tanh", heads=2, initialgraph=g)
    layer._graph(g).handle()          # (the graph with the self loops, from host lists: built before the inputs are drawn)
    return layer_both_ways(d, layer, d.randn(20, N), composed_too=False)


# -- message-passing primitives and readouts: n = 300, e = 1000, d in {1, 64}

def mp_graph(d, weighted=False):
    s, t = random_coo(300, 1000, 5)
    return graph_of(d, s, t, 300, edge_weight=d.rand(1000, lo=0.5, hi=1.5) if weighted else None)


for _w in (1, 64):
    @case(f"propagate: copy_xj / e_mul_xj / w_mul_xj, + and mean, d = {_w}", "ngpde_propagate_emul_forward", "ngpde_propagate_emul_backward")
    def _propagate_fused(d, w=_w):
        g = mp_graph(d, weighted=True)
        out = []
        for f, aggr, e in ((ng.copy_xj, "+", None), (ng.e_mul_xj, "mean", d.randn(w, 1000, grad=True)), (ng.e_mul_xj, "+", d.randn(1, 1000, grad=True)),
                           (ng.w_mul_xj, "+", None)):
            x = d.randn(w, 300, grad=True)
            out += pulled(d, ng.propagate(f, g, aggr, xj=x, e=e), x, *([e] if e is not None else []))
        return out

    @case(f"propagate: a user message, every aggregation, d = {_w}", "ngpde_gather_forward", "ngpde_gather_backward", "ngpde_edge_permute",
          "ngpde_segment_reduce_forward", "ngpde_segment_reduce_backward")
    def _propagate_user(d, w=_w):
        g = mp_graph(d)
        out = []
        for aggr in ("+", "mean", "max", "min", "*"):
            xi, xj, e = d.randn(w, 300, grad=True), d.randn(w, 300, grad=True), d.randn(w, 1000, grad=True)
            out += pulled(d, ng.propagate(lambda a, b, c: a * b + c, g, aggr, xi=xi, xj=xj, e=e), xi, xj, e)
        return out

    @case(f"apply_edges: xi_dot_xj, a user function, propagate(xi_dot_xj, max), d = {_w}", "ngpde_apply_edges_dot_forward",
          "ngpde_apply_edges_dot_backward", "ngpde_gather_forward", "ngpde_gather_backward", "ngpde_edge_permute")
    def _apply_edges(d, w=_w):
        g = mp_graph(d)
        out = []
        for call in (lambda a, b: ng.apply_edges(ng.xi_dot_xj, g, xi=a, xj=b), lambda a, b: ng.apply_edges(lambda p, q, e: p - q, g, xi=a, xj=b),
                     lambda a, b: ng.propagate(ng.xi_dot_xj, g, "max", xi=a, xj=b)):
            xi, xj = d.randn(w, 300, grad=True), d.randn(w, 300, grad=True)
            out += pulled(d, call(xi, xj), xi, xj)
        return out

    @case(f"softmax_edge_neighbors and aggregate_neighbors, d = {_w}", "ngpde_softmax_edge_neighbors_forward", "ngpde_softmax_edge_neighbors_backward",
          "ngpde_edge_permute", "ngpde_segment_reduce_forward", "ngpde_segment_reduce_backward")
    def _edge_softmax(d, w=_w):
        g = mp_graph(d)
        e, m = d.randn(w, 1000, grad=True), d.randn(w, 1000, grad=True)
        return pulled(d, ng.softmax_edge_neighbors(g, e), e) + pulled(d, ng.aggregate_neighbors(g, "mean", m), m)

    @case(f"readouts: reduce, softmax and broadcast over the nodes and edges of a three-member batch, d = {_w}",
          "ngpde_readout_reduce_forward", "ngpde_readout_reduce_backward", "ngpde_readout_softmax_forward", "ngpde_readout_softmax_backward",
          "ngpde_readout_broadcast_forward", "ngpde_readout_broadcast_backward")
    def _readouts(d, w=_w):
        s, t, n, gi = batch_coo(31)
        g = graph_of(d, s, t, n, gi=gi, num_graphs=3)
        out = []
        for aggr in ("+", "mean", "max", "min"):
            x, e = d.randn(w, n, grad=True), d.randn(w, s.size, grad=True)
            out += pulled(d, ng.reduce_nodes(aggr, g, x), x) + pulled(d, ng.reduce_edges(aggr, g, e), e)
        x, e, u, v = d.randn(w, n, grad=True), d.randn(w, s.size, grad=True), d.randn(w, 3, grad=True), d.randn(w, 3, grad=True)
        out += pulled(d, ng.softmax_nodes(g, x), x) + pulled(d, ng.softmax_edges(g, e), e)
        out += pulled(d, ng.broadcast_nodes(g, u), u) + pulled(d, ng.broadcast_edges(g, v), v)
        return out


@case("readouts: the plan through the C ABI (the package uploads the graph ids right before its create)", "ngpde_readout_create",
      "ngpde_readout_reduce_forward")
def _abi_readout(d):
    lib, (s, t, n, gi) = _lib.load(), batch_coo(31)
    ids, index, x = d.ints(gi), d.ints(s), d.randn(s.size, 5)
    plan, out = C.c_void_p(), torch.empty(3, 5, device=DEV)
    _lib.check(lib.ngpde_readout_create(s.size, _lib.ptr(ids), _lib.ptr(index), 0, 3, _lib.current_stream(), C.byref(plan)))
    try:
        d.rearm()
        ws = F._ws(lib.ngpde_readout_workspace_bytes(plan, 5), out.device)
        _lib.check(lib.ngpde_readout_reduce_forward(plan, 5, _lib.AGGR["max"], _lib.ptr(x), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.current_stream()))
    finally:
        torch.cuda.current_stream().synchronize()
        _lib.destroy_later("ngpde_readout_destroy", plan)
    return [out]


# -- graph construction and lists

for _n, _e in SIZES:
    @case(f"handles: the device build with all three normalisations, ({_n}, {_e})", *HANDLE, "ngpde_gcn_forward")
    def _handles(d, n=_n, e=_e):
        s, t = random_coo(n, e, 3)
        g = graph_of(d, s, t, n, norms=())          # (armed: the three builds below read the lists behind a pending delay)
        w = d.rand(e, lo=0.5, hi=1.5)
        handles = [g.handle(norm) for norm in (GCN_NORM, (False, None, False), (True, w, True))]
        d.rearm()
        x, wt, b = d.randn(n, 12), d.randn(12, 20), d.randn(20)
        with torch.no_grad():
            return [F.gcn_conv(x, wt, b, h, _lib.ACT["tanh"]) for h in handles]

    @case(f"neighbour search: radius_graph, knn_graph and the spatial order, {_n} points", "ngpde_radius_graph", "ngpde_knn_graph",
          "ngpde_spatial_order")
    def _neighbours(d, n=_n):
        pts, rows = d.rand(2, n), d.rand(n, 2)
        out = []
        for locality in ("bfs", "spatial"):
            out += each(d, lambda: ng.radius_graph(pts, 0.12 if n > 2 else 2.0, locality=locality), lambda: ng.knn_graph(pts, min(3, n - 1), locality=locality))
            for g in out[-2:]:
                g.handle()
            out += [g.node_order() for g in out[-2:]]
        d.rearm()          # (the package orders the points after it has downloaded the lists: the entry itself, behind a delay)
        order = torch.empty(n, dtype=torch.int32, device=DEV)
        _lib.check(_lib.load().ngpde_spatial_order(n, 2, _lib.ptr(rows), None, 1, 1, _lib.ptr(order), _lib.current_stream()))
        return out + [order]

    @case(f"graph queries and transforms: degree, coalesce, bidirect, self loops, induced subgraph, ({_n}, {_e})", "ngpde_coo_degree",
          "ngpde_coo_flags", "ngpde_coo_coalesce", "ngpde_group_reduce_forward", "ngpde_group_reduce_backward", "ngpde_coo_add_self_loops",
          "ngpde_coo_compact", "ngpde_rows_index", "ngpde_coo_orient")
    def _transforms(d, n=_n, e=_e):
        s, t = random_coo(n, e, 9)
        w, f, x = d.rand(e, lo=0.5, hi=1.5, grad=True), d.randn(3, e, grad=True), d.randn(2, n, grad=True)
        g = graph_of(d, s, t, n, ndata={"x": x}, edata={"e": f}, edge_weight=w)
        out = each(d, lambda: ng.degree(g, "out"), lambda: ng.degree(g, "in"), lambda: ng.degree(g, "both"), lambda: ng.degree(g, "in", edge_weight=False),
                   lambda: [ng.has_self_loops(g), ng.has_multi_edges(g), ng.is_bidirected(g)])
        for make in (lambda: ng.remove_multi_edges(g, "+"), lambda: ng.remove_multi_edges(g, "max"), lambda: ng.to_bidirected(g), lambda: ng.to_unidirected(g),
                     lambda: ng.remove_self_loops(g), lambda: ng.induced_subgraph(g, d.ints(np.arange(0, n, 2), torch.int64))):
            (h,) = each(d, make)
            loss = h.edge_weight.sum() + (h.edata["e"] * h.edata["e"]).sum() + (h.ndata["x"] * h.ndata["x"]).sum()
            d.rearm()          # (every transform ends with a download of its lists: the pullbacks get a delay of their own)
            loss.backward()
            out += [h, w.grad.clone(), f.grad.clone(), x.grad.clone()]
        coal = graphops._Coalesced(g, graphops._device(), False)          # (the groups are counted on the host before the package reduces over them)
        d.rearm()
        rows = d.randn(e, 3, grad=True)
        out += pulled(d, graphops._GroupReduceFn.apply(rows, coal, _lib.AGGR["max"]), rows)
        bare = graph_of(d, s, t, n, edge_weight=w.detach())
        return out + each(d, lambda: ng.add_self_loops(bare)) + [ng.add_self_loops(graph_of(d, s, t, n))]

    @case(f"graph editing and sampling on the device lists, ({_n}, {_e})", "ngpde_coo_remove_edges", "ngpde_coo_append", "ngpde_coo_complement_nodes",
          "ngpde_coo_negative_sample", "ngpde_coo_sample_neighbors", "ngpde_coo_rand_split", "ngpde_coo_flags")
    def _editing(d, n=_n, e=_e):
        s, t = random_coo(n, e, 15)
        w, f = d.rand(e, lo=0.5, hi=1.5, grad=True), d.randn(2, e, grad=True)
        g = graph_of(d, s, t, n, edata={"e": f}, edge_weight=w)
        m = max(e // 10, 1)
        out = each(d, lambda: ng.remove_edges(g, d.ints(np.arange(0, e, 3), torch.int64)), lambda: ng.remove_edges(g, d.ints(s[:m]), d.ints(t[:m])),
                   lambda: ng.add_edges(g, d.ints(t[:m]), d.ints(s[:m]), edata=d.randn(2, m), edge_weight=d.rand(m)),
                   lambda: ng.remove_nodes(g, d.ints([0], torch.int64)), lambda: ng.add_nodes(g, 3),
                   lambda: ng.negative_sample(g, max(e // 2, 1), bidirected=False, seed=3))
        for replace in (False, True):
            (h,) = each(d, lambda: ng.sample_neighbors(g, d.ints(np.arange(0, n, 2), torch.int64), 2, replace=replace, seed=5))
            out.append(h)
            (h.edge_weight.sum() + (h.edata["e"] * h.edata["e"]).sum()).backward()
            out += [w.grad.clone(), f.grad.clone()]
        out += each(d, lambda: list(ng.rand_edge_split(g, 0.3, bidirected=False, seed=7)))
        ss, ts = random_coo(n, e, 16, symmetric=True)
        sym = graph_of(d, ss, ts, n)
        return out + each(d, lambda: list(ng.rand_edge_split(sym, 0.5, seed=8)), lambda: ng.negative_sample(sym, 2 * (e // 4), seed=9) if n > 2 else None)

    # (ngpde_coo_adjacency_fill: the count pass before it reads the total back)
    @case(f"neighbourhood queries: has_edge, adjacency_list, intersect, random_walk_pe, ({_n}, {_e})", "ngpde_coo_sort_keys", "ngpde_coo_has_edge",
          "ngpde_coo_adjacency_count", "ngpde_coo_adjacency_fill", "ngpde_coo_intersect", "ngpde_csr_random_walk_pe", "ngpde_coo_matrix",
          drained=("ngpde_coo_adjacency_fill",))
    def _queries(d, n=_n, e=_e):
        s, t = random_coo(n, e, 21)
        g = graph_of(d, s, t, n, edge_weight=d.rand(e, lo=0.5, hi=1.5))
        s2, t2 = np.concatenate([s[::2], t[:3]]), np.concatenate([t[::2], s[:3]])
        g2 = graph_of(d, s2, t2, n)
        qs, qt = d.ints(np.concatenate([s[:5], t[:5]]), torch.int64), d.ints(np.concatenate([t[:5], s[:5]]), torch.int64)
        out = each(d, lambda: ng.has_edge(g, qs, qt), lambda: ng.has_edge(g, qs, qt, return_eid=True), lambda: ng.adjacency_list(g),
                   lambda: ng.adjacency_list(g, d.ints([n - 1, 0, 0], torch.int64), dir="in"), lambda: ng.intersect(g, g2, return_eid=True),
                   lambda: ng.intersect(g, g2, return_eid=True),          # (the second time both key plans exist)
                   lambda: ng.adjacency_matrix(g, dir="out", weighted=True))
        return out + each(d, lambda: ng.random_walk_pe(out[-1], 4))


@case("handles through the C ABI: the build and the weighted normalisation, each behind a delay of its own", "ngpde_graph_create_device",
      "ngpde_graph_set_gcn_norm_device", "ngpde_gcn_forward")
def _abi_handle(d):
    lib, (s, t) = _lib.load(), random_coo(300, 1000, 3)
    sd, td, w = d.ints(s), d.ints(t), d.rand(1000, lo=0.5, hi=1.5)
    out = C.c_void_p()
    _lib.check(lib.ngpde_graph_create_device(300, 1000, _lib.ptr(sd), _lib.ptr(td), 32, 0, 1, None, _lib.current_stream(), C.byref(out)))
    try:
        d.rearm()
        _lib.check(lib.ngpde_graph_set_gcn_norm_device(out, 1, _lib.ptr(w), 1, _lib.current_stream()))
        d.rearm()
        x, wt, b = d.randn(300, 12), d.randn(12, 20), d.randn(20)
        handle = type("Handle", (), {"ptr": out})
        with torch.no_grad():
            return [F.gcn_conv(x, wt, b, handle, _lib.ACT["tanh"])]
    finally:
        torch.cuda.current_stream().synchronize()
        _lib.destroy_later("ngpde_graph_destroy", out)


# (ngpde_components_rank: the labelling before it reads its round counters back; getgraph uploads its node list before ngpde_coo_compact, which
#  the transforms case above enters behind a delay)
@case("per-graph transforms on a three-member batch: unbatch, degree, components, induced subgraph", "ngpde_coo_degree",
      "ngpde_coo_components", "ngpde_components_rank", drained=("ngpde_components_rank",))
def _batch_ops(d):
    s, t, n, gi = batch_coo(41)
    g = graph_of(d, s, t, n, gi=gi, num_graphs=3, ndata={"x": d.randn(2, n)}, edata={"e": d.randn(1, s.size)}, gdata={"u": d.randn(2, 3)})
    return each(d, lambda: ng.getgraph(g, 0), lambda: ng.getgraph(g, 1), lambda: ng.getgraph(g, 2), lambda: ng.degree(g, "both"),
                lambda: ng.connected_components(g), lambda: ng.is_connected(g), lambda: ng.getgraph(g, [0, 2], nmap=True))


# -- matrices and solves: test_workspace_gpu's two-graph, 65-column shape

MATRIX = ("ngpde_coo_matrix", "ngpde_coo_degree")


# (on a batch the assembly uploads the graph ids before ngpde_coo_matrix -- the neighbourhood-queries case assembles on one graph -- and it
#  reads the entry count back: what runs on the assembled matrix inside the same package call -- the symmetry check, the Lanczos iteration, the
#  product's count and, after the count's read-back, the product -- is entered with the delay run out)
@case("matrices: adjacency, Laplacian, normalised and scaled Laplacian with their pullbacks, khop_adj(2), matmul", *MATRIX, "ngpde_csr_spgemm_count",
      "ngpde_csr_spgemm", "ngpde_csr_check_symmetric", "ngpde_csr_lambda_max", "ngpde_propagate_emul_forward", "ngpde_propagate_emul_backward",
      drained=("ngpde_coo_matrix", "ngpde_csr_spgemm_count", "ngpde_csr_spgemm", "ngpde_csr_check_symmetric", "ngpde_csr_lambda_max"))
def _matrices(d):
    half = RING_S < RING_T
    w_half = d.rand(int(half.sum()), lo=0.5, hi=1.5, grad=True)          # a symmetric weight: both directions of a pair share it
    pair = {}
    for k, (a, b) in enumerate(zip(RING_S[half], RING_T[half])):
        pair[(a, b)] = pair[(b, a)] = k
    index = d.ints([pair[(a, b)] for a, b in zip(RING_S, RING_T)], torch.int64)
    g0 = rings(d)
    out = []
    for make in (ng.adjacency_matrix, ng.laplacian_matrix, ng.normalized_laplacian, ng.scaled_laplacian):
        g = ng.set_edge_weight(g0, w_half[index])          # (a copy that shares the structure; a new autograd node per matrix)
        m = make(g)
        m.as_graph().handle()          # (downloads the matrix's lists and builds the handle: before X is drawn)
        X = d.randn(65, N, grad=True)
        y = m.matmul(X)
        y.backward(d.like(y))
        out += [m, y, X.grad, w_half.grad.clone()]
    return out + [ng.khop_adj(g, 2), ng.adjacency_matrix(g, dir="in", weighted=False)]


@case("solves: laplacian_lambda_max and cg_solve with return_info, the solve's pullback", "ngpde_coo_matrix", "ngpde_csr_check_symmetric",
      "ngpde_csr_lambda_max", "ngpde_csr_cg", drained=("ngpde_coo_matrix", "ngpde_csr_check_symmetric", "ngpde_csr_lambda_max"))          # (as above)
def _solves(d):
    g = rings(d)
    lam, info = ng.laplacian_lambda_max(g, return_info=True)
    B = d.randn(65, N, grad=True)
    X, cg = ng.cg_solve(ng.laplacian_matrix(g), B, shift=1.0, return_info=True)
    X.backward(d.like(X))
    return [lam, info, X, cg, B.grad]


# (ngpde_components_rank and ngpde_hop_reached_nodes follow the read-backs of the rounds / levels of the same package call)
@case("traversals: connected_components, hop_distance (shared, separate), neighborhood, shortest_paths with parents", "ngpde_coo_components",
      "ngpde_components_rank", "ngpde_coo_rows", "ngpde_csr_hop_distance", "ngpde_hop_reached_nodes", "ngpde_coo_rows_eid",
      "ngpde_csr_shortest_paths", drained=("ngpde_components_rank", "ngpde_hop_reached_nodes"))
def _traversals(d):
    g = rings(d)
    src, w = d.ints([0, 40, 7], torch.int64), d.rand(g.num_edges, lo=0.1, hi=1.1)
    out = each(d, lambda: ng.connected_components(g), lambda: ng.hop_distance(g, src, dir="both", separate=True),
               lambda: ng.hop_distance(g, d.ints([3, 69], torch.int64)), lambda: ng.hop_distance(g, src, dir="both"),
               lambda: ng.neighborhood(g, d.ints([3], torch.int64), 2),
               lambda: ng.shortest_paths(g, src, edge_weight=w, dir="both", separate=True, return_parents=True),
               lambda: ng.shortest_paths(g, src, edge_weight=w, dir="both", separate=True, return_parents=True),          # (the rows exist now)
               lambda: ng.shortest_paths(g, d.ints([5], torch.int64)).dist)
    return out + [out[-2].rounds]


# -- solvers: the 96-node three-tile graph of test_plan_memory_gpu; every plan is created inside the run

DT = 0.05


def tile_graph(d, **kw):
    s, t, n, order = H.tile_count(96)
    return graph_of(d, s, t, n, order=order, **kw)


def solved(d, node, ps, u):
    """two solves with their pullbacks: the first creates the plan (a create works on the NULL stream and may read back), the second
    finds it and is enqueued behind a delay of its own"""
    _, st = ng.setup(0, node)
    out = []
    for k in range(2):
        y, _ = node(u, ps, st)
        out += pulled(d, y, u, *leaves_of(ps))
        for leaf in [u] + leaves_of(ps):
            leaf.grad = None
        d.rearm()
    return out


@case("solver: the GCN2 plan, Tsit5 x 2 forward and backward", "ngpde_node_gcn2_forward", "ngpde_node_gcn2_backward")
def _node_gcn2(d):
    g = tile_graph(d, norms=[GCN_NORM])
    rhs = ng.Chain(ng.GCNConv((64, 64), "relu", initialgraph=g), ng.GCNConv((64, 64), "relu", initialgraph=g))
    node = ng.NeuralODE(rhs, solver="tsit5", n_steps=2, dt=0.1)
    ps = {f"layer_{k}": {"weight": d.randn(64, 64, grad=True, scale=0.125), "bias": d.randn(64, 1, grad=True, scale=0.1)} for k in (1, 2)}
    out = solved(d, node, ps, d.randn(64, 96, grad=True))
    plan = next(iter(node._plans.values()))[0]
    assert {"persistent_fwd", "persistent_bwd"} <= plan.flags(), plan.flags()
    return out


@case("solver: the GAT plan (2 x 32), Tsit5 x 2 forward and backward", "ngpde_ode_create", "ngpde_ode_forward", "ngpde_ode_backward")
def _node_gat(d):
    g = tile_graph(d)
    node = ng.NeuralODE(ng.GATConv((64, 32), "tanh", heads=2, add_self_loops=False, initialgraph=g), solver="tsit5", n_steps=2, dt=DT)
    ps = {"weight": d.randn(64, 64, grad=True, scale=1.5 / 8), "a": d.randn(64, 2, grad=True, scale=1.0 / np.sqrt(32)), "bias": d.randn(64, 1, grad=True, scale=0.1)}
    return solved(d, node, ps, d.randn(64, 96, grad=True))


def vmh_layer(g):
    return ng.VMHConv(mlp([4, 16, 8], ["tanh", "identity"]), mlp([9, 16, 1], ["tanh", "identity"]), initialgraph=g)


def positioned(d):
    """the tile graph with its handle built, then the copy that carries the positions (updategraph with a new cloud on a known structure):
    the handle build synchronises the stream, so it comes first -- what the plan's create is given is then packed behind a pending delay"""
    g = tile_graph(d)          # (builds the plain handle and arms again)
    return ng.GNNGraph(g, ndata={"x": d.rand(2, 96)})


def vmh_params(d):
    ps0, _ = ng.setup(3, vmh_layer(None))
    return d.leaves(ps0)


@case("solver: the VMH plan (scalar state, 2 coordinates), Tsit5 x 2 forward and backward; its positions are packed on the side stream",
      "ngpde_ode_create", "ngpde_ode_forward", "ngpde_ode_backward")
def _node_vmh(d):
    g = positioned(d)
    node = ng.NeuralODE(vmh_layer(g), solver="tsit5", n_steps=2, dt=DT)
    out = solved(d, node, vmh_params(d), d.randn(1, 96, grad=True))
    assert any(k[0] == "vmh" for k in node._plans), list(node._plans)
    return out


@case("solver: the VMH plan with saveat", "ngpde_ode_create", "ngpde_ode_forward", "ngpde_ode_backward")
def _node_vmh_saveat(d):
    g = positioned(d)
    node = ng.NeuralODE(vmh_layer(g), solver="tsit5", n_steps=2, dt=DT, saveat=DT)
    out = solved(d, node, vmh_params(d), d.randn(1, 96, grad=True))
    assert any(k[0] == "vmh" for k in node._plans), list(node._plans)
    return out


@case("solver: ngpde_node_gat_* through the C ABI", "ngpde_node_gat_forward", "ngpde_node_gat_backward")
def _abi_gat(d):
    lib, heads, c = _lib.load(), 2, 32
    h = tile_graph(d).handle()
    assert lib.ngpde_node_gat_supported(h.ptr, 64, heads, c) == 1
    wt, a, b = d.randn(64, 64, scale=1.5 / 8), d.randn(heads, 2 * c, scale=1.0 / np.sqrt(c)), d.randn(64, scale=0.1)
    u0, R = d.randn(96, 64), d.randn(96, 64)
    uT, du0, gw, ga, gb = (torch.empty_like(v) for v in (u0, u0, wt, a, b))
    plan = C.c_void_p()
    _lib.check(lib.ngpde_node_gat_create(h.ptr, heads, c, 0.2, _lib.ACT["tanh"], _lib.TABLEAU["tsit5"], 2, DT, 1, C.byref(plan)))
    try:
        d.rearm()
        stream = _lib.current_stream()
        _lib.check(lib.ngpde_node_gat_forward(plan, _lib.ptr(u0), _lib.ptr(wt), _lib.ptr(a), _lib.ptr(b), _lib.ptr(uT), stream))
        _lib.check(lib.ngpde_node_gat_backward(plan, _lib.ptr(wt), _lib.ptr(a), _lib.ptr(R), _lib.ptr(du0), _lib.ptr(gw), _lib.ptr(ga), _lib.ptr(gb), stream))
    finally:
        torch.cuda.current_stream().synchronize()
        _lib.check(lib.ngpde_node_gat_destroy(plan))
    return [uT, du0, gw, ga, gb]


def abi_vmh(d, save):
    """test_node_vmh_forms_gpu.run_plan with its inputs through the draws.  ngpde_node_vmh_create has no stream parameter: the caller
    completes `pos` first (include/ngpde.h, "Creates"); the other inputs go behind a new delay"""
    lib, m = _lib.load(), V.tutorial(2, pd=2, width=16, msg=8)
    h = tile_graph(d).handle()
    pos = d.rand(96, 2)
    W_ = [[d.tensor(lambda w=w: w) for w in ws] for ws in m.W]
    b_ = [[d.tensor(lambda v=v: v) for v in bs] for bs in m.b]
    T = 1 if save is None else 2 // save[0] + save[1]
    u0, R = d.randn(96), d.randn(T, 96)
    torch.cuda.current_stream().synchronize()
    plan = C.c_void_p()
    _lib.check(lib.ngpde_node_vmh_create(h.ptr, 1, m.pd, _lib.ptr(pos), *m.abi_shape(), _lib.AGGR["mean"], _lib.TABLEAU["tsit5"], 2, DT, 1, C.byref(plan)))
    d.rearm()
    out, du0 = torch.empty(T, 96, device=DEV), torch.empty(96, device=DEV)
    dW, db = [[torch.empty_like(w) for w in ws] for ws in W_], [[torch.empty_like(v) for v in bs] for bs in b_]
    wp, bp, dwp, dbp = ([_ptr_array(x) for x in k] for k in (W_, b_, dW, db))
    try:
        stream = _lib.current_stream()
        if save is None:
            _lib.check(lib.ngpde_node_vmh_forward(plan, _lib.ptr(u0), wp[0], bp[0], wp[1], bp[1], _lib.ptr(out), stream))
            _lib.check(lib.ngpde_node_vmh_backward(plan, wp[0], wp[1], _lib.ptr(R), _lib.ptr(du0), dwp[0], dbp[0], dwp[1], dbp[1], stream))
        else:
            _lib.check(lib.ngpde_node_vmh_forward_saveat(plan, _lib.ptr(u0), wp[0], bp[0], wp[1], bp[1], save[0], save[1], _lib.ptr(out), stream))
            _lib.check(lib.ngpde_node_vmh_backward_saveat(plan, wp[0], wp[1], save[0], save[1], _lib.ptr(R), _lib.ptr(du0), dwp[0], dbp[0], dwp[1], dbp[1],
                                                          stream))
    finally:
        torch.cuda.current_stream().synchronize()
        _lib.check(lib.ngpde_node_vmh_destroy(plan))
    return [out, du0, dW, db]


case("solver: ngpde_node_vmh_* through the C ABI", "ngpde_node_vmh_create", "ngpde_node_vmh_forward", "ngpde_node_vmh_backward")(lambda d: abi_vmh(d, None))
case("solver: ngpde_node_vmh_*_saveat through the C ABI", "ngpde_node_vmh_create", "ngpde_node_vmh_forward_saveat",
     "ngpde_node_vmh_backward_saveat")(lambda d: abi_vmh(d, (1, 1)))


@case("solver: the generic fixed-step path (one GCNConv, Tsit5 x 2)", "ngpde_rk_stage_combine", "ngpde_accumulate_many", "ngpde_gcn_forward",
      "ngpde_gcn_backward")
def _node_generic(d):
    g = rings(d, norms=[GCN_NORM])
    node = ng.NeuralODE(ng.Chain(ng.GCNConv((8, 8), "tanh", initialgraph=g)), solver="tsit5", n_steps=2, dt=DT)
    ps = {"layer_1": {"weight": d.randn(8, 8, grad=True, scale=0.35), "bias": d.randn(8, 1, grad=True, scale=0.1)}}
    return solved(d, node, ps, d.randn(8, N, grad=True))


def linear_rhs(d):
    """test_node_adaptive_gpu.test_linear_rhs_against_expm: d = 8, W = -0.3 I + 0.8 N(0, 1) / sqrt(d)"""
    w = d.tensor(lambda: (-0.3 * np.eye(8) + 0.8 * d.rng.normal(size=(8, 8)) / np.sqrt(8)).astype(np.float32), grad=True)
    return {"weight": w, "bias": d.randn(8, 1, grad=True, scale=0.1)}


@case("solver: the adaptive path (d = 8, linear), its statistics and pullback", "ngpde_rk_error_norm", "ngpde_rk_stage_combine", "ngpde_dense_forward",
      "ngpde_dense_backward")
def _node_adaptive(d):
    node = ng.NeuralODE(ng.Dense(8, 8), tspan=(0.0, 2.0), adaptive=True, reltol=1e-3, abstol=1e-6)
    out = solved(d, node, linear_rhs(d), d.randn(8, 64, grad=True))
    return out + [{k: v for k, v in node.stats.items()}]


# (every step reads its error estimate back before it interpolates; the C-ABI case below runs ngpde_rk_dense_output behind a delay)
@case("solver: the adaptive path with interpolated save points", "ngpde_rk_error_norm", "ngpde_rk_dense_output", "ngpde_rk_dense_output_pullback",
      drained=("ngpde_rk_dense_output",))
def _node_dense_output(d):
    node = ng.NeuralODE(ng.Dense(8, 8), tspan=(0.0, 2.0), adaptive=True, reltol=1e-3, abstol=1e-6, saveat=0.3, interpolate_saveat=True)
    out = solved(d, node, linear_rhs(d), d.randn(8, 64, grad=True))
    return out + [{k: v for k, v in node.stats.items()}]


@case("solver kernels through the C ABI: rk_error_norm, rk_stage_combine, the dense-output combine and its pullback, 4099 elements",
      "ngpde_rk_error_norm", "ngpde_rk_stage_combine", "ngpde_rk_dense_output", "ngpde_rk_dense_output_pullback")
def _rk_kernels(d):
    lib, n, stream = _lib.load(), 4099, _lib.current_stream()
    ks = [d.randn(n) for _ in range(7)]
    up, un = d.randn(n), d.randn(n)
    karr = (C.c_void_p * 7)(*[k.data_ptr() for k in ks])
    cf = (C.c_float * 7)(*[0.01 * (j + 1) * (-1) ** j for j in range(7)])
    ws = torch.empty(lib.ngpde_rk_error_norm_workspace_bytes(n), dtype=torch.uint8, device=DEV)
    norm = torch.empty(1, dtype=torch.float64, device=DEV)
    _lib.check(lib.ngpde_rk_error_norm(n, 7, karr, cf, up.data_ptr(), un.data_ptr(), 1e-6, 1e-3, ws.data_ptr(), norm.data_ptr(), stream))
    comb = torch.empty(n, device=DEV)
    _lib.check(lib.ngpde_rk_stage_combine(n, 1.0, up.data_ptr(), 7, karr, cf, comb.data_ptr(), stream))
    outs = [torch.empty(n, device=DEV) for _ in range(3)]
    cf3 = (C.c_float * 21)(*[0.02 * (j + 1) * (-1) ** j for j in range(21)])
    oarr = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
    _lib.check(lib.ngpde_rk_dense_output(n, up.data_ptr(), 7, karr, 3, cf3, oarr, stream))
    douts = [d.randn(n) for _ in range(3)]
    ubar, kbar = d.randn(n), [torch.empty(n, device=DEV) for _ in range(7)]
    darr, kbarr = (C.c_void_p * 3)(*[t.data_ptr() for t in douts]), (C.c_void_p * 7)(*[t.data_ptr() for t in kbar])
    _lib.check(lib.ngpde_rk_dense_output_pullback(n, 3, darr, 7, cf3, ubar.data_ptr(), kbarr, stream))
    return [norm, comb, outs, ubar, kbar]


# -- the optimiser and the flat-vector kernels at 4099 elements

@case("optimiser: fused Adam and Rprop, two steps each, 4099 elements", "ngpde_adam_step", "ngpde_rprop_step")
def _optimisers(d):
    out = []
    for rule in (optim.Adam(eta=0.01), optim.Rprop()):
        flat_ = optim.FlatParameters(d.randn(4099), d.randn(4099), [])
        st = optim.setup(rule, flat_)
        for _ in range(2):
            st = optim.update(st, flat_)
        out += [flat_.data, flat_.grad] + [v for v in st["state"].values()]
    return out


@case("flat-vector kernels: accumulate_many, row-block gather and scatter, transpose, rows_scale, rows_index, activation, bias_act, 4099 elements",
      "ngpde_accumulate_many", "ngpde_row_blocks_gather", "ngpde_row_blocks_scatter", "ngpde_transpose", "ngpde_rows_scale", "ngpde_rows_index",
      "ngpde_activation_forward", "ngpde_bias_act_forward", "ngpde_bias_act_backward", "ngpde_random_keys", "ngpde_spectral_weights")
def _flat_kernels(d):
    lib, stream = _lib.load(), _lib.current_stream()
    counts = [4099, 1, 64]
    accs, gs = [d.randn(c) for c in counts], [d.randn(c) for c in counts]
    _lib.check(lib.ngpde_accumulate_many(3, _ptr_array(accs), _ptr_array(gs), (C.c_int64 * 3)(*counts), stream))
    wt = d.randn(4099, 3, grad=True)
    blocks = composed.row_blocks(wt, [[(2000, [(0, 1), (2000, -1)]), (99, [(4000, 1)])], [(2000, [(2000, 1)])]])
    (blocks[0] * d.like(blocks[0])).sum().backward(retain_graph=True)
    (blocks[1] * d.like(blocks[1])).sum().backward()
    a = d.randn(4099, 5, grad=True)
    tr = pulled(d, composed.transpose(a), a)
    scaled = composed.rows_scale(d.randn(4099, 3), d.randn(4099, 1))
    x = d.randn(2, 4099, grad=True)
    index = d.ints(np.random.default_rng(1).permutation(4099)[:1000], torch.int64)
    picked = pulled(d, graphops._rows_index(x, index, 4099, False), x)
    z, act = d.randn(4099), torch.empty(4099, device=DEV)
    _lib.check(lib.ngpde_activation_forward(4099, _lib.ACT["gelu"], _lib.ptr(z), _lib.ptr(act), stream))
    s, addend, bias = d.randn(4099, 8, grad=True), d.randn(4099, 8, grad=True), d.randn(8, grad=True)
    ba = pulled(d, F.bias_act(s, addend, bias, _lib.ACT["tanh"]), s, addend, bias)
    keys = torch.empty(4099, dtype=torch.int64, device=DEV)
    _lib.check(lib.ngpde_random_keys(12345, 3, 7, 1 << 33, 4099, _lib.ptr(keys), stream))
    return [accs, blocks, wt.grad, tr, scaled, picked, act, ba, keys, F.spectral_weights(d.rand(4099, lo=0.1, hi=6.0), 8)]


# ---- the test ---------------------------------------------------------------------------------------------------------------------

DECLARED = frozenset(e for _, entries, _ in CASES.values() for e in entries)
_FAULTED = []          # the case after which the device reported an error: nothing more is launched in this process


def poison_side_pool(st):
    """torch keeps freed blocks per stream: what the side-stream run allocates first comes out of blocks that hold NaN"""
    with torch.cuda.stream(st.side):
        hold = [torch.full((1 << 18,), float("nan"), device=DEV) for _ in range(16)] + [torch.full((1 << 24,), float("nan"), device=DEV)]
        del hold
    st.side.synchronize()


@pytest.mark.parametrize("name", list(CASES))
def test_side_stream_run_equals_the_default_stream_run(name, streams, monkeypatch):
    fn, entries, drained = CASES[name]
    if _FAULTED:
        pytest.fail(f"not run: the device reported an error in {_FAULTED[0]!r}")
    try:
        run_case(name, fn, entries, drained, streams, monkeypatch)
    except Exception as e:
        if re.search(r"HIP error|hipError|illegal memory access|unspecified launch failure", str(e)):
            _FAULTED.append(name)
        raise


def run_case(name, fn, entries, drained, streams, monkeypatch):
    if name.startswith("solver"):
        needs_persistent_plan(monkeypatch)
    st = streams
    rec = Recorder(_lib.load())
    monkeypatch.setattr(_lib, "_lib", rec)
    seed = sum(name.encode()) + 1000 * len(name)
    # 1. the expected result on the default stream
    torch.manual_seed(1234)
    record = Draws(seed, monkeypatch)
    t0 = time.perf_counter()
    want = fn(record)
    wall = time.perf_counter() - t0
    torch.cuda.synchronize()
    ms = min(max(MIN_MS, WALL_FACTOR * wall * 1e3), MAX_MS)
    # 2. stale inputs
    replay = Replay(record.real, st, ms)
    poison_side_pool(st)
    torch.cuda.synchronize()
    # 3. the side-stream run
    torch.manual_seed(1234)
    with torch.cuda.stream(st.side):
        rec.expect, rec.replay = st.side.cuda_stream, replay
        try:
            replay.arm(len(replay.bufs))
            got = fn(Draws(seed, monkeypatch, replay))
        finally:
            rec.expect = None
    # 4. the comparison
    st.side.synchronize()
    torch.cuda.synchronize()
    reached = set(rec.reached)
    print(f"\n[streams] {name}: host wall {wall * 1e3:.1f} ms, delay {ms:.0f} ms x {replay.armed}, {len(record.real)} inputs, reached {sorted(reached)}, "
          f"never behind a pending delay {sorted(reached - rec.behind)}")
    assert_same(name, got, want)
    assert entries <= reached, (name, "declared but not reached:", sorted(entries - reached))
    late = entries - drained - rec.behind - set(CREATES)
    assert not late, (name, "declared, but every call found the delay run out (a read-back between the inputs and the entry):", sorted(late))
