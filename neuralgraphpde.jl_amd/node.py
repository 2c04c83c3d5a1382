"""NeuralODE -- the caller of the hot path in the reference's tutorial
(/root/reference/docs/src/tutorials/graph_node.md:44-66): `dudt(u, p, t) = model(u, p, st)` integrated
by an explicit Runge-Kutta scheme.  BASELINE configs fix the step count (Euler x 10, Tsit5 x 50); the tutorials themselves
solve with adaptive Tsit5 (graph_node.md:80-81, VMH.md:87), which NeuralODE(..., adaptive=True) runs on the generic path below.
Its saveat either cuts the steps to land on the save points (a scalar, by default) or, as DiffEq does, leaves the steps alone and
evaluates Tsit5's free interpolant at them (interpolate_saveat=True, or a vector of save times).
The pullback is the discrete adjoint of the steps taken.

When the right-hand side is Chain(GCNConv(d => d, act), GCNConv(d => d, act)) on one graph (the
tutorial's `node_chain`, graph_node.md:78) the whole solve and its adjoint run device-resident from
HIP graphs (ngpde_node_gcn2_*).  Any other right-hand side (a GAT-style layer, VMHConv as in
docs/src/tutorials/VMH.md:85-89, ...) is stepped stage by stage through the layers' own kernels with
every Runge-Kutta combination -- forward and in the discrete adjoint -- as one ngpde_rk_stage_combine
launch (_NodeGenericFn): no torch element-wise kernel on the path.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import torch

from . import _lib
from . import functional as F
from .graphs import GNNGraph
from .layers import AbstractExplicitLayer, Chain, GCNConv, check_params, rows_of
from .layers_mp import GATConv, VMHConv, _dense_stack, _node_data
from .batches import _padded_batch, _canonical_batch
from .plans import _rows_index, _check_plan_shapes, _Plan, _NodeGCN2Fn, _OdePlan, _ode_desc, _NodeOdeFn  # noqa: F401 (tools import _Plan from here)
from .plans import _PlanPool, _Recent

_TSIT5_A = [
    [],
    [0.161],
    [-0.008480655492356989, 0.335480655492357],
    [2.8971530571054935, -6.359448489975075, 4.3622954328695815],
    [5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525],
    [5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383],
]
_TSIT5_B = [0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081,
            2.324710524099774]
TABLEAUS = {"euler": ([[]], [1.0]), "tsit5": (_TSIT5_A, _TSIT5_B)}
# Tsit5's embedded error weights (OrdinaryDiffEq's btilde1..7; the seventh stage is f(u_new), FSAL): utilde = dt sum_j btilde_j k_j
# is the difference of the 5th- and 4th-order solutions, so sum_j btilde_j c_j^(q-1) = 0 for q = 1..4 and not for q = 5
_TSIT5_BTILDE = [-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629, 0.5823571654525552,
                 -0.45808210592918697, 1.0 / 66.0]


# ---- any right-hand side: explicit RK stepping with every combination as ONE library launch ---------------------------------


def _combine(base, c_self, terms, coefs, out=None):
    """out = c_self * base + sum_k coefs[k] * terms[k]  (ngpde_rk_stage_combine; row-major [N][D] float32 tensors of one size)"""
    lib = _lib.load()
    ref = base if base is not None else terms[0]
    if out is None:
        out = torch.empty_like(ref, memory_format=torch.contiguous_format)
    arr = (C.c_void_p * max(len(terms), 1))(*[t.data_ptr() for t in terms])
    cf = (C.c_float * max(len(coefs), 1))(*[float(c) for c in coefs])
    _lib.check(lib.ngpde_rk_stage_combine(ref.numel(), float(c_self), _lib.ptr(base), len(terms), arr, cf, _lib.ptr(out),
                                          _lib.current_stream()))
    return out


def _dense(t):
    """a view of `t` whose memory order is its index order (the cotangent of a (out x in) weight arrives as the transpose of
    the kernels' [in][out] array): element-wise combinations then need no copy"""
    if t.is_contiguous():
        return t
    if t.dim() == 2 and t.T.is_contiguous():
        return t.T
    return t.contiguous()


def _leaves(tree):
    out = []
    for v in tree.values():
        if isinstance(v, dict):
            out += _leaves(v)
        else:
            out.append(v)
    return out


def _graph_leaves(st):
    """the GNNGraph leaves of a state tree, in traversal order (the leaves updategraph replaces, src/utils.jl:24-31)"""
    out = []
    if isinstance(st, dict):
        for v in st.values():
            if isinstance(v, GNNGraph):
                out.append(v)
            elif isinstance(v, dict):
                out += _graph_leaves(v)
    return out


def _shared_members(g):
    """the members of a batch of graphs that share ONE structure (batch([g, g, ...]) or copies of g with other features), else None"""
    members = getattr(g, "_members", None)
    if members is not None and len(members) > 1 and all(m._handles is members[0]._handles for m in members):
        return members
    return None


def _rebuild(tree, it):
    return {k: (_rebuild(v, it) if isinstance(v, dict) else next(it)) for k, v in tree.items()}


def _fixed_schedule(node):
    """(dts, saved) of the fixed-step solve: n_steps steps of node.dt, every save_every-th one ending on a save point"""
    k = node.save_every
    return [node.dt] * node.n_steps, [bool(k) and (n + 1) % k == 0 for n in range(node.n_steps)]


def _error_norm(terms, coefs, u_prev, u_new, abstol, reltol, ws, out):
    """the scaled RMS norm of sum_j coefs[j] terms[j] (ngpde_rk_error_norm), read back: one device-to-host synchronisation"""
    arr = (C.c_void_p * len(terms))(*[t.data_ptr() for t in terms])
    cf = (C.c_float * len(coefs))(*[float(c) for c in coefs])
    _lib.check(_lib.load().ngpde_rk_error_norm(u_prev.numel(), len(terms), arr, cf, u_prev.data_ptr(), u_new.data_ptr(), float(abstol),
                                               float(reltol), ws.data_ptr(), out.data_ptr(), _lib.current_stream()))
    return float(out.item())


def _zero(ref):
    """a float32 array of ref's size holding zeros (ngpde_rk_stage_combine with no base and no terms)"""
    out = torch.empty_like(ref, memory_format=torch.contiguous_format)
    _lib.check(_lib.load().ngpde_rk_stage_combine(out.numel(), 0.0, None, 0, None, None, out.data_ptr(), _lib.current_stream()))
    return out


def tsit5_interp_coefs(theta, dt):
    """dt b_i(theta), i = 1..7: Tsit5's free interpolant over a step of size dt (ngpde_rk_tsit5_interp_coefs, in double)"""
    out = (C.c_double * 7)()
    _lib.check(_lib.load().ngpde_rk_tsit5_interp_coefs(float(theta), float(dt), out))
    return list(out)


def _dense_output(u_prev, ks, rows, outs):
    """outs[j] = u_prev + sum_i rows[j][i] ks[i] for every j (ngpde_rk_dense_output: one pass over u_prev and the stages)"""
    karr = (C.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
    cf = (C.c_float * (len(rows) * len(ks)))(*[float(c) for r in rows for c in r])
    oarr = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    _lib.check(_lib.load().ngpde_rk_dense_output(u_prev.numel(), u_prev.data_ptr(), len(ks), karr, len(outs), cf, oarr,
                                                  _lib.current_stream()))


def _dense_output_pullback(douts, rows, n_stages, ubar):
    """the stage cotangents sum_j rows[j][i] douts[j], i < n_stages, and ubar += sum_j douts[j] (ngpde_rk_dense_output_pullback)"""
    kbar = [torch.empty_like(douts[0]) for _ in range(n_stages)]
    darr = (C.c_void_p * len(douts))(*[d.data_ptr() for d in douts])
    cf = (C.c_float * (len(rows) * n_stages))(*[float(c) for r in rows for c in r])
    karr = (C.c_void_p * n_stages)(*[k.data_ptr() for k in kbar])
    _lib.check(_lib.load().ngpde_rk_dense_output_pullback(douts[0].numel(), len(douts), darr, n_stages, cf, _lib.ptr(ubar), karr,
                                                           _lib.current_stream()))
    return kbar


def _is_vector(saveat):
    return isinstance(saveat, (list, tuple)) or getattr(saveat, "ndim", 0) >= 1


def dense_save_times(tspan, saveat, save_start):
    """the save times of an interpolating solve (DiffEq's saveat): a scalar gives t0 (with save_start), t0 + k saveat for every
    k >= 1 below t_end, and t_end, a point within 1e-12 (t_end - t0) of t_end counting as t_end; a vector gives its own times, t0
    dropped when save_start is False"""
    t0, t1 = float(tspan[0]), float(tspan[1])
    if _is_vector(saveat):
        times = [float(s) for s in saveat]
        return times[1:] if (times and times[0] == t0 and not save_start) else times
    saveat, span = float(saveat), t1 - t0
    times = [t0] if save_start else []
    k = 1
    while t0 + k * saveat < t1 - 1e-12 * span:
        times.append(t0 + k * saveat)
        k += 1
    return times + [t1]


def saves_in_step(times, j, t_n, t_next, dt):
    """the save times of the accepted step [t_n, t_next] of size dt, from times[j] on: (interior [(slot, theta)] with t_n < s <
    t_next and theta = (s - t_n) / dt, the slot of s == t_next or None, the next j).  A time equal to the step's end is the step's
    state itself (DiffEq's curt == t); theta is clamped to [0, 1] against the last bit of t_n + dt."""
    interior = []
    while j < len(times) and times[j] < t_next:
        interior.append((j, min(max((times[j] - t_n) / dt, 0.0), 1.0)))
        j += 1
    end = None
    if j < len(times) and times[j] == t_next:
        end, j = j, j + 1
    return interior, end, j


class _Control:
    """the library's step-size controller (ngpde_rk_control_*) for one adaptive solve (an interpolating solve stops at t_end only)"""

    def __init__(self, node):
        self.state = _lib.RkControl()
        t0, t1 = node.tspan
        saveat = 0.0 if node.save_times is not None else float(node.saveat or 0.0)
        _lib.check(_lib.load().ngpde_rk_control_init(C.byref(self.state), float(t0), float(t1), float(node.dt or 0.0),
                                                     float(node.dtmax or 0.0), saveat, int(node.maxiters)))

    def trial_dt(self, d0, d1):
        dt0 = C.c_double()
        _lib.check(_lib.load().ngpde_rk_control_trial_dt(C.byref(self.state), d0, d1, C.byref(dt0)))
        return dt0.value

    def initial_dt(self, d0, d1, norm_df):
        _lib.check(_lib.load().ngpde_rk_control_initial_dt(C.byref(self.state), d0, d1, norm_df))

    def step(self, eest):
        action = C.c_int32()
        _lib.check(_lib.load().ngpde_rk_control_step(C.byref(self.state), eest, C.byref(action)))
        return action.value


def _rk_forward(node, u, ps_in, st, needs, fresh=False):
    """u(T) (or the saved states) of the solve; with `needs` also the tape: per step and stage the (stage input, stage output) pair
    whose autograd closure is the layers' pullback.  The last item is the schedule (dts, saved) of the steps taken: fixed, or the
    accepted steps of an adaptive solve -- an interpolating one (node.save_times) adds a third item, its record of the saves: the
    slot of t0, per step the slot its end fills and its interpolated (slots, coefficient rows), the final step's seventh-stage
    pair when that step interpolates.  fresh: the stage inputs get version counters of their own (a captured solve refills its
    static input buffer before every replay; the closures are only ever run at capture time)"""
    a, b = TABLEAUS[node.solver]
    S = len(b)
    ucur, tape, st_out = u, [], st
    saving = node.saving
    saves = [ucur] if (saving and node.save_start) else []      # saveat: the states at t0 (+ j saveat), as DiffEq's sol.u
    times = node.save_times if node.adaptive else None
    dense = None
    if times is not None:    # interpolating saveat: the output is filled step by step (the steps are the solve's own)
        saves = []
        out = torch.empty((len(times),) + tuple(ucur.shape), dtype=ucur.dtype, device=ucur.device)
        dense = dict(t0=None, end=[], interp=[], last=None)
        jt = 0
        if times and times[0] == float(node.tspan[0]):
            dense["t0"], jt = 0, 1
            _combine(ucur, 1.0, [], [], out=out[0])

    def stage(U):
        nonlocal st_out
        if needs:
            U = (U.data if fresh else U.detach()).requires_grad_(True)
        k, st_out = node.model(U.T, ps_in, st_out)
        k = rows_of(k)
        if k.shape != ucur.shape:
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH,
                                         f"DimensionMismatch: the right-hand side maps {tuple(ucur.shape[::-1])} to "
                                         f"{tuple(k.shape[::-1])}; du/dt must have the shape of u")
        return U, k

    dts, saved = ([], []) if node.adaptive else _fixed_schedule(node)
    ctl, first, nf, eests, init_norms = None, None, 0, [], None
    with (torch.enable_grad() if needs else torch.no_grad()):
        if node.adaptive:
            ctl = _Control(node)
            ws = torch.empty(max(int(_lib.load().ngpde_rk_error_norm_workspace_bytes(ucur.numel())), 8), dtype=torch.uint8, device=ucur.device)
            eout = torch.empty(1, dtype=torch.float64, device=ucur.device)
            tol = (node.abstol, node.reltol)
            first = stage(ucur)                      # f0: the first step's first stage
            nf = 1
            if node.dt is None:                      # Hairer-Norsett-Wanner's starting step (ode_determine_initdt, order 5)
                f0 = first[1].detach()
                d0 = _error_norm([ucur], [1.0], ucur, ucur, *tol, ws, eout)
                d1 = _error_norm([f0], [1.0], ucur, ucur, *tol, ws, eout)
                dt0 = ctl.trial_dt(d0, d1)
                with torch.no_grad():
                    f1 = rows_of(node.model(_combine(ucur, 1.0, [f0], [dt0]).T, ps_in, st_out)[0])
                nf += 1
                init_norms = (d0, d1, _error_norm([f1, f0], [1.0, -1.0], ucur, ucur, *tol, ws, eout))
                ctl.initial_dt(*init_norms)
                del f1
        n_step = 0
        while ctl is not None or n_step < len(dts):
            dt = ctl.state.dt if ctl is not None else dts[n_step]
            ks, pairs = [], []
            for i in range(S):
                if i == 0 and first is not None:      # FSAL: f(u_new) of the last accepted step, or f0
                    U, k = first
                else:
                    terms = [ks[j] for j in range(i) if a[i][j] != 0.0]
                    coefs = [dt * a[i][j] for j in range(i) if a[i][j] != 0.0]
                    U, k = stage(_combine(ucur, 1.0, terms, coefs) if terms else ucur)
                ks.append(k.detach())
                pairs.append((U, k))
            unew = _combine(ucur, 1.0, ks, [dt * bi for bi in b])
            if ctl is not None:
                last = stage(unew)                   # the seventh stage: the embedded estimate's, and the next step's first
                nf += S
                eest = _error_norm(ks + [last[1].detach()], [dt * bt for bt in _TSIT5_BTILDE], ucur, unew, *tol, ws, eout)
                eests.append(eest)
                t_n = ctl.state.t
                action = ctl.step(eest)              # (raises NgpdeError(ERR_STATE) when maxiters / dtmin end the solve)
                if action == _lib.RK_REJECT:
                    first = pairs[0]                 # the attempt's other stages are dropped
                    continue
                first = last
                dts.append(dt)
                saved.append(bool(ctl.state.saved))
                if dense is not None:
                    # Tsit5's free interpolant over [t_n, t_n + dt] at the step's interior save times, k_7 = f(u_new): one launch
                    # writing into the output; a save time on the step's end is u_new itself
                    interior, end, jt = saves_in_step(times, jt, t_n, ctl.state.t, dt)
                    rows = [tsit5_interp_coefs(th, dt) for _, th in interior]
                    if interior:
                        _dense_output(ucur, ks + [last[1].detach()], rows, [out[sl] for sl, _ in interior])
                        if needs and action == _lib.RK_DONE:
                            dense["last"] = last     # the final step's seventh stage: its pullback carries g_7 (no step n+1 does)
                    if end is not None:
                        _combine(unew, 1.0, [], [], out=out[end])
                    dense["end"].append(end)
                    dense["interp"].append(([sl for sl, _ in interior], rows) if interior else None)
            ucur = unew
            if needs:
                tape.append(pairs)
            if saved[n_step]:
                saves.append(ucur)
            n_step += 1
            if ctl is not None and action == _lib.RK_DONE:
                break
    if ctl is not None:
        c = ctl.state
        node.stats = dict(naccept=int(c.naccept), nreject=int(c.nreject), nf=nf, dts=list(dts), t=float(c.t), eests=eests,
                          init_norms=init_norms)
        if dense is not None:
            assert jt == len(times)
            node.stats.update(save_times=list(times), ninterp=sum(len(r[0]) for r in dense["interp"] if r is not None))
    if dense is not None:
        return out, tape, st_out, (dts, saved, dense)
    if saving:      # [T][N][D]: the memory layout of the reference's (D x N x T) array; rows written by library launches
        out = torch.empty((len(saves),) + tuple(ucur.shape), dtype=ucur.dtype, device=ucur.device)
        for j, s_ in enumerate(saves):
            _combine(s_, 1.0, [], [], out=out[j])
        ucur = out
    return ucur, tape, st_out, (dts, saved)


def _accumulate_many(pairs):
    """acc += g for every (acc, g) pair of dense float32 tensors of equal size (ngpde_accumulate_many: one launch per 24 arrays)"""
    if not pairs:
        return
    for a_, g_ in pairs:
        if a_.numel() != g_.numel() or a_.dtype != torch.float32 or g_.dtype != torch.float32:
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, "parameter cotangent and its accumulator differ in size or type")
    n = len(pairs)
    accs = (C.c_void_p * n)(*[a_.data_ptr() for a_, _ in pairs])
    gs = (C.c_void_p * n)(*[g_.data_ptr() for _, g_ in pairs])
    cnt = (C.c_int64 * n)(*[a_.numel() for a_, _ in pairs])
    _lib.check(_lib.load().ngpde_accumulate_many(n, accs, gs, cnt, _lib.current_stream()))


def _rk_backward(node, tape, duT, params, schedule, retain=False):
    """discrete adjoint of _rk_forward over the steps of `schedule` (dts, saved[, dense]), their sizes held fixed: (du0, cotangents
    of `params`).  An interpolating solve's saves inside step n are pulled back by one ngpde_rk_dense_output_pullback launch into g_1..g_7
    and a cotangent of u_n: g_i joins stage i's K-bar, g_7 -- the cotangent of f(u_{n+1}) -- joins the first stage's K-bar of step n + 1
    (the same evaluation, FSAL), or for the final step the taped seventh stage's pullback before the reverse sweep starts."""
    a, b = TABLEAUS[node.solver]
    S = len(b)
    dts, saved = schedule[:2]
    dense = schedule[2] if len(schedule) > 2 else None
    acc = [None] * len(params)
    saving = node.saving

    def absorb(grads):
        pairs_ag = []
        for n, g in enumerate(grads):
            if g is None:
                continue
            if acc[n] is None:
                # own the accumulator in a layout _dense can view without a copy (an expanded / strided cotangent would make
                # _dense return a temporary, and the sum written into it would be lost)
                acc[n] = g if (g.is_contiguous() or (g.dim() == 2 and g.T.is_contiguous())) else g.contiguous()
            elif acc[n].stride() == g.stride():
                # same layout for every stage's cotangent of one parameter: add in memory order
                pairs_ag.append((_dense(acc[n]), _dense(g)))
            else:       # layouts differ (one transposed, one not): index-wise sum in the accumulator's own layout
                pairs_ag.append((_dense(acc[n]), _dense(g.contiguous() if acc[n].is_contiguous() else g.T.contiguous().T)))
        _accumulate_many(pairs_ag)      # ONE launch for all parameters of this stage (sixteen arrays in the VMH tutorial's model)

    if dense is None:
        # slot of duT holding the cotangent of u_n, the state at the start of step n (None: not saved)
        n_saved = 1 if node.save_start else 0
        slot, start_slot = (0 if node.save_start else None), []
        for n in range(len(dts)):
            start_slot.append(slot)
            slot, n_saved = (n_saved, n_saved + 1) if saved[n] else (None, n_saved)
        lam = duT[n_saved - 1] if saving else duT     # (a solve with saveat ends on its last save point)
    else:
        start_slot = [dense["t0"]] + dense["end"][:-1]
        lam = duT[dense["end"][-1]] if dense["end"][-1] is not None else _zero(duT[0])
    pulled = {}      # step -> (g_1..g_7, the cotangent of u_n) of its interpolated saves

    def pull(n):
        if dense is not None and n >= 0 and dense["interp"][n] is not None:
            slots, rows = dense["interp"][n]
            h = _zero(duT[0])
            pulled[n] = (_dense_output_pullback([duT[sl] for sl in slots], rows, S + 1, h), h)

    if dense is not None:
        pull(len(dts) - 1)
        if len(dts) - 1 in pulled:         # the final step's seventh stage f(u_N): its taped pair, K-bar = g_7
            U, k = dense["last"]
            grads = torch.autograd.grad(k, [U] + params, pulled[len(dts) - 1][0][S], allow_unused=True, retain_graph=retain)
            absorb(grads[1:])
            if grads[0] is not None:
                lam = _combine(lam, 1.0, [grads[0].contiguous()], [1.0])
    for n_step, pairs in zip(range(len(tape) - 1, -1, -1), reversed(tape)):
        dt = dts[n_step]
        pull(n_step - 1)                   # step n - 1's g_7 is a cotangent of this step's first stage
        ubar = [None] * S
        for i in reversed(range(S)):
            terms = [ubar[j] for j in range(i + 1, S) if a[j][i] != 0.0 and ubar[j] is not None]
            coefs = [dt * a[j][i] for j in range(i + 1, S) if a[j][i] != 0.0 and ubar[j] is not None]
            if n_step in pulled:
                terms.append(pulled[n_step][0][i])
                coefs.append(1.0)
            if i == 0 and n_step - 1 in pulled:
                terms.append(pulled[n_step - 1][0][S])
                coefs.append(1.0)
            if b[i] == 0.0 and not terms:
                continue
            kbar = _combine(lam, dt * b[i], terms, coefs)
            U, k = pairs[i]
            grads = torch.autograd.grad(k, [U] + params, kbar, allow_unused=True, retain_graph=retain)
            if grads[0] is not None:
                ubar[i] = grads[0].contiguous()
            absorb(grads[1:])
        live = [x for x in ubar if x is not None]
        if saving and start_slot[n_step] is not None:
            live.append(duT[start_slot[n_step]])              # lambda(t_n) also carries the cotangent of the state saved there
        if n_step in pulled:
            live.append(pulled.pop(n_step)[1])                # ... and that of u_n in the step's interpolated saves
        if live:
            lam = _combine(lam, 1.0, live, [1.0] * len(live))
    return lam, acc


def _inner_params(ps, leaves, fresh=False):
    """aliases of the parameters that are leaves of the stages' autograd closures, and the tree holding them (fresh: with
    version counters of their own, so that an optimiser's in-place update between the captures does not invalidate them)"""
    inner = [(p.data if fresh else p.detach()).requires_grad_(p.requires_grad) if isinstance(p, torch.Tensor) else p for p in leaves]
    return inner, _rebuild(ps, iter(inner))


class _NodeGenericFn(torch.autograd.Function):
    """Explicit Runge-Kutta solve of du/dt = model(u) for ANY model made of this package's layers -- fixed-step, or adaptive Tsit5 --
    and its discrete adjoint.  Forward: the stage inputs u + dt sum_j a_ij k_j and the step update are one ngpde_rk_stage_combine launch each,
    the stages are the layers' own kernels; every stage keeps its (input, output) pair with the layer's pullback closure.
    Backward: per stage, in reverse, K-bar_i = dt b_i lambda + dt sum_{j>i} a_ji U-bar_j (one launch), U-bar_i and the parameter
    cotangents from the stage's pullback (the layers' backward kernels), parameter gradients accumulated by one launch each,
    lambda += sum_j U-bar_j (one launch).  No torch element-wise kernel takes part.
    [docs/src/tutorials/VMH.md:85-89 NeuralODE(VMHConv); graph_node.md:44-66; BASELINE config 3 "GAT as ODE RHS"]"""

    @staticmethod
    def forward(ctx, u, node, ps, st, *leaves):
        needs = any(ctx.needs_input_grad)
        inner, ps_in = _inner_params(ps, leaves) if needs else (list(leaves), ps)
        uT, tape, _, schedule = _rk_forward(node, u.detach().contiguous(), ps_in, st, needs)
        ctx.node, ctx.tape, ctx.inner, ctx.schedule = node, tape if needs else None, inner, schedule
        return uT

    @staticmethod
    def backward(ctx, duT):
        params = [p for p in ctx.inner if isinstance(p, torch.Tensor) and p.requires_grad]
        lam, acc = _rk_backward(ctx.node, ctx.tape, duT.contiguous(), params, ctx.schedule)
        ctx.tape = None
        it = iter(acc)
        out = [next(it) if (isinstance(p, torch.Tensor) and p.requires_grad) else None for p in ctx.inner]
        return (lam, None, None, None, *out)


class _NoCyclicGC:
    """No cyclic garbage collection while a HIP graph is being captured: a collection in the middle of a capture may finalise an older
    captured solve, and destroying ITS graphs is an operation the capturing stream does not permit (the capture dies with
    hipErrorStreamCaptureUnsupported).  torch.cuda.graph collects once before the capture starts; this keeps it that way until it ends."""

    def __enter__(self):
        import gc
        self.was = gc.isenabled()
        gc.disable()

    def __exit__(self, *exc):
        import gc
        if self.was:
            gc.enable()
        return False


class _CapturedSolve:
    """The generic solve as two HIP graphs (NeuralODE(..., capture=True)): the forward stepping loop -- every layer launch
    and every Runge-Kutta combination of all steps -- is captured once and replayed per call, and so is the whole discrete
    adjoint the first time a backward pass asks for it.  Static buffers: the input is copied in, u(T) and the cotangents are
    the graphs' own buffers (valid until the next call of the same NeuralODE on the same arguments).  The captures bake in the
    addresses of the parameters and of the graph's derived arrays: a call with other parameter tensors, another graph or
    another input shape captures anew (NeuralODE keeps the most recent few)."""

    def __init__(self, node, u, ps, st, leaves, needs):
        self.node, self.needs = node, needs
        self.leaves = list(leaves)                         # keeps the captured addresses alive
        self.inner, self.ps_in = _inner_params(ps, leaves, fresh=True) if needs else (list(leaves), ps)
        self.params = [p for p in self.inner if isinstance(p, torch.Tensor) and p.requires_grad] if needs else []
        self.u_static = u.detach().clone()
        self.st = st
        # one eager solve on a side stream first: graph handles, workspaces and lazily built tables exist before the capture
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            _rk_forward(node, self.u_static, self.ps_in, st, False)
        torch.cuda.current_stream().wait_stream(side)
        self.fwd_graph = torch.cuda.CUDAGraph()
        # (relaxed: a finaliser that frees device memory in the middle of the capture must not invalidate it)
        with _NoCyclicGC(), torch.cuda.graph(self.fwd_graph, capture_error_mode="relaxed"):
            self.uT_static, self.tape, _, self.schedule = _rk_forward(node, self.u_static, self.ps_in, st, needs, fresh=True)
        self.bwd_graph = None
        self.generation = 0                                # forward replays so far: the single static tape belongs to the last one

    def forward(self, u):
        self.u_static.copy_(u)
        self.fwd_graph.replay()
        self.generation += 1
        return self.uT_static

    def backward(self, duT, generation):
        if generation != self.generation:
            # `y1 = node(u1); y2 = node(u2); (y1 + y2).backward()`: the second replay has overwritten the first solve's tape
            raise _lib.NgpdeError(_lib.ERR_STATE, "NeuralODE(capture=True): another forward solve has replaced this solve's tape "
                                                  "(a captured solve holds ONE tape); run each backward before the next forward "
                                                  "on the same arguments, or use capture=False")
        if self.bwd_graph is None:
            self.duT_static = duT.detach().clone()
            self.bwd_graph = torch.cuda.CUDAGraph()
            with _NoCyclicGC(), torch.cuda.graph(self.bwd_graph, pool=self.fwd_graph.pool(), capture_error_mode="relaxed"):
                self.lam_static, self.acc_static = _rk_backward(self.node, self.tape, self.duT_static, self.params, self.schedule,
                                                                retain=True)
        else:
            self.duT_static.copy_(duT)
        self.bwd_graph.replay()
        return self.lam_static, self.acc_static


class _NodeCapturedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, solve, *leaves):
        ctx.solve = solve
        uT = solve.forward(u.detach().contiguous()).clone()
        ctx.generation = solve.generation
        return uT

    @staticmethod
    def backward(ctx, duT):
        lam, acc = ctx.solve.backward(duT.contiguous(), ctx.generation)
        it = iter(acc)
        out = [next(it) if (isinstance(p, torch.Tensor) and p.requires_grad) else None for p in ctx.solve.inner]
        return (lam.clone(), None, *[None if g is None else g.clone() for g in out])


class NeuralODE(AbstractExplicitLayer):
    """NeuralODE(model; solver="tsit5", tspan=(0, 1), n_steps=..., dt=None)

    A Lux container with the single field `model`, so `ps` and `st` are the model's own
    (graph_node.md:44-52, :59-66).  `solver` is "euler" or "tsit5"; the step is fixed:
    dt = (tspan[1] - tspan[0]) / n_steps unless given.  capture=True (an extension, for right-hand sides other than the
    two-GCNConv chain, which is always device-resident): the whole solve and its adjoint are captured into HIP graphs at
    the first call and replayed afterwards (_CapturedSolve).

    adaptive=True (graph_node.md:80-81, VMH.md:87): Tsit5 with step-size control, DiffEq's names and defaults -- reltol=1e-3,
    abstol=1e-6 (scalars), dtmax=None (t_end - t0), maxiters=100_000 (attempts, rejected ones included); dt is the first step
    (None: Hairer-Norsett-Wanner's choice) and n_steps is ignored.  Every attempt forms the stages as the fixed step does, evaluates
    f(u_new) (the next step's first stage), gets EEst from one ngpde_rk_error_norm launch pair and reads it back (one synchronisation
    per attempt); the library's controller (ngpde_rk_control_step, OrdinaryDiffEq's PI controller) accepts or rejects.  saveat has
    two meanings here.  Landing (a scalar saveat, interpolate_saveat=None or False): the steps are cut to end on t0 + k saveat, which
    must divide tspan.  Interpolating (interpolate_saveat=True, or a 1-D sequence of strictly increasing times in tspan, which always
    interpolates), DiffEq's own: the steps are those of the same solve without saveat, and a save time inside an accepted step is
    Tsit5's free 4th-order interpolant there (ngpde_rk_dense_output, no extra right-hand-side evaluation); a save time on a step's
    end is that step's state.  A scalar gives t0 + k saveat below t_end and t_end (it need not divide tspan), a vector its own times
    (t0 and t_end only when listed); save_start=False drops t0.  It always runs the generic path (the device-resident plans are
    fixed-step), and capture=True is refused: the step count depends on the data.  The pullback is the discrete adjoint of the
    accepted steps with their sizes held fixed -- rejected attempts contribute nothing and the controller is not differentiated; the
    reference's InterpolatingAdjoint is a continuous adjoint, so the gradients differ by O(tol).  NeuralODE.stats holds the last
    solve's naccept, nreject, nf, accepted step sizes (dts) and final t, as DiffEq's sol.stats (and every attempt's EEst, and the
    starting step's three norms when it was chosen; an interpolating solve adds its save_times and ninterp, the saves interpolated).
    """

    def __init__(self, model, *, solver="tsit5", tspan=(0.0, 1.0), n_steps=10, dt=None, capture=False, saveat=None, save_start=True,
                 adaptive=False, reltol=1e-3, abstol=1e-6, dtmax=None, maxiters=100_000, interpolate_saveat=None):
        solver = solver.lower()
        if solver not in TABLEAUS:
            raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, f"unknown solver {solver!r}; one of {list(TABLEAUS)}")
        self.model, self.solver, self.tspan, self.n_steps = model, solver, tuple(tspan), int(n_steps)
        self.adaptive, self.saveat, self.stats = bool(adaptive), None, None
        self.save_times, self.interpolate_saveat = None, False     # (an interpolating adaptive solve's save times)
        self._plans, self._no_member_plan = _PlanPool(), False
        self.capture = bool(capture)      # generic right-hand sides: replay the whole solve / adjoint from HIP graphs (adaptive: refused)
        self._captured = _Recent()
        self._gat_ok = _Recent()          # (id(graph handle), heads) -> (handle, does the device-resident GAT solver take it?)
        if self.adaptive:
            self._init_adaptive(dt, capture, saveat, save_start, reltol, abstol, dtmax, maxiters, interpolate_saveat)
            return
        if interpolate_saveat is not None or _is_vector(saveat):
            raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, "NeuralODE: a vector saveat and interpolate_saveat need adaptive=True "
                                                                "(a fixed-step solve lands on its save points)")
        self.dt = float(dt) if dt is not None else (self.tspan[1] - self.tspan[0]) / self.n_steps
        # saveat (VMH.md:85 `NeuralODE(gnn, tspan, Tsit5(); saveat=dt_train)`): the output is the solution at t0, t0 + saveat, ..., T --
        # a (D x N x T) array -- instead of u(T).  The step is fixed, so saveat must be a whole number of steps.
        self.save_every, self.save_start = 0, bool(save_start)
        if saveat is not None:
            k = round(float(saveat) / self.dt)
            if k < 1 or abs(k * self.dt - float(saveat)) > 1e-6 * max(abs(float(saveat)), 1.0) or self.n_steps % k:
                raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, f"NeuralODE: saveat = {saveat} must be a whole number of steps "
                                                                  f"(dt = {self.dt}) that divides n_steps = {self.n_steps}")
            self.save_every = k

    def _init_adaptive(self, dt, capture, saveat, save_start, reltol, abstol, dtmax, maxiters, interpolate_saveat):
        def bad(msg):
            return _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, f"NeuralODE(adaptive=True): {msg}")
        if self.solver != "tsit5":
            raise bad(f"solver {self.solver!r} has no embedded error estimate; adaptive stepping takes \"tsit5\"")
        if capture:
            raise bad("capture=True needs a fixed step count (one captured graph); an adaptive solve's depends on the data")
        for name, v in (("reltol", reltol), ("abstol", abstol)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not math.isfinite(v) or v < 0:
                raise bad(f"{name} must be a finite scalar >= 0 (vector tolerances are not supported), got {v!r}")
        if reltol == 0 and abstol == 0:
            raise bad("reltol and abstol are both 0")
        for name, v in (("dt", dt), ("dtmax", dtmax)):
            if v is not None and not (isinstance(v, numbers.Real) and math.isfinite(v) and v > 0):
                raise bad(f"{name} must be a finite step > 0 or None, got {v!r}")
        if int(maxiters) < 1:
            raise bad(f"maxiters must be >= 1, got {maxiters!r}")
        self.reltol, self.abstol = float(reltol), float(abstol)
        self.dt = float(dt) if dt is not None else None
        self.dtmax = float(dtmax) if dtmax is not None else None
        self.maxiters = int(maxiters)
        if interpolate_saveat is not None and not isinstance(interpolate_saveat, bool):
            raise bad(f"interpolate_saveat must be None, True or False, got {interpolate_saveat!r}")
        vector = _is_vector(saveat)
        if vector:
            if interpolate_saveat is False:
                raise bad("a vector saveat is always interpolated (the steps cannot land on arbitrary times); interpolate_saveat=False "
                          "takes a scalar saveat")
            if getattr(saveat, "ndim", 1) != 1:
                raise bad(f"saveat must be a scalar or a 1-D sequence of times, got {getattr(saveat, 'ndim', '?')} dimensions")
            times = list(saveat.tolist() if hasattr(saveat, "tolist") else saveat)
            if not all(isinstance(v, numbers.Real) and not isinstance(v, bool) for v in times):
                raise bad(f"saveat must be a scalar or a 1-D sequence of times, got {saveat!r}")
            times = [float(v) for v in times]
            t0, t1 = float(self.tspan[0]), float(self.tspan[1])
            if not times:
                raise bad("saveat is an empty vector")
            if not all(math.isfinite(v) and t0 <= v <= t1 for v in times):
                raise bad(f"every saveat time must lie in tspan [{t0}, {t1}], got {times!r}")
            if any(b_ <= a_ for a_, b_ in zip(times, times[1:])):
                raise bad(f"saveat times must be strictly increasing, got {times!r}")
            saveat = tuple(times)
        elif interpolate_saveat:
            if saveat is None:
                raise bad("interpolate_saveat=True without saveat")
            if isinstance(saveat, bool) or not isinstance(saveat, numbers.Real) or not math.isfinite(saveat) or saveat <= 0:
                raise bad(f"saveat must be a finite spacing > 0, got {saveat!r}")
            if (self.tspan[1] - self.tspan[0]) / float(saveat) > 1e7:
                raise bad(f"saveat = {saveat} makes more than 1e7 save points")
        self.saveat = saveat if vector else (float(saveat) if saveat is not None else None)
        self.save_every, self.save_start = 0, bool(save_start)
        self.interpolate_saveat = vector or bool(interpolate_saveat)
        if self.interpolate_saveat:
            self.save_times = dense_save_times(self.tspan, self.saveat, self.save_start)
        _Control(self)        # the library checks tspan and, when the steps land on them, that saveat divides it (ArgumentError)

    @property
    def saving(self):
        """does the solve return the states at the save points (saveat) rather than u(T)?"""
        return bool(self.save_every) or self.saveat is not None

    def initialparameters(self, rng):
        return self.model.initialparameters(rng)

    def initialstates(self, rng):
        return self.model.initialstates(rng)

    def statelength(self):
        return self.model.statelength()

    # -- is the right-hand side the tutorial's two-GCNConv chain on one graph? ---------------------
    max_plans = 2   # cached solver-plan keys per NeuralODE (forward-only and forward+backward of the current graph)
    max_outstanding = 8   # plans per key: one per solve whose backward is still outstanding (each owns a tape)

    def _gcn2(self, ps, st):
        m = self.model
        if not (isinstance(m, Chain) and len(m.chain) == 2 and all(isinstance(l, GCNConv) for l in m.chain)):
            return None
        l1, l2 = m.chain
        d = l1.in_chs
        same = (l1.out_chs == d and l2.in_chs == d and l2.out_chs == d and l1.act == l2.act
                and l1.add_self_loops == l2.add_self_loops and l1.use_edge_weight == l2.use_edge_weight
                and l1.bias == l2.bias)
        if not same or d not in (16, 32, 64, 128):
            return None
        g1, g2 = st["layer_1"]["graph"], st["layer_2"]["graph"]
        # copies made by wrapgraph / updategraph share one handle cache: same structure without comparing arrays
        if g1 is not g2 and g1._handles is not g2._handles and g1 != g2:
            return None
        if l1.use_edge_weight and (g1.edge_weight is None or g2.edge_weight is not g1.edge_weight):
            return None      # (the generic solver raises the layer's own error / handles two weight vectors)
        return l1, g1, d

    def plan_for(self, ps, st, with_backward):
        info = self._gcn2(ps, st)
        if info is None:
            return None
        l1, g, d = info
        # use_edge_weight=true: the graph's stored weights in the messages, the unweighted degree in the normalisation
        # (src/layers.jl:224 vs :230, as GCNConv.__call__ does); the plan's kernels read them from the handle's slot lists
        norm = (l1.add_self_loops, g.edge_weight if l1.use_edge_weight else None, False)
        # a batch that shares ONE structure: the plan is built on the member and solves the trajectories one after the other inside
        # its persistent launches
        members = None if (self._no_member_plan or l1.use_edge_weight) else _shared_members(g)
        handle = members[0].handle(norm) if members else g.handle(norm)
        n_members = len(members) if members else 1
        key = (id(handle), d, l1.act, bool(with_backward), n_members)
        make = lambda: _Plan(handle, d, l1.act, self.solver, self.n_steps, self.dt, with_backward, members=n_members)
        try:
            return self._plans.acquire(key, with_backward, make, self)
        except _lib.NgpdeError as e:
            if not (members and e.code == _lib.ERR_UNSUPPORTED):
                raise
            self._no_member_plan = True     # not a case of the persistent plan: one handle for the whole batch instead
            return self.plan_for(ps, st, with_backward)

    def _solve_gcn2(self, u, ps, st, needs_grad):
        """u(T) as (D x N) through the device-resident plan of the two-GCNConv chain; None when the right-hand side is not that chain"""
        plan = self.plan_for(ps, st, needs_grad)
        if plan is None:
            return None
        if not u.is_cuda:
            raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, "NeuralODE: inputs must live on the GPU (no CPU fallback)")
        (w1, b1), (w2, b2) = (l.kernel_params(ps[n]) for n, l in zip(self.model.names(), self.model.chain))
        # the plan's entries take no sizes (they walk the handle's rows): what GCNConv.__call__ would have checked
        # (check_num_nodes, the matrix product's own DimensionMismatch) is checked here, before any kernel runs
        d = self.model.chain[0].in_chs
        _check_plan_shapes("NeuralODE(GCNConv, GCNConv)", u, plan.n_nodes * plan.members, d,
                           [("layer_1.weight", w1, (d, d)), ("layer_2.weight", w2, (d, d))],
                           [("layer_1.bias", b1, d), ("layer_2.bias", b2, d)])
        return _NodeGCN2Fn.apply(u, w1, b1, w2, b2, plan).T

    def _solve_gat(self, u, ps, st, needs_grad):
        """u(T) as (D x N) through the device-resident plan when the right-hand side is ONE GAT-style layer in the one-launch shape (64 =>
        heads x c = 64, concat, tiles fit the LDS halo) and the library takes it (ngpde_node_gat_supported); None otherwise"""
        m = self.model
        if isinstance(m, Chain) and len(m.chain) == 1 and isinstance(m.chain[0], GATConv):    # Chain(GATConv(...)): the same solve
            m, ps, st = m.chain[0], ps["layer_1"], st["layer_1"]
        if not (isinstance(m, GATConv) and m.concat and u.is_cuda and m.in_chs == 64 and m.heads * m.out_chs == 64):
            return None
        g = st["graph"]
        members = _shared_members(g)      # the plan is built on the member, two members per workgroup
        handle = m._graph(members[0] if members else g).handle()
        n_members = len(members) if members else 1
        key = ("gat", id(handle), m.heads, m.act, m.negative_slope, bool(needs_grad), n_members)
        if key not in self._plans:
            # asked once per (graph handle, head count) of this NeuralODE: the check compares the two directions' schedules on the
            # device and synchronises (the entry keeps the handle alive, so its id cannot be recycled)
            ok = self._gat_ok.get((id(handle), m.heads))
            if ok is None:
                ok = self._gat_ok.put((id(handle), m.heads),
                                      (handle, bool(_lib.load().ngpde_node_gat_supported(handle.ptr, 64, m.heads, m.out_chs))), 8)
            if not ok[1]:
                return None
        make = lambda: _OdePlan(handle, _ode_desc(_lib.RHS_GAT, self.solver, self.n_steps, self.dt, needs_grad, n_members, width=64, act=int(m.act),
                                                  heads=int(m.heads), head_width=int(m.out_chs), negative_slope=float(m.negative_slope)), "gat")
        plan = self._plans.acquire(key, needs_grad, make, self)      # (what the create raises goes to the caller)
        w, a, b = m.kernel_params(ps)
        _check_plan_shapes("NeuralODE(GATConv)", u, plan.n_nodes * plan.members, 64, [("weight", w, (64, 64))], [("bias", b, 64)])
        if a.numel() != 2 * m.out_chs * m.heads:
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, f"DimensionMismatch: NeuralODE(GATConv): attention vector has "
                                         f"{a.numel()} entries, expected 2 x {m.out_chs} x {m.heads}")
        return _NodeOdeFn.apply(u, plan, None, a, w, b).T

    def _vmh_plan(self, ps, st, u, needs_grad):
        """the device-resident plan when the right-hand side is VMHConv(phi, gamma) on a scalar state in the shapes the library takes
        (ngpde_node_vmh_supported: docs/src/tutorials/VMH.md:75-89's model); (plan, weights and biases, a padded batch's index map) or None"""
        m = self.model
        if not (isinstance(m, VMHConv) and u.is_cuda and u.dim() == 2 and u.shape[1] == 1):
            return None
        g = st["graph"]
        if list(g.ndata) != ["x"]:      # (a batched graph is one block-diagonal graph to this plan: its members' tiles never neighbour)
            return None
        remap = _canonical_batch(g, u.device)      # the members of an earlier batch in a new order: that batch's graph and plan serve
        nodemap, g_given = None, g
        if remap is not None:
            g, nodemap = remap
        try:
            phi, gam = _dense_stack(m.ϕ, ps["ϕ"], "ϕ"), _dense_stack(m.γ, ps["γ"], "γ")
        except _lib.NgpdeError:
            return None
        pos = _node_data(g, u.device)
        pd = pos.shape[1]
        wb, dims, acts = [], [], []
        for stack in (phi, gam):
            d, a = [], []
            for layer, p in stack:
                wt, b = layer.kernel_params(p)
                wb += [wt, b]
                d.append(wt.shape[0])
                a.append(layer.act)
            d.append(rows_of(stack[-1][1]["weight"]).shape[1])
            dims.append(d)
            acts.append(a)
        aggr = _lib.AGGR.get(m.aggr)
        if aggr is None:
            return None
        # the plan's entries take pointers only: a parameter tree that does not chain (layer l's output width against layer l + 1's
        # input width, every bias against its layer, phi's input = [h_i; h_j - h_i; x_j - x_i], gamma's = [h_i; m_i]) would make the
        # kernels read past the weight arrays -- the reference fails in the matrix product with a DimensionMismatch
        k = 0
        for name, d in (("ϕ", dims[0]), ("γ", dims[1])):      # (that the stacks chain as the layer feeds them is ngpde_ode_create's check)
            _check_plan_shapes("NeuralODE(VMHConv)", u, u.shape[0], 1,
                               [(f"{name}.layer_{l + 1}.weight", wb[k + 2 * l], (d[l], d[l + 1])) for l in range(len(d) - 1)],
                               [(f"{name}.layer_{l + 1}.bias", wb[k + 2 * l + 1], d[l + 1]) for l in range(len(d) - 1)])
            k += 2 * (len(d) - 1)
        lib = _lib.load()
        ia = lambda v: (C.c_int32 * len(v))(*[int(t) for t in v])
        supported = lambda h: lib.ngpde_node_vmh_supported(h.ptr, 1, pd, len(acts[0]), ia(dims[0]), ia(acts[0]), len(acts[1]), ia(dims[1]),
                                                            ia(acts[1]), aggr)
        members = getattr(g, "_members", None)
        straddles = bool(members) and len(members) > 1 and any(mg.num_nodes % 32 for mg in members)
        index, hit, key, handle = None, False, None, None
        if not straddles:      # (a batch whose clouds share tiles goes to its padded form at once: no handle of the unpadded union is built)
            handle = g.handle()
            key = ("vmh", id(handle), tuple(dims[0]), tuple(acts[0]), tuple(dims[1]), tuple(acts[1]), aggr, bool(needs_grad))
            hit = key in self._plans
        if not hit and (straddles or not supported(handle)):
            # a batch of point clouds whose sizes are not multiples of the 32-row tile (VMH.md:120-134: 24 clouds of 3 000 points): a tile
            # that holds the end of one cloud and the start of the next stages two neighbourhoods and can overflow its halo, which takes
            # the persistent forms away from the whole handle.  The same batch with every cloud padded to whole tiles by isolated nodes
            # (no edges: no messages, a zero cotangent on their outputs) is served; u goes in and out through an index map.
            pad = _padded_batch(g, u.device)
            if pad is None:
                return None
            g, index = pad
            handle, pos = g.handle(), _node_data(g, u.device)
            key = ("vmh", id(handle), tuple(dims[0]), tuple(acts[0]), tuple(dims[1]), tuple(acts[1]), aggr, bool(needs_grad))
            hit = key in self._plans
            if not hit and not supported(handle):
                return None
        if nodemap is not None:      # node of the given batch -> node of the earlier batch (-> its row among the padding nodes'), kept on the batch
            comp = getattr(g_given, "_vmh_comp", None)
            if comp is None or comp[0] is not index or comp[1] is not nodemap:
                comp = g_given._vmh_comp = (index, nodemap, nodemap if index is None else index.index_select(0, nodemap))
            index = comp[2]

        def make():
            # plans of this right-hand side on OTHER graphs are of no use any more (updategraph per minibatch, VMH.md:132-134): their tapes --
            # tens of GB at the tutorial's batch size -- go back to the library's pool before the new plan asks for its own
            # (only when THIS plan needs tapes, and only plans that hold tapes: a forward-only validation solve between training steps
            # must not evict the training graph's plan and make the next step rebuild it)
            if needs_grad:
                for old_key in [k for k in self._plans if k[0] == "vmh" and k[1] != id(handle) and k[-1]]:
                    self._plans.pop(old_key)
            return _OdePlan(handle, _ode_desc(_lib.RHS_VMH, self.solver, self.n_steps, self.dt, needs_grad, width=1, pos_width=int(pd), aggr=int(aggr),
                                              pos=pos.data_ptr(), n_phi=len(acts[0]), phi_dims=dims[0], phi_acts=acts[0], n_gamma=len(acts[1]),
                                              gamma_dims=dims[1], gamma_acts=acts[1]), "vmh")
        try:
            return self._plans.acquire(key, needs_grad, make, self), wb, index
        except _lib.NgpdeError as e:
            # the tapes of a solve -- every layer's input rows and dz rows of every right-hand-side evaluation, 64 floats wide -- did not
            # fit the device (the library parks and re-uses the tapes of plans that went away, and frees them before it gives up): the
            # generic solver, which keeps O(stages) arrays, takes the solve
            # ... or the library found, while building the plan, that the graph is not the plan's after all: the same way out
            if e.code not in (_lib.ERR_HIP, _lib.ERR_UNSUPPORTED):
                raise
            return None

    def _solve_vmh(self, u, ps, st, needs_grad):
        """u(T) as (1 x N) -- with saveat the (1 x N x T) array of the solution at t0 (+ j saveat) -- through the device-resident
        VMHConv plan; None when _vmh_plan finds none"""
        found = self._vmh_plan(ps, st, u, needs_grad)
        if found is None:
            return None
        plan, wb, index = found
        # a state whose node count is not the plan's graph's (a forgotten updategraph in the minibatch loop): the reference's
        # check_num_nodes DimensionMismatch, not N floats read and written through buffers of N'
        n_expected = plan.n_nodes if index is None else int(index.numel())
        if u.shape[0] != n_expected:
            raise _lib.DimensionMismatch(_lib.ERR_DIMENSION_MISMATCH, f"DimensionMismatch: NeuralODE(VMHConv): the state has {u.shape[0]} "
                                         f"nodes, the graph in the layer's state has {n_expected}")
        uin = u.reshape(-1)
        if index is not None:      # (a padded batch: the real nodes' rows among the isolated padding nodes')
            uin = _rows_index(uin, index, plan.n_nodes, True)
        out = _NodeOdeFn.apply(uin, plan, (self.save_every, self.save_start) if self.save_every else None, None, *wb)
        if index is not None:
            out = _rows_index(out, index, plan.n_nodes, False)
        return out.T.unsqueeze(0) if self.save_every else out.reshape(u.shape).T

    def __call__(self, x, ps, st):
        u = rows_of(x)
        # every parameter against its layer, before a plan, a graph handle or a library entry sees it (the rule at layers.rows_of):
        # the device-resident plans' entries take pointers only
        check_params(self.model, ps)
        if u.is_cuda:      # one device for the call: a plan's entries take pointers, and a host pointer among them is a device fault
            F._need_cuda(*[p for p in _leaves(ps) if isinstance(p, torch.Tensor)])
        needs_grad = torch.is_grad_enabled() and (u.requires_grad or any(
            isinstance(v, torch.Tensor) and v.requires_grad for v in _leaves(ps)))      # (parameter trees of any depth: VMHConv's phi / gamma chains)
        if not self.adaptive:      # (an adaptive solve's statistics are set by the solve itself)
            self.stats = dict(naccept=self.n_steps, nreject=0, nf=len(TABLEAUS[self.solver][1]) * self.n_steps, dts=[self.dt] * self.n_steps,
                              t=float(self.tspan[1]))
            # the device-resident plans: fixed-step by construction (adaptive stepping is always the generic path), saveat in VMH's only
            for solve in (self._solve_vmh,) if self.save_every else (self._solve_gcn2, self._solve_gat, self._solve_vmh):
                out = solve(u, ps, st, needs_grad)
                if out is not None:
                    return out, st
        # any other right-hand side: explicit RK stepping through the layers' own kernels, every Runge-Kutta combination (and
        # every combination of the discrete adjoint) one library launch
        if not u.is_cuda:
            raise _lib.ArgumentError(_lib.ERR_INVALID_ARGUMENT, "NeuralODE: inputs must live on the GPU (no CPU fallback)")
        leaves = _leaves(ps)
        if any(isinstance(p, torch.Tensor) and p.dtype != torch.float32 for p in leaves):
            # the stages' cotangents are summed by float32 launches (ngpde_accumulate_many): parameters of another real type enter
            # the solve through the differentiable conversion, whose pullback casts the sum back to the leaf's type
            leaves = [p.to(torch.float32) if isinstance(p, torch.Tensor) else p for p in leaves]
            ps = _rebuild(ps, iter(leaves))
        if self.capture:
            # every GNNGraph leaf of the state tree (a container's graphs sit in st["layer_k"]["graph"]): the captures bake in
            # the addresses of their derived arrays.  The entry keeps `st` -- and with it the graphs -- alive, so an id cannot be
            # recycled while its key is cached.
            key = (tuple(u.shape), needs_grad, tuple(id(g) for g in _graph_leaves(st)),
                   tuple(p.data_ptr() if isinstance(p, torch.Tensor) else id(p) for p in leaves))
            solve = self._captured.get(key)
            if solve is None:
                solve = self._captured.put(key, _CapturedSolve(self, u, ps, st, leaves, needs_grad), self.max_plans)
            uT = _NodeCapturedFn.apply(u, solve, *leaves)
            return (uT.permute(2, 1, 0) if self.save_every else uT.T), st
        uT = _NodeGenericFn.apply(u, self, ps, st, *leaves)
        return (uT.permute(2, 1, 0) if self.saving else uT.T), st      # saveat: (D x N x T), the reference's array of the solution
