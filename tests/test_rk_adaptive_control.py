"""The adaptive Tsit5 step-size controller (ngpde_rk_control_*, host only) on the CPU, against a float64 restatement of its rules
written here: OrdinaryDiffEq's PI controller with the Tsit5 defaults and Hairer-Norsett-Wanner's starting step as
ode_determine_initdt applies it (docs/src/tutorials/graph_node.md:80-81 and VMH.md:87 solve with adaptive Tsit5).  OrdinaryDiffEq
cannot run here: parity with its step sequence holds by construction of these rules and is not pinned by a run of it.  Also: the
embedded weights' order conditions and NeuralODE(adaptive=True)'s argument errors."""
import ctypes as C
import math

import pytest

import ngpde_amd as ng
from ngpde_amd import _lib
from ngpde_amd import node as N

BETA1, BETA2, GAMMA, QMIN, QMAX, QOLDINIT = 7 / 50, 2 / 25, 9 / 10, 1 / 5, 10.0, 1e-4
REJECT, ACCEPT, DONE = 0, 1, 2


class Failed(Exception):
    pass


class Restated:
    """float64 restatement of the controller's rules (the contract the library's entries are held to)"""

    def __init__(self, t0, t_end, dt, dtmax, saveat, maxiters):
        span = t_end - t0
        self.t0, self.t, self.t_end = t0, t0, t_end
        self.dtmax = dtmax if dtmax > 0 else span
        self.dtmin = 1e-12 * span
        self.saveat = saveat
        self.n_save = int(round(span / saveat)) if saveat > 0 else 0
        self.next_save = 1
        self.maxiters = maxiters if maxiters > 0 else 100_000
        self.qold, self.q11, self.eest = QOLDINIT, 0.0, 0.0
        self.naccept = self.nreject = self.nattempt = 0
        self.lands = self.saved = self.done = 0
        self.dt = 0.0
        if dt > 0:
            self.propose(dt)

    def stop(self):
        if self.saveat > 0 and self.next_save < self.n_save:
            return self.t0 + self.next_save * self.saveat
        return self.t_end

    def propose(self, dt_next):
        dt = dt_next if dt_next < self.dtmax else self.dtmax
        if not dt >= self.dtmin:
            self.done = -1
            raise Failed("dtmin")
        stop = self.stop()
        if dt >= stop - self.t:
            self.dt, self.lands = stop - self.t, 1
        else:
            self.dt, self.lands = dt, 0

    def trial_dt(self, d0, d1):
        d = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * (d0 / d1)
        return d if d < self.dtmax else self.dtmax

    def initial_dt(self, d0, d1, norm_df):
        dt0 = self.trial_dt(d0, d1)
        d2 = norm_df / dt0
        m = max(d1, d2)
        dt1 = max(1e-6, 1e-3 * dt0) if m <= 1e-15 else (0.01 / m) ** (1 / 5)
        self.propose(min(100 * dt0, dt1, self.dtmax))

    def step(self, eest):
        self.nattempt += 1
        if self.nattempt > self.maxiters:
            self.done = -1
            raise Failed("maxiters")
        self.eest, self.saved = eest, 0
        if not math.isfinite(eest):
            dt_next, action = self.dt * QMIN, REJECT
            self.nreject += 1
        else:
            if eest == 0:
                q = 1 / QMAX
            else:
                self.q11 = eest ** BETA1
                q = min(max(self.q11 / self.qold ** BETA2 / GAMMA, 1 / QMAX), 1 / QMIN)
            if eest <= 1:
                self.qold = max(eest, QOLDINIT)
                dt_next = self.dt / q
                stop = self.stop()
                self.t = stop if self.lands else self.t + self.dt
                self.naccept += 1
                action = ACCEPT
                if self.lands:
                    if self.saveat > 0:
                        self.saved, self.next_save = 1, self.next_save + 1
                    if stop == self.t_end:
                        self.done = 1
                        return DONE
            else:
                dt_next, action = self.dt / min(1 / QMIN, self.q11 / GAMMA), REJECT
                self.nreject += 1
        self.propose(dt_next)
        return action


FIELDS = [f for f, _ in _lib.RkControl._fields_ if f != "reserved"]


def same_state(lib_state, ref):
    for f in FIELDS:
        a, b = getattr(lib_state, f), getattr(ref, f)
        assert a == b or (isinstance(b, float) and math.isnan(a) and math.isnan(b)), f"{f}: library {a!r}, restatement {b!r}"


def lib_init(*args):
    s = _lib.RkControl()
    _lib.check(_lib.load().ngpde_rk_control_init(C.byref(s), *args))
    return s


def lib_step(s, eest):
    act = C.c_int32(-7)
    st = _lib.load().ngpde_rk_control_step(C.byref(s), eest, C.byref(act))
    return st, act.value


def fifth_order(h, special=None):
    """an EEst script: (dt / h)^5, the error of a 5th-order step, with the attempts listed in `special` given other values"""
    special = special or {}
    return lambda n, dt: special.get(n, (dt / h) ** 5)


def run_script(args, script):
    """both controllers through the EEst script (a list, cycled, or a function of (attempt, dt)) until the solve ends or fails;
    returns (actions, failure)"""
    s, ref = lib_init(*args), Restated(*args)
    same_state(s, ref)
    actions = []
    for n in range(10_000):
        e = script(n, s.dt) if callable(script) else script[n % len(script)]
        st, act = lib_step(s, e)
        try:
            ref_act = ref.step(e)
        except Failed as f:
            assert st == _lib.ERR_STATE, st
            msg = _lib.load().ngpde_last_error().decode()
            assert str(f) in msg and "t = " in msg, msg
            same_state(s, ref)
            assert lib_step(s, 0.5)[0] == _lib.ERR_STATE          # a failed solve stays failed
            return actions, str(f)
        assert st == _lib.OK, _lib.load().ngpde_last_error()
        assert act == ref_act
        same_state(s, ref)
        actions.append(act)
        if act == DONE:
            assert s.t == s.t_end
            assert lib_step(s, 0.5)[0] == _lib.ERR_STATE          # nothing after the end
            return actions, None
    raise AssertionError("the script did not end")


def test_accepts_rejects_zero_and_nan():
    script = fifth_order(0.08, {0: 0.5, 1: 2.0, 3: 0.0, 5: float("nan"), 6: 1.0, 8: 7.5, 10: float("inf"), 12: 1e-30})
    actions, failure = run_script((0.0, 1.0, 0.05, 0.0, 0.0, 0), script)
    assert failure is None and actions[-1] == DONE
    assert REJECT in actions and ACCEPT in actions


def test_every_eest_zero_grows_by_qmax_up_to_dtmax():
    s = lib_init(0.0, 10.0, 1e-3, 0.5, 0.0, 0)
    ref = Restated(0.0, 10.0, 1e-3, 0.5, 0.0, 0)
    for _ in range(4):
        assert lib_step(s, 0.0) == (0, ACCEPT)
        ref.step(0.0)
        same_state(s, ref)
    assert s.dt == 0.5                       # 1e-3 -> 1e-2 -> 0.1 -> 0.5 (dtmax)
    run_script((0.0, 10.0, 1e-3, 0.5, 0.0, 0), [0.0])


@pytest.mark.parametrize("t0,t_end,saveat", [(0.0, 1.0, 0.25), (0.0, 2.0, 0.1), (1.5, 4.5, 0.3)])
def test_steps_land_on_save_points_and_t_end(t0, t_end, saveat):
    args = (t0, t_end, 0.07, 0.0, saveat, 0)
    script = fifth_order(0.06, {2: 3.0, 7: 40.0})
    actions, failure = run_script(args, script)
    assert failure is None
    # replay to collect the save times: every one is t0 + k saveat exactly, and the last is t_end
    s, times = lib_init(*args), []
    while True:
        st, act = lib_step(s, script(int(s.nattempt), s.dt))
        assert st == 0
        if act != REJECT and s.saved:
            times.append(s.t)
        if act == DONE:
            break
    n = int(round((t_end - t0) / saveat))
    assert times == [t0 + k * saveat for k in range(1, n)] + [t_end]


def test_the_first_step_is_cut_to_the_first_stop():
    s = lib_init(0.0, 1.0, 5.0, 0.0, 0.25, 0)
    assert s.dt == 0.25 and s.lands == 1
    s = lib_init(0.0, 1.0, 5.0, 0.0, 0.0, 0)
    assert s.dt == 1.0 and s.lands == 1


def test_maxiters_failure():
    actions, failure = run_script((0.0, 1.0, 0.1, 0.0, 0.0, 5), [2.0])
    assert failure == "maxiters" and actions == [REJECT] * 5
    _, failure = run_script((0.0, 1.0, 0.01, 0.0, 0.0, 40), [0.5])      # accepted attempts count too
    assert failure == "maxiters"


@pytest.mark.parametrize("eest", [1e6, float("nan")])
def test_dtmin_failure(eest):
    actions, failure = run_script((0.0, 1.0, 0.1, 0.0, 0.0, 0), [eest])
    assert failure == "dtmin" and set(actions) == {REJECT} and len(actions) < 40


@pytest.mark.parametrize("d0,d1,norm_df,dtmax", [
    (1.0, 2.0, 0.5, 0.0), (3e-6, 2.0, 0.5, 0.0), (1.0, 3e-6, 1e-9, 0.0), (1.0, 1e-20, 1e-25, 0.0), (10.0, 1.0, 100.0, 0.0),
    (50.0, 0.1, 0.3, 0.0), (50.0, 0.1, 0.3, 0.02), (0.7, 40.0, 3000.0, 0.0), (1.0, 2.0, 0.0, 0.0),
])
def test_initial_step_matches_the_restatement(d0, d1, norm_df, dtmax):
    for t0, t_end, saveat in ((0.0, 1.0, 0.0), (0.0, 1.0, 1e-3), (2.0, 12.0, 0.0)):
        s, ref = lib_init(t0, t_end, 0.0, dtmax, saveat, 0), Restated(t0, t_end, 0.0, dtmax, saveat, 0)
        same_state(s, ref)
        dt0 = C.c_double()
        assert _lib.load().ngpde_rk_control_trial_dt(C.byref(s), d0, d1, C.byref(dt0)) == 0
        assert dt0.value == ref.trial_dt(d0, d1)
        assert _lib.load().ngpde_rk_control_initial_dt(C.byref(s), d0, d1, norm_df) == 0
        ref.initial_dt(d0, d1, norm_df)
        same_state(s, ref)
        assert 0 < s.dt <= s.t_end - s.t0


def test_initial_step_refuses_non_finite_norms():
    s = lib_init(0.0, 1.0, 0.0, 0.0, 0.0, 0)
    dt0 = C.c_double()
    assert _lib.load().ngpde_rk_control_trial_dt(C.byref(s), 1.0, float("nan"), C.byref(dt0)) == _lib.ERR_STATE
    assert _lib.load().ngpde_rk_control_initial_dt(C.byref(s), 1.0, 1.0, float("inf")) == _lib.ERR_STATE
    assert lib_step(s, 0.5)[0] == _lib.ERR_STATE            # no step size was chosen


def test_init_refuses_bad_arguments():
    lib, s = _lib.load(), _lib.RkControl()
    assert lib.ngpde_rk_control_init(C.byref(s), 1.0, 1.0, 0.1, 0.0, 0.0, 0) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_rk_control_init(C.byref(s), 0.0, 1.0, 0.1, 0.0, 0.3, 0) == _lib.ERR_INVALID_ARGUMENT   # 0.3 does not divide 1
    assert lib.ngpde_rk_control_init(C.byref(s), 0.0, 1.0, float("nan"), 0.0, 0.0, 0) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_rk_control_init(None, 0.0, 1.0, 0.1, 0.0, 0.0, 0) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_rk_control_init(C.byref(s), 0.0, 1.0, 0.1, 0.0, 0.1, 0) == 0
    assert s.n_save == 10 and s.maxiters == 100_000 and s.dtmax == 1.0 and s.dtmin == 1e-12


def test_error_norm_argument_checks_without_gpu():
    lib = _lib.load()
    assert lib.ngpde_rk_error_norm_workspace_bytes(0) == 0
    assert lib.ngpde_rk_error_norm_workspace_bytes(1) == 8
    assert lib.ngpde_rk_error_norm_workspace_bytes(1 << 20) == 2048 * 8
    terms = (C.c_void_p * 1)(None)
    coefs = (C.c_float * 1)(1.0)
    assert lib.ngpde_rk_error_norm(16, 0, terms, coefs, None, None, 1e-6, 1e-3, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_rk_error_norm(16, 1, terms, coefs, None, None, 1e-6, 1e-3, None, None, None) == _lib.ERR_INVALID_ARGUMENT


def test_btilde_order_conditions():
    a, b = N.TABLEAUS["tsit5"]
    assert len(b) == 6 and len(N._TSIT5_BTILDE) == 7
    c = [sum(row) for row in a] + [sum(b)]          # the seventh stage is f(u_new): c7 = 1
    assert abs(c[-1] - 1.0) < 1e-14
    for q in range(1, 5):
        assert abs(sum(bt * ci ** (q - 1) for bt, ci in zip(N._TSIT5_BTILDE, c))) < 1e-14, q
    assert abs(sum(bt * ci ** 4 for bt, ci in zip(N._TSIT5_BTILDE, c))) > 1e-5


def test_neuralode_adaptive_argument_errors():
    m = ng.Dense(4, 4)
    with pytest.raises(ng.ArgumentError):
        ng.NeuralODE(m, solver="euler", adaptive=True)
    with pytest.raises(ng.ArgumentError):
        ng.NeuralODE(m, adaptive=True, capture=True)
    with pytest.raises(ng.ArgumentError):
        ng.NeuralODE(m, adaptive=True, tspan=(0.0, 1.0), saveat=0.3)
    with pytest.raises(ng.ArgumentError):
        ng.NeuralODE(m, adaptive=True, reltol=[1e-3, 1e-3])
    with pytest.raises(ng.ArgumentError):
        ng.NeuralODE(m, adaptive=True, abstol=-1.0)
    with pytest.raises(ng.ArgumentError):
        ng.NeuralODE(m, adaptive=True, dt=0.0)
    node = ng.NeuralODE(m, adaptive=True, tspan=(0.0, 1.0), saveat=0.25, reltol=1e-9, abstol=1e-3)
    assert node.adaptive and node.saving and node.dt is None and node.reltol == 1e-9
    assert (node.reltol, node.abstol, node.maxiters) == (1e-9, 1e-3, 100_000)
    assert ng.NeuralODE(m, adaptive=True).abstol == 1e-6          # DiffEq's defaults
    fixed = ng.NeuralODE(m, n_steps=4)
    assert not fixed.adaptive and fixed.dt == 0.25 and not fixed.saving
