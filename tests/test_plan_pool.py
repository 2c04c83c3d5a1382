"""NeuralODE's plan pool and the host side of a device-resident plan (ngpde_amd/plans.py: _PlanPool, _Recent, _ResidentPlan), driven with
stand-in plans: which plan a solve gets, which keys stay, what happens at max_outstanding and when a create raises, and how long a claimed
plan is busy.  No library object is built: a stand-in's `ptr` stays None, so its destroy entry is never reached."""
import gc
import types

import pytest

from ngpde_amd import _lib
from ngpde_amd.node import NeuralODE
from ngpde_amd.plans import _PlanPool, _Recent, _ResidentPlan


class StandIn(_ResidentPlan):
    """the base with a flag for "backward pending" """
    _entries = "never_called"

    def __init__(self):
        super().__init__(types.SimpleNamespace(_n_nodes=5), members=2)
        self.pending = False

    def _backward_pending(self):
        return self.pending


class Maker:
    """make() of a caller: counts its calls, keeps the plans it made (and the tokens that keep them busy)"""

    def __init__(self):
        self.made, self.tokens = [], []

    def __call__(self):
        self.made.append(StandIn())
        return self.made[-1]

    def busy_plan(self):
        plan = self()
        plan.pending = True
        self.tokens.append(plan.claim())
        return plan


def limits(max_plans=2, max_outstanding=8):
    return types.SimpleNamespace(max_plans=max_plans, max_outstanding=max_outstanding)


def test_the_oldest_key_goes_when_a_new_one_is_inserted():
    pool, make = _PlanPool(), Maker()
    for key in "abc":
        pool.acquire(key, True, make, limits(max_plans=2))
    assert list(pool) == ["b", "c"] and len(make.made) == 3
    assert all(isinstance(v, list) and len(v) == 1 for v in pool.values())


def test_a_hit_moves_its_key_to_the_back_and_evicts_nothing():
    pool, make = _PlanPool(), Maker()
    pa = pool.acquire("a", True, make, limits())
    pool.acquire("b", True, make, limits())
    assert pool.acquire("a", True, make, limits()) is pa and list(pool) == ["b", "a"] and len(make.made) == 2
    pool.acquire("c", True, make, limits())
    assert list(pool) == ["a", "c"]
    # a hit under a limit lowered since evicts nothing: only an insertion does
    assert pool.acquire("a", True, make, limits(max_plans=1)) is pa and list(pool) == ["c", "a"]


def test_a_busy_plan_is_skipped_by_a_solve_with_backward_and_taken_by_one_without():
    pool, make = _PlanPool(), Maker()
    first = pool.acquire("k", True, make.busy_plan, limits())
    assert first.busy()
    second = pool.acquire("k", True, make, limits())
    assert second is not first and pool["k"] == [first, second] and len(make.made) == 2
    second.pending = True
    token = second.claim()
    assert pool.acquire("k", False, make, limits()) is first and len(make.made) == 2      # forward only: no tape to protect
    del token


def test_freed_plans_are_handed_out_in_creation_order():
    pool, make = _PlanPool(), Maker()
    plans = [pool.acquire("k", True, make.busy_plan, limits()) for _ in range(3)]
    assert pool["k"] == plans and all(p.busy() for p in plans)
    plans[1].pending = False
    assert pool.acquire("k", True, make, limits()) is plans[1]
    for p in plans:
        p.pending = False
    assert pool.acquire("k", True, make, limits()) is plans[0] and len(make.made) == 3


def test_max_outstanding_busy_plans_raise_err_state_and_the_limit_is_read_per_call(monkeypatch):
    pool, make = _PlanPool(), Maker()
    for _ in range(NeuralODE.max_outstanding):
        pool.acquire("k", True, make.busy_plan, NeuralODE)
    n = len(make.made)
    assert n == NeuralODE.max_outstanding == len(pool["k"])
    with pytest.raises(_lib.NgpdeError) as err:
        pool.acquire("k", True, make, NeuralODE)
    assert err.value.code == _lib.ERR_STATE and "max_outstanding" in str(err.value) and f"{n} solves" in str(err.value)
    assert len(make.made) == n and len(pool["k"]) == n
    monkeypatch.setattr(NeuralODE, "max_outstanding", n + 1)
    assert pool.acquire("k", True, make, NeuralODE) is make.made[-1] and len(make.made) == n + 1 == len(pool["k"])


def test_a_create_that_raises_leaves_no_empty_pool_and_is_the_callers_to_handle():
    pool, make = _PlanPool(), Maker()
    kept = pool.acquire("old", True, make.busy_plan, limits())

    def refuse():
        raise _lib.NgpdeError(_lib.ERR_UNSUPPORTED, "not this graph")

    with pytest.raises(_lib.NgpdeError) as err:
        pool.acquire("fresh", True, refuse, limits())
    assert err.value.code == _lib.ERR_UNSUPPORTED and "fresh" not in pool and pool == {"old": [kept]}
    with pytest.raises(_lib.NgpdeError):
        pool.acquire("old", True, refuse, limits())      # every plan busy: a create is tried, and refused
    assert pool == {"old": [kept]}


def test_a_claimed_plan_is_busy_while_its_token_lives_and_its_backward_is_pending():
    plan = StandIn()
    assert (plan.ptr, plan.members, plan.n_nodes) == (None, 2, 5) and not plan.busy()
    plan.pending = True
    assert not plan.busy()              # never claimed
    token = plan.claim()
    assert token is not None and plan.busy()
    plan.pending = False                # the backward ran
    assert not plan.busy()
    plan.pending = True
    del token                           # the autograd node went away: nobody can ask for that backward any more
    gc.collect()
    assert not plan.busy()


def test_a_second_claim_replaces_the_first():
    plan = StandIn()
    plan.pending = True
    first = plan.claim()
    second = plan.claim()
    assert second is not first
    del second
    gc.collect()
    assert not plan.busy()              # the first solve's token no longer holds the plan
    del first


def test_the_bounded_dictionary_keeps_its_limit_and_drops_the_oldest():
    d = _Recent()
    for k in range(5):
        assert d.put(k, str(k), 3) == str(k) and len(d) <= 3
    assert list(d.items()) == [(2, "2"), (3, "3"), (4, "4")]
    d.put(2, "again", 3)                # an existing key keeps its place
    assert list(d) == [2, 3, 4] and d[2] == "again"
    d.put(5, "5", 2)
    assert list(d) == [4, 5]


def test_neuralode_keeps_its_caches_in_the_pool_types():
    class Rhs:
        pass
    for kw in (dict(), dict(adaptive=True)):
        node = NeuralODE(Rhs(), **kw)
        assert type(node._plans) is _PlanPool and type(node._captured) is _Recent and type(node._gat_ok) is _Recent
        assert node._plans == {} and node._no_member_plan is False and node.capture is False
