"""Tsit5's free interpolant for saveat in adaptive NeuralODE, on the CPU: ngpde_rk_tsit5_interp_coefs (host only) against a float64
restatement of the coefficient table and against the order conditions it must meet with the node's own Tsit5 tableau, the placement
of save times within the accepted steps, and NeuralODE's argument errors for saveat / interpolate_saveat."""
import ctypes as C
import math

import numpy as np
import pytest

import ngpde_amd as ng
from ngpde_amd import _lib
from ngpde_amd import node as N

# r_i1 .. r_i4 of b_i(theta) = r_i1 theta + r_i2 theta^2 + r_i3 theta^3 + r_i4 theta^4 (Tsitouras 2011; OrdinaryDiffEq's Tsit5 dense output)
R = np.array([
    [1.0, -2.763706197274826, 2.9132554618219126, -1.0530884977290216],
    [0.0, 0.13169999999999998, -0.2234, 0.1017],
    [0.0, 3.9302962368947516, -5.941033872131505, 2.490627285651253],
    [0.0, -12.411077166933676, 30.33818863028232, -16.548102889244902],
    [0.0, 37.50931341651104, -88.1789048947664, 47.37952196281928],
    [0.0, -27.896526289197286, 65.09189467479366, -34.87065786149661],
    [0.0, 1.5, -4.0, 2.5],
])
THETAS = [0.0, 0.1, 0.25, 0.37, 0.5, 0.81, 0.999, 1.0]


def interp_b(theta):
    """b_1..b_7 at theta, float64 (the GPU test's replay uses it too)"""
    return R @ np.array([theta, theta ** 2, theta ** 3, theta ** 4])


def lib_coefs(theta, dt=1.0):
    out = (C.c_double * 7)()
    st = _lib.load().ngpde_rk_tsit5_interp_coefs(theta, dt, out)
    return st, np.array(list(out))


def tableau():
    """the node's Tsit5 tableau extended by the FSAL seventh stage (a_7j = b_j, c_7 = 1)"""
    a = np.zeros((7, 7))
    for i, row in enumerate(N._TSIT5_A):
        a[i, :len(row)] = row
    a[6, :6] = N._TSIT5_B
    return a, a.sum(axis=1)


# ---- the coefficients ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("theta", THETAS)
def test_coefs_against_the_table(theta):
    st, got = lib_coefs(theta)
    assert st == 0
    ref = interp_b(theta)
    assert np.abs(got - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max()), (got, ref)


def test_ends_of_the_step():
    assert np.abs(lib_coefs(0.0)[1]).max() <= 1e-13
    b1 = lib_coefs(1.0)[1]
    assert np.abs(b1 - np.array(list(N._TSIT5_B) + [0.0])).max() <= 1e-13, b1


@pytest.mark.parametrize("theta", [0.1, 0.37, 0.5, 0.81, 1.0])
def test_order_conditions_up_to_order_four(theta):
    a, c = tableau()
    b = lib_coefs(theta)[1]
    ac, c2 = a @ c, c * c
    conds = [
        (b.sum(), theta),                              # order 1
        (b @ c, theta ** 2 / 2),                       # order 2
        (b @ c2, theta ** 3 / 3),                      # order 3
        (b @ ac, theta ** 3 / 6),
        (b @ (c2 * c), theta ** 4 / 4),                # order 4
        (b @ (c * ac), theta ** 4 / 8),
        (b @ (a @ c2), theta ** 4 / 12),
        (b @ (a @ ac), theta ** 4 / 24),
    ]
    for k, (got, ref) in enumerate(conds):
        assert abs(got - ref) <= 1e-12, (k, got, ref)
    if theta == 1.0:     # the interpolant is 4th order only: at the step's end the 5th-order conditions hold (it is the step),
        assert abs(b @ (c2 * c2) - 1 / 5) <= 1e-12     # in between they do not
    else:
        assert abs(b @ (c2 * c2) - theta ** 5 / 5) > 1e-6


def test_dt_scaling():
    for theta in (0.2, 0.9):
        ref = lib_coefs(theta, 1.0)[1]
        for dt in (1e-3, 0.37, 5.0):
            assert np.abs(lib_coefs(theta, dt)[1] - dt * ref).max() <= 1e-15 * dt * np.abs(ref).max() * 4


@pytest.mark.parametrize("theta", [-1e-12, 1.0 + 1e-12, 2.0, math.nan, math.inf, -math.inf])
def test_theta_outside_the_step_is_refused(theta):
    st, _ = lib_coefs(theta)
    assert st == _lib.ERR_INVALID_ARGUMENT
    assert b"theta" in _lib.load().ngpde_last_error()


def test_null_and_nonfinite_dt_are_refused():
    assert _lib.load().ngpde_rk_tsit5_interp_coefs(0.5, 1.0, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib_coefs(0.5, math.nan)[0] == _lib.ERR_INVALID_ARGUMENT


def test_dense_entries_refuse_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.ngpde_rk_dense_output(16, None, 9, None, 1, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_rk_dense_output(16, None, 7, None, 1, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_rk_dense_output(0, None, 7, None, 3, None, None, None) == 0          # nothing to do
    assert lib.ngpde_rk_dense_output_pullback(16, 0, None, 7, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT
    assert lib.ngpde_rk_dense_output_pullback(16, 2, None, 7, None, None, None, None) == _lib.ERR_INVALID_ARGUMENT


# ---- where the save times fall -----------------------------------------------------------------------------------------------------

def test_scalar_save_times():
    assert N.dense_save_times((0.0, 1.0), 0.25, True) == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert N.dense_save_times((0.0, 1.0), 0.25, False) == [0.25, 0.5, 0.75, 1.0]
    assert N.dense_save_times((0.0, 1.0), 0.3, False) == [0.3, 0.6, 0.8999999999999999, 1.0]     # need not divide tspan
    # 0.1 * 10 in floating point, or any point within 1e-12 of the span from t_end, is t_end itself
    t = N.dense_save_times((0.0, 1.0), 0.1, True)
    assert len(t) == 11 and t[-1] == 1.0 and t[-2] < 1.0 - 0.05
    t = N.dense_save_times((0.0, 1.0), (1.0 - 5e-13) / 3, False)
    assert len(t) == 3 and t[-1] == 1.0
    t = N.dense_save_times((0.0, 1.0), (1.0 - 5e-12) / 3, False)
    assert len(t) == 4 and t[-1] == 1.0


def test_vector_save_times():
    assert N.dense_save_times((0.0, 2.0), [0.0, 0.5, 1.5], True) == [0.0, 0.5, 1.5]
    assert N.dense_save_times((0.0, 2.0), [0.0, 0.5, 1.5], False) == [0.5, 1.5]
    assert N.dense_save_times((0.0, 2.0), np.array([0.5, 2.0]), False) == [0.5, 2.0]


def test_saves_in_step():
    times = [0.1, 0.2, 0.3, 0.5, 0.9, 1.0]
    interior, end, j = N.saves_in_step(times, 0, 0.0, 0.3, 0.3)
    assert [s for s, _ in interior] == [0, 1] and end == 2 and j == 3
    assert abs(interior[0][1] - 1 / 3) < 1e-15 and abs(interior[1][1] - 2 / 3) < 1e-15
    interior, end, j = N.saves_in_step(times, j, 0.3, 0.4, 0.1)          # a step with no save
    assert interior == [] and end is None and j == 3
    interior, end, j = N.saves_in_step(times, j, 0.4, 1.0, 0.6)          # the final step ends on t_end
    assert [s for s, _ in interior] == [3, 4] and end == 5 and j == 6
    # theta stays within [0, 1] when t_n + dt rounds past the step's end
    interior, _, _ = N.saves_in_step([0.3 - 1e-17, 0.3], 0, 0.1, 0.3, 0.19999999999999998)
    assert all(0.0 <= th <= 1.0 for _, th in interior)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------

def dense_node(**kw):
    return ng.NeuralODE(ng.Dense(4, 4), tspan=(0.0, 1.0), **kw)


@pytest.mark.parametrize("saveat", [[0.5, 0.2], [0.2, 0.2], [-0.1, 0.5], [0.5, 1.5], [], [math.nan], [[0.1, 0.2]],
                                    np.array([[0.1, 0.2]])])
def test_bad_vector_saveat(saveat):
    with pytest.raises(ng.ArgumentError):
        dense_node(adaptive=True, saveat=saveat)


def test_interpolation_mode_errors():
    with pytest.raises(ng.ArgumentError):
        dense_node(adaptive=True, saveat=[0.2, 0.5], interpolate_saveat=False)
    with pytest.raises(ng.ArgumentError):
        dense_node(adaptive=False, saveat=[0.2, 0.5])
    for flag in (True, False):
        with pytest.raises(ng.ArgumentError):
            dense_node(adaptive=False, interpolate_saveat=flag)
        with pytest.raises(ng.ArgumentError):
            dense_node(adaptive=False, saveat=0.1, n_steps=10, interpolate_saveat=flag)
    with pytest.raises(ng.ArgumentError):
        dense_node(adaptive=True, interpolate_saveat=True)                    # nothing to interpolate
    with pytest.raises(ng.ArgumentError):
        dense_node(adaptive=True, saveat=0.0, interpolate_saveat=True)
    with pytest.raises(ng.ArgumentError):
        dense_node(adaptive=True, saveat=0.3)                                 # landing: saveat must divide tspan
    with pytest.raises(ng.ArgumentError):
        dense_node(adaptive=True, saveat=0.3, interpolate_saveat=1)


def test_modes_and_save_times():
    n = dense_node(adaptive=True, saveat=0.3, interpolate_saveat=True)        # interpolating: need not divide tspan
    assert n.save_times == [0.0, 0.3, 0.6, 0.8999999999999999, 1.0] and n.saving
    n = dense_node(adaptive=True, saveat=0.25)                                # landing stays the scalar default
    assert n.save_times is None and n.saving and not n.interpolate_saveat
    import torch
    n = dense_node(adaptive=True, saveat=torch.tensor([0.0, 0.5]), save_start=False)
    assert n.interpolate_saveat and n.save_times == [0.5]
    n = dense_node(adaptive=False, saveat=0.5, n_steps=4)                     # fixed step: today's meaning
    assert n.save_every == 2 and n.save_times is None
