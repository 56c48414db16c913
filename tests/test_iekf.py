"""Banks of iterated extended Kalman filters, the part that needs no GPU: the iterated correct! of csrc/shared/llpf_ekf.h (the device
order, built for the host by tests/ekf_host.c) against the plain filter of the same header where the two must coincide, against a numpy
restatement of the textbook Gauss-Newton formulas where they do not, the posterior mode as a known answer, and the argument checks of
llpf_ekf_bank_set_iterations."""
import ctypes as C
import os

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import iekf_common as ic
import kalman_common as kc
import models as M
import ukf_common as uc
from test_ukf import linear_systems, T_LIN

OUTPUTS = _capi.KALMAN_OUTPUTS


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ic.build_host(tmp_path_factory.mktemp("iekf_host"))


@pytest.fixture(scope="module")
def ekf_host(tmp_path_factory):
    return ec.build_host(tmp_path_factory.mktemp("ekf_host"))


@pytest.fixture(scope="module")
def systems():
    """(name, models, U, Y, T, kind, t_index0, linear measurement): the 32 linear systems of test_ukf.py, the quad-tank across TSWITCH,
    the pendulum with Jacobians and x0^2, each with missing rows"""
    out = [("LG %d x %d" % (m.nx, m.ny), [m], U, Y, T_LIN, ec.KIND_LG, 0.0, True) for m, D, mats, U, Y in linear_systems()]
    U, Y = M.quadtank_data(60)
    Y = Y.copy()
    Y[[7, 31], 0] = np.nan
    out.append(("quad-tank", [M.quadtank_model()], U, Y, 60, ec.KIND_QUADTANK, 470.0, True))
    U, Y = uc.pendulum_data(300)
    Y = Y.copy()
    Y[[3, 200, 298], 0] = np.nan
    out.append(("pendulum", [uc.pendulum_model()], U, Y, 300, ec.KIND_PENDULUM, 0.0, False))
    Ysq = 3.0 + 0.5 * np.random.default_rng(3).standard_normal((80, 1))
    Ysq[[0, 40], 0] = np.nan
    out.append(("square", [ec.square_model(1.0, 0.36)], None, Ysq, 80, ec.KIND_SQUARE, 0.0, False))
    return out


@pytest.fixture(scope="module")
def plain(ekf_host, systems):
    """the plain filter of tests/ekf_host.c on every system, computed once"""
    return [ec.host_run(ekf_host, models, U, Y, T, t_index0=t0, kind=kind) for _, models, U, Y, T, kind, t0, _ in systems]


def test_one_iteration_is_the_extended_kalman_filter_bit_for_bit(host, systems, plain):
    """1. maxiters = 1, and maxiters = 10 with epsilon = 1e300 (the stop rule firing after one move), give the bits of the plain filter's
    host build in every output, ll and the final state, on every system; each step with a measurement ran one linearisation."""
    for (name, models, U, Y, T, kind, t0, _), (ref, ref_state) in zip(systems, plain):
        for maxiters, eps in ((1, 0.0), (10, 1e300)):
            got, state = ic.host_run(host, models, U, Y, T, maxiters, eps, t_index0=t0, kind=kind)
            for k in OUTPUTS + ("ll",):
                assert kc.bits_equal(got[k], ref[k]), (name, maxiters, k)
            assert kc.bits_equal(state[0], ref_state[0]) and kc.bits_equal(state[1], ref_state[1]), (name, maxiters, "final state")
            assert np.array_equal(got["iters"][:, 0], np.where(np.isnan(Y[:, 0]), 0, 1)), (name, maxiters)
        # ... and the plain filter inside the iterated library is the plain library's
        again, _ = ec.host_run(host, models, U, Y, T, t_index0=t0, kind=kind)
        for k in OUTPUTS + ("ll",):
            assert kc.bits_equal(again[k], ref[k]), (name, k)


def test_a_linear_measurement_stops_after_two_linearisations(host, systems, plain):
    """2. With a linear measurement the first Gauss-Newton step lands on the posterior mean and the second confirms it: at maxiters = 10,
    epsilon = 1e-8 every output is within 1e-10 of the plain filter ("same filter, different rounding"), a step with a measurement runs
    at most 2 linearisations and a missing row none."""
    worst, n = 0.0, 0
    for (name, models, U, Y, T, kind, t0, linear), (ref, _) in zip(systems, plain):
        if not linear:
            continue
        n += 1
        got, _ = ic.host_run(host, models, U, Y, T, 10, 1e-8, t_index0=t0, kind=kind)
        for k in OUTPUTS:
            worst = max(worst, uc.rel_err(got[k], ref[k]))
            assert kc.close(got[k], ref[k]), (name, k, uc.rel_err(got[k], ref[k]))
        assert kc.close(got["ll"], ref["ll"]), name
        missing = np.isnan(Y[:, 0])
        it = got["iters"][:, 0]
        assert np.all(it[missing] == 0) and np.all((it[~missing] >= 1) & (it[~missing] <= 2)), (name, it.min(), it.max())
    assert n == 33
    print("linear measurement, (10, 1e-8) against the plain filter: worst relative difference %.2e" % worst)


def _measured(case, kind, host, maxiters, what):
    """header against restatement with test_ekf.py's bar: 1e-10 where ten times the restatement's own float64-against-long-double error
    is below it, otherwise ten times that error, measured in the same run.  epsilon = 0: both sides run `maxiters` iterations unless an
    iterate repeats exactly."""
    m, U, Y, fg, fgl, jac, jacl, t0 = case
    R1, R2 = S.gaussian_cov_matrix(m.dynamics_density), S.gaussian_cov_matrix(m.measurement_density)
    x0, P0 = S.gaussian_mean(m.initial_density), S.gaussian_cov_matrix(m.initial_density)
    a = ic.numpy_iekf(fg[0], fg[1], jac[0], jac[1], R1, R2, x0, P0, U, Y, maxiters, 0.0, m.Ts, t0)
    b = ic.numpy_iekf(fgl[0], fgl[1], jacl[0], jacl[1], R1, R2, x0, P0, U, Y, maxiters, 0.0, m.Ts, t0, lin=uc.LinLong)
    own = {k: uc.rel_err(a[k], b[k]) for k in OUTPUTS + ("ll",)}
    got, _ = ic.host_run(host, [m], U, Y, Y.shape[0], maxiters, 0.0, t_index0=t0, kind=kind)
    assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), what
    err = {k: uc.rel_err(got[k][:, 0], a[k]) for k in OUTPUTS}
    err["ll"] = uc.rel_err(got["ll"][0], a["ll"])
    print(what, "ll %.6f" % got["ll"][0], "mean linearisations %.2f (restatement %.2f)" % (got["iters"].mean(), a["iters"].mean()))
    print(what, "restatement float64 vs long double:", {k: "%.2e" % v for k, v in own.items()})
    print(what, "header vs restatement:", {k: "%.2e" % v for k, v in err.items()})
    for k in err:
        bar = 1e-10 if 10.0 * own[k] <= 1e-10 else 10.0 * own[k]
        assert err[k] <= bar, (what, k, err[k], bar)


@pytest.mark.parametrize("maxiters", [2, 5])
def test_header_equals_the_formulas_on_the_pendulum(host, maxiters):
    """3a. The pendulum through its C twin (T = 300, three missing rows, epsilon = 0) against the restatement with np.sin / np.cos.
    Measured in this test, restatement float64 against long double | header against restatement — maxiters = 2: ll_steps 1.1e-13 | 1.2e-13,
    x 6.0e-16 | 7.3e-16, xt 5.3e-16 | 6.2e-16, R 3.9e-16 | 7.0e-16, Rt 4.0e-16 | 6.8e-16, e 2.3e-13 | 3.3e-13, ll 5.8e-19 | 6.6e-16;
    maxiters = 5: ll_steps 9.1e-14 | 6.2e-14, x 4.9e-16 | 5.7e-16, xt 4.2e-16 | 5.5e-16, R 3.3e-16 | 4.1e-16, Rt 3.4e-16 | 4.0e-16,
    e 1.3e-13 | 6.3e-13, ll 1.5e-16 | 2.6e-16: every output at the 1e-10 bar.  The bar is always derived from the run at hand, never
    these."""
    m = uc.pendulum_model()
    U, Y = uc.pendulum_data(300)
    Y = Y.copy()
    Y[[3, 200, 298], 0] = np.nan
    _measured((m, U, Y, uc.pendulum_fg(m), uc.pendulum_fg(m, np.longdouble), ec.pendulum_jacs(m), ec.pendulum_jacs(m, np.longdouble), 0.0),
              ec.KIND_PENDULUM, host, maxiters, "pendulum, maxiters %d" % maxiters)


@pytest.mark.parametrize("maxiters", [2, 5])
def test_header_equals_the_formulas_on_the_square_measurement(host, maxiters):
    """3b. f(x) = x, g(x) = x_0^2 (T = 80, two missing rows, epsilon = 0).  Measured in this test, restatement float64 against long
    double | header against restatement — maxiters = 2: ll_steps 2.9e-16 | 3.6e-16, x 7.1e-17 | 7.5e-17, xt 7.1e-17 | 7.5e-17,
    R 1.2e-16 | 3.1e-16, Rt 6.6e-16 | 1.9e-15, e 1.2e-14 | 2.3e-15, ll 7.1e-17 | 5.4e-16; maxiters = 5: ll_steps 3.2e-16 | 5.6e-16,
    x 7.6e-17 | 1.1e-16, xt 7.6e-17 | 1.1e-16, R 1.1e-16 | 5.2e-16, Rt 9.2e-16 | 1.9e-15, e 6.7e-15 | 4.0e-15, ll 2.3e-17 | 0: every
    output at the 1e-10 bar.  The bar is always derived from the run at hand, never these."""
    m = ec.square_model(1.0, 0.36)
    Y = 3.0 + 0.5 * np.random.default_rng(3).standard_normal((80, 1))
    Y[[0, 40], 0] = np.nan
    fg, jac = ic.square_fg_jacs()
    fgl, jacl = ic.square_fg_jacs(np.longdouble)
    _measured((m, None, Y, fg, fgl, jac, jacl, 0.0), ec.KIND_SQUARE, host, maxiters, "square, maxiters %d" % maxiters)


def _one_step(host, model, kind, y, maxiters, epsilon):
    got, _ = ic.host_run(host, [model], np.zeros((1, 1)), np.array([[y]]), 1, maxiters, epsilon, kind=kind)
    return got["xt"][0, 0], got["Rt"][0, 0], int(got["iters"][0, 0])


def test_known_answer_the_posterior_mode(host):
    """4. One step at maxiters = 50, epsilon = 0 returns the mode of p(x | y): the gradient of -log p there,
    -C' R2^-1 (y - g(x)) + Rb^-1 (x - xb), is at most 1e-10 max(1, size of its two terms) in the infinity norm, while after the single
    step of the plain filter (maxiters = 1) it exceeds 1e-3 — the loop does something.  x0^2 with m = 1.7, P = 0.36, R2 = 0.25, y = 3:
    xt = 1.73029496 and Rt = P R2 / (4 x^2 P + R2) = 0.0197314518 to 1e-9, x the last linearisation point.  The pendulum's sin(x0) with
    m = (0.8, 0), P = 0.3 I, R2 = 0.05^2, y = 0.95; with epsilon = 1e-8 it stops after 9 linearisations.
    Measured here: x0^2 2.1e-15 after 6 linearisations (plain step 1.1e-2), pendulum 2.3e-14 after 15 (plain step 6.8)."""
    (_, gs), (_, gjs) = ic.square_fg_jacs()
    sq = ec.square_model(1.7, 0.36, 0.25)
    xb, Rb, R2 = np.array([1.7]), np.array([[0.36]]), np.array([[0.25]])
    xt, Rt, n = _one_step(host, sq, ec.KIND_SQUARE, 3.0, 50, 0.0)
    grad, size = ic.stationarity(gs, gjs, R2, xb, Rb, [3.0], xt)
    xt1, _, n1 = _one_step(host, sq, ec.KIND_SQUARE, 3.0, 1, 0.0)
    grad1, _ = ic.stationarity(gs, gjs, R2, xb, Rb, [3.0], xt1)
    print("square: |gradient| %.2e after %d linearisations, %.2e after the plain step" % (grad, n, grad1))
    assert grad <= 1e-10 * max(1.0, size), (grad, size)
    assert n1 == 1 and grad1 > 1e-3, grad1
    # the mode is the root near m of the cubic 8 x^3 - 24 x + (x - m) / P = 0 (the gradient above, R2 = 0.25, y = 3), found by numpy's
    # companion-matrix eigenvalues.  The literal 1.73029496 has nine digits: it is the mode, 1.730294958..., rounded, and can be met to
    # half a unit of its last digit only (5e-9); the 1e-9 bar is held against the root itself.
    roots = np.roots([8.0, 0.0, 1.0 / 0.36 - 24.0, -1.7 / 0.36])
    mode = float(roots[np.argmin(np.abs(roots - 1.7))].real)
    assert abs(xt[0] - mode) <= 1e-9 and abs(mode - 1.73029496) <= 5e-9 and abs(xt[0] - 1.73029496) <= 5e-9, (xt, mode)
    assert abs(Rt[0, 0] - 0.0197314518) <= 1e-9, Rt
    # with epsilon = 0 the last linearisation point is xt itself to the last bit or two
    assert abs(Rt[0, 0] - 0.36 * 0.25 / (4 * xt[0] ** 2 * 0.36 + 0.25)) <= 1e-13

    pm = uc.pendulum_model()
    _, gp = uc.pendulum_fg(pm)
    _, gjp = ec.pendulum_jacs(pm)
    xb, Rb, R2 = np.array([0.8, 0.0]), 0.3 * np.eye(2), np.array([[0.05 ** 2]])
    xt, _, n = _one_step(host, pm, ec.KIND_PENDULUM, 0.95, 50, 0.0)
    grad, size = ic.stationarity(gp, gjp, R2, xb, Rb, [0.95], xt)
    xt1, _, _ = _one_step(host, pm, ec.KIND_PENDULUM, 0.95, 1, 0.0)
    grad1, _ = ic.stationarity(gp, gjp, R2, xb, Rb, [0.95], xt1)
    print("pendulum: |gradient| %.2e after %d linearisations, %.2e after the plain step" % (grad, n, grad1))
    assert grad <= 1e-10 * max(1.0, size), (grad, size)
    assert grad1 > 1e-3, grad1
    assert _one_step(host, pm, ec.KIND_PENDULUM, 0.95, 50, 1e-8)[2] == 9


def _set_iterations(h, maxiters, epsilon):
    L = _capi.lib()
    return L.llpf_ekf_bank_set_iterations(h, maxiters, epsilon), L.llpf_last_error().decode()


def test_arguments_are_refused_before_the_handle_is_looked_at():
    """5a. maxiters outside 1..100, an epsilon that is negative or not finite, and a null handle: LLPF_ERR_ARG with a message that starts
    with `ekf`, on a machine with or without a device (the two numbers are checked before the handle)."""
    for maxiters in (0, -1, 101, 2 ** 31 - 1):
        rc, msg = _set_iterations(None, maxiters, 1e-8)
        assert rc == _capi.ERR_ARG and msg.startswith("ekf") and "1..100" in msg and "LLPF_IEKF_MAXITERS" in msg, (maxiters, rc, msg)
    for eps in (-1e-300, -1.0, float("inf"), float("-inf"), float("nan")):
        rc, msg = _set_iterations(None, 10, eps)
        assert rc == _capi.ERR_ARG and msg.startswith("ekf") and "epsilon" in msg, (eps, rc, msg)
    for maxiters, eps in ((1, 0.0), (100, 0.0), (10, 1e-8)):
        rc, msg = _set_iterations(None, maxiters, eps)
        assert rc == _capi.ERR_ARG and msg.startswith("ekf") and "null handle" in msg, (rc, msg)


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    """5b. Valid arguments on a machine without a device: LLPF_ERR_NO_DEVICE from the filter and from the bank."""
    spec = (llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
            llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    iekf = llpf_amd.IteratedExtendedKalmanFilter(*spec)
    assert (iekf.maxiters, iekf.epsilon) == (10, 1e-8)
    with pytest.raises(_capi.LLPFError) as ei:
        llpf_amd.loglik(iekf, *M.quadtank_data(5))
    assert ei.value.code == _capi.ERR_NO_DEVICE
    with pytest.raises(_capi.LLPFError) as ei:
        llpf_amd.IteratedExtendedKalmanFilterBank([spec], maxiters=3)
    assert ei.value.code == _capi.ERR_NO_DEVICE


def test_the_symbol_is_declared_exported_and_bound_and_the_classes_are_public(monkeypatch):
    """5c. llpf_ekf_bank_set_iterations in include/llpf.h, in the library and in _capi.SYMBOLS; both classes exported, subclasses of the
    extended filter and bank, with the documented defaults; the handle has the method; a snippet without Jacobians is refused as the
    extended filter refuses it"""
    n = "llpf_ekf_bank_set_iterations"
    header = open(os.path.join(ec.ROOT, "include", "llpf.h")).read()
    assert n + "(" in header and hasattr(_capi.lib(), n) and n in _capi.SYMBOLS
    assert _capi.SYMBOLS[n] == [C.c_void_p, C.c_int32, C.c_double]
    assert hasattr(_capi.EkfBankHandle, "set_iterations")
    assert issubclass(llpf_amd.IteratedExtendedKalmanFilter, llpf_amd.ExtendedKalmanFilter)
    assert issubclass(llpf_amd.IteratedExtendedKalmanFilterBank, llpf_amd.ExtendedKalmanFilterBank)
    assert "IteratedExtendedKalmanFilter" in llpf_amd.api.__all__ and "IteratedExtendedKalmanFilterBank" in llpf_amd.api.__all__
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")      # the traced snippet compiles without a device
    d0 = llpf_amd.MvNormal(np.array([1.0]), 0.36)
    f = llpf_amd.IteratedExtendedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25, d0, nu=0, ny=1,
                                              maxiters=4, epsilon=1e-6)
    assert (f.maxiters, f.epsilon, f.nx, f.ny) == (4, 1e-6, 1, 1) and "measurement_jac" in f.dynamics.src
    major, minor = C.c_int32(), C.c_int32()
    assert _capi.lib().llpf_version(C.byref(major), C.byref(minor)) == _capi.OK and (major.value, minor.value) == (0, 7)


def test_a_filter_that_loses_definiteness_inside_an_iteration_is_nan_from_that_step_on(host):
    """5d. x0^2 from covariances that are not positive definite, beside a healthy neighbour, at maxiters = 10, epsilon = 1e-8.  Filter 0
    (P = -5) has S = 4 m^2 P + R2 < 0 at the first linearisation.  Filter 1 (m = 1, P = -0.01, y = -30) has S = 0.21 > 0 there, moves to
    x_1 = 3.95 and has S = 4 x_1^2 P + R2 < 0 at the second: NaN inside the iteration, which stops at once.  Both are NaN from the first
    step on, and filter 2 is bit for bit what it is alone."""
    Y = np.stack([np.full((30, 1), 3.0), np.full((30, 1), -30.0), np.full((30, 1), 3.0)])
    models = [ec.square_model(1.7, 0.36), ec.square_model(1.0, 0.36), ec.square_model(1.5, 0.2)]
    x0 = np.array([[1.7], [1.0], [1.5]])
    P0 = np.array([[[-5.0]], [[-0.01]], [[0.2]]])
    both, _ = ic.host_run(host, models, None, Y, 30, 10, 1e-8, per_filter=2, kind=ec.KIND_SQUARE, state=(x0, P0))
    for f, first in ((0, 1), (1, 2)):
        assert np.isnan(both["ll_steps"][:, f]).all() and np.isnan(both["xt"][:, f]).all() and np.isnan(both["Rt"][:, f]).all(), f
        assert np.isnan(both["ll"][f]) and not np.isnan(both["x"][0, f]).any() and np.isnan(both["x"][1:, f]).all(), f
        assert both["iters"][0, f] == first and np.all(both["iters"][1:, f] == 1), (f, both["iters"][:, f])
    assert not np.isnan(both["ll_steps"][:, 2]).any() and not np.isnan(both["Rt"][:, 2]).any() and both["iters"][:, 2].max() > 2
    solo, _ = ic.host_run(host, models[2:], None, Y[2:], 30, 10, 1e-8, per_filter=2, kind=ec.KIND_SQUARE, state=(x0[2:], P0[2:]))
    for k in OUTPUTS:
        assert kc.bits_equal(both[k][:, 2], solo[k][:, 0]), k
    assert np.array_equal(both["iters"][:, 2], solo["iters"][:, 0])
    assert kc.bits_equal(both["ll"][2:], solo["ll"])
