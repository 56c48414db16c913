"""Banks of extended Kalman filters, the part that needs no GPU: csrc/shared/llpf_ekf.h (the device order, built for the host by
tests/ekf_host.c) against the Kalman filter on linear models — R and Rt bit for bit — and against a numpy restatement of the textbook
formulas on nonlinear ones, the quad-tank's shared Jacobian header against the oracle, the traced model and central differences, a known
answer, and the argument checks of the C ABI (llpf_ekf_bank_*)."""
import ctypes as C
import os

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S, tracing as tr
import ekf_common as ec
import kalman_common as kc
import models as M
import oracle_binding as ob
import ukf_common as uc
import user_models as UM
from test_ukf import linear_systems, T_LIN

OUTPUTS = _capi.KALMAN_OUTPUTS


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ec.build_host(tmp_path_factory.mktemp("ekf_host"))


@pytest.fixture(scope="module")
def kalman_host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kf_host"))


def test_linear_model_is_the_kalman_filter_with_its_covariance_bits(host, kalman_host):
    """1. On the 32 random linear systems of test_ukf.py the host build of the header equals the restatement and the host build of the
    Kalman header to 1e-10 in every output, and its R and Rt are the Kalman header's bit for bit: the covariance arithmetic is
    llpf_kf_correct's / llpf_kf_predict's with C / A read from the Jacobian arrays."""
    worst = 0.0
    for m, D, mats, U, Y in linear_systems():
        f, g = uc.linear_fg(mats)
        fj, gj = ec.linear_jacs(mats)
        ref = ec.numpy_ekf(f, g, fj, gj, mats["R1"], mats["R2"], mats["x0"], mats["P0"], U, Y)
        kf, _ = kc.host_run(kalman_host, [(m, D)], U, Y, T_LIN)
        got, _ = ec.host_run(host, [m], U, Y, T_LIN)
        assert not np.isnan(got["ll"]).any(), (m.nx, m.ny)
        for k in OUTPUTS:
            worst = max(worst, uc.rel_err(got[k][:, 0], ref[k]))
            assert kc.close(got[k][:, 0], ref[k]), (m.nx, m.ny, k, "restatement")
            assert kc.close(got[k][:, 0], kf[k][:, 0]), (m.nx, m.ny, k, "Kalman header")
        assert kc.close(got["ll"][0], ref["ll"]) and kc.close(got["ll"][0], kf["ll"][0]), (m.nx, m.ny)
        for k in ("R", "Rt"):
            assert np.array_equal(got[k].view(np.uint64), kf[k].view(np.uint64)), (m.nx, m.ny, k, "bits of the Kalman header")
    print("linear => Kalman: worst relative error against the restatement %.2e" % worst)


def _orc_dynamics(model, x, u, t):
    out = np.empty(model.nx)
    fn = C.cast(ob.lib().orc_dynamics, C.CFUNCTYPE(None, C.POINTER(S.Model), ec._dp, ec._dp, C.c_double, ec._dp))
    x, u = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
    fn(C.byref(model), ec._p(x), ec._p(u), float(t), ec._p(out))
    return out


def test_quadtank_jacobian_header(host):
    """2. llpf_quadtank_jac.h: fx is the oracle's RK4 bit for bit; J is the traced quad-tank's forward-mode Jacobian to 1e-10 relative
    where that has an entry and exactly 0 where it has none; J is the central difference of fx to 1e-7 (roundoff eps |f| / h ~ 1e-9)."""
    rng = np.random.default_rng(7)
    Q = dict(S.QUADTANK_DEFAULTS)
    base = M.quadtank_model()
    worst_tr = worst_fd = 0.0
    for ss in (1, 2):
        m = S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, ss)
        g, outs = tr.trace(tr.rk4(ec.quadtank_rhs, 1.0, ss), 4, 2, p=Q)
        Jn = tr.jacobian(g, outs, 4)
        for k in range(500):
            x = rng.uniform(0.05, 6.0, 4)
            u = rng.uniform(0.0, 0.5, 2)
            t = (3.0, 499.5, 500.0, 777.0)[k % 4] if ss == 2 else (3.0, 499.0, 500.0, 501.0)[k % 4]
            fx, J = ec.host_qt_jac(host, m, x, u, t)
            assert np.array_equal(fx.view(np.uint64), _orc_dynamics(m, x, u, t).view(np.uint64)), (ss, k)
            if k % 5:
                continue
            Jt = np.array(tr.evaluate(g, Jn, x, u, t))
            for r in range(4):
                for c in range(4):
                    if Jn[r][c] is None:
                        assert J[r, c] == 0.0, (r, c)
                    else:
                        worst_tr = max(worst_tr, abs(J[r, c] - Jt[r, c]) / abs(Jt[r, c]))
                        assert abs(J[r, c] - Jt[r, c]) <= 1e-10 * abs(Jt[r, c]), (ss, k, r, c, J[r, c], Jt[r, c])
            fd = ec.central_differences(lambda z: ec.host_qt_jac(host, m, z, u, t)[0], list(x), 4)
            worst_fd = max(worst_fd, float(np.max(np.abs(J - fd))))
            assert np.all(np.abs(J - fd) <= 1e-7), (ss, k, J, fd)
    print("quad-tank Jacobian header: worst relative difference to the traced Jacobian %.2e, worst |J - central difference| %.2e" % (worst_tr, worst_fd))


def _measured(case, kind, host, what):
    """header vs restatement with the bar of test_ukf_smooth.py (3)-(4): the restatement's own float64-against-long-double error is
    measured in the same run; the bar is 1e-10 where ten times that error is below it, otherwise ten times the measured error"""
    m, U, Y, fg, fgl, jac, jacl, t0 = case
    R1, R2 = S.gaussian_cov_matrix(m.dynamics_density), S.gaussian_cov_matrix(m.measurement_density)
    x0, P0 = S.gaussian_mean(m.initial_density), S.gaussian_cov_matrix(m.initial_density)
    a = ec.numpy_ekf(fg[0], fg[1], jac[0], jac[1], R1, R2, x0, P0, U, Y, m.Ts, t0)
    b = ec.numpy_ekf(fgl[0], fgl[1], jacl[0], jacl[1], R1, R2, x0, P0, U, Y, m.Ts, t0, lin=uc.LinLong)
    own = {k: uc.rel_err(a[k], b[k]) for k in OUTPUTS + ("ll",)}
    got, _ = ec.host_run(host, [m], U, Y, Y.shape[0], t_index0=t0, kind=kind)
    assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), what
    err = {k: uc.rel_err(got[k][:, 0], a[k]) for k in OUTPUTS}
    err["ll"] = uc.rel_err(got["ll"][0], a["ll"])
    print(what, "ll %.6f" % got["ll"][0], "restatement float64 vs long double:", {k: "%.2e" % v for k, v in own.items()})
    print(what, "header vs restatement:", {k: "%.2e" % v for k, v in err.items()})
    for k in err:
        bar = 1e-10 if 10.0 * own[k] <= 1e-10 else 10.0 * own[k]
        assert err[k] <= bar, (what, k, err[k], bar)
    return got, a


def test_header_equals_the_formulas_on_the_quadtank(host):
    """3a. The quad-tank on models.quadtank_data(1000) with three missing rows, across tau = TSWITCH: the header around the shared
    Jacobian header against the restatement with the analytic Jacobian written in numpy (dense chain rule through the stages).
    Measured in this test (relative, ukf_common.rel_err): restatement float64 against long double ll_steps 2.6e-15, x 1.1e-15, xt 1.1e-15,
    R 2.5e-15, Rt 2.5e-15, e 7.4e-13, ll 1.8e-16; header against restatement ll_steps 2.0e-15, x 1.2e-16, xt 1.2e-16, R 9.3e-17,
    Rt 1.9e-16, e 5.0e-14, ll 2.5e-16: every output at the 1e-10 bar.  The bar is always derived from the run at hand, never these."""
    m = M.quadtank_model()
    U, Y = M.quadtank_data(1000)
    Y = Y.copy()
    Y[[5, 400, 777], 0] = np.nan
    _measured((m, U, Y, uc.quadtank_fg(m), uc.quadtank_fg(m, np.longdouble), ec.quadtank_jacs(m), ec.quadtank_jacs(m, np.longdouble), 1.0),
              ec.KIND_QUADTANK, host, "quad-tank")


def test_header_equals_the_formulas_on_the_pendulum(host):
    """3b. The pendulum through its C twin with hand-written Jacobians (the device snippet's expressions) against the restatement with
    np.sin / np.cos.  Measured in this test: restatement float64 against long double ll_steps 4.8e-13, x 5.8e-16, xt 5.8e-16, R 5.1e-16,
    Rt 5.0e-16, e 1.0e-11, ll 9.5e-17; header against restatement ll_steps 1.9e-13, x 9.3e-16, xt 9.6e-16, R 1.5e-15, Rt 1.5e-15,
    e 2.9e-11, ll 4.7e-16: 1e-10 everywhere except e, where ten times the measured error is 1.0e-10 and is the bar (the innovation of a
    measurement with 0.05 noise around sin(x0) cancels two digits).  The bar is always derived from the run at hand, never these."""
    m = uc.pendulum_model()
    U, Y = uc.pendulum_data(1000)
    Y = Y.copy()
    Y[[3, 500, 998], 0] = np.nan
    _measured((m, U, Y, uc.pendulum_fg(m), uc.pendulum_fg(m, np.longdouble), ec.pendulum_jacs(m), ec.pendulum_jacs(m, np.longdouble), 0.0),
              ec.KIND_PENDULUM, host, "pendulum")


def test_known_answer_of_the_linearisation(host):
    """4. g(x) = x_0^2, f(x) = x with prior (m, P): e = y - m^2 and S = 4 m^2 P + R2 — not the unscented m^2 + P and 2 P^2 + 4 m^2 P —
    to 1e-13; ll, xt, Rt by hand.  S is not an output: it is recovered from Rt = P - (2 m P)^2 / S."""
    m0, P, r2, y = 1.7, 0.36, 0.25, 3.0
    got, _ = ec.host_run(host, [ec.square_model(m0, P, r2)], None, np.array([[y]]), 1, kind=ec.KIND_SQUARE)
    e, S_ = y - m0 * m0, 4 * m0 * m0 * P + r2
    assert abs(got["e"][0, 0, 0] - e) <= 1e-13 * abs(e)
    assert abs(got["e"][0, 0, 0] - (y - (m0 * m0 + P))) > 0.3, "the unscented prediction is another number"
    CR = 2 * m0 * P
    S_got = CR * CR / (P - got["Rt"][0, 0, 0, 0])
    assert abs(S_got - S_) <= 1e-13 * S_ * (P / (P - got["Rt"][0, 0, 0, 0])), (S_got, S_)
    K = CR / S_
    assert abs(got["xt"][0, 0, 0] - (m0 + K * e)) <= 1e-13 * abs(m0 + K * e)
    assert abs(got["Rt"][0, 0, 0, 0] - (P - K * CR)) <= 1e-13 * P
    ll = -0.5 * (np.log(2 * np.pi) + np.log(S_) + e * e / S_)
    assert abs(got["ll_steps"][0, 0] - ll) <= 1e-13 * abs(ll) and got["ll"][0] == got["ll_steps"][0, 0]
    # predict: x stays, R grows by R1
    got2, st = ec.host_run(host, [ec.square_model(m0, P, r2)], None, np.array([[y], [y]]), 2, kind=ec.KIND_SQUARE)
    assert got2["x"][1, 0, 0] == got["xt"][0, 0, 0] and got2["R"][1, 0, 0, 0] == got["Rt"][0, 0, 0, 0] + 0.1


def _create(models):
    L = _capi.lib()
    arr = (S.Model * len(models))(*models)
    h = C.c_void_p()
    rc = L.llpf_ekf_bank_create(0, arr, len(models), C.byref(h))
    if rc == _capi.OK:
        L.llpf_ekf_bank_destroy(h)
    return rc, L.llpf_last_error().decode()


def test_arguments_are_refused_before_a_device_is_looked_for():
    """5a. Every argument check answers LLPF_ERR_ARG with its message on a machine with or without a device."""
    lg = M.lg_test_model()
    for mid in (S.MODEL_RB_LINEAR, S.MODEL_RB_BILINEAR):
        m = S.Model.from_buffer_copy(bytes(lg))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "Rao-Blackwellized" in msg and msg.startswith("ekf"), (mid, rc, msg)
    rng = np.random.default_rng(0)
    for nx, ny in ((9, 1), (2, 5)):
        m, _ = kc.random_system(rng, nx, ny, 1, D=False)
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "1..8" in msg, (rc, msg)
    qt = S.Model.from_buffer_copy(bytes(M.quadtank_model()))
    qt.nu = 1
    rc, msg = _create([qt])
    assert rc == _capi.ERR_ARG and "quad-tank" in msg
    g = S.make_gaussian
    A, B, Cm = np.eye(2) * 0.9, np.zeros((2, 1)), np.array([[1.0, 0.0]])
    bad = np.array([[1.0, 2.0], [2.0, 1.0]])
    ok2, ok1 = g(np.zeros(2), 0.1), g(np.zeros(1), 0.1)
    for df, dg, d0, word in ((ok2, g(np.zeros(1), -1.0), ok2, "R2"), (ok2, ok1, g(np.zeros(2), bad, S.COV_FULL), "cov(d0)"),
                             (g(np.zeros(2), bad, S.COV_FULL), ok1, ok2, "R1"), (g(np.ones(2), 0.1), ok1, ok2, "zero mean"),
                             (ok2, g(np.ones(1), 0.1), ok2, "zero mean")):
        rc, msg = _create([S.make_lg_model(A, B, Cm, df, dg, d0)])
        assert rc == _capi.ERR_ARG and word in msg, (word, rc, msg)
    rc, msg = _create([lg, M.lg_c1_model()])
    assert rc == _capi.ERR_ARG and "differ from filter 0" in msg
    rc, msg = _create([lg, M.quadtank_model()])
    assert rc == _capi.ERR_ARG and "differ from filter 0" in msg
    L = _capi.lib()
    h = C.c_void_p()
    arr = (S.Model * 1)(lg)
    assert L.llpf_ekf_bank_create(0, None, 1, C.byref(h)) == _capi.ERR_ARG
    assert L.llpf_ekf_bank_create(0, arr, 0, C.byref(h)) == _capi.ERR_ARG
    assert L.llpf_ekf_bank_create(0, arr, 1, None) == _capi.ERR_ARG
    assert L.llpf_ekf_bank_reset(None) == _capi.ERR_ARG and L.llpf_ekf_bank_set_models(None, arr) == _capi.ERR_ARG
    assert L.llpf_ekf_bank_run(None, None, None, 1, 0, 0.0, None, None) == _capi.ERR_ARG
    assert L.llpf_ekf_bank_get_state(None, None, None) == _capi.ERR_ARG and L.llpf_ekf_bank_set_state(None, None, None) == _capi.ERR_ARG
    assert L.llpf_ekf_bank_destroy(None) == _capi.OK


def test_models_without_jacobians_or_with_members_of_their_own_are_refused(monkeypatch):
    """5b. A compiled model with `loglik`, `noise` or `initial` is refused as the unscented bank refuses it; one without dynamics_jac
    or without measurement_jac is refused by this bank — and only by it — with a message that names the member; the Python filter
    raises TypeError naming the members (the snippets compile without a device)."""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    cases = [(UM.LAPLACE_SRC, 2, 1, "loglik"), (UM.LAPLACE_NOISE_SRC, 2, 1, "noise"), (UM.MULT_NOISE_BOX_SRC, 2, 1, "noise"),
             (ec.SQUARE_JAC_INITIAL_SRC, 1, 1, "initial"), (UM.PENDULUM_SRC, 2, 1, "dynamics_jac"),
             (ec.SQUARE_DYN_JAC_ONLY_SRC, 1, 1, "measurement_jac")]
    for src, nx, ny, word in cases:
        mid = _capi.model_compile(src + "\n// test_ekf\n", nx, ny)
        if word == "initial":      # the member alone: nothing else of the snippet is refused first
            assert _capi.model_traits(mid) == _capi.TRAIT_INITIAL | _capi.TRAIT_DYNAMICS_JAC | _capi.TRAIT_MEASUREMENT_JAC
        m = S.Model.from_buffer_copy(bytes(M.lg_test_model() if nx == 2 else ec.square_model(1.0, 0.3)))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and word in msg and msg.startswith("ekf"), (word, rc, msg)
    m = S.Model.from_buffer_copy(bytes(M.lg_test_model()))
    m.model_id = 999999
    assert _create([m])[0] == _capi.ERR_ARG
    # the unscented bank takes the pendulum without the members: past the argument checks (no device here: NO_DEVICE, with one: OK)
    pend = S.Model.from_buffer_copy(bytes(uc.pendulum_model()))
    pend.model_id = _capi.model_compile(UM.PENDULUM_SRC + "\n// test_ekf\n", 2, 1)
    L = _capi.lib()
    h = C.c_void_p()
    ws = _capi.ukf_weights((1.0, 0.0, 2.0, 0.5))
    rc = L.llpf_ukf_bank_create(0, (S.Model * 1)(pend), 1, C.byref(ws), C.byref(h))
    assert rc in (_capi.OK, _capi.ERR_NO_DEVICE)
    if rc == _capi.OK:
        L.llpf_ukf_bank_destroy(h)
    d0 = llpf_amd.MvNormal(np.array([0.8, 0.0]), np.array([0.3, 0.3]))
    dyn = llpf_amd.UserDynamics(UM.PENDULUM_SRC, 2, 1, 1, qt=(9.81, 0.05))
    with pytest.raises(TypeError, match="dynamics_jac.*measurement_jac"):
        llpf_amd.ExtendedKalmanFilter(dyn, llpf_amd.UserMeasurement(), np.array([1e-4, 4e-3]), 0.05 ** 2, d0, Ts=0.05)
    ok = llpf_amd.ExtendedKalmanFilter(llpf_amd.UserDynamics(ec.PENDULUM_JAC_SRC, 2, 1, 1, qt=(9.81, 0.05)), llpf_amd.UserMeasurement(),
                                       np.array([1e-4, 4e-3]), 0.05 ** 2, d0, Ts=0.05)
    assert ok.nx == 2 and ok.ny == 1
    traced = llpf_amd.ExtendedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25,
                                           llpf_amd.MvNormal(np.array([1.0]), 0.36), nu=0, ny=1)
    assert "measurement_jac" in traced.dynamics.src


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    """5c. Valid arguments on a machine without a device: LLPF_ERR_NO_DEVICE."""
    for m in (M.lg_test_model(), M.quadtank_model()):
        rc, msg = _create([m])
        assert rc == _capi.ERR_NO_DEVICE, (rc, msg)
    ekf = llpf_amd.ExtendedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                        llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    with pytest.raises(_capi.LLPFError) as ei:
        llpf_amd.loglik(ekf, *M.quadtank_data(5))
    assert ei.value.code == _capi.ERR_NO_DEVICE


def test_the_symbols_are_declared_exported_and_bound():
    """5d. the seven llpf_ekf_bank_* symbols: in include/llpf.h, in the library, in _capi.SYMBOLS; both classes exported"""
    names = ["llpf_ekf_bank_" + v for v in ("create", "destroy", "reset", "set_models", "run", "get_state", "set_state")]
    header = open(os.path.join(ec.ROOT, "include", "llpf.h")).read()
    L = _capi.lib()
    for n in names:
        assert n + "(" in header and hasattr(L, n) and n in _capi.SYMBOLS, n
    assert "llpf_ekf_bank_smooth" not in header
    assert llpf_amd.ExtendedKalmanFilter is not None and issubclass(llpf_amd.ExtendedKalmanFilterBank, llpf_amd.api._KfBank)
    assert "ExtendedKalmanFilter" in llpf_amd.api.__all__ and "ExtendedKalmanFilterBank" in llpf_amd.api.__all__


def test_a_filter_that_loses_definiteness_is_nan_from_that_step_on(host):
    """5e. A filter started from a covariance that is not positive definite has S = 4 m^2 P + R2 < 0: in the host build it is NaN from
    the first step on, while its neighbour in the same call is bit for bit what it is alone."""
    Ysq = np.full((30, 1), 3.0)
    models = [ec.square_model(1.7, 0.36), ec.square_model(1.5, 0.2)]
    x0 = np.array([[1.7], [1.5]])
    P0 = np.array([[[-5.0]], [[0.2]]])
    both, _ = ec.host_run(host, models, None, Ysq, 30, kind=ec.KIND_SQUARE, state=(x0, P0))
    assert np.isnan(both["ll_steps"][:, 0]).all() and np.isnan(both["xt"][:, 0]).all() and np.isnan(both["Rt"][:, 0]).all() and np.isnan(both["ll"][0])
    assert not np.isnan(both["x"][0, 0]).any() and np.isnan(both["x"][1:, 0]).all()
    assert not np.isnan(both["ll_steps"][:, 1]).any() and not np.isnan(both["Rt"][:, 1]).any()
    solo, _ = ec.host_run(host, models[1:], None, Ysq, 30, kind=ec.KIND_SQUARE, state=(x0[1:], P0[1:]))
    for k in OUTPUTS:
        assert kc.bits_equal(both[k][:, 1], solo[k][:, 0]), k
    assert kc.bits_equal(both["ll"][1:], solo["ll"])
