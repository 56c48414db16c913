"""Banks of square-root extended Kalman filters (llpf_sqekf_bank_*), the checks that need no GPU: the host build of
csrc/shared/llpf_sqekf.h (tests/sqekf_host.c) — the definition the device reproduces bit for bit (tests/test_gpu_sqekf.py) — carries the
square-root Kalman twin's factor on linear models, computes the extended Kalman filter on nonlinear ones, stays finite where the
covariance form of the extended filter turns NaN; the ABI refuses its arguments before a device is looked for; the run-time program of
k_sqekf compiles for gfx950 without a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import kalman_common as kc
import models as M
import sqekf_common as qc
import sqkf_common as sc
import ukf_common as uc
import user_models as UM

ROOT = kc.ROOT
PKG = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd")
OUTPUTS = _capi.KALMAN_OUTPUTS
ARITY = {"llpf_sqekf_bank_create": 4, "llpf_sqekf_bank_destroy": 1, "llpf_sqekf_bank_reset": 1, "llpf_sqekf_bank_set_models": 2,
         "llpf_sqekf_bank_run": 8, "llpf_sqekf_bank_get_state": 4, "llpf_sqekf_bank_set_state": 4}


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    """(the square-root Kalman twin, the square-root extended twin with ekf_host.c's ekf_host_run beside it)"""
    d = tmp_path_factory.mktemp("sqekf_host")
    return sc.build_host(d), qc.build_host(d)


# ------------------------------------------------------------------------------------------------
# 1. linear models: the square-root Kalman filter, its factor bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", range(1, 5))
def test_linear_model_is_the_square_root_kalman_filter_with_its_factor_bits(hosts, nx):
    """every ny 1..4, F = 6 random systems in the three covariance kinds with D = 0, nu drawn in 0..3, T = 100, rows 0, 50 and 99
    missing: R, Rt and the final L (and the final R) are the square-root Kalman twin's bits — the factor arithmetic is llpf_sq_predict's /
    llpf_sq_correct's with A / C read from the Jacobian arrays; x, xt, e, ll_steps within kc.close (rtol 1e-10) and ll within 1e-10
    relative, the bar test_sqkf.py uses between twins (the mean goes through the model's own functions here)"""
    hs, hq = hosts
    for ny in range(1, 5):
        rng = np.random.default_rng(2000 + 10 * nx + ny)
        nu = int(rng.integers(0, 4))
        systems = [kc.random_system(rng, nx, ny, nu, k % 3, D=False) for k in range(6)]
        U, Y = kc._data(rng, 100, nu, ny, missing=(0, 50, 99))
        ref, (xr, Rr, Lr) = sc.host_run(hs, systems, U, Y, 100)
        got, (xg, Rg, Lg) = qc.host_run(hq, [m for m, _ in systems], U, Y, 100)
        for k in ("R", "Rt"):
            assert kc.bits_equal(got[k], ref[k]), (nx, ny, k)
        assert kc.bits_equal(Lg, Lr) and kc.bits_equal(Rg, Rr), (nx, ny, "final factor")
        for k in ("x", "xt", "e", "ll_steps"):
            assert kc.close(got[k], ref[k]), (nx, ny, k)
        assert kc.close(xg, xr), (nx, ny, "final x")
        assert np.all(np.abs(got["ll"] - ref["ll"]) <= 1e-10 * np.abs(ref["ll"])), (nx, ny)
        assert np.all(got["ll_steps"][[0, 50, 99]] == 0.0) and np.all(np.isnan(got["e"][[0, 50, 99]]))


# ------------------------------------------------------------------------------------------------
# 2. nonlinear models: the extended Kalman filter of the textbook formulas
# ------------------------------------------------------------------------------------------------
MULTIPLE = 10.0


def _measured(case, kind, hq, what):
    """header vs restatement with the bar of test_ekf.py's _measured: the restatement's own float64-against-long-double error is measured
    in the same run; the bar is 1e-10 where MULTIPLE times that error is below it, otherwise MULTIPLE times the measured error"""
    m, U, Y, fg, fgl, jac, jacl, t0 = case
    R1, R2 = S.gaussian_cov_matrix(m.dynamics_density), S.gaussian_cov_matrix(m.measurement_density)
    x0, P0 = S.gaussian_mean(m.initial_density), S.gaussian_cov_matrix(m.initial_density)
    a = ec.numpy_ekf(fg[0], fg[1], jac[0], jac[1], R1, R2, x0, P0, U, Y, m.Ts, t0)
    b = ec.numpy_ekf(fgl[0], fgl[1], jacl[0], jacl[1], R1, R2, x0, P0, U, Y, m.Ts, t0, lin=uc.LinLong)
    own = {k: uc.rel_err(a[k], b[k]) for k in OUTPUTS + ("ll",)}
    got, _ = qc.host_run(hq, [m], U, Y, Y.shape[0], t_index0=t0, kind=kind)
    assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), what
    err = {k: uc.rel_err(got[k][:, 0], b[k].astype(np.float64)) for k in OUTPUTS}
    err["ll"] = uc.rel_err(got["ll"][0], float(b["ll"]))
    print(what, "ll %.6f" % got["ll"][0], "restatement float64 vs long double:", {k: "%.2e" % v for k, v in own.items()})
    print(what, "header vs long-double restatement:", {k: "%.2e" % v for k, v in err.items()})
    for k in err:
        bar = 1e-10 if MULTIPLE * own[k] <= 1e-10 else MULTIPLE * own[k]
        assert err[k] <= bar, (what, k, err[k], bar)


def test_header_equals_the_formulas_on_the_quadtank(hosts):
    """The quad-tank on models.quadtank_data(1000) with three missing rows, across tau = TSWITCH, against ekf_common.numpy_ekf in
    np.longdouble; the bar is test_ekf.py's: ten times the float64 restatement's own error against long double, floor 1e-10.  The
    multiple of ten was enough (measured figures in DESIGN.md 7); the bar is always derived from the run at hand."""
    m = M.quadtank_model()
    U, Y = M.quadtank_data(1000)
    Y = Y.copy()
    Y[[5, 400, 777], 0] = np.nan
    _measured((m, U, Y, uc.quadtank_fg(m), uc.quadtank_fg(m, np.longdouble), ec.quadtank_jacs(m), ec.quadtank_jacs(m, np.longdouble), 1.0),
              ec.KIND_QUADTANK, hosts[1], "quad-tank")


def test_header_equals_the_formulas_on_the_pendulum(hosts):
    """The pendulum through its C twin with hand-written Jacobians against the long-double restatement with np.sin / np.cos, T = 1000
    with three missing rows; the bar as above."""
    m = uc.pendulum_model()
    U, Y = uc.pendulum_data(1000)
    Y = Y.copy()
    Y[[3, 500, 998], 0] = np.nan
    _measured((m, U, Y, uc.pendulum_fg(m), uc.pendulum_fg(m, np.longdouble), ec.pendulum_jacs(m), ec.pendulum_jacs(m, np.longdouble), 0.0),
              ec.KIND_PENDULUM, hosts[1], "pendulum")


def test_header_equals_the_formulas_on_the_square_model(hosts):
    """f(x) = x, g(x) = x_0^2 from the prior (1.7, 0.36), Y = 3 + 0.5 N(0, 1), T = 80 with one missing row; the bar as above.  And the
    known answer of one step: e = y - m^2, S = 4 m^2 P + R2, to 1e-13."""
    m = ec.square_model(1.7, 0.36)
    rng = np.random.default_rng(3)
    Y = 3.0 + 0.5 * rng.standard_normal((80, 1))
    Y[40, 0] = np.nan

    def fg(dt):
        return (lambda x, u, tau: np.asarray(x, dtype=dt)), (lambda x, u, tau: np.array([x[0] * x[0]], dtype=dt))

    def jacs(dt):
        return (lambda x, u, tau: np.eye(1, dtype=dt)), (lambda x, u, tau: np.array([[x[0] + x[0]]], dtype=dt))

    _measured((m, None, Y, fg(np.float64), fg(np.longdouble), jacs(np.float64), jacs(np.longdouble), 0.0), ec.KIND_SQUARE, hosts[1], "square")
    m0, P, r2, y = 1.7, 0.36, 0.25, 3.0
    got, _ = qc.host_run(hosts[1], [m], None, np.array([[y]]), 1, kind=ec.KIND_SQUARE)
    e, S_ = y - m0 * m0, 4 * m0 * m0 * P + r2
    K = 2 * m0 * P / S_
    ll = -0.5 * (np.log(2 * np.pi) + np.log(S_) + e * e / S_)
    assert abs(got["e"][0, 0, 0] - e) <= 1e-13 * abs(e)
    assert abs(got["xt"][0, 0, 0] - (m0 + K * e)) <= 1e-13 * abs(m0 + K * e)
    assert abs(got["Rt"][0, 0, 0, 0] - (P - K * 2 * m0 * P)) <= 1e-13 * P
    assert abs(got["ll_steps"][0, 0] - ll) <= 1e-13 * abs(ll) and got["ll"][0] == got["ll_steps"][0, 0]


# ------------------------------------------------------------------------------------------------
# 3. the point of the filter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_ill_conditioned_systems_stay_finite_where_the_extended_filter_is_nan(hosts, case):
    """sqkf_common.ill_conditioned run as models with Jacobians.  The precondition: tests/ekf_host.c's ekf_host_run gives a NaN ll
    there (its covariance arithmetic is the Kalman twin's).  The new twin is finite at every step, and its factor — R, Rt, the final L —
    is the square-root Kalman twin's bits."""
    hs, hq = hosts
    system, model, Y = qc.ill_conditioned_models(case)
    plain = qc.ekf_host_run(hq, [model], None, Y, 50)
    assert np.isnan(plain["ll"][0])                       # the condition on the inputs: the covariance form fails here
    got, (xg, Rg, Lg) = qc.host_run(hq, [model], None, Y, 50)
    for k in OUTPUTS + ("ll",):
        assert np.all(np.isfinite(got[k])), k
    ref, (xr, Rr, Lr) = sc.host_run(hs, [system], None, Y, 50)
    for k in ("R", "Rt"):
        assert kc.bits_equal(got[k], ref[k]), k
    assert kc.bits_equal(Lg, Lr) and kc.bits_equal(Rg, Rr)
    assert min(np.linalg.eigvalsh(R).min() for R in got["Rt"][:, 0]) >= 0.0


def test_diffuse_pendulum_with_a_near_exact_sensor_stays_finite(hosts):
    """The nonlinear case of the same kind: the pendulum with cov(d0) = 1e10 I, R2 = 1e-10, R1 = 1e-14 I (sqekf_common.diffuse_pendulum).
    The precondition: ekf_host_run's ll is NaN on it.  The new twin is finite at every step with Rt positive semidefinite."""
    _, hq = hosts
    m, U, Y = qc.diffuse_pendulum()
    plain = qc.ekf_host_run(hq, [m], U, Y, 50, kind=ec.KIND_PENDULUM)
    assert np.isnan(plain["ll"][0])                       # the condition on the inputs
    got, _ = qc.host_run(hq, [m], U, Y, 50, kind=ec.KIND_PENDULUM)
    for k in OUTPUTS + ("ll",):
        assert np.all(np.isfinite(got[k])), k
    assert min(np.linalg.eigvalsh(R).min() for R in got["Rt"][:, 0]) >= 0.0


def test_twin_continues_through_the_factor_bit_for_bit(hosts):
    """run(a) then run(b) from the factor the first run left is run(a + b), on the quad-tank across the switch time; a state given as a
    covariance starts from llpf_kf_chol of it"""
    _, hq = hosts
    m = M.quadtank_model()
    U, Y = M.quadtank_data(40)
    whole, (xw, Rw, Lw) = qc.host_run(hq, [m], U, Y, 40, t_index0=480.0)
    a, (xa, Ra, La) = qc.host_run(hq, [m], U[:15], Y[:15], 15, t_index0=480.0)
    assert np.array_equal(La, np.tril(La)) and np.all(np.diagonal(La, axis1=1, axis2=2) >= 0.0)
    b, (xb, Rb, Lb) = qc.host_run(hq, [m], U[15:], Y[15:], 25, t_index0=495.0, factor=(xa, La))
    for k in OUTPUTS:
        assert kc.bits_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    assert kc.bits_equal(xb, xw) and kc.bits_equal(Lb, Lw) and kc.bits_equal(Rb, Rw)
    facs = np.stack([sc.host_chol(hosts[0], R)[1] for R in Ra])
    viaR, _ = qc.host_run(hq, [m], U[15:], Y[15:], 25, t_index0=495.0, state=(xa, Ra))
    viaL, _ = qc.host_run(hq, [m], U[15:], Y[15:], 25, t_index0=495.0, factor=(xa, facs))
    for k in OUTPUTS:
        assert kc.bits_equal(viaR[k], viaL[k]), k


# ------------------------------------------------------------------------------------------------
# 4. the ABI without a device
# ------------------------------------------------------------------------------------------------
def _create(models):
    L = _capi.lib()
    arr = (S.Model * len(models))(*models)
    h = C.c_void_p()
    rc = L.llpf_sqekf_bank_create(0, arr, len(models), C.byref(h))
    if rc == _capi.OK:
        L.llpf_sqekf_bank_destroy(h)
    return rc, L.llpf_last_error().decode()


def test_header_binding_library_and_julia_name_the_same_exports():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    capi = open(os.path.join(PKG, "csrc", "capi.hip")).read()
    jl = open(os.path.join(PKG, "julia", "LLPFAmd.jl")).read()
    L = _capi.lib()
    declared = sorted(set(re.findall(r"\b(llpf_sqekf_[a-z_]+)\s*\(", hdr)))
    assert declared == sorted(ARITY)
    assert sorted(n for n in _capi.SYMBOLS if n.startswith("llpf_sqekf_")) == declared
    assert sorted(set(re.findall(r"ccall\(\(:(llpf_sqekf_[a-z_]+), LIB\)", jl))) == declared
    for name in declared:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert len(m.group(1).split(",")) == ARITY[name], name
        assert hasattr(L, name) and len(_capi.SYMBOLS[name]) == ARITY[name], name
        assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % name, capi, re.M) and "LLPF_GUARD(%s)" % name in capi, name
        j = re.search(r"ccall\(\(:%s, LIB\),\s*\w+,\s*\((.*?)\),\s" % name, jl, re.S).group(1)
        assert len([a for a in re.sub(r"\{[^}]*\}", "", j).split(",") if a.strip()]) == ARITY[name], (name, j)
    exported = re.search(r"^export (.*?)\n\n", jl, re.S | re.M).group(1)
    for name in ("GPUSqExtendedKalmanFilter", "GPUSqExtendedKalmanFilterBank", "sqekf_run"):
        assert re.search(r"\b%s\b" % name, exported), name
    for name in ("SqExtendedKalmanFilter", "SqExtendedKalmanFilterBank"):
        assert name in llpf_amd.api.__all__ and hasattr(llpf_amd, name)
    assert "llpf_sqekf_bank_smooth" not in hdr and "llpf_sqekf_bank_set_iterations" not in hdr


def test_arguments_are_refused_before_a_device_is_looked_for():
    """every argument check of create answers LLPF_ERR_ARG under this bank's prefix on a machine with or without a device; every export
    answers a null handle with "null handle", create a null out pointer with "null out pointer" """
    lg = M.lg_test_model()
    for mid in (S.MODEL_RB_LINEAR, S.MODEL_RB_BILINEAR):
        m = S.Model.from_buffer_copy(bytes(lg))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "Rao-Blackwellized" in msg and "square-root extended Kalman filter" in msg and msg.startswith("sqekf: "), msg
    rng = np.random.default_rng(0)
    for nx, ny in ((9, 1), (2, 5)):
        m, _ = kc.random_system(rng, nx, ny, 1, D=False)
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "1..8" in msg, (rc, msg)
    qt = S.Model.from_buffer_copy(bytes(M.quadtank_model()))
    qt.nu = 1
    rc, msg = _create([qt])
    assert rc == _capi.ERR_ARG and "quad-tank" in msg
    rc, msg = _create([lg, M.lg_c1_model()])
    assert rc == _capi.ERR_ARG and "differ from filter 0" in msg
    g = S.make_gaussian
    rc, msg = _create([S.make_lg_model(np.eye(2) * 0.9, np.zeros((2, 1)), np.array([[1.0, 0.0]]), g(np.ones(2), 0.1), g(np.zeros(1), 0.1), g(np.zeros(2), 0.1))])
    assert rc == _capi.ERR_ARG and "zero mean" in msg
    L = _capi.lib()
    h = C.c_void_p()
    arr = (S.Model * 1)(lg)
    err = lambda: L.llpf_last_error().decode()
    assert L.llpf_sqekf_bank_create(0, None, 1, C.byref(h)) == _capi.ERR_ARG and err() == "sqekf: models is null"
    assert L.llpf_sqekf_bank_create(0, arr, 0, C.byref(h)) == _capi.ERR_ARG and "n_filters must be >= 1" in err()
    assert L.llpf_sqekf_bank_create(0, arr, 1, None) == _capi.ERR_ARG and err() == "null out pointer"
    assert not h.value
    x = np.zeros(4)
    for rc in (L.llpf_sqekf_bank_reset(None), L.llpf_sqekf_bank_set_models(None, arr),
               L.llpf_sqekf_bank_run(None, None, _capi.dptr(x), 1, 0, 0.0, None, None),
               L.llpf_sqekf_bank_get_state(None, None, None, None), L.llpf_sqekf_bank_set_state(None, _capi.dptr(x), _capi.dptr(x), None)):
        assert rc == _capi.ERR_ARG and err() == "null handle"
    assert L.llpf_sqekf_bank_destroy(None) == _capi.OK


def test_the_three_not_positive_definite_messages():
    """R1, R2 and cov(d0) are factored at create: one that is not positive definite — indefinite, or singular as a Kalman filter's may
    be — is LLPF_ERR_ARG naming the filter and which of the three, in the square-root Kalman bank's words under this bank's prefix"""
    rng = np.random.default_rng(1)
    m, _ = kc.random_system(rng, 3, 2, 1, D=False)
    indefinite = {3: np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), 2: np.array([[1.0, 2.0], [2.0, 1.0]])}
    for field, n, word in (("dynamics_density", 3, "R1 (dynamics_density)"), ("measurement_density", 2, "R2 (measurement_density)"),
                           ("initial_density", 3, "cov(d0) (initial_density)")):
        bad = S.Model.from_buffer_copy(m)
        setattr(bad, field, S.make_gaussian(np.zeros(n), indefinite[n], S.COV_FULL))
        rc, msg = _create([m, bad])
        assert rc == _capi.ERR_ARG and msg == "sqekf: filter 1: %s is not positive definite" % word, msg
    bad = S.Model.from_buffer_copy(m)
    bad.dynamics_density = S.make_gaussian(np.zeros(3), np.array([1.0, 0.0, 1.0]))
    rc, msg = _create([bad])
    assert rc == _capi.ERR_ARG and msg.startswith("sqekf: filter 0: R1") and "positive definite" in msg, msg


def test_models_without_jacobians_or_with_members_of_their_own_are_refused(monkeypatch):
    """the refusals of kf_pack_models hold unchanged: a compiled model with `loglik`, `noise` or `initial`, one without dynamics_jac or
    without measurement_jac (the message names the member), an unknown id; the Python filter raises TypeError naming the members"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    cases = [(UM.LAPLACE_SRC, 2, 1, "loglik"), (UM.LAPLACE_NOISE_SRC, 2, 1, "noise"), (ec.SQUARE_JAC_INITIAL_SRC, 1, 1, "initial"),
             (UM.PENDULUM_SRC, 2, 1, "dynamics_jac"), (ec.SQUARE_DYN_JAC_ONLY_SRC, 1, 1, "measurement_jac")]
    for src, nx, ny, word in cases:
        mid = _capi.model_compile(src + "\n// test_sqekf\n", nx, ny)
        m = S.Model.from_buffer_copy(bytes(M.lg_test_model() if nx == 2 else ec.square_model(1.0, 0.3)))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and word in msg and msg.startswith("sqekf: "), (word, rc, msg)
    m = S.Model.from_buffer_copy(bytes(M.lg_test_model()))
    m.model_id = 999999
    rc, msg = _create([m])
    assert rc == _capi.ERR_ARG and "unknown model id 999999" in msg
    d0 = llpf_amd.MvNormal(np.array([0.8, 0.0]), np.array([0.3, 0.3]))
    dyn = llpf_amd.UserDynamics(UM.PENDULUM_SRC, 2, 1, 1, qt=(9.81, 0.05))
    with pytest.raises(TypeError, match="dynamics_jac.*measurement_jac"):
        llpf_amd.SqExtendedKalmanFilter(dyn, llpf_amd.UserMeasurement(), np.array([1e-4, 4e-3]), 0.05 ** 2, d0, Ts=0.05)


def test_python_classes_without_a_device(monkeypatch):
    """both classes are built without a device (the bank of a filter is created on first use; the traced snippet compiles without one);
    plain callables are traced with their Jacobians; smooth of either raises TypeError with "no smoother"; the filter is not a mode of an
    IMM"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    d1 = llpf_amd.MvNormal(np.array([1.0]), 0.36)
    traced = llpf_amd.SqExtendedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25, d1, nu=0, ny=1)
    assert traced._handle is None and (traced.nx, traced.nu, traced.ny) == (1, 0, 1)
    assert "measurement_jac" in traced.dynamics.src and "dynamics_jac" in traced.dynamics.src
    qt = llpf_amd.SqExtendedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                         llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    assert qt._handle is None and qt._model.model_id == S.MODEL_QUADTANK_RK4
    assert not isinstance(qt, llpf_amd.ExtendedKalmanFilter) and issubclass(llpf_amd.SqExtendedKalmanFilterBank, llpf_amd.ExtendedKalmanFilterBank)
    assert llpf_amd.SqExtendedKalmanFilterBank._AT_LOGLIK == {"t_index0": 1.0} and llpf_amd.SqExtendedKalmanFilterBank._AT_FORWARD == {"t_index0": 0.0}
    models = llpf_amd.SqExtendedKalmanFilterBank._models([qt, (llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1),
                                                               np.full(2, 1e-4), llpf_amd.MvNormal(np.zeros(4), np.full(4, 0.1)))], 1.0)
    assert [mm.model_id for mm in models] == [S.MODEL_QUADTANK_RK4] * 2
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(qt, np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.SqExtendedKalmanFilterBank.smooth(None, None, None)
    with pytest.raises(TypeError, match="SqExtendedKalmanFilter"):
        llpf_amd.IMM([qt, qt], np.full((2, 2), 0.5), np.full(2, 0.5))


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    """valid arguments on a machine without a device: LLPF_ERR_NO_DEVICE, from the ABI and through the Python filter"""
    for m in (M.lg_test_model(), M.quadtank_model()):
        rc, msg = _create([m])
        assert rc == _capi.ERR_NO_DEVICE, (rc, msg)
    kf = llpf_amd.SqExtendedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                         llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    with pytest.raises(_capi.LLPFError) as ei:
        llpf_amd.loglik(kf, *M.quadtank_data(5))
    assert ei.value.code == _capi.ERR_NO_DEVICE


# ------------------------------------------------------------------------------------------------
# 5. the run-time program of k_sqekf
# ------------------------------------------------------------------------------------------------
def test_runtime_program_compiles_for_gfx950_without_a_device(tmp_path):
    """tests/jit_sqekf_host.cpp links libllpf_hip.so and calls sqekf_prepare the way tests/jit_programs_host.cpp calls the other units':
    (LG, 5, 1) and the quad-tank as a snippet at (4, 2) compile and are found again, the precompiled shapes need nothing, an unknown id
    fails with the message the other units give, a model without measurement_jac with the compiler's log under the kernel's name"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    if not os.path.exists(os.path.join(PKG, "libllpf_hip.so")):
        pytest.skip("libllpf_hip.so not built")
    exe = str(tmp_path / "jit_sqekf_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jit_sqekf_host.cpp"), "-L", PKG,
                    "-lllpf_hip", "-Wl,-rpath," + PKG, "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failed", r.stdout
    assert len([ln for ln in lines if ln.startswith("ok  ")]) == 11 and not [ln for ln in lines if ln.startswith("FAIL")]
