"""The IMM filter over first-order extended Kalman filter modes on the host (tests/imm_ekf_host.c, the build of csrc/shared/llpf_imm.h over
csrc/shared/llpf_ekf.h — the six stages of tests/kf_host_frame.h over the extended family — that the device is held to in
test_gpu_imm_ekf.py): with one mode it is the extended Kalman filter of
tests/ekf_host.c bit for bit, on linear modes it is the Kalman IMM of tests/imm_host.c, it is the textbook recursion (a numpy
restatement in literal formulas, float64 and long double), it has the known answer of the linearisation, it finds the mode of switching
data, and the C ABI and the Python classes refuse what they cannot run.  No GPU needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import imm_common as ic
import kalman_common as kc
import models as M
import ukf_common as uc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ic.build_host(tmp_path_factory.mktemp("imm_ekf_host"))


def _pendulum_modes(n, r1=False):
    """n pendulum descriptors that differ in g / l and the damping (and, r1, in R1)"""
    out = []
    for j in range(n):
        m = uc.pendulum_model()
        m.qt[0], m.qt[1] = 9.81 * (1.0 - 0.25 * j), 0.05 + 0.04 * j
        if r1:
            m.dynamics_density = S.make_gaussian(np.zeros(2), np.array([1e-4, 4e-3]) * (1.0 + j))
        out.append(m)
    return out


def _quadtank_modes(n):
    """n quad-tank descriptors that differ in gamma1 and a1"""
    base = M.quadtank_model()
    return [S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, 2, gamma1=0.2 + 0.1 * j,
                                  a1=0.03 + 0.006 * j) for j in range(n)]


def _missing(Y, rows):
    Y = Y.copy()
    Y[list(rows), 0] = np.nan
    return Y


def test_one_mode_is_the_extended_kalman_filter_bit_for_bit(host):
    """1. M = 1, P = [[1]], mu = [1]: x, xt, R, Rt, ll_steps and ll are ekf_host_run's bits — LG (3, 2, 1), the quad-tank across the switch
    time and the pendulum, with missing rows, three filters each"""
    rng = np.random.default_rng(1)
    lg = [kc.random_system(rng, 3, 2, 1, k, D=False)[0] for k in range(3)]
    Ul, Yl = kc._data(rng, 80, 1, 2, missing=(5, 6, 40))
    Uq, Yq = M.quadtank_data(80)
    Up, Yp = uc.pendulum_data(80)
    for what, models, kind, U, Y, t0 in (("LG", lg, ec.KIND_LG, Ul, Yl, 0.0), ("quad-tank", _quadtank_modes(3), ec.KIND_QUADTANK, Uq, _missing(Yq, (3, 50, 51)), 460.0),
                                         ("pendulum", _pendulum_modes(3), ec.KIND_PENDULUM, Up, _missing(Yp, (0, 33)), 1.0)):
        imms = [ic.imm([m], P=[[1.0]], mu0=[1.0]) for m in models]
        h, (mu, xm, Rm) = ic.host_run(host, imms, U, Y, 80, t_index0=t0, kind=kind)
        e, (x, R) = ec.host_run(host, models, U, Y, 80, t_index0=t0, kind=kind)
        for k in ("x", "xt", "R", "Rt", "ll_steps", "ll"):
            assert kc.bits_equal(h[k], e[k]), (what, k)
        assert kc.bits_equal(h["ll_modes"][:, :, 0], e["ll_steps"]) and np.all(h["mu"] == 1.0) and np.all(mu == 1.0), what
        assert kc.bits_equal(xm[:, 0], x) and kc.bits_equal(Rm[:, 0], R), (what, "final state")
        assert np.isfinite(h["ll"]).all(), what


def test_linear_modes_agree_with_the_kalman_imm(host):
    """2. LG modes, M = 3, (3, 2, 1), T = 100: every output of the twin against imm_host_run (the Kalman IMM, D = 0) at the bar
    tests/test_ekf.py test 1 holds the EKF to against the Kalman header (1e-10 relative, kalman_common.close)"""
    rng = np.random.default_rng(2)
    imms = ic.lg_imms(rng, 2, 3, 3, 2, 1)
    U, Y = kc.simulate(rng, kc.matrices(imms[0]["models"][0], np.zeros((2, 1))), 100, missing=(7, 8, 60))
    for interact in (True, False):
        h, st = ic.host_run(host, imms, U, Y, 100, interact=interact)
        k_, stk = ic.host_run(host, ic.as_kalman(imms), U, Y, 100, interact=interact)
        for k in ic.OUTS:
            assert kc.close(h[k], k_[k]), (interact, k)
        assert np.all(np.abs(h["ll"] - k_["ll"]) <= 1e-10 * np.abs(k_["ll"])), interact
        for a, b in zip(st, stk):
            assert kc.close(a, b), (interact, "final state")
        assert np.all(h["ll_steps"][[7, 8, 60]] == 0.0) and np.all(h["ll_modes"][[7, 8, 60]] == 0.0)
        assert np.all(np.abs(h["mu"].sum(axis=2) - 1.0) <= 1e-12)


def _measured(host, imm, kind, mode_of, U, Y, t0, what):
    """the twin against the restatement with the bar of test_ekf.py::_measured: the restatement's own float64-against-long-double error
    is measured in the same run; the bar per output is 1e-10 where ten times that error is below it, otherwise ten times that error"""
    Ts = imm["models"][0].Ts
    a = ic.numpy_imm([mode_of(m) for m in imm["models"]], imm["P"], imm["mu0"], U, Y, Ts, t0)
    b = ic.numpy_imm([mode_of(m, np.longdouble) for m in imm["models"]], imm["P"], imm["mu0"], U, Y, Ts, t0, lin=uc.LinLong)
    own = {k: uc.rel_err(a[k], b[k]) for k in ic.OUTS + ("ll",)}
    got, _ = ic.host_run(host, [imm], U, Y, Y.shape[0], t_index0=t0, kind=kind)
    assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), what
    err = {k: uc.rel_err(got[k][:, 0], a[k]) for k in ic.OUTS}
    err["ll"] = uc.rel_err(got["ll"][0], a["ll"])
    print(what, "ll %.6f" % got["ll"][0], "restatement float64 vs long double:", {k: "%.2e" % v for k, v in own.items()})
    print(what, "twin vs restatement:", {k: "%.2e" % v for k, v in err.items()})
    for k in err:
        bar = 1e-10 if 10.0 * own[k] <= 1e-10 else 10.0 * own[k]
        assert err[k] <= bar, (what, k, err[k], bar)
    return got


def test_twin_equals_the_formulas_on_pendulum_modes(host):
    """3a. M = 3 pendulum modes that differ in qt[0] (g / l), qt[1] (damping) and R1, T = 300 with missing rows.
    Measured in this test (relative, ukf_common.rel_err): restatement float64 against long double ll_steps 4.7e-14, x 5.2e-16, xt 5.0e-16,
    R 1.7e-15, Rt 1.7e-15, mu 3.9e-15, ll_modes 2.0e-14, ll 9.2e-17; twin against restatement ll_steps 8.2e-14, x 1.4e-15, xt 1.3e-15,
    R 2.4e-15, Rt 2.5e-15, mu 7.0e-15, ll_modes 4.4e-14, ll 3.0e-16: the bar is 1e-10 for every output.  It is always derived from the run
    at hand, never from these."""
    rng = np.random.default_rng(3)
    U, Y = uc.pendulum_data(300)
    imm = ic.imm(_pendulum_modes(3, r1=True), rng=rng)
    got = _measured(host, imm, ec.KIND_PENDULUM, ic.pendulum_mode, U, _missing(Y, (3, 150, 298)), 0.0, "pendulum modes")
    assert np.all(np.abs(got["mu"].sum(axis=2) - 1.0) <= 1e-12)


def test_twin_equals_the_formulas_on_quadtank_modes(host):
    """3b. M = 2 quad-tank modes that differ in gamma1 and a1, T = 200 from t_index0 = 400 (tau crosses the switch time 500), missing rows.
    Measured in this test: restatement float64 against long double ll_steps 2.3e-15, x 1.1e-15, xt 1.1e-15, R 2.8e-15, Rt 2.9e-15,
    mu 5.3e-16, ll_modes 2.1e-15, ll 1.6e-17; twin against restatement ll_steps 2.7e-15, x 1.3e-15, xt 1.3e-15, R 9.0e-16, Rt 1.0e-15,
    mu 6.7e-16, ll_modes 2.9e-15, ll 3.3e-16: the bar is 1e-10 for every output, derived from the run at hand."""
    rng = np.random.default_rng(4)
    U, Y = M.quadtank_data(200)
    imm = ic.imm(_quadtank_modes(2), rng=rng)
    _measured(host, imm, ec.KIND_QUADTANK, ic.quadtank_mode, U, _missing(Y, (5, 99, 100)), 400.0, "quad-tank modes")


def test_known_answer_of_two_linearised_modes(host):
    """4. M = 2, nx = ny = 1, g(x) = x^2, one step: mu_j proportional to c_j N(y; m_j^2, 4 m_j^2 P_j + r2) with c_j = sum_i P_ij mu_i, and
    ll the log of the normaliser, by hand, to 1e-13 relative"""
    ms, Ps, r2, y = (1.7, 1.2), (0.36, 0.5), 0.25, 3.0
    Pt, mu0 = np.array([[0.9, 0.1], [0.3, 0.7]]), np.array([0.6, 0.4])
    imm = ic.imm([ec.square_model(ms[j], Ps[j], r2) for j in range(2)], P=Pt, mu0=mu0)
    got, _ = ic.host_run(host, [imm], None, np.array([[y]]), 1, kind=ec.KIND_SQUARE)
    c = [Pt[0, j] * mu0[0] + Pt[1, j] * mu0[1] for j in range(2)]
    Sj = [4 * ms[j] * ms[j] * Ps[j] + r2 for j in range(2)]
    Nj = [math.exp(-0.5 * (y - ms[j] ** 2) ** 2 / Sj[j]) / math.sqrt(2 * math.pi * Sj[j]) for j in range(2)]
    z = c[0] * Nj[0] + c[1] * Nj[1]
    for j in range(2):
        assert abs(got["mu"][0, 0, j] - c[j] * Nj[j] / z) <= 1e-13 * (c[j] * Nj[j] / z), j
        assert abs(got["ll_modes"][0, 0, j] - math.log(Nj[j])) <= 1e-13 * abs(math.log(Nj[j])), j
    assert abs(got["ll_steps"][0, 0] - math.log(z)) <= 1e-13 * abs(math.log(z)) and got["ll"][0] == got["ll_steps"][0, 0]
    # the combined prior is the mixture of the two priors
    xbar = mu0[0] * ms[0] + mu0[1] * ms[1]
    Rbar = sum(mu0[j] * (Ps[j] + (ms[j] - xbar) ** 2) for j in range(2))
    assert abs(got["x"][0, 0, 0] - xbar) <= 1e-13 * xbar and abs(got["R"][0, 0, 0, 0] - Rbar) <= 1e-13 * Rbar


SWITCH_GL, SWITCH_EVERY = (9.81, 2.5), 150


def _switching_pendulum(T, seed=11):
    """data from a pendulum whose g / l switches between the two values of SWITCH_GL every SWITCH_EVERY steps; the true mode per step"""
    ms = []
    for gl in SWITCH_GL:
        m = uc.pendulum_model()
        m.qt[0] = gl
        ms.append(m)
    fg = [uc.pendulum_fg(m) for m in ms]
    rng = np.random.default_rng(seed)
    U = 0.5 * np.sin(0.1 * np.arange(T)).reshape(T, 1)
    Y, mode = np.zeros((T, 1)), np.zeros(T, dtype=int)
    x = np.array([1.0, 0.0])
    for k in range(T):
        mode[k] = (k // SWITCH_EVERY) % 2
        f, g = fg[mode[k]]
        Y[k] = g(x, U[k], 0.0) + 0.05 * rng.standard_normal()
        x = f(x, U[k], 0.0) + np.sqrt(np.array([1e-4, 4e-3])) * rng.standard_normal(2)
    return ms, U, Y, mode


def test_switching_data_prefers_the_imm_and_the_true_mode(host):
    """5. sanity, not a tolerance: on T = 600 steps simulated from a pendulum whose g_over_l switches between 9.81 and 2.5 every 150
    steps (noise as ukf_common.pendulum_data, seed 11) the two-mode IMM's ll exceeds the ll of each single-mode EKF, and its mean
    posterior probability of the true mode exceeds 1/2.  Measured on the twin: ll IMM 763.2, EKF(9.81) -3531.9, EKF(2.5) -24.1; mean
    posterior probability of the true mode 0.839."""
    ms, U, Y, mode = _switching_pendulum(600)
    imm = ic.imm(ms, P=[[0.98, 0.02], [0.02, 0.98]], mu0=[0.5, 0.5])
    got, _ = ic.host_run(host, [imm], U, Y, 600, kind=ec.KIND_PENDULUM)
    single = [ec.host_run(host, [m], U, Y, 600, kind=ec.KIND_PENDULUM)[0]["ll"][0] for m in ms]
    p_true = float(np.mean(got["mu"][np.arange(600), 0, mode]))
    print("switching pendulum: ll IMM %.3f, EKF(g/l = %.2f) %.3f, EKF(g/l = %.2f) %.3f; mean posterior probability of the true mode %.4f"
          % (got["ll"][0], SWITCH_GL[0], single[0], SWITCH_GL[1], single[1], p_true))
    assert np.isfinite(got["ll"][0]) and got["ll"][0] > single[0] and got["ll"][0] > single[1]
    assert p_true > 0.5


def test_header_binding_and_julia_wrapper_name_the_new_export():
    """6. llpf_imm_bank_run_at in the header, the library and _capi.SYMBOLS with eight arguments; LLPF_IMM_EXTENDED in the header; the
    Julia ccall has the prototype's arity"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    proto = re.search(r"\bllpf_imm_bank_run_at\s*\(([^)]*)\)", hdr)
    assert proto and len(proto.group(1).split(",")) == 8, proto
    assert "double t_index0" in proto.group(1)
    assert len(_capi.SYMBOLS["llpf_imm_bank_run_at"]) == 8 and _capi.SYMBOLS["llpf_imm_bank_run_at"][5] is C.c_double
    assert hasattr(_capi.lib(), "llpf_imm_bank_run_at")
    assert re.search(r"^#define\s+LLPF_IMM_EXTENDED\s+2\s*$", hdr, re.M) and _capi.IMM_EXTENDED == 2
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    call = re.search(r"ccall\(\(:llpf_imm_bank_run_at, LIB\), Cint, \(([^)]*)\)", jl)
    assert call and [s.strip() for s in call.group(1).split(",")] == ["Ptr{Cvoid}", "Ptr{Float64}", "Ptr{Float64}", "Int64", "Int32", "Float64",
                                                                      "Ptr{Float64}", "Ptr{CImmOutputs}"]


def _create(imms, flags=3, D=None):
    models, _, P, mu0 = ic.bank_args(imms)
    flat = [m for row in models for m in row]
    arr = (S.Model * len(flat))(*flat)
    P, mu0 = _capi.f64(P), _capi.f64(mu0)
    h = C.c_void_p()
    L = _capi.lib()
    rc = L.llpf_imm_bank_create(0, arr, _capi.dptr(None if D is None else _capi.f64(D)), _capi.dptr(P), _capi.dptr(mu0), len(models), len(models[0]),
                                flags, C.byref(h))
    assert not h.value or rc == _capi.OK
    if h.value:
        L.llpf_imm_bank_destroy(h)
    return rc, L.llpf_last_error().decode()


def test_what_cannot_run_is_refused_before_a_device_is_looked_for(monkeypatch):
    """7. LLPF_ERR_ARG with a message naming filter and mode where there is one; a valid extended spec gets as far as asking for a device"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    rng = np.random.default_rng(7)
    # mixed model ids among the modes
    imms = ic.grouped(_pendulum_modes(4), rng, 2, 2)
    pid = _capi.model_compile(ec.PENDULUM_JAC_SRC + "\n// test_imm_ekf\n", 2, 1)
    mixed = ic.with_id(imms, pid)
    mixed[1]["models"][1] = imms[1]["models"][1]              # (the linear-Gaussian id)
    rc, msg = _create(mixed)
    assert rc == _capi.ERR_ARG and "filter 1, mode 1" in msg and "model_id" in msg, (rc, msg)
    # ... and a Kalman bank (no flag) still refuses a mode that is not linear-Gaussian, by filter and mode
    back = ic.with_id(imms, pid)
    back[0]["models"][0] = imms[0]["models"][0]
    rc, msg = _create(back, flags=1)
    assert rc == _capi.ERR_ARG and "filter 0, mode 1" in msg, (rc, msg)
    # dimensions
    odd = ic.lg_imms(rng, 2, 2, 3, 2, 1)
    odd[1]["models"][0] = kc.random_system(rng, 3, 1, 1, D=False)[0]
    rc, msg = _create(odd)
    assert rc == _capi.ERR_ARG and "filter 1, mode 0" in msg and "dimensions" in msg, (rc, msg)
    # the checks of llpf_ekf_bank_create: one Jacobian member only; a member `initial`
    for src, word in ((ec.SQUARE_DYN_JAC_ONLY_SRC, "measurement_jac"), (ec.SQUARE_JAC_INITIAL_SRC, "initial")):
        mid = _capi.model_compile(src + "\n// test_imm_ekf\n", 1, 1)
        sq = ic.with_id(ic.grouped([ec.square_model(1.0 + 0.1 * k, 0.3) for k in range(4)], rng, 2, 2), mid)
        for flags in (1, 3):                                     # the flag is implied by the model id
            rc, msg = _create(sq, flags=flags)
            assert rc == _capi.ERR_ARG and word in msg and msg.startswith("imm"), (word, flags, rc, msg)
    rb = ic.with_id(ic.lg_imms(rng, 1, 2, 2, 1, 1), S.MODEL_RB_LINEAR)
    rc, msg = _create(rb)
    assert rc == _capi.ERR_ARG and "Rao-Blackwellized" in msg, (rc, msg)
    # per mode: a density that is not positive definite
    bad = ic.lg_imms(rng, 2, 2, 2, 1, 1)
    bad[1]["models"][1].measurement_density = S.make_gaussian(np.zeros(1), -1.0)
    rc, msg = _create(bad)
    assert rc == _capi.ERR_ARG and "filter 1, mode 1" in msg and "R2" in msg, (rc, msg)
    # D with the flag; flags with bit 2; P that is not stochastic
    lg = ic.lg_imms(rng, 2, 3, 2, 1, 1)
    rc, msg = _create(lg, D=np.zeros((2, 3, 1, 1)))
    assert rc == _capi.ERR_ARG and "D must be NULL" in msg, (rc, msg)
    rc, msg = _create(lg, flags=4 | 3)
    assert rc == _capi.ERR_ARG and "flags" in msg, (rc, msg)
    rc, msg = _create(lg, flags=4)
    assert rc == _capi.ERR_ARG and "flags" in msg, (rc, msg)
    worse = [dict(s) for s in lg]
    worse[1]["P"] = lg[1]["P"] + 1e-9
    rc, msg = _create(worse)
    assert rc == _capi.ERR_ARG and "filter 1" in msg and "row 0" in msg, (rc, msg)
    # a time that is not finite, before the handle is looked at
    L = _capi.lib()
    for t0 in (math.nan, math.inf):
        assert L.llpf_imm_bank_run_at(None, None, None, 1, 0, t0, None, None) == _capi.ERR_ARG
        assert "t_index0" in L.llpf_last_error().decode()
    assert L.llpf_imm_bank_run_at(None, None, None, 1, 0, 0.0, None, None) == _capi.ERR_ARG and "handle" in L.llpf_last_error().decode()
    # valid: linear-Gaussian with the flag, the quad-tank with and without it, a snippet with both members
    ok = _capi.OK if _capi.device_count() > 0 else _capi.ERR_NO_DEVICE
    for spec, flags in ((lg, 3), (lg, 2), (ic.grouped(_quadtank_modes(6), rng, 2, 3), 1), (ic.grouped(_quadtank_modes(6), rng, 2, 3), 3),
                        (ic.with_id(imms, pid), 1)):
        rc, msg = _create(spec, flags=flags)
        assert rc == ok, (flags, rc, msg)


def test_python_classes_refuse_what_is_not_one_model():
    """7. IMM(models, P, mu) over ExtendedKalmanFilter: one model, no iterated or other filter types; a list of KalmanFilter is as it was"""
    d2 = llpf_amd.MvNormal(np.zeros(2), np.eye(2))
    lin = lambda n: llpf_amd.ExtendedKalmanFilter(llpf_amd.LinearDynamics(0.9 * np.eye(n), np.zeros((n, 1))), llpf_amd.LinearMeasurement(np.eye(1, n)),
                                                  0.1, 0.1, llpf_amd.MvNormal(np.zeros(n), np.eye(n)))
    qt = lambda g1: llpf_amd.ExtendedKalmanFilter(llpf_amd.QuadTankDynamics(supersample=2, gamma1=g1), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1),
                                                  np.full(2, 1e-4), llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    P, mu = [[0.9, 0.1], [0.1, 0.9]], [0.5, 0.5]
    imm = llpf_amd.IMM([qt(0.2), qt(0.3)], P, mu)
    assert imm.extended and imm._handle is None and imm.nx == 4
    models, D, _, _ = imm._spec()
    assert D is None and [m.model_id for m in models] == [S.MODEL_QUADTANK_RK4] * 2
    with pytest.raises(TypeError, match="mode 1"):
        llpf_amd.IMM([qt(0.2), lin(4)], P, mu)                   # another model id
    with pytest.raises(TypeError, match="mode 1"):
        llpf_amd.IMM([lin(2), lin(3)], P, mu)                    # other dimensions
    it = llpf_amd.IteratedExtendedKalmanFilter(llpf_amd.LinearDynamics(0.9 * np.eye(2), np.zeros((2, 1))), llpf_amd.LinearMeasurement(np.eye(1, 2)), 0.1, 0.1, d2)
    with pytest.raises(TypeError, match="mode 1.*IteratedExtendedKalmanFilter"):
        llpf_amd.IMM([lin(2), it], P, mu)
    uk = llpf_amd.UnscentedKalmanFilter(llpf_amd.LinearDynamics(0.9 * np.eye(2), np.zeros((2, 1))), llpf_amd.LinearMeasurement(np.eye(1, 2)), 0.1, 0.1, d2)
    with pytest.raises(TypeError, match="mode 0.*UnscentedKalmanFilter"):
        llpf_amd.IMM([uk, lin(2)], P, mu)
    kf = llpf_amd.KalmanFilter(0.9 * np.eye(2), np.zeros((2, 1)), np.eye(1, 2), None, 0.1 * np.eye(2), 0.1 * np.eye(1), d2)
    with pytest.raises(TypeError, match="mode 1"):
        llpf_amd.IMM([kf, lin(2)], P, mu)
    with pytest.raises(TypeError, match="mode 1.*KalmanFilter"):
        llpf_amd.IMM([lin(2), kf], P, mu)
    with pytest.raises(TypeError):
        llpf_amd.IMM([], P, mu)
    plain = llpf_amd.IMM([kf, kf], P, mu)
    assert not plain.extended and plain._spec()[1].shape == (2, 1, 1)
    with pytest.raises(TypeError, match="filter 1"):
        llpf_amd.IMMBank._pack([plain, imm])
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(imm, np.zeros((3, 2)), np.zeros((3, 2)))
    assert imm._handle is None
