"""The unscented Rauch-Tung-Striebel smoother of the unscented bank (llpf_ukf_smooth_finish, llpf_ukf_bank_smooth), the checks that need no
GPU: the host build of the header's backward step (tests/ukf_host.c) — the definition the device reproduces bit for bit
(tests/test_gpu_ukf_smooth.py) — is the RTS smoother on linear models, the conditional law of the joint Gaussian, and the textbook
formulas (ukf_smooth_common.numpy_ukf_smooth) on nonlinear ones; the ABI is declared, exported, bound, guarded and mirrored in Julia;
arguments are refused before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import kalman_common as kc
import kalman_smooth_common as ks
import models as M
import ukf_common as uc
import ukf_smooth_common as us
import test_ukf as tu

ROOT = kc.ROOT
NAME = "llpf_ukf_bank_smooth"
SM = ("xT", "RT")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return uc.build_host(tmp_path_factory.mktemp("ukf_host"))


@pytest.fixture(scope="module")
def hsmooth(tmp_path_factory):
    return us.build_host_smooth(tmp_path_factory.mktemp("ukf_smooth_host"))


@pytest.fixture(scope="module")
def kalman_host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kf_host"))


@pytest.fixture(scope="module")
def kalman_hsmooth(tmp_path_factory):
    return ks.build_host_smooth(tmp_path_factory.mktemp("kf_smooth_host"))


@pytest.fixture(scope="module")
def systems():
    return tu.linear_systems()


def test_linear_model_is_the_rts_smoother(host, hsmooth, kalman_host, kalman_hsmooth, systems):
    """1. On a linear model the unscented transform is exact, so the unscented smoother is the Rauch-Tung-Striebel smoother: on the 32
    systems of test_ukf.linear_systems() and the three alpha = 1 weight sets, the host smoother over the host unscented forward outputs
    equals the reference's literal formulas over the reference's forward pass (ks.numpy_smooth over kc.numpy_reference) and the host build
    of llpf_kf_smooth over the Kalman header's forward pass, to the project's 1e-10.  Worst relative error against the numpy reference
    measured here: 1.8e-14 (xT), 1.3e-14 (RT)."""
    worst = {k: 0.0 for k in SM}
    for m, D, mats, U, Y in systems:
        ref = kc.numpy_reference(mats, U, Y)
        rx, rR = ks.numpy_smooth(mats, ref["x"], ref["xt"], ref["R"], ref["Rt"])
        kf, _ = kc.host_run(kalman_host, [(m, D)], U, Y, tu.T_LIN)
        kh = ks.host_smooth(kalman_hsmooth, [(m, D)], U, kf, tu.T_LIN)
        for abk in uc.ALPHA1_SETS:
            w = uc.merwe_set(m.nx, abk)
            fw, _ = uc.host_run(host, [m], w, U, Y, tu.T_LIN)
            got = us.host_smooth(hsmooth, [m], w, U, fw, tu.T_LIN)
            assert not np.isnan(got["xT"]).any() and not np.isnan(got["RT"]).any(), (m.nx, m.ny, abk)
            for k, r in (("xT", rx), ("RT", rR)):
                worst[k] = max(worst[k], uc.rel_err(got[k][:, 0], r))
                assert kc.close(got[k][:, 0], r), (m.nx, m.ny, abk, k, "numpy reference")
                assert kc.close(got[k][:, 0], kh[k][:, 0]), (m.nx, m.ny, abk, k, "Kalman header")
            assert np.array_equal(got["RT"], np.swapaxes(got["RT"], -1, -2))
    print("linear => RTS: worst relative error against the numpy reference", {k: "%.2e" % v for k, v in worst.items()})


def test_host_smoother_is_the_conditional_law_of_the_joint_gaussian(host, hsmooth):
    """2. nx <= 3, T = 30, one missing row: E[x_t | y_1..y_T] and Cov[x_t | y_1..y_T] of the dense joint Gaussian
    (ks.joint_smoother), an oracle that shares nothing with the recursion, to 1e-8 relative as in test_kalman_smooth.py"""
    rng = np.random.default_rng(31)
    T = 30
    for nx in (1, 2, 3):
        for ny in (1, 2, 3):
            for kind in range(3):
                nu = int(rng.integers(0, 3))
                m, D = kc.random_system(rng, nx, ny, nu, kind, D=False)
                mats = kc.matrices(m, D)
                U, Y = kc.simulate(rng, mats, T, missing=(11,))
                jx, jR = ks.joint_smoother(mats, U, Y)
                for abk in uc.ALPHA1_SETS:
                    w = uc.merwe_set(nx, abk)
                    fw, _ = uc.host_run(host, [m], w, U, Y, T)
                    h = us.host_smooth(hsmooth, [m], w, U, fw, T)
                    assert kc.close(h["xT"][:, 0], jx, 1e-8), (nx, ny, kind, abk)
                    assert kc.close(h["RT"][:, 0], jR, 1e-8), (nx, ny, kind, abk)


def _measured(f64, fl, R1, w, U, xt, Rt, Ts, t0):
    """the float64 restatement, and its worst error against the same code in long double over the same posteriors, per output"""
    a = us.numpy_ukf_smooth(f64, R1, w, U, xt, Rt, Ts, t0)
    b = us.numpy_ukf_smooth(fl, R1, w, U, xt, Rt, Ts, t0, lin=uc.LinLong)
    return a, {k: uc.rel_err(a[i], b[i]) for i, k in enumerate(SM)}


def _nonlinear(host, hsmooth, m, U, Y, f, f64, fl, twin, t0, what):
    """header vs restatement over the header's own forward outputs for the four weight sets: 1e-10 for the alpha = 1 sets; for the
    small-alpha one 10 x the restatement's float64-vs-long-double error of the same run, per output.  No output may be NaN."""
    R1 = S.gaussian_cov_matrix(m.dynamics_density)
    T = Y.shape[0]
    for abk, w in tu._weight_sets(m.nx):
        fw, _ = uc.host_run(host, [m], w, U, Y, T, t_index0=t0, twin=twin)
        got = us.host_smooth(hsmooth, [m], w, U, fw, T, t_index0=t0, twin=twin)
        assert not np.isnan(got["xT"]).any() and not np.isnan(got["RT"]).any(), (what, abk)
        xt, Rt = fw["xt"][:, 0], fw["Rt"][:, 0]
        ref = us.numpy_ukf_smooth(f, R1, w, U, xt, Rt, m.Ts, t0)
        err = {k: uc.rel_err(got[k][:, 0], ref[i]) for i, k in enumerate(SM)}
        _, own = _measured(f64, fl, R1, w, U, xt, Rt, m.Ts, t0)
        print(what, abk, "header vs restatement:", {k: "%.2e" % v for k, v in err.items()},
              "restatement float64 vs long double:", {k: "%.2e" % v for k, v in own.items()})
        if abk[0] == 1.0:
            for i, k in enumerate(SM):
                assert kc.close(got[k][:, 0], ref[i]), (what, abk, k, err[k])
        else:
            for k in SM:
                assert err[k] <= 10.0 * own[k], (what, abk, k, err[k], 10.0 * own[k])


def test_header_equals_the_formulas_on_the_quadtank(host, hsmooth):
    """3a / 4. The quad-tank on models.quadtank_data(1000) with three missing rows, across tau = TSWITCH, t_index0 = 1: the header
    around the oracle's RK4 against the restatement driving the Python QuadTankDynamics callable, over the header's forward outputs.
    Measured first, as the issue asks (the quad-tank's own error was not known): the restatement in float64 against the same code in long
    double over the same posteriors is at most 1.7e-15 (xT) and 3.6e-15 (RT) for the alpha = 1 sets, so ten times it is far below 1e-10 and
    the 1e-10 bar stands; header against restatement 1.4e-15 / 2.4e-15.  Merwe (1e-3, 2, 0): restatement 1.1e-9 (xT), 1.3e-11 (RT); header
    against restatement 7.3e-10, 1.2e-11.  The small-alpha bar is always the value of the run at hand (printed with -s), never these."""
    m, U, Y = tu._quadtank_case()
    dyn = llpf_amd.QuadTankDynamics(supersample=2)
    f = lambda x, u, tau: dyn(x, u, None, tau, m.Ts)
    _nonlinear(host, hsmooth, m, U, Y, f, uc.quadtank_fg(m)[0], uc.quadtank_fg(m, np.longdouble)[0], 0, 1.0, "quad-tank")


def test_header_equals_the_formulas_on_the_pendulum(host, hsmooth):
    """3b / 4. The pendulum of tests/user_models.py through its C twin against the restatement with np.sin, T = 1000, three missing rows.
    Recorded from this test: alpha = 1 sets, restatement float64 against long double at most 7.2e-16 (xT), 7.1e-15 (RT), header against
    restatement 7.1e-16, 5.7e-15.  Merwe (1e-3, 2, 0): restatement 6.1e-10 (xT), 5.7e-11 (RT); header against restatement 7.7e-10,
    6.2e-11.  The small-alpha bar is always the value of the run at hand (printed with -s), never these."""
    m = uc.pendulum_model()
    U, Y = uc.pendulum_data(1000)
    Y = Y.copy()
    for t in (3, 500, 998):
        Y[t, 0] = np.nan
    f = uc.pendulum_fg(m)[0]
    _nonlinear(host, hsmooth, m, U, Y, f, f, uc.pendulum_fg(m, np.longdouble)[0], uc.TWIN_PENDULUM, 0.0, "pendulum")


def test_small_alpha_weights_hold_to_the_measured_rounding_error(host, hsmooth, systems):
    """4. Merwe (1e-3, 2, 0) on the 32 linear systems: weights of order +-1e6 cancel, so no bar is fixed in advance (test_ukf.py's method).
    The float64 restatement is run against the long-double one over the same forward outputs (the header's xt, Rt), and
    header-vs-restatement is held to 10 x the worst value per output: two independent float64 evaluations may each be off by it in
    opposite directions.
    Recorded from this test (worst of the 32 systems): restatement float64 against long double xT 4.0e-9, RT 2.2e-12; header against
    restatement in the same run xT 6.4e-10, RT 1.6e-12.  The bar is always the value measured in the run at hand (printed with -s)."""
    w_of = lambda L: uc.merwe(L, *uc.SMALL_ALPHA)
    own = {k: 0.0 for k in SM}
    seen = {k: 0.0 for k in SM}
    for m, D, mats, U, Y in systems:
        w = w_of(m.nx)
        fw, _ = uc.host_run(host, [m], w, U, Y, tu.T_LIN)
        got = us.host_smooth(hsmooth, [m], w, U, fw, tu.T_LIN)
        assert not np.isnan(got["xT"]).any() and not np.isnan(got["RT"]).any(), (m.nx, m.ny)
        ref, e = _measured(uc.linear_fg(mats)[0], uc.linear_fg(mats, np.longdouble)[0], mats["R1"], w, U, fw["xt"][:, 0], fw["Rt"][:, 0], 1.0, 0.0)
        for i, k in enumerate(SM):
            own[k] = max(own[k], e[k])
            seen[k] = max(seen[k], uc.rel_err(got[k][:, 0], ref[i]))
    print("small alpha, restatement float64 vs long double (worst of 32):", {k: "%.2e" % v for k, v in own.items()})
    print("small alpha, header vs restatement (worst of 32):", {k: "%.2e" % v for k, v in seen.items()})
    for k in SM:
        assert seen[k] <= 10.0 * own[k], (k, seen[k], 10.0 * own[k])


def _bank(rng, n=4):
    """n pendulums with different parameters and covariances, shared data"""
    models = []
    for k in range(n):
        m = uc.pendulum_model()
        m.qt[0], m.qt[1] = 9.81 * (1 + 0.1 * k), 0.05 * (1 + k)
        models.append(m)
    U, Y = uc.pendulum_data(60, seed=3)
    Y = Y.copy()
    Y[20, 0] = np.nan
    return models, U, Y


def test_the_last_step_is_the_posterior_and_healthy_filters_have_no_nan(host, hsmooth):
    """5a. xT[T-1], RT[T-1] are xt[T-1], Rt[T-1] bit for bit (T = 1 included); no output of a healthy filter is NaN; RT is symmetric."""
    models, U, Y = _bank(np.random.default_rng(0))
    for abk, w in tu._weight_sets(2):
        for T in (1, 2, 60):
            fw, _ = uc.host_run(host, models, w, U[:T], Y[:T], T, twin=uc.TWIN_PENDULUM)
            sm = us.host_smooth(hsmooth, models, w, U[:T], fw, T, twin=uc.TWIN_PENDULUM)
            assert kc.bits_equal(sm["xT"][-1], fw["xt"][-1]) and kc.bits_equal(sm["RT"][-1], fw["Rt"][-1]), (abk, T)
            assert not np.isnan(sm["xT"]).any() and not np.isnan(sm["RT"]).any(), (abk, T)
            assert np.array_equal(sm["RT"], np.swapaxes(sm["RT"], -1, -2))


def test_an_indefinite_filter_is_nan_only_in_its_own_outputs(host, hsmooth):
    """5b. A filter with an indefinite initial covariance is NaN in all of its own outputs, forward and smoothed; its neighbours are bit
    for bit what they are without it.  A posterior that loses definiteness at one step is NaN at that step and every earlier one only."""
    models, U, Y = _bank(np.random.default_rng(1))
    w = uc.merwe_set(2, uc.ALPHA1_SETS[0])
    T = 60
    x0 = np.stack([S.gaussian_mean(m.initial_density) for m in models])
    P0 = np.stack([S.gaussian_cov_matrix(m.initial_density) for m in models])
    ok_fw, _ = uc.host_run(host, models, w, U, Y, T, twin=uc.TWIN_PENDULUM, state=(x0, P0))
    ok = us.host_smooth(hsmooth, models, w, U, ok_fw, T, twin=uc.TWIN_PENDULUM)
    Pb = P0.copy()
    Pb[1] = np.array([[1.0, 2.0], [2.0, 1.0]])
    fw, _ = uc.host_run(host, models, w, U, Y, T, twin=uc.TWIN_PENDULUM, state=(x0, Pb))
    sm = us.host_smooth(hsmooth, models, w, U, fw, T, twin=uc.TWIN_PENDULUM)
    assert np.isnan(sm["xT"][:, 1]).all() and np.isnan(sm["RT"][:, 1]).all()
    assert np.isnan(fw["xt"][:, 1]).all() and np.isnan(fw["Rt"][:, 1]).all() and np.isnan(fw["ll"][1])
    for f in (0, 2, 3):
        for k in SM:
            assert kc.bits_equal(sm[k][:, f], ok[k][:, f]), (k, f)
    bad = {k: ok_fw[k].copy() for k in ("xt", "Rt")}
    bad["Rt"][30, 2] = -np.eye(2)
    sm = us.host_smooth(hsmooth, models, w, U, bad, T, twin=uc.TWIN_PENDULUM)
    assert np.isnan(sm["xT"][:31, 2]).all() and np.isnan(sm["RT"][:31, 2]).all()
    for k in SM:
        assert kc.bits_equal(sm[k][31:, 2], ok[k][31:, 2]), k
        for f in (0, 1, 3):
            assert kc.bits_equal(sm[k][:, f], ok[k][:, f]), (k, f)


def test_shared_against_per_filter_inputs(host, hsmooth):
    """5c. Shared U against the same rows given per filter, and every filter alone against its column of the bank: the same bits."""
    models, U, Y = _bank(np.random.default_rng(2))
    w = uc.merwe_set(2, uc.ALPHA1_SETS[1])
    T, F = 60, len(models)
    fw, _ = uc.host_run(host, models, w, U, Y, T, twin=uc.TWIN_PENDULUM, t_index0=1.0)
    shared = us.host_smooth(hsmooth, models, w, U, fw, T, twin=uc.TWIN_PENDULUM, t_index0=1.0)
    per = us.host_smooth(hsmooth, models, w, np.ascontiguousarray(np.broadcast_to(U, (F, T, 1))), fw, T, per_filter=1, twin=uc.TWIN_PENDULUM,
                         t_index0=1.0)
    for k in SM:
        assert kc.bits_equal(shared[k], per[k]), k
    for f, m in enumerate(models):
        one = us.host_smooth(hsmooth, [m], w, U, {"xt": fw["xt"][:, f:f + 1], "Rt": fw["Rt"][:, f:f + 1]}, T, twin=uc.TWIN_PENDULUM, t_index0=1.0)
        for k in SM:
            assert kc.bits_equal(one[k][:, 0], shared[k][:, f]), (k, f)


def test_the_symbol_is_declared_exported_bound_and_guarded():
    """6a."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "capi.hip")).read()
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, hdr, re.S)
    assert m and len(m.group(1).split(",")) == 9
    L = _capi.lib()
    assert hasattr(L, NAME) and len(_capi.SYMBOLS[NAME]) == 9
    assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % NAME, capi, re.M) and "LLPF_GUARD(%s)" % NAME in capi
    ma, mi = C.c_int32(), C.c_int32()
    L.llpf_version(C.byref(ma), C.byref(mi))
    assert (ma.value, mi.value) == (0, 7)
    # the fault-injection site of the call: ukf_smooth names it, kf_smooth (host/kfbank.hpp) reads it
    host = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "host")
    assert 'out, "ukf_smooth",' in open(os.path.join(host, "ukf.hpp")).read()
    assert "test_throw(site);\n    if (!w) return forward(nullptr);" in open(os.path.join(host, "kfbank.hpp")).read()


def test_julia_ccall_has_the_prototypes_arity():
    """6b."""
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    m = re.search(r"ccall\(\(:%s, LIB\),\s*\w+,\s*\((.*?)\),\s*" % NAME, jl, re.S)
    assert m
    depth, n, cur = 0, 0, ""
    for ch in m.group(1):
        depth += ch in "({"
        depth -= ch in ")}"
        if ch == "," and depth == 0:
            n, cur = n + 1, ""
        else:
            cur += ch
    assert n + (1 if cur.strip() else 0) == 9
    assert re.search(r"^function LowLevelParticleFilters\.smooth\(ukf::GPUUnscentedKalmanFilter, u, y, p = NullParameters\(\)\)", jl, re.M)
    assert re.search(r"^function smooth\(b::GPUUnscentedKalmanFilterBank, u, y\)", jl, re.M)
    assert re.search(r"^function ukf_smooth\(b::GPUUnscentedKalmanFilterBank, u, y; outputs = false, t_index0 = 0.0\)", jl, re.M)


def test_bad_arguments_are_refused_before_any_device_lookup():
    """6c. A null handle, and — on a handle — T < 1, stray per_filter bits, a non-finite t_index0 and a short struct_size: LLPF_ERR_ARG."""
    L = _capi.lib()
    out = S.KalmanSmoothOutputs()
    out.struct_size = C.sizeof(S.KalmanSmoothOutputs)
    y = np.zeros(8)
    yp = y.ctypes.data_as(C.POINTER(C.c_double))
    assert L.llpf_ukf_bank_smooth(None, None, yp, 4, 0, 0.0, None, None, C.byref(out)) == _capi.ERR_ARG
    assert b"null handle" in L.llpf_last_error()
    if _capi.device_count() < 1:
        return
    h = _capi.UkfBankHandle(0, [M.quadtank_model()], (1.0, 0.0, 2.0, 0.5))
    u = np.zeros(8)
    up = u.ctypes.data_as(C.POINTER(C.c_double))
    assert L.llpf_ukf_bank_smooth(h.h, up, yp, 0, 0, 0.0, None, None, C.byref(out)) == _capi.ERR_ARG
    assert L.llpf_ukf_bank_smooth(h.h, up, None, 4, 0, 0.0, None, None, C.byref(out)) == _capi.ERR_ARG
    assert L.llpf_ukf_bank_smooth(h.h, up, yp, 4, 4, 0.0, None, None, C.byref(out)) == _capi.ERR_ARG
    for t0 in (np.nan, np.inf):
        assert L.llpf_ukf_bank_smooth(h.h, up, yp, 4, 0, t0, None, None, C.byref(out)) == _capi.ERR_ARG
    small = S.KalmanSmoothOutputs()
    small.struct_size = 8
    assert L.llpf_ukf_bank_smooth(h.h, up, yp, 4, 0, 0.0, None, None, C.byref(small)) == _capi.ERR_ARG
    assert b"struct_size" in L.llpf_last_error()
    fsmall = S.KalmanOutputs()
    fsmall.struct_size = 8
    assert L.llpf_ukf_bank_smooth(h.h, up, yp, 4, 0, 0.0, None, C.byref(fsmall), C.byref(out)) == _capi.ERR_ARG
    h.close()


def test_unscented_smooth_dispatch_needs_the_device():
    """smooth(ukf, u, y) is the unscented smoother, not the particle smoother's argument unpacking"""
    ukf = llpf_amd.UnscentedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                         llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    U, Y = M.quadtank_data(5)
    if _capi.device_count() > 0:
        sol = llpf_amd.smooth(ukf, U, Y)
        assert isinstance(sol, llpf_amd.KalmanSmoothingSolution) and sol.xT.shape == (5, 4) and sol.RT.shape == (5, 4, 4)
    else:
        with pytest.raises(_capi.LLPFError) as ei:
            llpf_amd.smooth(ukf, U, Y)
        assert ei.value.code == _capi.ERR_NO_DEVICE
