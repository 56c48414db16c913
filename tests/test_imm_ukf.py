"""The IMM filter over unscented Kalman filter modes on the host (tests/imm_ukf_host.c, the build of csrc/shared/llpf_imm.h over
csrc/shared/llpf_ukf.h — the six stages of tests/kf_host_frame.h over the unscented family — that the device is held to in
test_gpu_imm_ukf.py): with one mode it is the unscented Kalman filter of tests/ukf_host.c bit for bit, on linear modes with weights for
which a linear map is exact it is the Kalman IMM of tests/imm_host.c, it is the textbook recursion (a numpy restatement in literal
formulas, float64 and long double), the C ABI and the Python classes refuse what they cannot run, and the run-time program of the
device kernel compiles for gfx950.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import imm_common as ic
import imm_ukf_common as iu
import kalman_common as kc
import models as M
import ukf_common as uc
import user_models as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRIVIAL = lambda nx: llpf_amd.TrivialParams().weights(nx)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return iu.build_host(tmp_path_factory.mktemp("imm_ukf_host"))


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


def test_one_mode_is_the_unscented_kalman_filter_bit_for_bit(host):
    """1. M = 1, P = [[1]], mu = [1]: ll_steps, x, xt, R, Rt (and ll, the final state) are ukf_host_run's bits — LG (2, 1, 1), the
    pendulum twin and the quad-tank across the switch time, T = 50 with a missing row, three filters each"""
    rng = np.random.default_rng(1)
    lg = [kc.random_system(rng, 2, 1, 1, k, D=False)[0] for k in range(3)]
    Ul, Yl = kc._data(rng, 50, 1, 1, missing=(17,))
    Uq, Yq = M.quadtank_data(50)
    Up, Yp = uc.pendulum_data(50)
    for what, models, twin, U, Y, t0, w in (("LG", lg, 0, Ul, Yl, 0.0, uc.merwe(2, 1.0, 0.0, 1.0)),
                                            ("pendulum", _pendulum_modes(3), uc.TWIN_PENDULUM, Up, _missing(Yp, (33,)), 1.0, TRIVIAL(2)),
                                            ("quad-tank", _quadtank_modes(3), 0, Uq, _missing(Yq, (20,)), 480.0, TRIVIAL(4))):
        imms = [ic.imm([m], P=[[1.0]], mu0=[1.0]) for m in models]
        h, (mu, xm, Rm) = iu.host_run(host, imms, w, U, Y, 50, t_index0=t0, twin=twin)
        e, (x, R) = uc.host_run(host, models, w, U, Y, 50, t_index0=t0, twin=twin)
        for k in ("ll_steps", "x", "xt", "R", "Rt", "ll"):
            assert kc.bits_equal(h[k], e[k]), (what, k)
        assert kc.bits_equal(h["ll_modes"][:, :, 0], e["ll_steps"]) and np.all(h["mu"] == 1.0) and np.all(mu == 1.0), what
        assert kc.bits_equal(xm[:, 0], x) and kc.bits_equal(Rm[:, 0], R), (what, "final state")
        assert np.isfinite(h["ll"]).all(), what


def test_linear_modes_agree_with_the_kalman_imm(host):
    """2. LG modes, M = 3, (3, 2, 1), T = 100, TrivialParams (sum wm = 1, wi gamma^2 = 1/2: a linear map is exact): every output of the
    twin against imm_host_run (the Kalman IMM, D = 0) at the project's bar for "unscented equals Kalman on a linear model", 1e-10
    relative (kalman_common.close).  The actual deviation is measured against the Kalman IMM restated in long double
    (imm_common.numpy_imm over linear modes) and printed.  Measured here (ukf_common.rel_err), interact on / off: ll_steps 7.6e-16 /
    1.1e-15, x 2.8e-15 / 3.9e-15, xt 4.3e-15 / 3.3e-15, R 2.6e-15 / 1.1e-15, Rt 3.1e-15 / 1.4e-15, mu 2.0e-15 / 1.6e-15, ll_modes
    1.5e-15 / 6.2e-16: every one more than 10^4 times below the bar."""
    rng = np.random.default_rng(2)
    imms = ic.lg_imms(rng, 2, 3, 3, 2, 1)
    U, Y = kc.simulate(rng, kc.matrices(imms[0]["models"][0], np.zeros((2, 1))), 100, missing=(7, 8, 60))
    w = TRIVIAL(3)
    for interact in (True, False):
        h, st = iu.host_run(host, imms, w, U, Y, 100, interact=interact)
        k_, stk = ic.host_run(host, ic.as_kalman(imms), U, Y, 100, interact=interact)
        for k in ic.OUTS:
            assert kc.close(h[k], k_[k]), (interact, k)
        assert np.all(np.abs(h["ll"] - k_["ll"]) <= 1e-10 * np.abs(k_["ll"])), interact
        for a, b in zip(st, stk):
            assert kc.close(a, b), (interact, "final state")
        assert np.all(h["ll_steps"][[7, 8, 60]] == 0.0) and np.all(h["ll_modes"][[7, 8, 60]] == 0.0)
        assert np.all(np.abs(h["mu"].sum(axis=2) - 1.0) <= 1e-12) and np.isfinite(h["ll"]).all()
        worst = {k: 0.0 for k in ic.OUTS}
        for f, s in enumerate(ic.as_kalman(imms)):
            ref = ic.numpy_imm([ic.linear_mode(m, D, np.longdouble) for m, D in ic.systems(s)], s["P"], s["mu0"], U, Y, interact=interact, lin=uc.LinLong)
            for k in ic.OUTS:
                worst[k] = max(worst[k], uc.rel_err(h[k][:, f], ref[k]))
        print("unscented IMM twin against the long-double Kalman IMM, interact", interact, {k: "%.2e" % v for k, v in worst.items()})


def test_the_twin_is_finite_on_the_precompiled_cases_of_the_gpu_test(host):
    """2b. the cases of test_gpu_imm_ukf.py's test a (imm_ukf_common.shape_case: the same seeds, the same order of draws), on the twin:
    ll is finite and mu a distribution for both weight sets, interact on and off, shared and per-filter inputs — what the GPU test then
    asserts of the device"""
    for nx, ny, nu in iu.SHAPES:
        for Mo in range(1, 5):
            for wi, w in enumerate(iu.shape_weights(nx)):
                imms, U, Y, Uf, Yf = iu.shape_case(nx, ny, nu, Mo, wi)
                for interact in (True, False):
                    h, _ = iu.host_run(host, imms, w, U, Y, iu.SHAPE_T, interact=interact)
                    hf, _ = iu.host_run(host, imms, w, Uf, Yf, iu.SHAPE_T, per_filter=3, interact=interact)
                    for g in (h, hf):
                        assert np.all(np.isfinite(g["ll"])), (nx, ny, nu, Mo, wi, interact)
                        assert np.all(g["mu"] >= 0.0) and np.all(np.abs(g["mu"].sum(axis=2) - 1.0) <= 1e-12), (nx, ny, nu, Mo, wi, interact)


# The bar of a restated output: MARGIN times the restatement's own float64-against-long-double error, measured in the same run.  The
# twin and the float64 restatement are two float64 evaluations of one quantity in different operation orders (packed triangles and fma
# against dense numpy), each off the long-double value by an error of that size: 2 would be the bar if both had exactly the measured
# one; 10 leaves room for the twin's other order.  ULPS: the floor under a measured error that comes out 0 or below one rounding.
MARGIN = 10.0
ULPS = 4.0 * np.finfo(np.float64).eps


def _measured(host, imm, w, twin, mode_of, U, Y, t0, what):
    """the twin against the restatement: the restatement's own float64-against-long-double error is measured in the same run; the bar per
    output is MARGIN times that error (at least ULPS)"""
    Ts = imm["models"][0].Ts
    a = iu.numpy_imm_ukf([mode_of(m) for m in imm["models"]], w, imm["P"], imm["mu0"], U, Y, Ts, t0)
    b = iu.numpy_imm_ukf([mode_of(m, np.longdouble) for m in imm["models"]], w, imm["P"], imm["mu0"], U, Y, Ts, t0, lin=uc.LinLong)
    own = {k: uc.rel_err(a[k], b[k]) for k in ic.OUTS + ("ll",)}
    got, _ = iu.host_run(host, [imm], w, U, Y, Y.shape[0], t_index0=t0, twin=twin)
    assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), what
    err = {k: uc.rel_err(got[k][:, 0], a[k]) for k in ic.OUTS}
    err["ll"] = uc.rel_err(got["ll"][0], a["ll"])
    print(what, "ll %.6f" % got["ll"][0], "restatement float64 vs long double:", {k: "%.2e" % v for k, v in own.items()})
    print(what, "twin vs restatement:", {k: "%.2e" % v for k, v in err.items()})
    for k in err:
        bar = max(MARGIN * own[k], ULPS)
        assert err[k] <= bar, (what, k, err[k], bar)
    return got


def test_twin_equals_the_formulas_on_pendulum_modes(host):
    """3a. M = 2 pendulum modes that differ in g / l, the damping and R1, T = 300 with missing rows, Merwe (1, 0, 1).
    Measured in this test (relative, ukf_common.rel_err): restatement float64 against long double ll_steps 7.3e-13, x 7.3e-16, xt 6.0e-16,
    R 3.7e-15, Rt 3.5e-15, mu 3.0e-15, ll_modes 2.5e-14, ll 1.5e-16; twin against restatement ll_steps 7.4e-13, x 1.6e-15, xt 1.2e-15,
    R 4.5e-15, Rt 3.5e-15, mu 5.5e-15, ll_modes 4.4e-14, ll 1.4e-16.  The bar of an output is MARGIN = 10 times its figure of the first
    set (ll_steps 7.3e-12, x 7.3e-15, ... ll 1.5e-15), always derived from the run at hand, never from these."""
    rng = np.random.default_rng(3)
    U, Y = uc.pendulum_data(300)
    imm = ic.imm(_pendulum_modes(2, r1=True), rng=rng)
    got = _measured(host, imm, uc.merwe(2, 1.0, 0.0, 1.0), uc.TWIN_PENDULUM, ic.pendulum_mode, U, _missing(Y, (3, 150, 298)), 0.0, "pendulum modes")
    assert np.all(np.abs(got["mu"].sum(axis=2) - 1.0) <= 1e-12)


def test_twin_equals_the_formulas_on_square_modes(host):
    """3b. M = 2 modes of f(x) = x, g(x) = x_0^2 (nx = 1) that differ in their prior, T = 60, TrivialParams.
    Measured in this test: restatement float64 against long double ll_steps 9.1e-16, x 1.6e-16, xt 1.6e-16, R 4.6e-16, Rt 2.5e-15,
    mu 9.8e-16, ll_modes 7.0e-16, ll 7.3e-17; twin against restatement ll_steps 1.4e-15, x 2.8e-16, xt 2.1e-16, R 6.9e-16, Rt 4.0e-15,
    mu 1.1e-15, ll_modes 7.1e-16, ll 0.  The bar of an output is MARGIN = 10 times its figure of the first set (x 1.6e-15, Rt 2.5e-14,
    ...; ll at the floor of 4 ulp, 8.9e-16), derived from the run at hand."""
    rng = np.random.default_rng(4)
    Y = 3.0 + 0.5 * rng.standard_normal((60, 1))
    imm = ic.imm([ec.square_model(1.7, 0.36, 0.25), ec.square_model(1.2, 0.5, 0.25)], rng=rng)
    _measured(host, imm, TRIVIAL(1), uc.TWIN_SQUARE, ic.square_mode, None, Y, 0.0, "x0^2 modes")


def _create(imms, w=(1.0, 0.0, 2.0, 0.5), flags=1, struct_size=None):
    """llpf_imm_bank_create_unscented over the IMMs: (status, message, handle or None — the caller destroys it)"""
    models, _, P, mu0 = ic.bank_args(imms)
    flat = [m for row in models for m in row]
    arr = (S.Model * len(flat))(*flat)
    P, mu0 = _capi.f64(P), _capi.f64(mu0)
    ws = _capi.ukf_weights(w)
    if struct_size is not None:
        ws.struct_size = struct_size
    h = C.c_void_p()
    L = _capi.lib()
    rc = L.llpf_imm_bank_create_unscented(0, arr, _capi.dptr(P), _capi.dptr(mu0), len(models), len(models[0]), flags, C.byref(ws), C.byref(h))
    msg = L.llpf_last_error().decode()
    assert not h.value or rc == _capi.OK
    return rc, msg, (h if h.value else None)


def _refused(imms, **kw):
    rc, msg, h = _create(imms, **kw)
    if h is not None:
        _capi.lib().llpf_imm_bank_destroy(h)
    return rc, msg


def test_what_cannot_run_is_refused_before_a_device_is_looked_for(monkeypatch):
    """4. LLPF_ERR_ARG with a message naming filter and mode where there is one; a valid spec gets as far as asking for a device"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    rng = np.random.default_rng(7)
    # a snippet with a member of its own: noise, loglik (nx = 2, ny = 1), initial (nx = 1)
    for src, word, nx in ((UM.LAPLACE_NOISE_SRC, "noise", 2), (UM.LAPLACE_SRC, "loglik", 2), (ec.SQUARE_JAC_INITIAL_SRC, "initial", 1)):
        mid = _capi.model_compile(src + "\n// test_imm_ukf\n", nx, 1)
        spec = ic.with_id(ic.lg_imms(rng, 2, 2, nx, 1, 1 if nx == 2 else 0), mid)
        rc, msg = _refused(spec)
        assert rc == _capi.ERR_ARG and word in msg and msg.startswith("imm"), (word, rc, msg)
    for rbid in (S.MODEL_RB_LINEAR, S.MODEL_RB_BILINEAR):
        rc, msg = _refused(ic.with_id(ic.lg_imms(rng, 1, 2, 2, 1, 1), rbid))
        assert rc == _capi.ERR_ARG and "Rao-Blackwellized" in msg and "unscented" in msg, (rc, msg)
    # the dimensions of a model id: the quad-tank has its own
    rc, msg = _refused(ic.with_id(ic.lg_imms(rng, 1, 2, 3, 2, 2), S.MODEL_QUADTANK_RK4))
    assert rc == _capi.ERR_ARG and "quad-tank" in msg, (rc, msg)
    # mixed model ids and mixed dimensions among the modes, by filter and mode
    imms = ic.grouped(_pendulum_modes(4), rng, 2, 2)
    pid = _capi.model_compile(UM.PENDULUM_SRC + "\n// test_imm_ukf\n", 2, 1)
    mixed = ic.with_id(imms, pid)
    mixed[1]["models"][1] = imms[1]["models"][1]              # (the linear-Gaussian id)
    rc, msg = _refused(mixed)
    assert rc == _capi.ERR_ARG and "filter 1, mode 1" in msg and "model_id" in msg, (rc, msg)
    odd = ic.lg_imms(rng, 2, 2, 3, 2, 1)
    odd[1]["models"][0] = kc.random_system(rng, 3, 1, 1, D=False)[0]
    rc, msg = _refused(odd)
    assert rc == _capi.ERR_ARG and "filter 1, mode 0" in msg and "dimensions" in msg, (rc, msg)
    # per mode: a density that is not positive definite
    bad = ic.lg_imms(rng, 2, 2, 2, 1, 1)
    bad[1]["models"][1].measurement_density = S.make_gaussian(np.zeros(1), -1.0)
    rc, msg = _refused(bad)
    assert rc == _capi.ERR_ARG and "filter 1, mode 1" in msg and "R2" in msg, (rc, msg)
    # the weights, as llpf_ukf_bank_create checks them
    lg = ic.lg_imms(rng, 2, 3, 2, 1, 1)
    for w in ((0.0, 0.0, 0.0, 0.5), (-1.0, 0.0, 0.0, 0.5), (np.nan, 0.0, 0.0, 0.5), (1.0, np.inf, 0.0, 0.5), (1.0, 0.0, np.nan, 0.5), (1.0, 0.0, 0.0, np.inf)):
        rc, msg = _refused(lg, w=w)
        assert rc == _capi.ERR_ARG and "ukf" in msg, (w, rc, msg)
    rc, msg = _refused(lg, struct_size=8)
    assert rc == _capi.ERR_ARG and "struct_size" in msg, (rc, msg)
    L = _capi.lib()
    models, _, P, mu0 = ic.bank_args(lg)
    flat = [m for row in models for m in row]
    h = C.c_void_p()
    assert L.llpf_imm_bank_create_unscented(0, (S.Model * 6)(*flat), _capi.dptr(_capi.f64(P)), _capi.dptr(_capi.f64(mu0)), 2, 3, 1, None,
                                            C.byref(h)) == _capi.ERR_ARG and "weights" in L.llpf_last_error().decode()
    # flags other than LLPF_IMM_INTERACT; P that is not stochastic
    for flags in (2, 3, 4, 5):
        rc, msg = _refused(lg, flags=flags)
        assert rc == _capi.ERR_ARG and "flags" in msg, (flags, rc, msg)
    worse = [dict(s) for s in lg]
    worse[1]["P"] = lg[1]["P"] + 1e-9
    rc, msg = _refused(worse)
    assert rc == _capi.ERR_ARG and "filter 1" in msg and "row 0" in msg, (rc, msg)
    # null arguments: the out pointer first, the handle first
    ws = _capi.ukf_weights((1.0, 0.0, 2.0, 0.5))
    assert L.llpf_imm_bank_create_unscented(0, None, None, None, 0, 0, 0, None, None) == _capi.ERR_ARG and "null out pointer" in L.llpf_last_error().decode()
    assert L.llpf_imm_bank_set_weights(None, C.byref(ws)) == _capi.ERR_ARG and "null handle" in L.llpf_last_error().decode()
    # valid: linear-Gaussian, the quad-tank, a snippet without Jacobian members — as far as asking for a device
    ok = _capi.OK if _capi.device_count() > 0 else _capi.ERR_NO_DEVICE
    for spec, flags in ((lg, 1), (lg, 0), (ic.grouped(_quadtank_modes(6), rng, 2, 3), 1), (ic.with_id(imms, pid), 1)):
        rc, msg = _refused(spec, flags=flags)
        assert rc == ok, (flags, rc, msg)
    # set_weights on a bank of Kalman modes (where a device exists)
    if _capi.device_count() > 0:
        kal = ic.bank(ic.as_kalman(lg))
        with pytest.raises(_capi.LLPFError) as ei:
            kal.set_weights((1.0, 0.0, 2.0, 0.5))
        assert ei.value.code == _capi.ERR_ARG and "unscented" in str(ei.value)
        ext = ic.bank(lg)
        with pytest.raises(_capi.LLPFError) as ei:
            ext.set_weights((1.0, 0.0, 2.0, 0.5))
        assert ei.value.code == _capi.ERR_ARG


def test_the_runtime_program_compiles_for_gfx950(monkeypatch):
    """5. under LLPF_JIT_COMPILE_ONLY=1 the creation of an unscented bank compiles k_imm_ukf with hiprtc before it asks for a device: a
    snippet without Jacobian members at M = 3 (G = 4, the mapped points a local array) and the linear-Gaussian model at 5 states and
    M = 4 (the first shape whose points are in LDS).  A compile error would be LLPF_ERR_HIP with the log."""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    rng = np.random.default_rng(8)
    ok = _capi.OK if _capi.device_count() > 0 else _capi.ERR_NO_DEVICE
    pid = _capi.model_compile(UM.PENDULUM_SRC + "\n// test_imm_ukf: compile\n", 2, 1)
    assert "dynamics_jac" not in UM.PENDULUM_SRC and "measurement_jac" not in UM.PENDULUM_SRC
    rc, msg = _refused(ic.with_id(ic.grouped(_pendulum_modes(3), rng, 1, 3), pid))
    assert rc == ok, (rc, msg)
    rc, msg = _refused(ic.lg_imms(rng, 2, 4, 5, 1, 0))
    assert rc == ok, (rc, msg)


def test_header_binding_and_julia_wrapper_name_the_new_exports():
    """6. llpf_imm_bank_create_unscented (nine arguments) and llpf_imm_bank_set_weights (two) in the header, the library and
    _capi.SYMBOLS; the Julia ccalls have the prototypes' arity"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    for name, n, jtypes in (("llpf_imm_bank_create_unscented", 9, ["Int32", "Ptr{CModel}", "Ptr{Float64}", "Ptr{Float64}", "Int32", "Int32", "Int32",
                                                                   "Ptr{CUkfWeights}", "Ref{Ptr{Cvoid}}"]),
                            ("llpf_imm_bank_set_weights", 2, ["Ptr{Cvoid}", "Ptr{CUkfWeights}"])):
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, hdr)
        assert proto and len(proto.group(1).split(",")) == n, (name, proto)
        assert "llpf_ukf_weights" in proto.group(1)
        assert len(_capi.SYMBOLS[name]) == n and hasattr(_capi.lib(), name), name
        call = re.search(r"ccall\(\(:%s, LIB\), Cint, \((.*?)\),\s" % name, jl, re.S)
        assert call and [s.strip() for s in call.group(1).split(",")] == jtypes, (name, call and call.group(1))
    assert "Unscented modes." in open(os.path.join(ROOT, "include", "llpf.h")).read()


def test_python_classes_take_unscented_modes_of_one_model():
    """7. IMM(models, P, mu) over UnscentedKalmanFilter: built without a device, one model, one set of weights; no smoother"""
    d2 = llpf_amd.MvNormal(np.zeros(2), np.eye(2))
    lin = lambda n, **kw: llpf_amd.UnscentedKalmanFilter(llpf_amd.LinearDynamics(0.9 * np.eye(n), np.zeros((n, 1))), llpf_amd.LinearMeasurement(np.eye(1, n)),
                                                         0.1, 0.1, llpf_amd.MvNormal(np.zeros(n), np.eye(n)), **kw)
    P, mu = [[0.9, 0.1], [0.1, 0.9]], [0.5, 0.5]
    imm = llpf_amd.IMM([lin(2), lin(2)], P, mu)
    assert imm.unscented and not imm.extended and imm._handle is None and imm.nx == 2 and imm.weights == lin(2).weights
    models, D, _, _ = imm._spec()
    assert D is None and [m.model_id for m in models] == [S.MODEL_LINEAR_GAUSSIAN] * 2
    with pytest.raises(TypeError, match="mode 1.*weights"):
        llpf_amd.IMM([lin(2), lin(2, weight_params=llpf_amd.MerweParams())], P, mu)
    with pytest.raises(TypeError, match="mode 1"):
        llpf_amd.IMM([lin(2), lin(3)], P, mu)                    # other dimensions
    qt = llpf_amd.UnscentedKalmanFilter(llpf_amd.QuadTankDynamics(supersample=2), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                        llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    with pytest.raises(TypeError, match="mode 1"):
        llpf_amd.IMM([qt, lin(4)], P, mu)                        # another model id
    ek = llpf_amd.ExtendedKalmanFilter(llpf_amd.LinearDynamics(0.9 * np.eye(2), np.zeros((2, 1))), llpf_amd.LinearMeasurement(np.eye(1, 2)), 0.1, 0.1, d2)
    with pytest.raises(TypeError, match="mode 0 is a UnscentedKalmanFilter and mode 1 a ExtendedKalmanFilter"):
        llpf_amd.IMM([lin(2), ek], P, mu)
    ext = llpf_amd.IMM([ek, ek], P, mu)
    assert ext.extended and not ext.unscented and ext.weights is None
    with pytest.raises(TypeError, match="filter 1"):
        llpf_amd.IMMBank._pack([imm, ext])
    with pytest.raises(TypeError, match="filter 1"):
        llpf_amd.IMMBank._pack([ext, imm])
    assert llpf_amd.IMMBank._pack([imm, ([lin(2), lin(2)], P, mu)])[5] is False
    assert llpf_amd.IMMBank._tables([imm, imm])[5:] == ("unscented", imm.weights) and llpf_amd.IMMBank._tables([ext])[5:] == ("extended", None)
    with pytest.raises(TypeError, match="filter 1.*weights"):
        llpf_amd.IMMBank._tables([imm, llpf_amd.IMM([lin(2, weight_params=llpf_amd.MerweParams())] * 2, P, mu)])
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(imm, np.zeros((3, 1)), np.zeros((3, 1)))
    assert imm._handle is None
