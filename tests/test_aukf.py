"""Banks of unscented Kalman filters with augmented (non-additive) process noise, the part that needs no GPU: csrc/shared/llpf_aukf.h (the
device order, built for the host by tests/aukf_host.c) against the Kalman filter on linear models, against a numpy restatement of the
textbook formulas on two models that form their own noise, known answers of one predict!, the unscented twin's bits in correct!, and the
argument checks of the C ABI (llpf_aukf_bank_*), the Python classes, the tracer and the run-time program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S, tracing
import aukf_common as ac
import kalman_common as kc
import models as M
import test_ukf as tu
import ukf_common as uc
import user_models as UM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd")
OUTPUTS = _capi.KALMAN_OUTPUTS
T_LIN = tu.T_LIN
ARITY = {"llpf_aukf_bank_create": 6, "llpf_aukf_bank_destroy": 1, "llpf_aukf_bank_reset": 1, "llpf_aukf_bank_set_models": 2,
         "llpf_aukf_bank_set_weights": 3, "llpf_aukf_bank_run": 8, "llpf_aukf_bank_get_state": 3, "llpf_aukf_bank_set_state": 3}
SMALL = uc.SMALL_ALPHA


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ac.build_host(tmp_path_factory.mktemp("aukf_host"))


@pytest.fixture(scope="module")
def ukf_host(tmp_path_factory):
    return uc.build_host(tmp_path_factory.mktemp("ukf_host"))


@pytest.fixture(scope="module")
def kalman_host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kf_host"))


@pytest.fixture(scope="module")
def systems():
    return tu.linear_systems()


def _alpha1_pairs(nx):
    return [(abk, ac.merwe_pair(nx, *abk)) for abk in uc.ALPHA1_SETS] + [("trivial", ac.trivial_pair(nx))]


# ------------------------------------------------------------------------------------------------
# 1. the definition against the Kalman filter and the restatement
# ------------------------------------------------------------------------------------------------
def test_linear_model_is_the_kalman_filter(host, kalman_host, systems):
    """On a linear model with additive noise the augmented transform is exact for every pair of sets with sum wm = 1 and wi gamma^2 = 1/2
    at its own L: the twin (additive path, around the oracle's functions) equals kalman_common.numpy_reference and the Kalman twin to the
    project's 1e-10 on test_ukf.linear_systems(), for Merwe (1, 0, 1), (1, 0, 0), (1, 0, 3 - L) and TrivialParams; no filter is NaN."""
    worst = 0.0
    for m, D, mats, U, Y in systems:
        ref = kc.numpy_reference(mats, U, Y)
        kf, _ = kc.host_run(kalman_host, [(m, D)], U, Y, T_LIN)
        for name, w in _alpha1_pairs(m.nx):
            got, _ = ac.host_run(host, [m], w, U, Y, T_LIN)
            assert not np.isnan(got["ll"]).any(), (m.nx, m.ny, name)
            for k in OUTPUTS:
                worst = max(worst, uc.rel_err(got[k][:, 0], ref[k]))
                assert kc.close(got[k][:, 0], ref[k]), (m.nx, m.ny, name, k, "numpy reference")
                assert kc.close(got[k][:, 0], kf[k][:, 0]), (m.nx, m.ny, name, k, "Kalman header")
            assert kc.close(got["ll"][0], ref["ll"]) and kc.close(got["ll"][0], kf["ll"][0]), (m.nx, m.ny, name)
    print("linear => Kalman: worst relative error against the numpy reference %.2e" % worst)


def _measured_bar(cases, w_of):
    """test_ukf._measured_bar's method for this filter: 10 x the worst error of the float64 restatement against the same code in long
    double, per output, over `cases` = [(f64 (fw, g), long (fw, g), R1, R2, x0, P0, U, Y, Ts, t_index0)], measured in the run at hand"""
    worst = {k: 0.0 for k in OUTPUTS + ("ll",)}
    for (fg, fgl, R1, R2, x0, P0, U, Y, Ts, t0) in cases:
        w = w_of(len(x0))
        a = ac.numpy_aukf(fg[0], fg[1], R1, R2, x0, P0, w, U, Y, Ts, t0)
        b = ac.numpy_aukf(fgl[0], fgl[1], R1, R2, x0, P0, w, U, Y, Ts, t0, lin=uc.LinLong)
        for k in worst:
            worst[k] = max(worst[k], uc.rel_err(a[k], b[k]))
    return worst, {k: 10.0 * v for k, v in worst.items()}


def test_small_alpha_weights_hold_to_the_measured_rounding_error(host, systems):
    """Merwe (1e-3, 2, 0) at both dimensions: weights of order +-1e6 that cancel.  The bar is test_ukf.py::_measured_bar's: 10 x the
    restatement's own float64-against-long-double error on the same systems in the same run, per output, never a recorded number (the
    figures are printed with -s)."""
    cases = [(ac.additive(uc.linear_fg(mats)), ac.additive(uc.linear_fg(mats, np.longdouble)), mats["R1"], mats["R2"], mats["x0"], mats["P0"],
              U, Y, 1.0, 0.0) for m, D, mats, U, Y in systems]
    w_of = lambda nx: ac.merwe_pair(nx, *SMALL)
    worst, bar = _measured_bar(cases, w_of)
    print("small alpha, restatement float64 vs long double (worst of 32):", {k: "%.2e" % v for k, v in worst.items()})
    seen = {k: 0.0 for k in bar}
    for (m, D, mats, U, Y), case in zip(systems, cases):
        w = w_of(m.nx)
        ref = ac.numpy_aukf(case[0][0], case[0][1], mats["R1"], mats["R2"], mats["x0"], mats["P0"], w, U, Y)
        got, _ = ac.host_run(host, [m], w, U, Y, T_LIN)
        assert not np.isnan(got["ll"]).any(), (m.nx, m.ny)
        for k in OUTPUTS:
            seen[k] = max(seen[k], uc.rel_err(got[k][:, 0], ref[k]))
        seen["ll"] = max(seen["ll"], uc.rel_err(got["ll"][0], ref["ll"]))
    print("small alpha, header vs restatement (worst of 32):", {k: "%.2e" % v for k, v in seen.items()})
    for k in bar:
        assert seen[k] <= bar[k], (k, seen[k], bar[k])


def _snippet_case(host, m, U, Y, fg, fgl, twin, what):
    """header vs restatement by the same two bars: 1e-10 for the alpha = 1 pairs and TrivialParams, the measured bar for the small-alpha
    pair; no filter may be NaN"""
    R1, R2 = S.gaussian_cov_matrix(m.dynamics_density), S.gaussian_cov_matrix(m.measurement_density)
    x0, P0 = S.gaussian_mean(m.initial_density), S.gaussian_cov_matrix(m.initial_density)
    T = Y.shape[0]
    for name, w in _alpha1_pairs(m.nx) + [(SMALL, ac.merwe_pair(m.nx, *SMALL))]:
        ref = ac.numpy_aukf(fg[0], fg[1], R1, R2, x0, P0, w, U, Y, m.Ts)
        got, _ = ac.host_run(host, [m], w, U, Y, T, twin=twin)
        assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), (what, name)
        err = {k: uc.rel_err(got[k][:, 0], ref[k]) for k in OUTPUTS}
        err["ll"] = uc.rel_err(got["ll"][0], ref["ll"])
        print(what, name, "ll %.6f" % got["ll"][0], "header vs restatement:", {k: "%.2e" % v for k, v in err.items()})
        if name != SMALL:
            for k in OUTPUTS:
                assert kc.close(got[k][:, 0], ref[k]), (what, name, k, err[k])
            assert kc.close(got["ll"][0], ref["ll"]), (what, name, err["ll"])
        else:
            worst, bar = _measured_bar([(fg, fgl, R1, R2, x0, P0, U, Y, m.Ts, 0.0)], lambda L: w)
            print(what, name, "restatement float64 vs long double:", {k: "%.2e" % v for k, v in worst.items()})
            for k in bar:
                assert err[k] <= bar[k], (what, name, k, err[k], bar[k])


def test_header_equals_the_formulas_on_the_noisy_pendulum(host):
    """the pendulum whose torque carries w[0] and whose damping is multiplied by (1 + w[1]), through its C twin (the device snippet's
    expressions) against the restatement with np.sin, T = 400 with three missing rows"""
    m = ac.noisy_pendulum_model()
    U, Y = uc.pendulum_data(400)
    Y = Y.copy()
    Y[[3, 200, 398], 0] = np.nan
    _snippet_case(host, m, U, Y, ac.noisy_pendulum_fg(m), ac.noisy_pendulum_fg(m, np.longdouble), ac.TWIN_NOISY_PENDULUM, "noisy pendulum")


def test_header_equals_the_formulas_on_the_multiplicative_scalar(host):
    """x' = a x (1 + w) + w^2 with g(x) = x^2, T = 300 with two missing rows"""
    m = ac.mult_model()
    U, Y = ac.mult_data(300)
    Y = Y.copy()
    Y[[7, 150], 0] = np.nan
    _snippet_case(host, m, U, Y, ac.mult_fg(m), ac.mult_fg(m, np.longdouble), ac.TWIN_MULT, "multiplicative scalar")


# ------------------------------------------------------------------------------------------------
# 2. known answers, and what the step shares with the unscented bank
# ------------------------------------------------------------------------------------------------
def _one_predict(host, m, w, twin):
    """(x, R) after one predict! from d0: a one-step run whose row is missing"""
    _, (x, R) = ac.host_run(host, [m], w, None, np.array([[np.nan]]), 1, twin=twin)
    return x[0, 0], R[0, 0, 0]


def test_known_answers_of_one_predict(host):
    """For every pair of sets with wia gamma_a^2 = 1/2 and sum wm = 1: x' = x + w^2 has the mean m + q, exactly what the transform gives
    for a quadratic; x' = a x (1 + w) has the variance a^2 (P + m^2 q) = 0.3726 for a = 0.9, m = 2, P = 0.3, q = 0.04, where the additive
    filter of the same a, P, q gives a^2 P + q = 0.283.  Each side is a dozen float64 operations on numbers of order 1 without
    cancellation: 1e-13 relative for the mean, 1e-12 for the variances."""
    a, m0, P, q = 0.9, 2.0, 0.3, 0.04
    model = ac.mult_model(a, q, m0, P)
    lin = S.make_lg_model(np.array([[a]]), np.zeros((1, 0)), np.eye(1), model.dynamics_density, model.measurement_density, model.initial_density)
    wiki = lambda L, kappa: (float(np.sqrt(kappa)), (kappa - L) / kappa, (kappa - L) / kappa, 1.0 / (2.0 * kappa))
    pairs = [ac.merwe_pair(1, 1.0, 0.0, 1.0), ac.merwe_pair(1, 1.0, 0.0, 0.0), ac.merwe_pair(1, 1.0, 0.0, 2.0), ac.trivial_pair(1),
             (wiki(1, 1.5), wiki(2, 2.5))]
    for w in pairs:
        gamma_a, wm0a, wc0a, wia = w[1]
        assert abs(wm0a + 4 * wia - 1) < 1e-15 and abs(wia * gamma_a * gamma_a - 0.5) < 1e-15, w
        mean, _ = _one_predict(host, model, w, ac.TWIN_SQUARE_NOISE)
        assert abs(mean - (m0 + q)) <= 1e-13 * (m0 + q), (w, mean)
        mean, var = _one_predict(host, model, w, ac.TWIN_MULT_ONLY)
        assert abs(mean - a * m0) <= 1e-13 * a * m0, (w, mean)
        assert abs(var - a * a * (P + m0 * m0 * q)) <= 1e-12 * 0.3726 and abs(var - 0.3726) < 1e-12, (w, var)
        mean, var = _one_predict(host, lin, w, 0)
        assert abs(mean - a * m0) <= 1e-13 * a * m0 and abs(var - 0.283) <= 1e-12 * 0.283, (w, mean, var)


def test_one_step_is_the_unscented_twins_correct_bit_for_bit(host, ukf_host, systems):
    """correct! is llpf_ukf.h's, call for call, with the measurement set: xt, Rt, e and ll of a one-step run are ukf_host_run's bits, on
    linear systems of every nx and on the quad-tank"""
    cases = [(m, U, Y) for m, D, mats, U, Y in systems[::5]] + [(M.quadtank_model(),) + tuple(M.quadtank_data(3))]
    for m, U, Y in cases:
        for name, w in _alpha1_pairs(m.nx) + [(SMALL, ac.merwe_pair(m.nx, *SMALL))]:
            got, _ = ac.host_run(host, [m], w, U[:1], Y[:1], 1)
            ref, _ = uc.host_run(ukf_host, [m], w[0], U[:1], Y[:1], 1)
            for k in ("x", "R", "xt", "Rt", "e", "ll_steps"):
                assert kc.bits_equal(got[k], ref[k]), (m.nx, m.ny, name, k)
            assert kc.bits_equal(got["ll"], ref["ll"])


def test_a_noise_covariance_without_a_factor_is_nan_from_the_first_predict(host):
    """R1 that is not positive definite has no C1: that filter's x and R are NaN from the first predict! on (its first correct!, from d0, is
    untouched), and its neighbour in the same call is bit for bit what it is alone"""
    rng = np.random.default_rng(9)
    good, _ = kc.random_system(rng, 2, 1, 1, D=False)
    bad = S.Model.from_buffer_copy(bytes(good))
    bad.dynamics_density = S.make_gaussian(np.zeros(2), np.array([[1.0, 2.0], [2.0, 1.0]]), S.COV_FULL)
    U, Y = kc._data(rng, 20, 1, 1)
    w = ac.merwe_pair(2, 1.0, 0.0, 1.0)
    both, (xb, Rb) = ac.host_run(host, [bad, good], w, U, Y, 20)
    solo, (xs, Rs) = ac.host_run(host, [good], w, U, Y, 20)
    assert np.isfinite(both["xt"][0, 0]).all() and np.isfinite(both["Rt"][0, 0]).all() and np.isfinite(both["ll_steps"][0, 0])
    assert np.isnan(both["x"][1:, 0]).all() and np.isnan(both["R"][1:, 0]).all() and np.isnan(both["ll_steps"][1:, 0]).all()
    assert np.isnan(both["ll"][0]) and np.isnan(xb[0]).all() and np.isnan(Rb[0]).all()
    for k in OUTPUTS:
        assert kc.bits_equal(both[k][:, 1], solo[k][:, 0]), k
    assert kc.bits_equal(both["ll"][1:], solo["ll"]) and kc.bits_equal(xb[1], xs[0]) and kc.bits_equal(Rb[1], Rs[0])


# ------------------------------------------------------------------------------------------------
# 3. the ABI without a device
# ------------------------------------------------------------------------------------------------
def _create(models, wm=(1.0, 0.0, 2.0, 0.5), wd=(1.0, 0.5, 0.5, 0.125), struct_size=None):
    L = _capi.lib()
    arr = (S.Model * len(models))(*models)
    a, b = _capi.ukf_weights(wm), _capi.ukf_weights(wd)
    if struct_size is not None:
        b.struct_size = struct_size
    h = C.c_void_p()
    rc = L.llpf_aukf_bank_create(0, arr, len(models), C.byref(a), C.byref(b), C.byref(h))
    if rc == _capi.OK:
        L.llpf_aukf_bank_destroy(h)
    return rc, L.llpf_last_error().decode()


def test_header_binding_library_and_julia_name_the_same_exports():
    """fails without the feature for want of llpf_aukf_bank_create"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    capi = open(os.path.join(PKG, "csrc", "capi.hip")).read()
    jl = open(os.path.join(PKG, "julia", "LLPFAmd.jl")).read()
    L = _capi.lib()
    assert hasattr(L, "llpf_aukf_bank_create")
    declared = sorted(set(re.findall(r"\b(llpf_aukf_[a-z_]+)\s*\(", hdr)))
    assert declared == sorted(ARITY)
    assert sorted(n for n in _capi.SYMBOLS if n.startswith("llpf_aukf_")) == declared
    assert sorted(set(re.findall(r"ccall\(\(:(llpf_aukf_[a-z_]+), LIB\)", jl))) == declared
    for name in declared:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert len(m.group(1).split(",")) == ARITY[name], name
        assert hasattr(L, name) and len(_capi.SYMBOLS[name]) == ARITY[name], name
        assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % name, capi, re.M) and "LLPF_GUARD(%s)" % name in capi, name
        j = re.search(r"ccall\(\(:%s, LIB\),\s*\w+,\s*\((.*?)\),\s" % name, jl, re.S).group(1)
        assert len([a for a in re.sub(r"\{[^}]*\}", "", j).split(",") if a.strip()]) == ARITY[name], (name, j)
    exported = re.search(r"^export (.*?)\n\n", jl, re.S | re.M).group(1)
    for name in ("GPUAugmentedUnscentedKalmanFilter", "GPUAugmentedUnscentedKalmanFilterBank", "aukf_run"):
        assert re.search(r"\b%s\b" % name, exported), name
    for name in ("AugmentedUnscentedKalmanFilter", "AugmentedUnscentedKalmanFilterBank"):
        assert name in llpf_amd.api.__all__ and hasattr(llpf_amd, name)
    assert "llpf_aukf_bank_smooth" not in hdr
    assert re.search(r"LLPF_TRAIT_DYNAMICS_W\s*=\s*64", hdr) and _capi.TRAIT_DYNAMICS_W == 64 and "TRAIT_DYNAMICS_W = Int32(64)" in jl
    ma, mi = C.c_int32(-1), C.c_int32(-1)
    assert L.llpf_version(C.byref(ma), C.byref(mi)) == 0 and (ma.value, mi.value) == (0, 7)


def test_arguments_are_refused_before_a_device_is_looked_for():
    """every argument check of create answers LLPF_ERR_ARG on a machine with or without a device: either weight set by the unscented
    bank's checks, the models by its pack under this bank's prefix; a null handle answers "null handle", a null out pointer "null out
    pointer" """
    lg = M.lg_test_model()
    assert _create([lg], struct_size=8)[0] == _capi.ERR_ARG
    ok = (1.0, 0.0, 2.0, 0.5)
    for w in ((0.0, 0.0, 0.0, 0.5), (-1.0, 0.0, 0.0, 0.5), (1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, -0.5), (np.nan, 0.0, 0.0, 0.5),
              (1.0, np.inf, 0.0, 0.5), (1.0, 0.0, np.nan, 0.5), (1.0, 0.0, 0.0, np.inf)):
        for wm, wd in ((w, ok), (ok, w)):
            rc, msg = _create([lg], wm, wd)
            assert rc == _capi.ERR_ARG and msg.startswith("ukf: "), (w, rc, msg)
    for mid in (S.MODEL_RB_LINEAR, S.MODEL_RB_BILINEAR):
        m = S.Model.from_buffer_copy(bytes(lg))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "Rao-Blackwellized" in msg and msg.startswith("aukf: "), (mid, rc, msg)
    rng = np.random.default_rng(0)
    for nx, ny in ((9, 1), (2, 5)):
        m, _ = kc.random_system(rng, nx, ny, 1, D=False)
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "1..8" in msg, (rc, msg)
    g = S.make_gaussian
    A, B, Cm = np.eye(2) * 0.9, np.zeros((2, 1)), np.array([[1.0, 0.0]])
    bad = np.array([[1.0, 2.0], [2.0, 1.0]])
    ok2, ok1 = g(np.zeros(2), 0.1), g(np.zeros(1), 0.1)
    for df, dg, d0, word in ((ok2, g(np.zeros(1), -1.0), ok2, "R2"), (ok2, ok1, g(np.zeros(2), bad, S.COV_FULL), "cov(d0)"),
                             (g(np.zeros(2), bad, S.COV_FULL), ok1, ok2, "R1"), (g(np.ones(2), 0.1), ok1, ok2, "zero mean")):
        rc, msg = _create([S.make_lg_model(A, B, Cm, df, dg, d0)])
        assert rc == _capi.ERR_ARG and word in msg, (word, rc, msg)
    rc, msg = _create([lg, M.lg_c1_model()])
    assert rc == _capi.ERR_ARG and "differ from filter 0" in msg
    L = _capi.lib()
    h = C.c_void_p()
    ws = _capi.ukf_weights(ok)
    arr = (S.Model * 1)(lg)
    err = lambda: L.llpf_last_error().decode()
    assert L.llpf_aukf_bank_create(0, None, 1, C.byref(ws), C.byref(ws), C.byref(h)) == _capi.ERR_ARG and err() == "aukf: models is null"
    assert L.llpf_aukf_bank_create(0, arr, 1, None, C.byref(ws), C.byref(h)) == _capi.ERR_ARG and "weights is null" in err()
    assert L.llpf_aukf_bank_create(0, arr, 1, C.byref(ws), None, C.byref(h)) == _capi.ERR_ARG and "weights is null" in err()
    assert L.llpf_aukf_bank_create(0, arr, 0, C.byref(ws), C.byref(ws), C.byref(h)) == _capi.ERR_ARG and "n_filters must be >= 1" in err()
    assert L.llpf_aukf_bank_create(0, arr, 1, C.byref(ws), C.byref(ws), None) == _capi.ERR_ARG and err() == "null out pointer"
    assert not h.value
    x = np.zeros(4)
    for rc in (L.llpf_aukf_bank_reset(None), L.llpf_aukf_bank_set_models(None, arr), L.llpf_aukf_bank_set_weights(None, C.byref(ws), C.byref(ws)),
               L.llpf_aukf_bank_run(None, None, _capi.dptr(x), 1, 0, 0.0, None, None), L.llpf_aukf_bank_get_state(None, None, None),
               L.llpf_aukf_bank_set_state(None, _capi.dptr(x), _capi.dptr(x))):
        assert rc == _capi.ERR_ARG and err() == "null handle"
    assert L.llpf_aukf_bank_destroy(None) == _capi.OK


def test_traits_and_the_refusals_of_members_of_their_own(monkeypatch):
    """model_traits reports bit 64 for the two snippets and for nothing that lacks the member (compile only); a compiled model with
    `loglik`, `noise` or `initial` is refused as the unscented bank refuses it, under this bank's prefix; an unknown id"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    assert _capi.model_traits(_capi.model_compile(ac.NOISY_PENDULUM_SRC, 2, 1)) == _capi.TRAIT_DYNAMICS_W
    assert _capi.model_traits(_capi.model_compile(ac.MULT_SRC, 1, 1)) == _capi.TRAIT_DYNAMICS_W
    assert _capi.model_traits(_capi.model_compile(UM.PENDULUM_SRC + "\n// test_aukf\n", 2, 1)) == 0
    assert _capi.model_traits(_capi.model_compile(uc.SQUARE_SRC + "\n// test_aukf\n", 1, 1)) == 0
    for src, word in ((UM.LAPLACE_SRC, "loglik"), (UM.LAPLACE_NOISE_SRC, "noise"), (UM.MULT_NOISE_BOX_SRC, "noise")):
        m = S.Model.from_buffer_copy(bytes(M.lg_test_model()))
        m.model_id = _capi.model_compile(src + "\n// test_aukf\n", 2, 1)
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and word in msg and msg.startswith("aukf: "), (word, rc, msg)
    m = S.Model.from_buffer_copy(bytes(M.lg_test_model()))
    m.model_id = 999999
    rc, msg = _create([m])
    assert rc == _capi.ERR_ARG and "unknown model id 999999" in msg


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    """valid arguments on a machine without a device: LLPF_ERR_NO_DEVICE, from the ABI and through the Python filter"""
    for m in (M.lg_test_model(), M.quadtank_model()):
        rc, msg = _create([m])
        assert rc == _capi.ERR_NO_DEVICE, (rc, msg)
    kf = llpf_amd.AugmentedUnscentedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                                 llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    with pytest.raises(_capi.LLPFError) as ei:
        llpf_amd.loglik(kf, *M.quadtank_data(5))
    assert ei.value.code == _capi.ERR_NO_DEVICE


# ------------------------------------------------------------------------------------------------
# 4. the Python classes and the tracer
# ------------------------------------------------------------------------------------------------
def _mult(x, u, p, t, w):
    return [p * x[0] * (1.0 + w[0]) + w[0] * w[0]]


def test_python_classes_without_a_device(monkeypatch):
    """both classes are built without a device; a preset gives weights(nx) and weights(2 nx), a pair of 4-tuples passes, one 4-tuple is
    a ValueError; smooth of either raises TypeError with "no smoother"; neither derives from the unscented classes, so IMM refuses the
    filter as a mode"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    d4 = llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1))
    qt = llpf_amd.AugmentedUnscentedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4), d4)
    assert qt._handle is None and qt._model.model_id == S.MODEL_QUADTANK_RK4
    assert qt.weights == (llpf_amd.TrivialParams().weights(4), llpf_amd.TrivialParams().weights(8))
    mp = llpf_amd.MerweParams(1.0, 0.0, 1.0)
    qm = llpf_amd.AugmentedUnscentedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4), d4,
                                                 weight_params=mp)
    assert qm.weights == (mp.weights(4), mp.weights(8)) == ac.merwe_pair(4, 1.0, 0.0, 1.0)
    pair = ((1.0, 0.0, 2.0, 0.5), (1.0, 0.5, 0.5, 0.125))
    qp = llpf_amd.AugmentedUnscentedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4), d4,
                                                 weight_params=pair)
    assert qp.weights == pair
    with pytest.raises(ValueError, match="pair"):
        llpf_amd.AugmentedUnscentedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4), d4,
                                                weight_params=(1.0, 0.0, 2.0, 0.5))
    assert not isinstance(qt, llpf_amd.UnscentedKalmanFilter)
    assert not issubclass(llpf_amd.AugmentedUnscentedKalmanFilterBank, llpf_amd.UnscentedKalmanFilterBank)
    B = llpf_amd.AugmentedUnscentedKalmanFilterBank
    assert B._AT_LOGLIK == {"t_index0": 1.0} and B._AT_FORWARD == {"t_index0": 0.0}
    models = B._models([qt, (llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4), d4)], 1.0)
    assert [mm.model_id for mm in models] == [S.MODEL_QUADTANK_RK4] * 2
    for name in ("from_filter_bank", "set_parameters", "set_weights", "loglik", "forward", "state"):
        assert hasattr(B, name), name
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(qt, np.zeros((3, 2)), np.zeros((3, 2)))
    with pytest.raises(TypeError, match="no smoother"):
        B.smooth(None, None, None)
    with pytest.raises(TypeError):
        llpf_amd.IMM([qt, qt], np.full((2, 2), 0.5), np.full(2, 0.5))
    # a UserDynamics snippet defines the member itself
    dyn = llpf_amd.UserDynamics(ac.MULT_SRC, 1, 0, 1, qt=(0.9,))
    us = llpf_amd.AugmentedUnscentedKalmanFilter(dyn, llpf_amd.UserMeasurement(), 0.04, 0.25, llpf_amd.MvNormal(np.array([2.0]), 0.3))
    assert _capi.model_traits(us._model.model_id) == _capi.TRAIT_DYNAMICS_W and us._model.qt[0] == 0.9


def test_a_callable_of_five_parameters_is_traced_into_both_members(monkeypatch):
    """dynamics(x, u, p, t, w) is emitted as dynamics_w and, at w = nx zeros, as dynamics; tracing.evaluate of either trace equals the
    callable; a callable of four parameters is traced as before (no member, the text it always had); the other filters keep tracing four
    parameters only"""
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    d1 = llpf_amd.MvNormal(np.array([2.0]), 0.3)
    meas = lambda x, u, p, t: [x[0] * x[0]]
    kf = llpf_amd.AugmentedUnscentedKalmanFilter(_mult, meas, 0.04, 0.25, d1, nu=0, ny=1, p=0.9)
    src = kf.dynamics.src
    assert "DEV void dynamics_w(const double* x, const double* w, double* out) const" in src and "w[0]" in src
    assert "DEV void dynamics(const double* x, double* out) const" in src
    assert _capi.model_traits(kf._model.model_id) == _capi.TRAIT_DYNAMICS_W
    g, outs = tracing.trace(_mult, 1, 0, 0.9, n_out=1, with_w=True)
    g0, outs0 = tracing.trace(lambda x, u, p, t: _mult(x, u, p, t, [0.0]), 1, 0, 0.9, n_out=1)
    for x, w in ((2.0, 0.3), (-1.25, -0.7), (0.0, 0.0), (3.5, 1e-3)):
        assert tracing.evaluate(g, outs, [x], w=[w]) == _mult([x], [], 0.9, 0.0, [w])
        assert tracing.evaluate(g0, outs0, [x]) == _mult([x], [], 0.9, 0.0, [0.0])
    four = lambda x, u, p, t: [0.9 * x[0]]
    plain = llpf_amd.AugmentedUnscentedKalmanFilter(four, meas, 0.04, 0.25, d1, nu=0, ny=1)
    assert "dynamics_w" not in plain.dynamics.src and _capi.model_traits(plain._model.model_id) == 0
    assert plain.dynamics.src == llpf_amd.UnscentedKalmanFilter(four, meas, 0.04, 0.25, d1, nu=0, ny=1).dynamics.src
    assert tracing.n_parameters(_mult) == 5 and tracing.n_parameters(four) == 4


# ------------------------------------------------------------------------------------------------
# 5. the run-time program of k_aukf
# ------------------------------------------------------------------------------------------------
def test_runtime_program_compiles_for_gfx950_without_a_device(tmp_path):
    """tests/jit_aukf_host.cpp links libllpf_hip.so and calls aukf_prepare the way tests/jit_sqekf_host.cpp calls sqekf_prepare: a snippet
    with dynamics_w, one without it and LinGauss (8, 4) — the 132 KiB array of mapped points in LDS — compile and are found again, the
    precompiled shapes need nothing, an unknown id fails with the message the other units give, a member of another signature with the
    compiler's log under the kernel's name"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    if not os.path.exists(os.path.join(PKG, "libllpf_hip.so")):
        pytest.skip("libllpf_hip.so not built")
    exe = str(tmp_path / "jit_aukf_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "jit_aukf_host.cpp"), "-L", PKG,
                    "-lllpf_hip", "-Wl,-rpath," + PKG, "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failed", r.stdout
    assert len([ln for ln in lines if ln.startswith("ok  ")]) == 14 and not [ln for ln in lines if ln.startswith("FAIL")]
