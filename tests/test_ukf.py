"""Banks of unscented Kalman filters, the part that needs no GPU: csrc/shared/llpf_ukf.h (the device order, built for the host by
tests/ukf_host.c around the oracle's model functions) against the Kalman filter on linear models, against a numpy restatement of the
textbook formulas on nonlinear ones, known answers of the transform, and the argument checks of the C ABI (llpf_ukf_bank_*)."""
import ctypes as C
import os

import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import kalman_common as kc
import models as M
import ukf_common as uc
import user_models as UM

OUTPUTS = _capi.KALMAN_OUTPUTS
T_LIN = 200
MISSING = (17, 120)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return uc.build_host(tmp_path_factory.mktemp("ukf_host"))


@pytest.fixture(scope="module")
def kalman_host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kf_host"))


def linear_systems():
    """the 32 systems of every nx 1..8 x ny 1..4 (seed 5): D = 0, nu = 1, the covariance kinds cycling, T = 200, two missing rows"""
    rng = np.random.default_rng(5)
    out = []
    for nx in range(1, 9):
        for ny in range(1, 5):
            m, D = kc.random_system(rng, nx, ny, 1, kind=nx + ny, D=False)
            mats = kc.matrices(m, D)
            U, Y = kc.simulate(rng, mats, T_LIN, MISSING)
            out.append((m, D, mats, U, Y))
    return out


@pytest.fixture(scope="module")
def systems():
    return linear_systems()


def test_linear_model_is_the_kalman_filter(host, kalman_host, systems):
    """1. On a linear model the unscented transform is exact for every weight set with sum wm = 1 and wi gamma^2 = 1/2: the host build of
    the header equals the reference's Kalman filter in its literal formulas (kalman_common.numpy_reference) and the host build of the
    Kalman header, to the project's 1e-10, for Merwe (1, 0, 1), (1, 0, 0) and (1, 0, 3 - L) — the last with a negative centre weight for
    nx > 3."""
    worst = 0.0
    for m, D, mats, U, Y in systems:
        ref = kc.numpy_reference(mats, U, Y)
        kf, _ = kc.host_run(kalman_host, [(m, D)], U, Y, T_LIN)
        for abk in uc.ALPHA1_SETS:
            w = uc.merwe_set(m.nx, abk)
            got, _ = uc.host_run(host, [m], w, U, Y, T_LIN)
            assert not np.isnan(got["ll"]).any(), (m.nx, m.ny, abk)
            for k in OUTPUTS:
                worst = max(worst, uc.rel_err(got[k][:, 0], ref[k]))
                assert kc.close(got[k][:, 0], ref[k]), (m.nx, m.ny, abk, k, "numpy reference")
                assert kc.close(got[k][:, 0], kf[k][:, 0]), (m.nx, m.ny, abk, k, "Kalman header")
            assert kc.close(got["ll"][0], ref["ll"]) and kc.close(got["ll"][0], kf["ll"][0]), (m.nx, m.ny, abk)
    print("linear => Kalman: worst relative error against the numpy reference %.2e" % worst)


def _measured_bar(cases, w_of, outputs=OUTPUTS):
    """10 x the worst error of the float64 restatement against the same code in long double, per output, over `cases` =
    [(f64 (f, g), long (f, g), R1, R2, x0, P0, U, Y, Ts, t_index0)]"""
    worst = {k: 0.0 for k in outputs + ("ll",)}
    for (fg, fgl, R1, R2, x0, P0, U, Y, Ts, t0) in cases:
        w = w_of(len(x0))
        a = uc.numpy_ukf(fg[0], fg[1], R1, R2, x0, P0, w, U, Y, Ts, t0)
        b = uc.numpy_ukf(fgl[0], fgl[1], R1, R2, x0, P0, w, U, Y, Ts, t0, lin=uc.LinLong)
        for k in worst:
            worst[k] = max(worst[k], uc.rel_err(a[k], b[k]))
    return worst, {k: 10.0 * v for k, v in worst.items()}


def test_small_alpha_weights_hold_to_the_measured_rounding_error(host, systems):
    """2. With Merwe (1e-3, 2, 0) the weights are of order +-1e6 and cancel: no bar is fixed in advance.  The test measures the
    restatement's own rounding error — the numpy UKF in float64 against the same code in np.longdouble, on the same 32 systems — and holds
    header-vs-restatement to 10 x the worst value per output (two independent float64 evaluations of an ill-conditioned sum may each be
    off by it in opposite directions, and the header orders its sums differently).
    Recorded from this test (float64 restatement against long double, worst of the 32 systems): x 3.0e-08, xt 3.4e-09, ll_steps 2.6e-09,
    R 3.5e-12, Rt 4.2e-12, e 1.4e-06, ll 9.5e-11; header against restatement in the same run: x 2.4e-08, xt 3.6e-09, ll_steps 4.1e-09,
    R 5.1e-12, Rt 8.2e-12, e 3.0e-06, ll 8.6e-11.  The bar is always the value measured in the run at hand (printed with -s), never these."""
    cases = [(uc.linear_fg(mats), uc.linear_fg(mats, np.longdouble), mats["R1"], mats["R2"], mats["x0"], mats["P0"], U, Y, 1.0, 0.0)
             for m, D, mats, U, Y in systems]
    w_of = lambda L: uc.merwe(L, *uc.SMALL_ALPHA)
    worst, bar = _measured_bar(cases, w_of)
    print("small alpha, restatement float64 vs long double (worst of 32):", {k: "%.2e" % v for k, v in worst.items()})
    seen = {k: 0.0 for k in bar}
    for (m, D, mats, U, Y), case in zip(systems, cases):
        w = w_of(m.nx)
        ref = uc.numpy_ukf(case[0][0], case[0][1], mats["R1"], mats["R2"], mats["x0"], mats["P0"], w, U, Y)
        got, _ = uc.host_run(host, [m], w, U, Y, T_LIN)
        assert not np.isnan(got["ll"]).any(), (m.nx, m.ny)
        for k in OUTPUTS:
            seen[k] = max(seen[k], uc.rel_err(got[k][:, 0], ref[k]))
        seen["ll"] = max(seen["ll"], uc.rel_err(got["ll"][0], ref["ll"]))
    print("small alpha, header vs restatement (worst of 32):", {k: "%.2e" % v for k, v in seen.items()})
    for k in bar:
        assert seen[k] <= bar[k], (k, seen[k], bar[k])


def _quadtank_case(T=1000):
    m = M.quadtank_model()
    U, Y = M.quadtank_data(T)
    Y = Y.copy()
    for t in (5, 400, 777):
        Y[t, 0] = np.nan
    return m, U, Y


def _weight_sets(L):
    return [(abk, uc.merwe_set(L, abk)) for abk in uc.ALPHA1_SETS] + [(uc.SMALL_ALPHA, uc.merwe(L, *uc.SMALL_ALPHA))]


def _nonlinear(host, m, U, Y, fg, fg64, fgl, twin, t0, what):
    """header vs restatement for the four weight sets: 1e-10 for the alpha = 1 sets, the measured bar (item 2's method) for the small-alpha
    one; no filter may be NaN"""
    R1, R2 = S.gaussian_cov_matrix(m.dynamics_density), S.gaussian_cov_matrix(m.measurement_density)
    x0, P0 = S.gaussian_mean(m.initial_density), S.gaussian_cov_matrix(m.initial_density)
    T = Y.shape[0]
    for abk, w in _weight_sets(m.nx):
        ref = uc.numpy_ukf(fg[0], fg[1], R1, R2, x0, P0, w, U, Y, m.Ts, t0)
        got, _ = uc.host_run(host, [m], w, U, Y, T, t_index0=t0, twin=twin)
        assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), (what, abk)
        err = {k: uc.rel_err(got[k][:, 0], ref[k]) for k in OUTPUTS}
        err["ll"] = uc.rel_err(got["ll"][0], ref["ll"])
        print(what, abk, "ll %.6f" % got["ll"][0], "header vs restatement:", {k: "%.2e" % v for k, v in err.items()})
        if abk[0] == 1.0:
            for k in OUTPUTS:
                assert kc.close(got[k][:, 0], ref[k]), (what, abk, k, err[k])
            assert kc.close(got["ll"][0], ref["ll"]), (what, abk, err["ll"])
        else:
            worst, bar = _measured_bar([(fg64, fgl, R1, R2, x0, P0, U, Y, m.Ts, t0)], lambda L: w)
            print(what, abk, "restatement float64 vs long double:", {k: "%.2e" % v for k, v in worst.items()})
            for k in bar:
                assert err[k] <= bar[k], (what, abk, k, err[k], bar[k])


def test_header_equals_the_formulas_on_the_quadtank(host):
    """3a. The quad-tank (BASELINE C3) on models.quadtank_data(1000) with three missing rows, across tau = TSWITCH: the header around the
    oracle's RK4 against the restatement driving the Python QuadTankDynamics callable."""
    import llpf_amd
    m, U, Y = _quadtank_case()
    dyn, meas = llpf_amd.QuadTankDynamics(supersample=2), llpf_amd.QuadTankMeasurement()
    fg = (lambda x, u, tau: dyn(x, u, None, tau, m.Ts)), (lambda x, u, tau: meas(x))
    _nonlinear(host, m, U, Y, fg, uc.quadtank_fg(m), uc.quadtank_fg(m, np.longdouble), 0, 1.0, "quad-tank")


def test_header_equals_the_formulas_on_the_pendulum(host):
    """3b. The pendulum of tests/user_models.py through its C twin (the same llpf_sincos2pi / llpf_rint expressions as the device
    snippet) against the restatement with np.sin."""
    m = uc.pendulum_model()
    U, Y = uc.pendulum_data(1000)
    Y = Y.copy()
    for t in (3, 500, 998):
        Y[t, 0] = np.nan
    fg = uc.pendulum_fg(m)
    _nonlinear(host, m, U, Y, fg, fg, uc.pendulum_fg(m, np.longdouble), uc.TWIN_PENDULUM, 0.0, "pendulum")


def _square_model(m0, R00, r2=0.25, r1=0.1):
    g = S.make_gaussian
    return S.make_lg_model(np.eye(1), np.zeros((1, 0)), np.eye(1), g(np.zeros(1), r1), g(np.zeros(1), r2), g(np.array([m0]), float(R00)))


def test_known_answer_of_the_transform(host):
    """4. g(x) = x_0^2, f(x) = x: the predicted measurement of the first step is m0^2 + R00 for every weight set with sum wm = 1 and
    wi gamma^2 = 1/2 — the transform is exact for a quadratic — to 1e-13 relative; and S00 - R2 = sum wc_i (Y_i - yh)^2 by hand (L = 1).
    The sets: Merwe alpha = 1 with kappa 1, 0, 2, the Wikipedia form (1, 0, 1.5) and equal weights.  (A small alpha is left to item 2: its
    centre weight of -1e6 cancels six digits, which no 1e-13 survives.)
    S is not an output; it is recovered twice, from Rt = R - Cxy^2 / S and from ll = -(log 2 pi + log S + e^2 / S) / 2.  Both sides are a
    dozen float64 operations on numbers of order 1 with no cancellation worse than R / (R - Rt) < 1.2 here: 1e-12 relative leaves two
    orders of magnitude over that."""
    m0, R00, r2 = 1.7, 0.36, 0.25
    m = _square_model(m0, R00, r2)
    y = 3.0
    sets = [uc.merwe(1, 1.0, 0.0, 1.0), uc.merwe(1, 1.0, 0.0, 0.0), uc.merwe(1, 1.0, 0.0, 2.0), (np.sqrt(1.5), -0.5 / 1.5 + 1 - 1 / 1.5 + 1 / 1.5, 0.0, 0.0),
            (np.sqrt(1.5), 1 / 3, 1 / 3, 1 / 3)]
    sets[3] = (1.0 * np.sqrt(1.5), (1.5 - 1) / 1.5, (1.5 - 1) / 1.5 + 1 - 1.0 + 0.0, 1 / (2 * 1.5))       # Wiki (alpha, beta, kappa) = (1, 0, 1.5)
    for w in sets:
        gamma, wm0, wc0, wi = w
        assert abs(wm0 + 2 * wi - 1) < 1e-15 and abs(wi * gamma * gamma - 0.5) < 1e-15, w
        got, _ = uc.host_run(host, [m], w, None, np.array([[y]]), 1, twin=uc.TWIN_SQUARE)
        yh = y - got["e"][0, 0, 0]
        want = m0 * m0 + R00
        assert abs(yh - want) <= 1e-13 * want, (w, yh, want)
        # by hand: the three points m0, m0 +- gamma sqrt(R00) through g
        c = gamma * np.sqrt(R00)
        Yp = np.array([m0 * m0, (m0 + c) ** 2, (m0 - c) ** 2])
        wc = np.array([wc0, wi, wi])
        S00 = wc @ (Yp - want) ** 2 + r2
        Cxy = wc @ (np.array([0.0, c, -c]) * (Yp - want))
        e = y - want
        S_got = Cxy * Cxy / (R00 - got["Rt"][0, 0, 0, 0])
        assert abs((S_got - r2) - (S00 - r2)) <= 1e-12 * S00, (w, S_got, S00)
        ll = -0.5 * (np.log(2 * np.pi) + np.log(S00) + e * e / S00)
        assert abs(got["ll_steps"][0, 0] - ll) <= 1e-12 * abs(ll), (w, got["ll_steps"][0, 0], ll)


def _create(models, w=(1.0, 0.0, 2.0, 0.5), struct_size=None):
    L = _capi.lib()
    arr = (S.Model * len(models))(*models)
    ws = _capi.ukf_weights(w)
    if struct_size is not None:
        ws.struct_size = struct_size
    h = C.c_void_p()
    rc = L.llpf_ukf_bank_create(0, arr, len(models), C.byref(ws), C.byref(h))
    if rc == _capi.OK:
        L.llpf_ukf_bank_destroy(h)
    return rc, L.llpf_last_error().decode()


def test_arguments_are_refused_before_a_device_is_looked_for():
    """5a. Every argument check answers LLPF_ERR_ARG on a machine with or without a device."""
    lg = M.lg_test_model()
    assert _create([lg], struct_size=8)[0] == _capi.ERR_ARG
    for w in ((0.0, 0.0, 0.0, 0.5), (-1.0, 0.0, 0.0, 0.5), (1.0, 0.0, 0.0, 0.0), (1.0, 0.0, 0.0, -0.5), (np.nan, 0.0, 0.0, 0.5),
              (1.0, np.inf, 0.0, 0.5), (1.0, 0.0, np.nan, 0.5), (1.0, 0.0, 0.0, np.inf)):
        rc, msg = _create([lg], w)
        assert rc == _capi.ERR_ARG and "ukf" in msg, (w, rc, msg)
    # Rao-Blackwellized model ids
    for mid in (S.MODEL_RB_LINEAR, S.MODEL_RB_BILINEAR):
        m = S.Model.from_buffer_copy(bytes(lg))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "Rao-Blackwellized" in msg, (mid, rc, msg)
    # nx > 8, ny > 4
    rng = np.random.default_rng(0)
    for nx, ny in ((9, 1), (2, 5)):
        m, _ = kc.random_system(rng, nx, ny, 1, D=False)
        assert _create([m])[0] == _capi.ERR_ARG
    # covariances that are not positive definite, a noise density with a non-zero mean
    g = S.make_gaussian
    A, B, Cm = np.eye(2) * 0.9, np.zeros((2, 1)), np.array([[1.0, 0.0]])
    bad = np.array([[1.0, 2.0], [2.0, 1.0]])
    ok2, ok1 = g(np.zeros(2), 0.1), g(np.zeros(1), 0.1)
    for df, dg, d0, word in ((ok2, g(np.zeros(1), -1.0), ok2, "R2"), (ok2, ok1, g(np.zeros(2), bad, S.COV_FULL), "cov(d0)"),
                             (g(np.zeros(2), bad, S.COV_FULL), ok1, ok2, "R1"), (g(np.ones(2), 0.1), ok1, ok2, "zero mean"),
                             (ok2, g(np.ones(1), 0.1), ok2, "zero mean")):
        rc, msg = _create([S.make_lg_model(A, B, Cm, df, dg, d0)])
        assert rc == _capi.ERR_ARG and word in msg, (word, rc, msg)
    # filters of one bank share the dimensions
    assert _create([lg, M.lg_c1_model()])[0] == _capi.ERR_ARG
    # null arguments
    L = _capi.lib()
    h = C.c_void_p()
    ws = _capi.ukf_weights((1.0, 0.0, 2.0, 0.5))
    assert L.llpf_ukf_bank_create(0, None, 1, C.byref(ws), C.byref(h)) == _capi.ERR_ARG
    arr = (S.Model * 1)(lg)
    assert L.llpf_ukf_bank_create(0, arr, 1, None, C.byref(h)) == _capi.ERR_ARG
    assert L.llpf_ukf_bank_create(0, arr, 0, C.byref(ws), C.byref(h)) == _capi.ERR_ARG
    assert L.llpf_ukf_bank_create(0, arr, 1, C.byref(ws), None) == _capi.ERR_ARG
    for fn in (L.llpf_ukf_bank_reset,):
        assert fn(None) == _capi.ERR_ARG
    assert L.llpf_ukf_bank_run(None, None, None, 1, 0, 0.0, None, None) == _capi.ERR_ARG
    assert L.llpf_ukf_bank_get_state(None, None, None) == _capi.ERR_ARG and L.llpf_ukf_bank_set_weights(None, C.byref(ws)) == _capi.ERR_ARG


def test_models_with_members_of_their_own_are_refused():
    """5b. A compiled model with a likelihood of its own has no Gaussian R2, one with `noise` is not additive: LLPF_ERR_ARG, before any
    device work (the snippets compile without a device)."""
    os.environ["LLPF_JIT_COMPILE_ONLY"] = "1"
    try:
        ids = [(_capi.model_compile(src + "\n// test_ukf\n", 2, 1), word) for src, word in ((UM.LAPLACE_SRC, "loglik"), (UM.LAPLACE_NOISE_SRC, "noise"),
                                                                                            (UM.MULT_NOISE_BOX_SRC, "noise"))]
    finally:
        del os.environ["LLPF_JIT_COMPILE_ONLY"]
    for mid, word in ids:
        m = S.Model.from_buffer_copy(bytes(M.lg_test_model()))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and word in msg, (word, rc, msg)
    m = S.Model.from_buffer_copy(bytes(M.lg_test_model()))
    m.model_id = 999999                                  # an id nothing was compiled for
    assert _create([m])[0] == _capi.ERR_ARG


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    """5c. Valid arguments on a machine without a device: LLPF_ERR_NO_DEVICE."""
    for m in (M.lg_test_model(), M.quadtank_model()):
        rc, msg = _create([m])
        assert rc == _capi.ERR_NO_DEVICE, (rc, msg)
    import llpf_amd
    ukf = llpf_amd.UnscentedKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                         llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))
    with pytest.raises(_capi.LLPFError) as ei:
        llpf_amd.loglik(ukf, *M.quadtank_data(5))
    assert ei.value.code == _capi.ERR_NO_DEVICE


def test_a_filter_that_loses_definiteness_is_nan_from_that_step_on(host):
    """5d. A very negative wc0 drives S = wc0 (Y_0 - yh)^2 + ... + R2 of the square model negative once R has grown: in the host build
    that filter is NaN from that step on, while its neighbour in the same call — the same model and weights with covariances so small
    that the centre term never matters — is untouched, bit for bit what it is alone."""
    w_bad = (1.0, 0.0, -40.0, 0.5)
    Ysq = np.full((50, 1), 3.0)
    small = _square_model(1.7, 1e-6, r1=1e-8)
    both, _ = uc.host_run(host, [_square_model(1.7, 0.36), small], w_bad, None, Ysq, 50, twin=uc.TWIN_SQUARE)
    nan0 = np.isnan(both["ll_steps"][:, 0])
    assert nan0.any()
    first = int(np.argmax(nan0))
    assert nan0[first:].all() and not nan0[:first].any()
    assert np.isnan(both["x"][first + 1:, 0]).all() and np.isnan(both["xt"][first:, 0]).all() and np.isnan(both["Rt"][first:, 0]).all()
    assert not np.isnan(both["x"][:first + 1, 0]).any()
    assert np.isnan(both["ll"][0])
    assert not np.isnan(both["ll_steps"][:, 1]).any() and not np.isnan(both["Rt"][:, 1]).any() and not np.isnan(both["ll"][1])
    solo, _ = uc.host_run(host, [small], w_bad, None, Ysq, 50, twin=uc.TWIN_SQUARE)
    for k in OUTPUTS:
        assert kc.bits_equal(both[k][:, 1], solo[k][:, 0]), k
    assert kc.bits_equal(both["ll"][1:], solo["ll"])
