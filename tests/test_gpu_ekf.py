"""Banks of extended Kalman filters on the device (llpf_ekf_bank_*; kernels/ekf.hpp, host/ekf.hpp): the GPU reproduces the host build of
csrc/shared/llpf_ekf.h (tests/ekf_host.c) bit for bit — precompiled and run-time compiled models, whatever the bank, the chunking of T
or the split of a run — and the Python API (ExtendedKalmanFilter, ExtendedKalmanFilterBank) is the filter the CPU tests pin down."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import kalman_common as kc
from kalman_common import _same
from gpu_common import _Inject
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS, lg_models, quadtank_models, with_id
import models as M
import ukf_common as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ec.build_host(tmp_path_factory.mktemp("ekf_host"))


def _bank(models):
    return _capi.EkfBankHandle(0, list(models))


EKF = kg.Family("ekf", _bank, ec.host_run, lg_models, True)


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_header_for_every_precompiled_shape(host, nx):
    """1. 16 of the 17 precompiled shapes: F = 1000 random filters, T = 200 with missing rows, every output and the final state"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        b, g, _, st, _, _ = kg.check_shape(EKF, host, rng, F=1000, T=200, nx=nx, ny=ny, nu=nu, missing=(50, 51, 120), what=(nx, ny))
        assert np.isfinite(g["ll"]).all()
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]), (nx, ny, "final state")
        b.close()


def test_quadtank_precompiled_shape_and_the_switch_time(host):
    """1., 2. the 17th shape: the built-in quad-tank, F = 1000 with per-filter parameters over T = 200 with missing rows, and across
    tau = TSWITCH = 500 (t_index0 = 470, T = 60): the device's RK4 and its Jacobian in the shared header's order"""
    models = quadtank_models(1000)
    U, Y = M.quadtank_data(200)
    Y = Y.copy()
    Y[[5, 120, 121], 0] = np.nan
    b = _bank(models)
    g = b.run(U, Y, outputs=OUTS, t_index0=1.0)
    h, st = ec.host_run(host, models, U, Y, 200, t_index0=1.0)
    _same(g, h, what="quad-tank")
    assert np.isfinite(g["ll"]).all() and len(set(g["ll"].tolist())) > 40
    x, R = b.get_state()
    assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1])
    b.reset()
    U, Y = M.quadtank_data(60)
    g = b.run(U, Y, outputs=OUTS, t_index0=470.0)
    h, _ = ec.host_run(host, models, U, Y, 60, t_index0=470.0)
    _same(g, h, what="quad-tank across the switch")
    b.close()


def test_each_output_alone(host):
    """every optional output asked for on its own is the column of the run with all of them: F = 65 (a full workgroup and a ragged one)"""
    kg.check_each_output_alone(EKF, host, seed=77, F=65, T=3, nx=2, ny=1, nu=1)


@pytest.mark.parametrize("F", [1, 63, 64, 65, 1000])
def test_bank_sizes_and_chunk_edges(host, F):
    """3. per-filter parameters at every bank size around the wave, T around the 256-step chunk of the staging pipe"""
    kg.check_bank_sizes_and_chunk_edges(EKF, host, seed=100 + F, F=F, nx=2, ny=1, nu=1, missing=(0, 255, 256, 699), Ts=(1, 255, 256, 257, 700))


def test_continuation_set_models_and_state(host):
    """4., 5. run(a) then run(b) is run(a + b); set_state / get_state round trip; set_models is a fresh bank"""
    rng, b, U, Y = kg.check_continuation(EKF, host, seed=5, F=300, T=600, nx=3, ny=2, nu=2, missing=(255, 256, 500), cut=300)
    other = lg_models(rng, 300, 3, 2, 2)
    b.set_models(other)
    b.reset()
    g = b.run(U, Y, outputs=OUTS)
    h, _ = ec.host_run(host, other, U, Y, 600)
    _same(g, h, what="set_models vs host")
    with pytest.raises(_capi.LLPFError):
        b.set_models(lg_models(rng, 300, 2, 2, 2))


def test_per_filter_inputs_missing_rows_and_a_nan_filter_beside_healthy_ones(host):
    """6., 9. per-filter U and Y over 4000 filters; a filter made NaN through set_state beside healthy ones whose bits do not move"""
    kg.check_per_filter_inputs_and_a_nan_filter(EKF, host, seed=6, F=4000, T=40, nx=2, ny=1, nu=1, missing=(5, 6, 30), stride=7, row=11,
                                                nan_filter=77)


def test_runtime_compiled_shapes(host):
    """7. k_ekf from a hiprtc program of the model's own: the linear-Gaussian model above 4 states, the pendulum and x0^2 as snippets
    with hand-written members against their C twins"""
    rng = np.random.default_rng(21)
    for nx, ny, nu in ((5, 1, 0), (6, 3, 2), (8, 4, 1)):
        kg.check_shape(EKF, host, rng, F=130, T=60, nx=nx, ny=ny, nu=nu, missing=(7,), what=("LG", nx, ny))
    pid = _capi.model_compile(ec.PENDULUM_JAC_SRC, 2, 1)
    pend = kg.pendulum_models(100)
    U, Y = uc.pendulum_data(300)
    Y = Y.copy()
    Y[[3, 256], 0] = np.nan
    g = _bank([with_id(m, pid) for m in pend]).run(U, Y, outputs=OUTS)
    h, _ = ec.host_run(host, pend, U, Y, 300, kind=ec.KIND_PENDULUM)
    _same(g, h, what="pendulum")
    assert np.isfinite(g["ll"]).all()
    sq = kg.square_models(64)
    Y = 3.0 + 0.5 * rng.standard_normal((80, 1))
    h, _ = ec.host_run(host, sq, None, Y, 80, kind=ec.KIND_SQUARE)
    sid = _capi.model_compile(ec.SQUARE_JAC_SRC, 1, 1)
    g = _bank([with_id(m, sid) for m in sq]).run(None, Y, outputs=OUTS)
    _same(g, h, what="square snippet")


def test_a_filter_alone_equals_its_column_of_the_bank_and_a_throw_is_a_status():
    """8., 10. one filter is its column of the bank; LLPF_TEST_THROW=error:ekf_run gives a status with the process alive"""
    models = quadtank_models(70)
    U, Y = M.quadtank_data(100)
    b = _bank(models)
    g = b.run(U, Y, outputs=OUTS, t_index0=1.0)
    for f in (0, 37, 69):
        one = _bank([models[f]]).run(U, Y, outputs=OUTS, t_index0=1.0)
        for k in OUTS:
            assert kc.bits_equal(one[k][:, 0], g[k][:, f]), (f, k)
        assert one["ll"][0] == g["ll"][f]
    b.reset()
    with _Inject("error:ekf_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y)
    assert ei.value.code == _capi.ERR_INTERNAL and "ekf_run" in str(ei.value)
    with _Inject("alloc:ekf_create"):
        with pytest.raises(_capi.LLPFError) as ei:
            _bank(models)
    assert ei.value.code == _capi.ERR_ALLOC
    again = b.run(U, Y, outputs=OUTS, t_index0=1.0)
    _same(again, g, what="after the throw")


def test_ekf_bank_on_the_linear_c1_model_is_the_kalman_bank():
    """11. from_filter_bank of the C1 linear bank against KalmanFilterBank: every output to 1e-10, R and Rt bit for bit"""
    _, U, Y = M.simulate_lg(M.lg_c1_model(0), 200)
    pf = llpf_amd.FilterBank(1000, kg.c1_specs(16), rng=1)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf)
    eb = llpf_amd.ExtendedKalmanFilterBank.from_filter_bank(pf)
    lk, le = kb.loglik(U, Y), eb.loglik(U, Y)
    assert np.all(np.abs(le - lk) <= 1e-10 * np.abs(lk)), np.max(np.abs(le - lk) / np.abs(lk))
    fk, fe = kb.forward(U, Y), eb.forward(U, Y)
    for k in OUTS:
        assert kc.close(fe[k], fk[k]), k
    for k in ("R", "Rt"):
        assert np.array_equal(fe[k].view(np.uint64), fk[k].view(np.uint64)), k


def test_traced_callables_against_the_builtin_model_and_the_snippet():
    """12. the quad-tank and x0^2 as traced callables (forward-mode Jacobians, another operation order than the hand-written ones)
    against the built-in model and the snippet, to 1e-10"""
    Q = dict(S.QUADTANK_DEFAULTS)
    d0 = llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1))
    U, Y = M.quadtank_data(520)
    built = llpf_amd.ExtendedKalmanFilter(llpf_amd.QuadTankDynamics(supersample=2), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4), d0)
    traced = llpf_amd.ExtendedKalmanFilter(llpf_amd.rk4(ec.quadtank_rhs, 1.0, 2), ec.quadtank_levels, np.full(4, 0.1), np.full(2, 1e-4), d0,
                                           nu=2, ny=2, p=Q)
    sb, st = llpf_amd.forward_trajectory(built, U, Y), llpf_amd.forward_trajectory(traced, U, Y)
    for k in ("x", "xt", "R", "Rt", "e"):
        assert kc.close(getattr(st, k), getattr(sb, k)), ("quad-tank", k, uc.rel_err(getattr(st, k), getattr(sb, k)))
    assert kc.bits_equal(st.x[1], sb.x[1]), "the value part of the traced model is the built-in model's bits"
    assert abs(st.ll - sb.ll) <= 1e-10 * abs(sb.ll)
    rng = np.random.default_rng(3)
    Ys = 3.0 + 0.5 * rng.standard_normal((80, 1))
    d1 = llpf_amd.MvNormal(np.array([1.0]), 0.36)
    snip = llpf_amd.ExtendedKalmanFilter(llpf_amd.UserDynamics(ec.SQUARE_JAC_SRC, 1, 0, 1), llpf_amd.UserMeasurement(), 0.1, 0.25, d1)
    tr_ = llpf_amd.ExtendedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25, d1, nu=0, ny=1)
    ss, st = llpf_amd.forward_trajectory(snip, None, Ys), llpf_amd.forward_trajectory(tr_, None, Ys)
    for k in ("x", "xt", "R", "Rt", "e"):
        assert kc.close(getattr(st, k), getattr(ss, k)), ("square", k)
    assert abs(st.ll - ss.ll) <= 1e-10 * abs(ss.ll)


def test_python_bank_equals_a_loop_of_single_filters_and_update_is_correct_then_predict(host):
    """13., 14. the Python bank against single ExtendedKalmanFilters; update = correct then predict, through the device"""
    specs = [(llpf_amd.QuadTankDynamics(supersample=2, gamma1=0.2 + 0.01 * k), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
              llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1))) for k in range(6)]
    U, Y = M.quadtank_data(300)
    eb = llpf_amd.ExtendedKalmanFilterBank(specs)
    ll = eb.loglik(U, Y)
    assert ll.shape == (6,) and np.isfinite(ll).all() and len(set(ll.tolist())) == 6
    singles = [llpf_amd.ExtendedKalmanFilter(*s) for s in specs]
    for k, one in enumerate(singles):
        lk = llpf_amd.loglik(one, U, Y)
        assert abs(lk - ll[k]) <= 1e-10 * abs(ll[k]) and lk == ll[k], k
    h, _ = ec.host_run(host, [one._model for one in singles], U, Y, 300, t_index0=1.0)
    assert kc.bits_equal(h["ll"], ll)
    fw = eb.forward(U, Y)
    assert fw["x"].shape == (300, 6, 4) and fw["Rt"].shape == (300, 6, 4, 4) and eb.state()[0].shape == (6, 4)
    eb.set_parameters(specs[::-1])
    assert kc.bits_equal(eb.loglik(U, Y), ll[::-1])
    one = singles[0]
    sol = llpf_amd.forward_trajectory(one, U[:20], Y[:20])
    assert sol.x.shape == (20, 4) and sol.Rt.shape == (20, 4, 4) and sol.e.shape == (20, 2)
    llpf_amd.reset(one)
    one._index = 0
    lls = []
    for t in range(20):
        if t % 2:
            lls.append(llpf_amd.update(one, U[t], Y[t])[0])
        else:
            l, e = llpf_amd.correct(one, U[t], Y[t])
            assert kc.bits_equal(llpf_amd.state(one), sol.xt[t]) and kc.bits_equal(np.tril(llpf_amd.covariance(one)), np.tril(sol.Rt[t]))
            llpf_amd.predict(one, U[t])
            lls.append(l)
    assert abs(sum(lls) - sol.ll) <= 1e-10 * abs(sol.ll)
    x_end = one.x
    llpf_amd.forward_trajectory(one, U[:20], Y[:20])
    assert kc.bits_equal(one.x, x_end), "correct + predict is update, bit for bit"
    with pytest.raises(TypeError, match="smoother"):
        llpf_amd.smooth(one, U[:20], Y[:20])


def test_the_filter_beats_the_prior_only_prediction_on_pendulum_data():
    """15. sanity, not a tolerance: on simulated pendulum data the filtered mean-square error of the angle and the rate is below that of
    the prediction that never sees a measurement.  Numbers in DESIGN.md 7."""
    m = uc.pendulum_model()
    f, g = uc.pendulum_fg(m)
    rng = np.random.default_rng(0)
    T = 400
    U = 0.5 * np.sin(0.1 * np.arange(T)).reshape(T, 1)
    X, Y = np.zeros((T, 2)), np.zeros((T, 1))
    x = np.array([1.0, 0.0])
    for k in range(T):
        X[k] = x
        Y[k] = g(x, U[k], 0.0) + 0.05 * rng.standard_normal()
        x = f(x, U[k], 0.0) + np.sqrt(np.array([1e-4, 4e-3])) * rng.standard_normal(2)
    d0 = llpf_amd.MvNormal(np.array([0.8, 0.0]), np.array([0.3, 0.3]))
    ekf = llpf_amd.ExtendedKalmanFilter(llpf_amd.UserDynamics(ec.PENDULUM_JAC_SRC, 2, 1, 1, qt=(9.81, 0.05)), llpf_amd.UserMeasurement(),
                                        np.array([1e-4, 4e-3]), 0.05 ** 2, d0, Ts=0.05)
    sol = llpf_amd.forward_trajectory(ekf, U, Y)
    blind = llpf_amd.forward_trajectory(ekf, U, np.full((T, 1), np.nan))
    mse_f = np.mean((sol.xt - X) ** 2, axis=0)
    mse_p = np.mean((blind.xt - X) ** 2, axis=0)
    print("pendulum: filtered MSE (angle, rate) %.3e %.3e; prior-only prediction %.3e %.3e" % (mse_f[0], mse_f[1], mse_p[0], mse_p[1]))
    assert np.isfinite(sol.ll) and np.all(mse_f < mse_p)
