"""Banks of iterated extended Kalman filters on the device (llpf_ekf_bank_set_iterations; kernels/ekf.hpp, host/ekf.hpp): the GPU
reproduces the host build of the iterated filter of csrc/shared/llpf_ekf.h (tests/ekf_host.c) bit for bit — precompiled and run-time
compiled models, lanes of one wave that stop after different numbers of linearisations, whatever the bank, the chunking of T or the
split of a run — and the Python API (IteratedExtendedKalmanFilter, IteratedExtendedKalmanFilterBank) is the filter the CPU tests pin
down."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import iekf_common as ic
import kalman_common as kc
from kalman_common import _same
from gpu_common import _Inject
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS, lg_models, quadtank_models, with_id
import models as M
import ukf_common as uc

pytestmark = pytest.mark.gpu
ITER = (10, 1e-8)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ic.build_host(tmp_path_factory.mktemp("iekf_host"))


@pytest.fixture(scope="module")
def pendulum_id():
    return _capi.model_compile(ec.PENDULUM_JAC_SRC, 2, 1)


@pytest.fixture(scope="module")
def square_id():
    return _capi.model_compile(ec.SQUARE_JAC_SRC, 1, 1)


def _bank(models, iterations=ITER):
    b = _capi.EkfBankHandle(0, list(models))
    if iterations is not None:
        b.set_iterations(*iterations)
    return b


IEKF = kg.Family("iekf", _bank, lambda host, models, U, Y, T, **kw: ic.host_run(host, models, U, Y, T, *ITER, **kw), lg_models, True)


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_header_for_every_precompiled_shape(host, nx):
    """6. 16 of the 17 precompiled shapes: F = 200 random filters, T = 60 with missing rows, maxiters = 10, epsilon = 1e-8; every output,
    ll and the final state.  The measurement is linear: no step runs more than two linearisations."""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        b, g, h, st, _, _ = kg.check_shape(IEKF, host, rng, F=200, T=60, nx=nx, ny=ny, nu=nu, missing=(0, 20, 21, 59), what=(nx, ny))
        assert np.isfinite(g["ll"]).all() and h["iters"].max() == 2
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]), (nx, ny, "final state")
        b.close()


def test_each_output_alone(host):
    """every optional output asked for on its own is the column of the run with all of them: F = 65 (a full workgroup and a ragged one)"""
    kg.check_each_output_alone(IEKF, host, seed=77, F=65, T=3, nx=2, ny=1, nu=1)


def test_quadtank_precompiled_shape_across_the_switch_time(host):
    """6. the 17th shape: the built-in quad-tank, F = 200 with per-filter parameters, T = 60 across tau = TSWITCH = 500 with missing rows"""
    models = quadtank_models(200)
    U, Y = M.quadtank_data(60)
    Y = Y.copy()
    Y[[5, 30, 31], 0] = np.nan
    b = _bank(models)
    g = b.run(U, Y, outputs=OUTS, t_index0=470.0)
    h, st = ic.host_run(host, models, U, Y, 60, *ITER, t_index0=470.0)
    _same(g, h, what="quad-tank")
    assert np.isfinite(g["ll"]).all() and len(set(g["ll"].tolist())) > 40 and h["iters"].max() == 2
    x, R = b.get_state()
    assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1])
    b.close()


@pytest.fixture(scope="module")
def pendulum_case(host):
    """the pendulum bank of 200 filters over 257 steps on the host, computed once: every smaller case of test 7 is a prefix of it in
    the filters, and a run of its own in T (the host run of a prefix of the steps is the prefix of the host run)"""
    models = ic.pendulum_bank_models(200)
    U, Y = uc.pendulum_data(257)
    Y = Y.copy()
    Y[[2, 255, 256], 0] = np.nan
    Y[0, 0] = 0.95
    h, _ = ic.host_run(host, models, U, Y, 257, *ITER, kind=ec.KIND_PENDULUM)
    return models, U, Y, h


@pytest.mark.parametrize("F", [1, 63, 64, 65, 200])
def test_pendulum_lanes_stop_after_different_iteration_counts(host, pendulum_id, pendulum_case, F):
    """7. the pendulum snippet with per-filter d0 at every bank size around the wave and T around the 256-step chunk of the staging pipe:
    bit for bit the host build, the lanes of one wave stopping after different numbers of linearisations, and every filter alone is its
    column of the bank"""
    models, U, Y, whole = pendulum_case
    if F > 1:
        counts = whole["iters"][0, :min(F, 64)]
        assert len(set(counts.tolist())) >= 3 and counts.max() > 2, counts
    dev = [with_id(m, pendulum_id) for m in models[:F]]
    b = _bank(dev)
    one = _bank(dev[:1])
    for T in (1, 255, 256, 257):
        b.reset()
        g = b.run(U[:T], Y[:T], outputs=OUTS)
        h, st = ic.host_run(host, models[:F], U[:T], Y[:T], T, *ITER, kind=ec.KIND_PENDULUM)
        for k in OUTS:
            assert kc.bits_equal(h[k], whole[k][:T, :F]), (F, T, k, "the host run of a prefix")
        _same(g, h, what=(F, T))
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]), (F, T, "final state")
        if T in (1, 257):
            for f in range(F):
                one.set_models(dev[f:f + 1])
                one.reset()
                solo = one.run(U[:T], Y[:T], outputs=OUTS)
                for k in OUTS:
                    assert kc.bits_equal(solo[k][:, 0], g[k][:, f]), (F, T, f, k)
                assert kc.bits_equal(solo["ll"], g["ll"][f:f + 1]), (F, T, f)
    b.close()
    one.close()


def test_square_snippet_traced_callable_and_lingauss_through_hiprtc(host, square_id):
    """8. x0^2 as a snippet against its C twin bit for bit, the same model as a traced callable against the snippet to 1e-10, and the
    linear-Gaussian model at (5, 1), above the precompiled dimensions, bit for bit"""
    rng = np.random.default_rng(21)
    sq = kg.square_models(64)
    Y = 3.0 + 0.5 * rng.standard_normal((80, 1))
    h, _ = ic.host_run(host, sq, None, Y, 80, *ITER, kind=ec.KIND_SQUARE)
    g = _bank([with_id(m, square_id) for m in sq]).run(None, Y, outputs=OUTS)
    _same(g, h, what="square snippet")
    assert h["iters"].max() > 2
    d1 = llpf_amd.MvNormal(np.array([1.0]), 0.36)
    snip = llpf_amd.IteratedExtendedKalmanFilter(llpf_amd.UserDynamics(ec.SQUARE_JAC_SRC, 1, 0, 1), llpf_amd.UserMeasurement(), 0.1, 0.25, d1)
    tr_ = llpf_amd.IteratedExtendedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25, d1, nu=0, ny=1)
    ss, st = llpf_amd.forward_trajectory(snip, None, Y), llpf_amd.forward_trajectory(tr_, None, Y)
    assert kc.bits_equal(ss.xt[:, 0], h["xt"][:, 0, 0]), "the Python filter is the bank's first column"
    for k in ("x", "xt", "R", "Rt", "e"):
        assert kc.close(getattr(st, k), getattr(ss, k)), ("square", k)
    assert abs(st.ll - ss.ll) <= 1e-10 * abs(ss.ll)
    kg.check_shape(IEKF, host, rng, F=130, T=60, nx=5, ny=1, nu=0, missing=(7,), what=("LG", 5, 1))


def test_set_iterations_between_runs(host, pendulum_id, pendulum_case):
    """9. iterated, then (1, 0): the second run is the plain kernel's bits; a split run equals the whole run; set_models and set_state
    keep the setting; a refused setting changes nothing; LLPF_TEST_THROW=error:ekf_run leaves a usable handle"""
    models, U, Y, whole = pendulum_case
    models, T = models[:100], 257
    dev = [with_id(m, pendulum_id) for m in models]
    b = _bank(dev)
    it = b.run(U, Y, outputs=OUTS)
    for k in OUTS:
        assert kc.bits_equal(it[k], whole[k][:, :100]), k
    b.set_iterations(1, 0.0)
    b.reset()
    g = b.run(U, Y, outputs=OUTS)
    plain = _bank(dev, None).run(U, Y, outputs=OUTS)
    _same(g, plain, what="(1, 0) after an iterated run")
    hp, _ = ec.host_run(host, models, U, Y, T, kind=ec.KIND_PENDULUM)
    _same(g, hp, what="(1, 0) against the plain host build")
    assert not kc.bits_equal(g["xt"], it["xt"])
    b.set_iterations(*ITER)
    for bad in ((0, 1e-8), (101, 1e-8), (10, -1.0), (10, float("nan"))):
        with pytest.raises(_capi.LLPFError) as ei:
            b.set_iterations(*bad)
        assert ei.value.code == _capi.ERR_ARG and "ekf" in str(ei.value)
    b.reset()
    first = b.run(U[:130], Y[:130], outputs=OUTS)
    x, R = b.get_state()
    second = b.run(U[130:], Y[130:], outputs=OUTS, t_index0=130.0)
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), it[k]), k
    fresh = _bank(dev)
    fresh.set_state(x, R)
    again = fresh.run(U[130:], Y[130:], outputs=OUTS, t_index0=130.0)
    _same(again, second, what="set_state keeps the setting")
    other = [with_id(m, pendulum_id) for m in ic.pendulum_bank_models(200)[100:]]
    b.set_models(other)
    b.reset()
    g = b.run(U, Y, outputs=OUTS)
    for k in OUTS:
        assert kc.bits_equal(g[k], whole[k][:, 100:]), ("set_models keeps the setting", k)
    b.reset()
    with _Inject("error:ekf_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y)
    assert ei.value.code == _capi.ERR_INTERNAL and "ekf_run" in str(ei.value)
    after = b.run(U, Y, outputs=OUTS)
    _same(after, g, what="after the throw")


def test_python_classes(host):
    """10. the Python bank against single filters; update = correct then predict through the device; IteratedExtendedKalmanFilter at
    maxiters = 1 is ExtendedKalmanFilter bit for bit; smooth raises for both classes"""
    d0s = [llpf_amd.MvNormal(np.array([0.3 + 0.2 * k, 0.0]), np.array([0.3, 0.3])) for k in range(6)]
    spec = lambda d0: (llpf_amd.UserDynamics(ec.PENDULUM_JAC_SRC, 2, 1, 1, qt=(9.81, 0.05)), llpf_amd.UserMeasurement(), np.array([1e-4, 4e-3]),
                       0.05 ** 2, d0)
    U, Y = uc.pendulum_data(120)
    eb = llpf_amd.IteratedExtendedKalmanFilterBank([spec(d) for d in d0s], Ts=0.05)
    assert (eb.maxiters, eb.epsilon) == (10, 1e-8)
    ll = eb.loglik(U, Y)
    assert ll.shape == (6,) and np.isfinite(ll).all() and len(set(ll.tolist())) == 6
    singles = [llpf_amd.IteratedExtendedKalmanFilter(*spec(d), Ts=0.05) for d in d0s]
    for k, one in enumerate(singles):
        assert llpf_amd.loglik(one, U, Y) == ll[k], k
    plain_models = [S.Model.from_buffer_copy(bytes(one._model)) for one in singles]
    h, _ = ic.host_run(host, plain_models, U, Y, 120, 10, 1e-8, t_index0=1.0, kind=ec.KIND_PENDULUM)
    assert kc.bits_equal(h["ll"], ll) and h["iters"].max() > 2
    plain_bank = llpf_amd.ExtendedKalmanFilterBank([spec(d) for d in d0s], Ts=0.05)
    assert not kc.bits_equal(plain_bank.loglik(U, Y), ll)
    eb.set_iterations(1, 0.0)
    assert kc.bits_equal(eb.loglik(U, Y), plain_bank.loglik(U, Y))
    one = singles[0]
    sol = llpf_amd.forward_trajectory(one, U[:20], Y[:20])
    assert sol.x.shape == (20, 2) and sol.Rt.shape == (20, 2, 2) and sol.e.shape == (20, 1)
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
    once = llpf_amd.IteratedExtendedKalmanFilter(*spec(d0s[0]), Ts=0.05, maxiters=1)
    ekf = llpf_amd.ExtendedKalmanFilter(*spec(d0s[0]), Ts=0.05)
    sa, sb = llpf_amd.forward_trajectory(once, U, Y), llpf_amd.forward_trajectory(ekf, U, Y)
    for k in ("x", "xt", "R", "Rt", "e"):
        assert kc.bits_equal(getattr(sa, k), getattr(sb, k)), k
    assert sa.ll == sb.ll and not kc.bits_equal(sa.xt, llpf_amd.forward_trajectory(one, U, Y).xt)
    with pytest.raises(TypeError, match="smoother"):
        llpf_amd.smooth(one, U[:20], Y[:20])
    with pytest.raises(TypeError, match="smoother"):
        eb.smooth(U[:20], Y[:20])
