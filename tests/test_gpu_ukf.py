"""Banks of unscented Kalman filters on the device (llpf_ukf_bank_*; kernels/ukf.hpp, host/ukf.hpp): the GPU reproduces the host build of
csrc/shared/llpf_ukf.h (tests/ukf_host.c around the oracle's model functions) bit for bit — precompiled and run-time compiled models,
whatever the bank, the chunking of T or the split of a run — and the Python API (UnscentedKalmanFilter, UnscentedKalmanFilterBank) is
the filter the CPU tests pin down."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import kalman_common as kc
from kalman_common import _data, _same
import models as M
import ukf_common as uc
import user_models as UM

pytestmark = pytest.mark.gpu
OUTS = ("ll_steps", "x", "xt", "R", "Rt", "e")
W1 = uc.merwe(2, 1.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return uc.build_host(tmp_path_factory.mktemp("ukf_host"))


def _bank(models, w):
    return _capi.UkfBankHandle(0, list(models), w)


def _with_id(m, model_id):
    c = S.Model.from_buffer_copy(bytes(m))
    c.model_id = model_id
    return c


def _lg_models(rng, F, nx, ny, nu):
    return [kc.random_system(rng, nx, ny, nu, k % 3, D=False)[0] for k in range(F)]


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_header_for_every_precompiled_shape(host, nx):
    """F = 1000 random filters, T = 200, every output, the three alpha = 1 weight sets and the small-alpha one in turn; shared and
    per-filter inputs give the same bits"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        models = _lg_models(rng, 1000, nx, ny, nu)
        U, Y = _data(rng, 200, nu, ny, missing=(50, 51, 120))
        w = (uc.merwe_set(nx, uc.ALPHA1_SETS[(nx + ny) % 3]), uc.merwe(nx, *uc.SMALL_ALPHA))[ny == 4]
        b = _bank(models, w)
        g = b.run(U, Y, outputs=OUTS)
        h, _ = uc.host_run(host, models, w, U, Y, 200)
        _same(g, h, what=(nx, ny))
        assert np.isfinite(g["ll"]).all()
        b.reset()
        gp = b.run(np.broadcast_to(U, (1000,) + U.shape), np.broadcast_to(Y, (1000,) + Y.shape), u_per_filter=nu > 0, y_per_filter=True, outputs=OUTS)
        _same(gp, g, what=(nx, ny, "per-filter"))
        b.close()


def _quadtank_models(F):
    base = M.quadtank_model()
    out = []
    for k in range(F):
        out.append(S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, 2,
                                         gamma1=0.2 + 0.001 * (k % 50), a1=0.03 + 0.0001 * (k % 7)))
    return out


def test_quadtank_across_the_switch_time(host):
    """the built-in quad-tank with per-filter parameters over T = 700 from t_index0 = 1 (tau crosses TSWITCH = 500; three chunks), three
    missing rows: the device's RK4 in the oracle's order"""
    F, T = 65, 700
    models = _quadtank_models(F)
    U, Y = M.quadtank_data(T)
    Y = Y.copy()
    Y[[5, 256, 600], 0] = np.nan
    for w in (uc.merwe(4, 1.0, 0.0, 1.0), uc.merwe(4, 1.0, 0.0, -1.0)):
        g = _bank(models, w).run(U, Y, outputs=OUTS, t_index0=1.0)
        h, _ = uc.host_run(host, models, w, U, Y, T, t_index0=1.0)
        _same(g, h, what="quad-tank")
        assert np.isfinite(g["ll"]).all() and len(set(g["ll"].tolist())) > 40


def test_runtime_compiled_shapes(host):
    """k_ukf from a hiprtc program of the model's own: the linear-Gaussian model above 4 states, the quad-tank as a snippet (the built-in
    quad-tank's bits), the pendulum, the x0^2 model as a snippet and as a traced Python callable"""
    rng = np.random.default_rng(21)
    for nx, ny, nu in ((6, 3, 2), (8, 4, 1), (5, 1, 0)):
        models = _lg_models(rng, 130, nx, ny, nu)
        U, Y = _data(rng, 60, nu, ny, missing=(7,))
        w = uc.merwe(nx, 1.0, 0.0, 1.0)
        g = _bank(models, w).run(U, Y, outputs=OUTS)
        h, _ = uc.host_run(host, models, w, U, Y, 60)
        _same(g, h, what=("LG", nx, ny))
    # the quad-tank as a snippet
    qid = _capi.model_compile(UM.QUADTANK_SRC, 4, 2)
    models = _quadtank_models(70)
    U, Y = M.quadtank_data(520)
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    g = _bank([_with_id(m, qid) for m in models], w).run(U, Y, outputs=OUTS, t_index0=1.0)
    gb = _bank(models, w).run(U, Y, outputs=OUTS, t_index0=1.0)
    _same(g, gb, what="quad-tank snippet vs built-in")
    h, _ = uc.host_run(host, models, w, U, Y, 520, t_index0=1.0)
    _same(g, h, what="quad-tank snippet vs host")
    # the pendulum: per-filter parameters, every weight set of the CPU test
    pid = _capi.model_compile(UM.PENDULUM_SRC, 2, 1)
    pend = []
    for k in range(100):
        m = uc.pendulum_model()
        m.qt[0], m.qt[1] = 9.81 * (1 + 0.002 * k), 0.05 + 0.001 * (k % 10)
        pend.append(m)
    U, Y = uc.pendulum_data(300)
    Y = Y.copy()
    Y[[3, 256], 0] = np.nan
    for w in (uc.merwe(2, 1.0, 0.0, 1.0), uc.merwe(2, 1.0, 0.0, 0.0), uc.merwe(2, *uc.SMALL_ALPHA)):
        g = _bank([_with_id(m, pid) for m in pend], w).run(U, Y, outputs=OUTS)
        h, _ = uc.host_run(host, pend, w, U, Y, 300, twin=uc.TWIN_PENDULUM)
        _same(g, h, what=("pendulum", w))
        assert np.isfinite(g["ll"]).all()
    # f(x) = x, g(x) = x0^2: as a snippet and as a traced Python callable
    g_ = S.make_gaussian
    sq = [S.make_lg_model(np.eye(1), np.zeros((1, 0)), np.eye(1), g_(np.zeros(1), 0.1), g_(np.zeros(1), 0.25), g_(np.array([1.0 + 0.01 * k]), 0.36))
          for k in range(64)]
    Y = 3.0 + 0.5 * rng.standard_normal((80, 1))
    w = uc.merwe(1, 1.0, 0.0, 1.0)
    h, _ = uc.host_run(host, sq, w, None, Y, 80, twin=uc.TWIN_SQUARE)
    sid = _capi.model_compile(uc.SQUARE_SRC, 1, 1)
    g = _bank([_with_id(m, sid) for m in sq], w).run(None, Y, outputs=OUTS)
    _same(g, h, what="square snippet")
    ukf = llpf_amd.UnscentedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25,
                                         llpf_amd.MvNormal(np.array([1.0]), 0.36), nu=0, ny=1, weight_params=w)
    sol = llpf_amd.forward_trajectory(ukf, None, Y)
    for k, v in (("x", sol.x), ("xt", sol.xt), ("R", sol.R), ("Rt", sol.Rt), ("e", sol.e)):
        assert kc.bits_equal(v, h[k][:, 0]), ("traced callable", k)
    assert sol.ll == h["ll"][0]


@pytest.mark.parametrize("F", [1, 63, 64, 65, 1000])
def test_bank_sizes_and_chunk_edges(host, F):
    """per-filter parameters at every bank size around the wave, T around the 256-step chunk of the staging pipe"""
    rng = np.random.default_rng(100 + F)
    models = _lg_models(rng, F, 2, 1, 1)
    U, Y = _data(rng, 700, 1, 1, missing=(0, 255, 256, 699))
    b = _bank(models, W1)
    for T in (1, 255, 256, 257, 700):
        b.reset()
        g = b.run(U[:T], Y[:T], outputs=OUTS)
        h, st = uc.host_run(host, models, W1, U[:T], Y[:T], T)
        _same(g, h, what=(F, T))
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]), (F, T, "final state")


def test_continuation_set_models_set_weights_and_state(host):
    rng = np.random.default_rng(5)
    models = _lg_models(rng, 300, 3, 2, 2)
    U, Y = _data(rng, 600, 2, 2, missing=(255, 256, 500))
    W3 = uc.merwe(3, 1.0, 0.0, 0.0)
    b = _bank(models, W3)
    whole = b.run(U, Y, outputs=OUTS)
    b.reset()
    first = b.run(U[:300], Y[:300], outputs=OUTS)
    x, R = b.get_state()
    second = b.run(U[300:], Y[300:], outputs=OUTS, t_index0=300.0)
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    h2, _ = uc.host_run(host, models, W3, U[300:], Y[300:], 300, state=(x, R), t_index0=300.0)
    _same(second, h2, what="second half")
    fresh = _bank(models, W3)
    fresh.set_state(x, R)
    xs, Rs = fresh.get_state()
    assert kc.bits_equal(xs, x) and kc.bits_equal(np.tril(Rs), np.tril(R))
    again = fresh.run(U[300:], Y[300:], outputs=OUTS, t_index0=300.0)
    _same(again, second, what="set_state")
    b.reset()
    bare = b.run(U, Y)                                  # ll only: nothing is staged per step
    assert kc.bits_equal(bare["ll"], whole["ll"])
    # set_models / set_weights = a fresh bank
    other = _lg_models(rng, 300, 3, 2, 2)
    W2 = uc.merwe(3, 1.0, 0.0, 1.0)
    b.set_models(other)
    b.set_weights(W2)
    b.reset()
    g = b.run(U, Y, outputs=OUTS)
    f2 = _bank(other, W2).run(U, Y, outputs=OUTS)
    _same(g, f2, what="set_models + set_weights")
    h, _ = uc.host_run(host, other, W2, U, Y, 600)
    _same(g, h, what="set_models + set_weights vs host")
    with pytest.raises(_capi.LLPFError):
        b.set_models(_lg_models(rng, 300, 2, 2, 2))
    with pytest.raises(_capi.LLPFError):
        b.set_weights((1.0, 0.0, 0.0, -1.0))


def test_per_filter_inputs_missing_rows_and_a_nan_filter_beside_healthy_ones(host):
    rng = np.random.default_rng(6)
    models = _lg_models(rng, 130, 2, 1, 1)
    U = rng.standard_normal((130, 40, 1))
    Y = 2.0 * rng.standard_normal((130, 40, 1))
    Y[:, [5, 6, 30], 0] = np.nan
    Y[::7, 11, 0] = np.nan
    b = _bank(models, W1)
    x, R = b.get_state()
    ok = b.run(U, Y, True, True, outputs=OUTS)
    assert np.all(ok["ll_steps"][[5, 6, 30]] == 0.0) and np.all(np.isnan(ok["e"][[5, 6, 30]]))
    h, _ = uc.host_run(host, models, W1, U, Y, 40, per_filter=3)
    _same(ok, h, what="per-filter inputs")
    R[77] = -100.0 * np.eye(2)
    b.set_state(x, R)
    bad = b.run(U, Y, True, True, outputs=OUTS)
    assert np.isnan(bad["ll"][77]) and np.all(np.isnan(bad["xt"][:, 77])) and np.all(np.isnan(bad["R"][1:, 77]))
    assert np.all(bad["ll_steps"][[5, 6, 30], 77] == 0.0)
    keep = [f for f in range(130) if f != 77]
    for k in OUTS:
        assert kc.bits_equal(bad[k][:, keep], ok[k][:, keep]), k
    hb, _ = uc.host_run(host, models, W1, U, Y, 40, per_filter=3, state=(x, R))
    _same(bad, hb, what="NaN filter")


def _quadtank_specs(n):
    specs = []
    for k in range(n):
        specs.append((llpf_amd.QuadTankDynamics(supersample=2, gamma1=0.2 + 0.01 * k), llpf_amd.QuadTankMeasurement(),
                      llpf_amd.MvNormal(np.zeros(4), np.full(4, 0.1)), llpf_amd.MvNormal(np.zeros(2), np.full(2, 1e-4)),
                      llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1))))
    return specs


def test_python_api_from_filter_bank_equals_a_loop_of_single_filters(host):
    specs = _quadtank_specs(6)
    U, Y = M.quadtank_data(300)
    pf = llpf_amd.FilterBank(1000, specs, rng=3)
    ub = llpf_amd.UnscentedKalmanFilterBank.from_filter_bank(pf)
    ll = ub.loglik(U, Y)
    assert ll.shape == (6,) and np.isfinite(ll).all() and len(set(ll.tolist())) == 6
    for k, (dy, me, df, dg, d0) in enumerate(specs):
        one = llpf_amd.UnscentedKalmanFilter(dy, me, np.full(4, 0.1), np.full(2, 1e-4), d0)
        assert llpf_amd.loglik(one, U, Y) == ll[k], k
    # the bank built from the same specs directly, and the host header with the default weights
    ub2 = llpf_amd.UnscentedKalmanFilterBank([(dy, me, np.full(4, 0.1), np.full(2, 1e-4), d0) for dy, me, df, dg, d0 in specs])
    assert kc.bits_equal(ub2.loglik(U, Y), ll)
    h, _ = uc.host_run(host, list(pf._models), llpf_amd.TrivialParams().weights(4), U, Y, 300, t_index0=1.0)
    assert kc.bits_equal(h["ll"], ll)
    fw = ub.forward(U, Y)
    assert fw["x"].shape == (300, 6, 4) and fw["Rt"].shape == (300, 6, 4, 4) and ub.state()[0].shape == (6, 4)
    # the stepping verbs of one filter: update = correct then predict, all through the device
    one = llpf_amd.UnscentedKalmanFilter(specs[0][0], specs[0][1], np.full(4, 0.1), np.full(2, 1e-4), specs[0][4], weight_params=llpf_amd.MerweParams(1.0, 0.0, 1.0))
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
    assert abs(sum(lls) - sol.ll) <= 1e-12 * abs(sol.ll)
    x_end = one.x
    llpf_amd.forward_trajectory(one, U[:20], Y[:20])
    assert kc.bits_equal(one.x, x_end), "correct + predict is update, bit for bit"


def test_ukf_bank_on_the_linear_c1_model_is_the_kalman_bank():
    """the statistical tie to the rest of the project: on the linear-Gaussian C1 model the UKF bank's log-likelihood equals
    KalmanFilterBank's to 1e-10 relative, on the device"""
    specs = []
    for k in range(16):
        model = M.lg_c1_model(seed=k)
        mt = kc.matrices(model, np.zeros((2, 2)))
        specs.append((llpf_amd.LinearDynamics(mt["A"], mt["B"]), llpf_amd.LinearMeasurement(mt["C"]), llpf_amd.MvNormal(np.zeros(2), mt["R1"]),
                      llpf_amd.MvNormal(np.zeros(2), mt["R2"]), llpf_amd.MvNormal(mt["x0"], mt["P0"])))
    _, U, Y = M.simulate_lg(M.lg_c1_model(0), 200)
    pf = llpf_amd.FilterBank(1000, specs, rng=1)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf).loglik(U, Y)
    for wp in (None, llpf_amd.MerweParams(1.0, 0.0, 1.0), llpf_amd.WikiParams(1.0, 0.0, 1.0)):
        ub = llpf_amd.UnscentedKalmanFilterBank.from_filter_bank(pf, weight_params=wp).loglik(U, Y)
        assert np.all(np.abs(ub - kb) <= 1e-10 * np.abs(kb)), (wp, np.max(np.abs(ub - kb) / np.abs(kb)))
