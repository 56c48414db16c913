"""Banks of unscented Kalman filters on the device (llpf_ukf_bank_*; kernels/ukf.hpp, host/ukf.hpp): the GPU reproduces the host build of
csrc/shared/llpf_ukf.h (tests/ukf_host.c around the oracle's model functions) bit for bit — precompiled and run-time compiled models,
whatever the bank, the chunking of T or the split of a run — and the Python API (UnscentedKalmanFilter, UnscentedKalmanFilterBank) is
the filter the CPU tests pin down."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi
import kalman_common as kc
from kalman_common import _same
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS, lg_models, quadtank_models, with_id
import models as M
import ukf_common as uc
import user_models as UM

pytestmark = pytest.mark.gpu
W1 = uc.merwe(2, 1.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return uc.build_host(tmp_path_factory.mktemp("ukf_host"))


def _bank(models, w):
    return _capi.UkfBankHandle(0, list(models), w)


def _family(w):
    """the unscented bank with the weights w"""
    return kg.Family("ukf", lambda models: _bank(models, w), lambda host, models, U, Y, T, **kw: uc.host_run(host, models, w, U, Y, T, **kw),
                     lg_models, True)


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_header_for_every_precompiled_shape(host, nx):
    """F = 1000 random filters, T = 200, every output, the three alpha = 1 weight sets and the small-alpha one in turn; shared and
    per-filter inputs give the same bits"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        fam = _family((uc.merwe_set(nx, uc.ALPHA1_SETS[(nx + ny) % 3]), uc.merwe(nx, *uc.SMALL_ALPHA))[ny == 4])
        b, g, _, _, U, Y = kg.check_shape(fam, host, rng, F=1000, T=200, nx=nx, ny=ny, nu=nu, missing=(50, 51, 120), what=(nx, ny))
        assert np.isfinite(g["ll"]).all()
        kg.check_broadcast_inputs(fam, b, g, U, Y, F=1000, nu=nu, what=(nx, ny, "per-filter"))
        b.close()


def test_each_output_alone(host):
    """every optional output asked for on its own is the column of the run with all of them: F = 65 (a full workgroup and a ragged one)"""
    kg.check_each_output_alone(_family(W1), host, seed=77, F=65, T=3, nx=2, ny=1, nu=1)


def test_quadtank_across_the_switch_time(host):
    """the built-in quad-tank with per-filter parameters over T = 700 from t_index0 = 1 (tau crosses TSWITCH = 500; three chunks), three
    missing rows: the device's RK4 in the oracle's order"""
    F, T = 65, 700
    models = quadtank_models(F)
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
        kg.check_shape(_family(uc.merwe(nx, 1.0, 0.0, 1.0)), host, rng, F=130, T=60, nx=nx, ny=ny, nu=nu, missing=(7,),
                       what=("LG", nx, ny))
    # the quad-tank as a snippet
    qid = _capi.model_compile(UM.QUADTANK_SRC, 4, 2)
    models = quadtank_models(70)
    U, Y = M.quadtank_data(520)
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    g = _bank([with_id(m, qid) for m in models], w).run(U, Y, outputs=OUTS, t_index0=1.0)
    gb = _bank(models, w).run(U, Y, outputs=OUTS, t_index0=1.0)
    _same(g, gb, what="quad-tank snippet vs built-in")
    h, _ = uc.host_run(host, models, w, U, Y, 520, t_index0=1.0)
    _same(g, h, what="quad-tank snippet vs host")
    # the pendulum: per-filter parameters, every weight set of the CPU test
    pid = _capi.model_compile(UM.PENDULUM_SRC, 2, 1)
    pend = kg.pendulum_models(100)
    U, Y = uc.pendulum_data(300)
    Y = Y.copy()
    Y[[3, 256], 0] = np.nan
    for w in (uc.merwe(2, 1.0, 0.0, 1.0), uc.merwe(2, 1.0, 0.0, 0.0), uc.merwe(2, *uc.SMALL_ALPHA)):
        g = _bank([with_id(m, pid) for m in pend], w).run(U, Y, outputs=OUTS)
        h, _ = uc.host_run(host, pend, w, U, Y, 300, twin=uc.TWIN_PENDULUM)
        _same(g, h, what=("pendulum", w))
        assert np.isfinite(g["ll"]).all()
    # f(x) = x, g(x) = x0^2: as a snippet and as a traced Python callable
    sq = kg.square_models(64)
    Y = 3.0 + 0.5 * rng.standard_normal((80, 1))
    w = uc.merwe(1, 1.0, 0.0, 1.0)
    h, _ = uc.host_run(host, sq, w, None, Y, 80, twin=uc.TWIN_SQUARE)
    sid = _capi.model_compile(uc.SQUARE_SRC, 1, 1)
    g = _bank([with_id(m, sid) for m in sq], w).run(None, Y, outputs=OUTS)
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
    kg.check_bank_sizes_and_chunk_edges(_family(W1), host, seed=100 + F, F=F, nx=2, ny=1, nu=1, missing=(0, 255, 256, 699),
                                        Ts=(1, 255, 256, 257, 700))


def test_continuation_set_models_set_weights_and_state(host):
    rng, b, U, Y = kg.check_continuation(_family(uc.merwe(3, 1.0, 0.0, 0.0)), host, seed=5, F=300, T=600, nx=3, ny=2, nu=2,
                                        missing=(255, 256, 500), cut=300)
    # set_models / set_weights = a fresh bank
    other = lg_models(rng, 300, 3, 2, 2)
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
        b.set_models(lg_models(rng, 300, 2, 2, 2))
    with pytest.raises(_capi.LLPFError):
        b.set_weights((1.0, 0.0, 0.0, -1.0))


def test_per_filter_inputs_missing_rows_and_a_nan_filter_beside_healthy_ones(host):
    kg.check_per_filter_inputs_and_a_nan_filter(_family(W1), host, seed=6, F=130, T=40, nx=2, ny=1, nu=1, missing=(5, 6, 30), stride=7, row=11,
                                                nan_filter=77)


def test_python_api_from_filter_bank_equals_a_loop_of_single_filters(host):
    specs = kg.quadtank_specs(6)
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
    _, U, Y = M.simulate_lg(M.lg_c1_model(0), 200)
    pf = llpf_amd.FilterBank(1000, kg.c1_specs(16), rng=1)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf).loglik(U, Y)
    for wp in (None, llpf_amd.MerweParams(1.0, 0.0, 1.0), llpf_amd.WikiParams(1.0, 0.0, 1.0)):
        ub = llpf_amd.UnscentedKalmanFilterBank.from_filter_bank(pf, weight_params=wp).loglik(U, Y)
        assert np.all(np.abs(ub - kb) <= 1e-10 * np.abs(kb)), (wp, np.max(np.abs(ub - kb) / np.abs(kb)))
