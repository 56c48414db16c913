"""Banks of IMM filters over unscented Kalman filter modes on the device (llpf_imm_bank_create_unscented and the shared llpf_imm_bank_*
verbs; kernels/imm_ukf.hpp, host/imm.hpp): the GPU reproduces the host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_ukf.h
(tests/imm_ukf_host.c) bit for bit — precompiled and run-time compiled models (the mapped points in registers and, from 5 states, in
LDS), whatever the number of modes, the weights, the bank, the chunking of T or the split of a run — it is the unscented Kalman bank
where it must be, and the Python API (IMM, IMMBank over UnscentedKalmanFilter) is that bank.  The bodies are those of imm_gpu_frame.py,
which this file runs on an unscented bank by binding the frame's `ic` to imm_ukf_common.Bound(weights, twin)."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi
import imm_common as ic
from imm_common import OUTS
import imm_gpu_frame as ig
import imm_ukf_common as iu
import kalman_common as kc
from kalman_common import _data
from gpu_common import _Inject
import kf_gpu_frame as kg
import models as M
import ukf_common as uc
import user_models as UM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return iu.build_host(tmp_path_factory.mktemp("imm_ukf_host"))


@pytest.fixture
def bind(monkeypatch):
    """bind(w, twin = 0): imm_gpu_frame's bodies run on unscented banks with the weights w, against imm_ukf_host_run with that twin"""
    def use(w, twin=0):
        b = iu.Bound(w, twin)
        monkeypatch.setattr(ig, "ic", b)
        return b
    return use


def _check(b, g, h, st, what):
    """every output and ll of a run `g` of bank `b` against the twin's `h`, and the bank's final (mu, x_modes, R_modes) against `st`"""
    iu.same(g, h, what=what)
    ig.same_final(b, st, what)


def _quadtank_imms(rng, F, M):
    return ic.grouped(kg.quadtank_models(F * M), rng, F, M)


def _pendulum_imms(rng, F, M):
    return ic.grouped(kg.pendulum_models(F * M), rng, F, M)


def _quadtank(t0):
    """the built-in quad-tank (its own shape) in runs from t_index0 = t0"""
    return ig.ImmFamily(lambda rng, F, M, nx=4, ny=2, nu=2: _quadtank_imms(rng, F, M), t0)


LG = ig.ImmFamily(ic.lg_imms, 0.0)


@pytest.mark.parametrize("shape", iu.SHAPES)
def test_lingauss_bit_identical_to_the_host_headers_for_the_precompiled_shapes(host, bind, shape):
    """a. LinGauss<nx, ny> at (1, 1, 0), (2, 1, 1), (3, 2, 1), (4, 4, 2) x M in 1..4: F = 70 (a ragged last workgroup at every G, an idle
    lane in every quad at M = 3), T = 40 with rows 5, 6 and 39 missing, interact on and off, TrivialParams and Merwe (1, 0, 1): every
    output, ll and the final state, get_state's combined estimate, the shared inputs handed per filter, per-filter inputs whose missing
    rows differ inside a wave.  The frame's isfinite(ll) is what test_imm_ukf.py asserts of the twin on these cases (the same seeds)."""
    nx, ny, nu = shape
    for Mo in range(1, 5):
        for wi, w in enumerate(iu.shape_weights(nx)):
            bind(w)
            ig.check_shape(LG, host, iu.shape_rng(nx, ny, nu, Mo, wi), F=iu.SHAPE_F, T=iu.SHAPE_T, M=Mo, nx=nx, ny=ny, nu=nu,
                           missing=iu.SHAPE_MISSING, what=(nx, ny, nu, Mo, wi))


def test_quadtank_modes_across_the_switch_time(host):
    """b. the built-in quad-tank, per-filter parameters (gamma1, a1), M = 3 (an idle lane per group), F = 70, T = 60 from
    t_index0 = 470 (tau crosses TSWITCH = 500, a branch of the model per lane) with a missing row"""
    rng = np.random.default_rng(23)
    imms = _quadtank_imms(rng, 70, 3)
    U, Y = M.quadtank_data(60)
    Y = Y.copy()
    Y[31, 0] = np.nan
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    for interact in (True, False):
        b = iu.bank(imms, w, interact)
        g = b.run(U, Y, outputs=OUTS, t_index0=470.0)
        h, st = iu.host_run(host, imms, w, U, Y, 60, t_index0=470.0, interact=interact)
        _check(b, g, h, st, ("quad-tank", interact))
        assert len(set(g["ll"].tolist())) > 40
        b.reset()
        assert not kc.bits_equal(b.run(U, Y, t_index0=0.0)["ll"], g["ll"])
        b.close()


def test_runtime_compiled_linear_models_with_their_points_in_lds(host):
    """c1. k_imm_ukf from a hiprtc program of the model's own, the mapped points [point][d][lane] in LDS: the linear-Gaussian model at
    (5, 1, 0), M = 2 and M = 4, and at (8, 4, 1), M = 4, F = 20 (the largest footprint, 17 points x 8 doubles x 64 lanes)"""
    rng = np.random.default_rng(31)
    for (nx, ny, nu), Mo, F in (((5, 1, 0), 2, 70), ((5, 1, 0), 4, 70), ((8, 4, 1), 4, 20)):
        w = uc.merwe(nx, 1.0, 0.0, 1.0)
        lg = ic.lg_imms(rng, F, Mo, nx, ny, nu)
        Ul, Yl = _data(rng, 40, nu, ny, missing=(7,))
        b = iu.bank(lg, w)
        g = b.run(Ul, Yl, outputs=OUTS)
        h, st = iu.host_run(host, lg, w, Ul, Yl, 40)
        _check(b, g, h, st, ("LG", nx, ny, nu, Mo))


def test_runtime_compiled_snippets_and_traced_callables(host):
    """c2. the pendulum snippet without Jacobian members (M = 3, an idle lane); x0^2 (M = 2); the quad-tank as a snippet against the
    built-in model's bits; callables traced without Jacobians through llpf_amd.IMM against the twin's column"""
    rng = np.random.default_rng(32)
    F = 70
    assert "dynamics_jac" not in UM.PENDULUM_SRC and "measurement_jac" not in UM.PENDULUM_SRC
    pid = _capi.model_compile(UM.PENDULUM_SRC, 2, 1)
    pend = _pendulum_imms(rng, F, 3)
    U, Y = uc.pendulum_data(80)
    Y = Y.copy()
    Y[[3, 40], 0] = np.nan
    w = uc.merwe(2, 1.0, 0.0, 1.0)
    b = iu.bank(ic.with_id(pend, pid), w)
    g = b.run(U, Y, outputs=OUTS)
    h, st = iu.host_run(host, pend, w, U, Y, 80, twin=uc.TWIN_PENDULUM)
    _check(b, g, h, st, "pendulum snippet")
    sid = _capi.model_compile(uc.SQUARE_SRC, 1, 1)
    sq = ic.grouped(kg.square_models(2 * F), rng, F, 2)
    Ys = 3.0 + 0.5 * rng.standard_normal((60, 1))
    w1 = uc.merwe(1, 1.0, 0.0, 1.0)
    b = iu.bank(ic.with_id(sq, sid), w1)
    g = b.run(None, Ys, outputs=OUTS)
    h, st = iu.host_run(host, sq, w1, None, Ys, 60, twin=uc.TWIN_SQUARE)
    _check(b, g, h, st, "square snippet")
    # the quad-tank as a snippet: the built-in model's bits
    qid = _capi.model_compile(UM.QUADTANK_SRC, 4, 2)
    qt = _quadtank_imms(rng, F, 3)
    Uq, Yq = M.quadtank_data(50)
    w4 = uc.merwe(4, 1.0, 0.0, 1.0)
    gb = iu.bank(qt, w4).run(Uq, Yq, outputs=OUTS, t_index0=480.0)
    gs = iu.bank(ic.with_id(qt, qid), w4).run(Uq, Yq, outputs=OUTS, t_index0=480.0)
    iu.same(gs, gb, what="quad-tank snippet against the built-in model")
    # traced callables (no Jacobians): x0^2 against the twin's column
    two = kg.square_models(2)
    P, mu = [[0.9, 0.1], [0.2, 0.8]], [0.6, 0.4]
    traced = llpf_amd.IMM([llpf_amd.UnscentedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25,
                                                          llpf_amd.MvNormal(np.array([1.0 + 0.01 * j]), 0.36), nu=0, ny=1, weight_params=w1)
                           for j in range(2)], P, mu)
    assert traced.unscented and not traced.extended
    sol = llpf_amd.forward_trajectory(traced, None, Ys)
    ht, _ = iu.host_run(host, [ic.imm(two, P=P, mu0=mu)], w1, None, Ys, 60, twin=uc.TWIN_SQUARE)
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        assert kc.bits_equal(getattr(sol, k), ht[k][:, 0]), ("traced", k)
    assert sol.ll == ht["ll"][0]


@pytest.mark.parametrize("Mo,F", [(2, 1), (2, 31), (2, 32), (2, 33), (4, 1), (4, 15), (4, 16), (4, 17)])
def test_bank_sizes_and_chunk_edges(host, Mo, F):
    """d. banks around the wave at M = 2 (32 groups of two lanes) and M = 4 (16 quads), T around the 256-step chunk of the staging pipe,
    from a reset each time: the outputs and the final state"""
    rng = np.random.default_rng(400 + 10 * F + Mo)
    imms = ic.lg_imms(rng, F, Mo, 2, 1, 1)
    U, Y = _data(rng, 257, 1, 1, missing=(0, 255, 256))
    w = uc.merwe(2, 1.0, 0.0, 1.0)
    b = iu.bank(imms, w)
    for T in (1, 255, 256, 257):
        b.reset()
        g = b.run(U[:T], Y[:T], outputs=OUTS)
        h, st = iu.host_run(host, imms, w, U[:T], Y[:T], T)
        _check(b, g, h, st, (F, Mo, T))
    b.close()


def test_continuation_state_and_new_parameters(host, bind):
    """e. on the quad-tank: run_at(a, t0) then run_at(b, t0 + len(a)) is run_at(a + b, t0), cut at 100 of T = 300; the second half
    against the twin from the state between; set_state on a fresh bank; ll alone.  set_models + set_weights + reset is a fresh bank
    of the new models and weights."""
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    bind(w)
    fam = _quadtank(250.0)
    rng = np.random.default_rng(5)
    imms = fam.imms(rng, 70, 3)
    U, Y = M.quadtank_data(300)
    Y = Y.copy()
    Y[[10, 100, 260], 0] = np.nan
    ig.check_continuation(fam, host, imms, U, Y, cut=100)
    new, w2 = ic.grouped(kg.quadtank_models(210)[::-1], rng, 70, 3), tuple(float(v) for v in llpf_amd.TrivialParams().weights(4))
    U, Y = U[:40], Y[:40]
    b = iu.bank(imms, w)
    b.run(U, Y, t_index0=1.0)
    b.set_models(*iu.bank_args(new))
    b.set_weights(w2)
    b.reset()
    g = b.run(U, Y, outputs=OUTS, t_index0=1.0)
    iu.same(g, iu.bank(new, w2).run(U, Y, outputs=OUTS, t_index0=1.0), what="set_models + set_weights")
    h, st = iu.host_run(host, new, w2, U, Y, 40, t_index0=1.0)
    _check(b, g, h, st, "set_models + set_weights against the twin")
    with pytest.raises(_capi.LLPFError):
        b.set_models(*iu.bank_args(ic.lg_imms(rng, 70, 3, 4, 2, 2)))
    with pytest.raises(_capi.LLPFError, match="D must be NULL"):
        b.set_models(iu.bank_args(new)[0], np.zeros((70, 3, 2, 2)), *iu.bank_args(new)[2:])


@pytest.mark.parametrize("interact", [True, False])
def test_a_nan_imm_stays_home(host, bind, interact):
    """f. one mode of one IMM starts from an indefinite covariance: its IMM is NaN from that step on (0 at missing rows), every other
    filter's bits are unmoved, and all are the twin's"""
    bind(uc.merwe(4, 1.0, 0.0, 1.0))
    fam = _quadtank(1.0)
    imms = fam.imms(np.random.default_rng(6), 70, 3)
    U, Y = M.quadtank_data(30)
    Y = Y.copy()
    Y[[5, 6, 20], 0] = np.nan
    ig.check_a_nan_imm(fam, host, imms, U, Y, interact=interact, missing=(5, 6, 20), nan_filter=13, nan_mode=1)


def test_a_mode_without_mass(host, bind):
    """g. P = I and a mu0 with a zero: that mode's probability is exactly 0 throughout and ll is finite; the twin's bits"""
    bind(uc.merwe(4, 1.0, 0.0, 1.0))
    fam = _quadtank(1.0)
    imms = fam.imms(np.random.default_rng(7), 70, 3)
    U, Y = M.quadtank_data(30)
    ig.check_a_mode_without_mass(fam, host, imms, U, Y, mu0=[0.5, 0.0, 0.5])


def test_one_mode_is_the_unscented_kalman_bank():
    """h. M = 1 is UnscentedKalmanFilterBank's handle over the same descriptors and weights on the device, bit for bit (ll, ll_steps, x,
    xt, R, Rt): the quad-tank and the pendulum snippet"""
    F = 70
    pid = _capi.model_compile(UM.PENDULUM_SRC, 2, 1)
    Uq, Yq = M.quadtank_data(60)
    Up, Yp = uc.pendulum_data(60)
    for what, models, U, Y, t0 in (("quad-tank", kg.quadtank_models(F), Uq, Yq, 470.0), ("pendulum", [kg.with_id(m, pid) for m in kg.pendulum_models(F)], Up, Yp, 0.0)):
        Y = Y.copy()
        Y[[4, 30], 0] = np.nan
        w = uc.merwe(models[0].nx, 1.0, 0.0, 1.0)
        g = iu.bank([ic.imm([m], P=[[1.0]], mu0=[1.0]) for m in models], w).run(U, Y, outputs=OUTS, t_index0=t0)
        e = _capi.UkfBankHandle(0, list(models), w).run(U, Y, outputs=kg.OUTS, t_index0=t0)
        for k in ("x", "xt", "R", "Rt", "ll_steps", "ll"):
            assert kc.bits_equal(g[k], e[k]), (what, k)
        assert np.all(g["mu"] == 1.0)


def test_a_throw_is_a_status(host):
    """i. a throw at error:imm_run is a status that leaves the state, and the handle runs on"""
    rng = np.random.default_rng(8)
    imms = _quadtank_imms(rng, 70, 2)
    U, Y = M.quadtank_data(40)
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    b = iu.bank(imms, w)
    g = b.run(U, Y, outputs=OUTS, t_index0=1.0)
    b.reset()
    before = ig.final(b)
    with _Inject("error:imm_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y, t_index0=1.0)
    assert ei.value.code == _capi.ERR_INTERNAL and "imm_run" in str(ei.value)
    for a, s in zip(ig.final(b), before):
        assert kc.bits_equal(a, s)
    iu.same(b.run(U, Y, outputs=OUTS, t_index0=1.0), g, what="after the throw")


def _ukf_qt(g1, a1, w):
    """a quad-tank mode whose outlet switches at t = 20: inside the 40 steps of the test below, so that the time of a step shows"""
    return llpf_amd.UnscentedKalmanFilter(llpf_amd.QuadTankDynamics(supersample=2, gamma1=g1, a1=a1, t_switch=20.0), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1),
                                          np.full(2, 1e-4), llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)), weight_params=w)


def test_the_python_api(host):
    """j. forward_trajectory(imm) is an IMMFilteringSolution with mu and ll_modes, loglik starts at t = 1 * Ts and forward_trajectory at 0,
    update twice is a two-step run and advances the step counter, IMMBank rows equal the single filters bit for bit"""
    rng = np.random.default_rng(9)
    U, Y = M.quadtank_data(40)
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    modes = [_ukf_qt(0.2, 0.03, w), _ukf_qt(0.3, 0.036, w), _ukf_qt(0.25, 0.03, w)]
    P, mu0 = ic.random_P(rng, 3), ic.random_mu(rng, 3)
    imm = llpf_amd.IMM(modes, P, mu0)
    assert imm._handle is None and imm.unscented and not imm.extended
    T = 40
    sol = llpf_amd.forward_trajectory(imm, U, Y)
    assert isinstance(sol, llpf_amd.IMMFilteringSolution) and sol.x.shape == (T, 4) and sol.Rt.shape == (T, 4, 4) and sol.mu.shape == (T, 3)
    assert sol.ll_modes.shape == (T, 3) and sol.e is None and np.isscalar(sol.ll)
    spec = [ic.imm([f._model for f in modes], P=P, mu0=mu0)]
    h0, _ = iu.host_run(host, spec, w, U, Y, T, t_index0=0.0)
    h1, _ = iu.host_run(host, spec, w, U, Y, T, t_index0=1.0)
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        assert kc.bits_equal(getattr(sol, k), h0[k][:, 0]), k
    assert sol.ll == h0["ll"][0] and llpf_amd.loglik(imm, U, Y) == h1["ll"][0] and h0["ll"][0] != h1["ll"][0]
    llpf_amd.reset(imm)
    assert kc.bits_equal(imm.mu, mu0) and imm._index == 1
    lls = [llpf_amd.update(imm, U[t], Y[t])[0] for t in range(2)]          # step t at (1 + t) Ts: loglik's times
    assert kc.bits_equal(np.array(lls), h1["ll_steps"][:2, 0]) and imm._index == 3
    h2, st2 = iu.host_run(host, spec, w, U[:2], Y[:2], 2, t_index0=1.0)
    assert kc.bits_equal(imm.mu, st2[0][0]) and kc.bits_equal(imm.x, iu.host_combine(host, *st2)[0][0])
    assert np.allclose(llpf_amd.state(imm), imm.x) and llpf_amd.covariance(imm).shape == (4, 4) and abs(imm.mu.sum() - 1.0) <= 1e-12
    others = [llpf_amd.IMM(modes[::-1], P.T / P.T.sum(axis=1, keepdims=True), mu0[::-1]), llpf_amd.IMM(modes[1:] + modes[:1], P, mu0)]
    bank = llpf_amd.IMMBank([imm] + others)
    assert bank.unscented and not bank.extended
    ll = bank.loglik(U, Y)
    fw = bank.forward(U, Y)
    for k, f in enumerate([imm] + others):
        assert ll[k] == llpf_amd.loglik(f, U, Y), k
        one = llpf_amd.forward_trajectory(f, U, Y)
        for name in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
            assert kc.bits_equal(fw[name][:, k], getattr(one, name)), (k, name)
    x, R, mu = bank.state()
    assert x.shape == (3, 4) and R.shape == (3, 4, 4) and mu.shape == (3, 3)
    bank.set_parameters([others[0]] * 3)
    ll2 = bank.loglik(U, Y)
    assert ll2[0] == ll2[1] == ll2[2] == ll[1]
    with pytest.raises(TypeError, match="no smoother"):
        bank.smooth(U, Y)
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(imm, U, Y)
