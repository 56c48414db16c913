"""Banks of IMM filters over extended Kalman filter modes on the device (llpf_imm_bank_* with LLPF_IMM_EXTENDED; kernels/imm_ekf.hpp,
host/imm.hpp): the GPU reproduces the host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_ekf.h (tests/imm_ekf_host.c) bit for bit
— precompiled and run-time compiled models, whatever the number of modes, the bank, the chunking of T or the split of a run — it is the
extended Kalman bank where it must be, and the Python API (IMM, IMMBank over ExtendedKalmanFilter) is that bank.  The bodies this file shares
with test_gpu_imm.py are in imm_gpu_frame.py."""
import ctypes as C

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import imm_common as ic
from imm_common import OUTS
import imm_gpu_frame as ig
import kalman_common as kc
from kalman_common import _data
from gpu_common import _Inject
import kf_gpu_frame as kg
import models as M
import ukf_common as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ic.build_host(tmp_path_factory.mktemp("imm_ekf_host"))


def _check(b, g, h, st, what):
    """every output and ll of a run `g` of bank `b` against the twin's `h`, and the bank's final (mu, x_modes, R_modes) against `st`"""
    ic.same(g, h, what=what)
    ig.same_final(b, st, what)


def _quadtank_imms(rng, F, M):
    return ic.grouped(kg.quadtank_models(F * M), rng, F, M)


def _pendulum_imms(rng, F, M):
    return ic.grouped(kg.pendulum_models(F * M), rng, F, M)


LG = ig.ImmFamily(ic.lg_imms, None)


def _quadtank(t0):
    """the built-in quad-tank (its own shape) in runs from t_index0 = t0"""
    return ig.ImmFamily(lambda rng, F, M, nx=4, ny=2, nu=2: _quadtank_imms(rng, F, M), t0)


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_headers_for_every_precompiled_shape(host, nx):
    """1. LLPF_IMM_EXTENDED over LinGauss<nx, ny>, ny and M in 1..4: F = 70 (a ragged last wave at every G, two workgroups at G = 4),
    T = 40 with missing rows, interact on and off; shared inputs, the same handed per filter, per-filter inputs of their own whose missing
    rows differ inside a wave; get_state's combined estimate; mu a distribution"""
    for ny in range(1, 5):
        for Mo in range(1, 5):
            rng = np.random.default_rng(1000 * Mo + 10 * nx + ny)
            nu = int(rng.integers(0, 3))
            ig.check_shape(LG, host, rng, F=70, T=40, M=Mo, nx=nx, ny=ny, nu=nu, missing=(5, 6, 30), what=(nx, ny, Mo))


def _run_c(b, U, Y, outputs):
    """llpf_imm_bank_run itself (the handle's run goes through llpf_imm_bank_run_at)"""
    U, Y, T, _ = b._inputs(U, Y, False, False)
    shapes = {"ll_steps": (T, b.F), "x": (T, b.F, b.nx), "xt": (T, b.F, b.nx), "R": (T, b.F, b.nx, b.nx), "Rt": (T, b.F, b.nx, b.nx),
              "mu": (T, b.F, b.M), "ll_modes": (T, b.F, b.M)}
    res = {k: np.empty(shapes[k]) for k in outputs}
    out = S.ImmOutputs()
    out.struct_size = C.sizeof(S.ImmOutputs)
    for k, a in res.items():
        setattr(out, k, _capi.dptr(a))
    res["ll"] = np.empty(b.F)
    _capi.check(_capi.lib().llpf_imm_bank_run(b.h, _capi.dptr(U), _capi.dptr(Y), T, 0, _capi.dptr(res["ll"]), C.byref(out)))
    return res


@pytest.mark.parametrize("Mo", [2, 3])
def test_quadtank_modes_across_the_switch_time(host, Mo):
    """2. the built-in quad-tank, modes that differ in gamma1 / a1, M = 2 and M = 3 (an idle lane per group), F = 70, T = 60 from
    t_index0 = 470 (tau crosses TSWITCH = 500, a branch of the model per lane); run is run_at(0.0)"""
    rng = np.random.default_rng(20 + Mo)
    imms = _quadtank_imms(rng, 70, Mo)
    U, Y = M.quadtank_data(60)
    Y = Y.copy()
    Y[[5, 31, 32], 0] = np.nan
    for interact in (True, False):
        b = ic.bank(imms, interact)
        g = b.run(U, Y, outputs=OUTS, t_index0=470.0)
        h, st = ic.host_run(host, imms, U, Y, 60, t_index0=470.0, interact=interact)
        _check(b, g, h, st, ("quad-tank", Mo, interact))
        assert np.isfinite(g["ll"]).all() and len(set(g["ll"].tolist())) > 40
        b.reset()
        at0 = b.run(U, Y, outputs=OUTS, t_index0=0.0)
        b.reset()
        ic.same(_run_c(b, U, Y, OUTS), at0, what=("run is run_at(0.0)", Mo, interact))
        assert not kc.bits_equal(at0["ll"], g["ll"])
        b.close()


def test_runtime_compiled_models(host):
    """3. k_imm_ekf from a hiprtc program of the model's own: the pendulum snippet (M = 3, an idle lane), x0^2 (M = 2), the
    linear-Gaussian model above 4 states with the flag (M = 4), the quad-tank as a snippet against the built-in model's bits, and traced
    callables against the snippet's bits"""
    rng = np.random.default_rng(31)
    F = 70
    pid = _capi.model_compile(ec.PENDULUM_JAC_SRC, 2, 1)
    pend = _pendulum_imms(rng, F, 3)
    U, Y = uc.pendulum_data(80)
    Y = Y.copy()
    Y[[3, 40], 0] = np.nan
    b = ic.bank(ic.with_id(pend, pid))
    g = b.run(U, Y, outputs=OUTS)
    h, st = ic.host_run(host, pend, U, Y, 80, kind=ec.KIND_PENDULUM)
    _check(b, g, h, st, "pendulum snippet")
    assert np.isfinite(g["ll"]).all()
    sid = _capi.model_compile(ec.SQUARE_JAC_SRC, 1, 1)
    sq = ic.grouped(kg.square_models(2 * F), rng, F, 2)
    Ys = 3.0 + 0.5 * rng.standard_normal((60, 1))
    b = ic.bank(ic.with_id(sq, sid))
    g = b.run(None, Ys, outputs=OUTS)
    h, st = ic.host_run(host, sq, None, Ys, 60, kind=ec.KIND_SQUARE)
    _check(b, g, h, st, "square snippet")
    lg = ic.lg_imms(rng, F, 4, 6, 3, 2)
    Ul, Yl = _data(rng, 40, 2, 3, missing=(7,))
    b = ic.bank(lg)
    g = b.run(Ul, Yl, outputs=OUTS)
    h, st = ic.host_run(host, lg, Ul, Yl, 40)
    _check(b, g, h, st, "LG (6, 3, 2)")
    # the quad-tank as a snippet: the built-in model's bits
    qid = _capi.model_compile(ic.QUADTANK_JAC_SRC, 4, 2)
    qt = _quadtank_imms(rng, F, 3)
    Uq, Yq = M.quadtank_data(50)
    gb = ic.bank(qt).run(Uq, Yq, outputs=OUTS, t_index0=480.0)
    gs = ic.bank(ic.with_id(qt, qid)).run(Uq, Yq, outputs=OUTS, t_index0=480.0)
    ic.same(gs, gb, what="quad-tank snippet against the built-in model")
    # traced callables: x0^2 against the snippet
    d = [llpf_amd.MvNormal(np.array([1.0 + 0.3 * j]), 0.36) for j in range(2)]
    P, mu = [[0.9, 0.1], [0.2, 0.8]], [0.6, 0.4]
    snip = llpf_amd.IMM([llpf_amd.ExtendedKalmanFilter(llpf_amd.UserDynamics(ec.SQUARE_JAC_SRC, 1, 0, 1), llpf_amd.UserMeasurement(), 0.1, 0.25, d[j])
                         for j in range(2)], P, mu)
    traced = llpf_amd.IMM([llpf_amd.ExtendedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25, d[j], nu=0, ny=1)
                           for j in range(2)], P, mu)
    ss, st_ = llpf_amd.forward_trajectory(snip, None, Ys), llpf_amd.forward_trajectory(traced, None, Ys)
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        print("traced against snippet", k, uc.rel_err(getattr(st_, k), getattr(ss, k)))
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        assert kc.bits_equal(getattr(st_, k), getattr(ss, k)), ("traced", k)
    assert st_.ll == ss.ll


@pytest.mark.parametrize("F", [1, 16, 17, 33, 65])
def test_bank_sizes_and_chunk_edges(host, F):
    """4. banks around the quad and the wave at M = 2 and M = 4, T around the 256-step chunk of the staging pipe, from a reset: the
    outputs and the final state"""
    for Mo in (2, 4):
        rng = np.random.default_rng(400 + 10 * F + Mo)
        imms = ic.lg_imms(rng, F, Mo, 2, 1, 1)
        U, Y = _data(rng, 600, 1, 1, missing=(0, 255, 256, 599))
        b = ic.bank(imms)
        for T in (1, 255, 256, 257, 600):
            b.reset()
            g = b.run(U[:T], Y[:T], outputs=OUTS)
            h, st = ic.host_run(host, imms, U[:T], Y[:T], T)
            _check(b, g, h, st, (F, Mo, T))
        b.close()


def test_continuation_and_set_state(host):
    """5. on the quad-tank: run_at(a, t0) then run_at(b, t0 + len(a)) is run_at(a + b, t0), cut at 37 of 90; set_state on a fresh bank;
    ll alone"""
    fam = _quadtank(450.0)
    imms = fam.imms(np.random.default_rng(5), 70, 3)
    U, Y = M.quadtank_data(90)
    Y = Y.copy()
    Y[[10, 37, 60], 0] = np.nan
    ig.check_continuation(fam, host, imms, U, Y, cut=37)


def test_a_filters_bits_do_not_depend_on_the_bank(host):
    """6. filters 0, 15, 16, 69 alone in a bank of one; an IMM started from an indefinite mode covariance is NaN in its own outputs from
    that step on and the other filters' bits are unmoved; a zero column of P (a mode without mass) against the twin"""
    fam = _quadtank(1.0)
    imms = fam.imms(np.random.default_rng(6), 70, 3)
    U, Y = M.quadtank_data(30)
    Y = Y.copy()
    Y[[5, 6, 20], 0] = np.nan
    _, ok = ig.check_a_nan_imm(fam, host, imms, U, Y, interact=True, missing=(5, 6, 20), nan_filter=13, nan_mode=1)
    for f in (0, 15, 16, 69):
        one = ic.bank([imms[f]]).run(U, Y, outputs=OUTS, t_index0=1.0)
        for k in OUTS:
            assert kc.bits_equal(one[k][:, 0], ok[k][:, f]), (f, k)
        assert one["ll"][0] == ok["ll"][f]
    ig.check_a_mode_without_mass(fam, host, imms, U, Y, mu0=[0.5, 0.0, 0.5])


def test_ties_to_the_extended_kalman_bank():
    """7. M = 1 is ExtendedKalmanFilterBank on the device bit for bit (x, xt, R, Rt, ll_steps, ll), the quad-tank and the pendulum; with
    interact = False, ll_modes[:, :, j] is the ll_steps of an extended bank built from the mode-j models"""
    rng = np.random.default_rng(7)
    F = 70
    pid = _capi.model_compile(ec.PENDULUM_JAC_SRC, 2, 1)
    Uq, Yq = M.quadtank_data(60)
    Up, Yp = uc.pendulum_data(60)
    for what, models, U, Y, t0 in (("quad-tank", kg.quadtank_models(F), Uq, Yq, 470.0), ("pendulum", [kg.with_id(m, pid) for m in kg.pendulum_models(F)], Up, Yp, 0.0)):
        Y = Y.copy()
        Y[[4, 30], 0] = np.nan
        g = ic.bank([ic.imm([m], P=[[1.0]], mu0=[1.0]) for m in models]).run(U, Y, outputs=OUTS, t_index0=t0)
        e = _capi.EkfBankHandle(0, list(models)).run(U, Y, outputs=kg.OUTS, t_index0=t0)
        for k in ("x", "xt", "R", "Rt", "ll_steps", "ll"):
            assert kc.bits_equal(g[k], e[k]), (what, k)
        assert np.all(g["mu"] == 1.0)
    Mo = 3
    imms = _quadtank_imms(rng, F, Mo)
    g = ic.bank(imms, interact=False).run(Uq, Yq, outputs=("ll_modes",), t_index0=470.0)
    for j in range(Mo):
        e = _capi.EkfBankHandle(0, [s["models"][j] for s in imms]).run(Uq, Yq, outputs=("ll_steps",), t_index0=470.0)
        assert kc.bits_equal(g["ll_modes"][:, :, j], e["ll_steps"]), j


def _ekf_qt(g1, a1):
    """a quad-tank mode whose outlet switches at t = 20: inside the 40 steps of the test below, so that the time of a step shows"""
    return llpf_amd.ExtendedKalmanFilter(llpf_amd.QuadTankDynamics(supersample=2, gamma1=g1, a1=a1, t_switch=20.0), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1),
                                         np.full(2, 1e-4), llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)))


def test_parameters_a_throw_and_the_python_api(host):
    """8. set_models gives a fresh bank; a throw at error:imm_run is a status that leaves the state and a usable handle; the Python API:
    forward_trajectory(imm) is an IMMFilteringSolution, loglik starts at t = 1 * Ts and forward_trajectory at 0, update advances the
    step counter, bank rows equal the single filters; a Kalman IMMBank beside it gives the bits of its own twin"""
    rng = np.random.default_rng(8)
    F, Mo = 70, 2
    old, new = _quadtank_imms(rng, F, Mo), ic.grouped(kg.quadtank_models(F * Mo)[::-1], rng, F, Mo)
    U, Y = M.quadtank_data(40)
    b, g = ig.check_set_models(_quadtank(1.0), old, new, U, Y)
    with pytest.raises(_capi.LLPFError):
        b.set_models(*ic.bank_args(ic.lg_imms(rng, F, Mo, 4, 2, 2)))
    b.reset()
    before = ig.final(b)
    with _Inject("error:imm_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y, t_index0=1.0)
    assert ei.value.code == _capi.ERR_INTERNAL and "imm_run" in str(ei.value)
    for a, s in zip(ig.final(b), before):
        assert kc.bits_equal(a, s)
    ic.same(b.run(U, Y, outputs=OUTS, t_index0=1.0), g, what="after the throw")
    # the Python API
    modes = [_ekf_qt(0.2, 0.03), _ekf_qt(0.3, 0.036), _ekf_qt(0.25, 0.03)]
    P, mu0 = ic.random_P(rng, 3), ic.random_mu(rng, 3)
    imm = llpf_amd.IMM(modes, P, mu0)
    assert imm._handle is None and imm.extended
    T = 40
    sol = llpf_amd.forward_trajectory(imm, U, Y)
    assert isinstance(sol, llpf_amd.IMMFilteringSolution) and sol.x.shape == (T, 4) and sol.Rt.shape == (T, 4, 4) and sol.mu.shape == (T, 3)
    assert sol.ll_modes.shape == (T, 3) and sol.e is None and np.isscalar(sol.ll)
    spec = [ic.imm([f._model for f in modes], P=P, mu0=mu0)]
    h0, _ = ic.host_run(host, spec, U, Y, T, t_index0=0.0)
    h1, _ = ic.host_run(host, spec, U, Y, T, t_index0=1.0)
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        assert kc.bits_equal(getattr(sol, k), h0[k][:, 0]), k
    assert sol.ll == h0["ll"][0] and llpf_amd.loglik(imm, U, Y) == h1["ll"][0] and h0["ll"][0] != h1["ll"][0]
    llpf_amd.reset(imm)
    assert kc.bits_equal(imm.mu, mu0) and imm._index == 1
    lls = [llpf_amd.update(imm, U[t], Y[t])[0] for t in range(T)]          # step t at (1 + t) Ts: loglik's times
    assert kc.bits_equal(np.array(lls), h1["ll_steps"][:, 0]) and imm._index == 1 + T
    assert np.allclose(llpf_amd.state(imm), imm.x) and llpf_amd.covariance(imm).shape == (4, 4) and abs(imm.mu.sum() - 1.0) <= 1e-12
    other = llpf_amd.IMM(modes[::-1], P.T / P.T.sum(axis=1, keepdims=True), mu0[::-1])
    bank = llpf_amd.IMMBank([imm, other, (modes, P, mu0)])
    ll = bank.loglik(U, Y)
    assert ll[0] == h1["ll"][0] and ll[2] == ll[0] and ll[1] == llpf_amd.loglik(other, U, Y)
    fw = bank.forward(U, Y)
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        assert kc.bits_equal(fw[k][:, 0], getattr(sol, k)), k
    x, R, mu = bank.state()
    assert x.shape == (3, 4) and R.shape == (3, 4, 4) and mu.shape == (3, 3)
    bank.set_parameters([other, other, other])
    ll2 = bank.loglik(U, Y)
    assert ll2[0] == ll2[1] == ll2[2] == ll[1]
    with pytest.raises(TypeError, match="no smoother"):
        bank.smooth(U, Y)
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(imm, U, Y)
    # a Kalman IMMBank beside it: the bits of the Kalman IMM's own twin (tests/imm_host.c), as before
    kimms = [ic.random_imm(rng, 3, 3, 2, 1, k % 3, D=k % 5 != 0) for k in range(F)]
    Uk, Yk = _data(rng, 30, 1, 2, missing=(7,))
    gk = ic.bank(kimms).run(Uk, Yk, outputs=OUTS)
    hk, _ = ic.host_run(host, kimms, Uk, Yk, 30)
    ic.same(gk, hk, what="the Kalman IMM bank")
