"""Banks of ensemble Kalman filters on the device (llpf_enkf_bank_*; kernels/enkf.hpp, host/enkf.hpp): the GPU reproduces the host build
of csrc/shared/llpf_enkf.h (tests/enkf_host.c) bit for bit — every output, the members and the state, precompiled and run-time compiled
models, whatever the ensemble size, the bank, the chunking of T or the split of a run —, its draws are the particle bank's
(llpf_bank_simulate), and the Python API (EnsembleKalmanFilter, EnsembleKalmanFilterBank) is the filter the CPU tests pin down."""
import ctypes as C

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import enkf_common as nc
import kalman_common as kc
from kalman_common import _data, _same
from gpu_common import _Inject, cfg_of
from kf_gpu_frame import c1_specs, lg_models, pendulum_models, quadtank_models, square_models, with_id
import models as M
import ukf_common as uc
import user_models as UM

pytestmark = pytest.mark.gpu
OUTS = nc.OUTPUTS


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return nc.build_host(tmp_path_factory.mktemp("enkf_host"))


def _bank(models, N, seed=0):
    return _capi.EnkfBankHandle(0, list(models), N, seed)


def _against_the_twin(host, b, models, U, Y, seed, what, twin_models=None, kind=None, outputs=OUTS, **kw):
    """one run of the bank `b` from its current members against the twin from the same members: outputs, members, state"""
    X0 = b.get_members()
    T = Y.shape[1] if np.ndim(Y) == 3 else len(Y)
    g = b.run(U, Y, bool(kw.get("per_filter", 0) & 1), bool(kw.get("per_filter", 0) & 2), outputs=outputs, t_index0=kw.get("t_index0", 0.0))
    h = nc.host_run(host, twin_models or models, X0, U, Y, T, seed, kind=kind, **kw)
    _same(g, h, keys=tuple(outputs) + ("ll",), what=what)
    assert kc.bits_equal(b.get_members(), h["members"]), (what, "members")
    x, R = b.get_state()
    assert kc.bits_equal(x, h["state"][0]) and kc.bits_equal(R, h["state"][1]), (what, "state")
    return g, h


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_twin_for_every_precompiled_shape(host, nx):
    """1a. the 16 precompiled linear-Gaussian shapes at F = 5, N = 300, T = 40 with missing rows, random nu in 0..3; the first ensemble
    is the twin's reset draw"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        models = lg_models(rng, 5, nx, ny, nu)
        U, Y = _data(rng, 40, nu, ny, missing=(5, 6, 30))
        b = _bank(models, 300, seed=77)
        assert kc.bits_equal(b.get_members(), nc.host_init(host, models, 300, 77)), (nx, ny, "reset")
        g, _ = _against_the_twin(host, b, models, U, Y, 77, (nx, ny))
        assert np.isfinite(g["ll"]).all() and np.all(g["ll_steps"][[5, 6, 30]] == 0.0) and np.all(np.isnan(g["e"][[5, 6, 30]]))
        b.close()


def test_quadtank_precompiled_shape_across_the_switch_time(host):
    """1b. the built-in quad-tank at F = 3, N = 128, T = 520 from t_index0 = 1 (three chunks, across tau = TSWITCH)"""
    models = quadtank_models(3)
    U, Y = M.quadtank_data(520)
    Y = Y.copy()
    Y[[5, 256, 511], 0] = np.nan
    g, _ = _against_the_twin(host, _bank(models, 128, seed=3), models, U, Y, 3, "quad-tank", t_index0=1.0)
    assert np.isfinite(g["ll"]).all() and len(set(g["ll"].tolist())) == 3


def test_runtime_compiled_models(host):
    """1c. k_enkf from a hiprtc program of the model's own at F = 4, N = 100: the linear-Gaussian model at (5, 1) and (8, 4), the pendulum
    and x0^2 as snippets against their C twins, and a traced callable (x0^2 again, through the tracer)"""
    rng = np.random.default_rng(21)
    for nx, ny, nu in ((5, 1, 0), (8, 4, 1)):
        models = lg_models(rng, 4, nx, ny, nu)
        U, Y = _data(rng, 30, nu, ny, missing=(7,))
        _against_the_twin(host, _bank(models, 100, seed=5), models, U, Y, 5, ("LG", nx, ny))
    pid = _capi.model_compile(UM.PENDULUM_SRC, 2, 1)
    pend = pendulum_models(4)
    U, Y = uc.pendulum_data(60)
    g, _ = _against_the_twin(host, _bank([with_id(m, pid) for m in pend], 100, seed=6), pend, U, Y, 6, "pendulum", twin_models=pend,
                             kind=nc.KIND_PENDULUM)
    assert np.isfinite(g["ll"]).all()
    sq = square_models(4)
    Y = 3.0 + 0.5 * rng.standard_normal((40, 1))
    sid = _capi.model_compile(ec.SQUARE_JAC_SRC, 1, 1)
    _against_the_twin(host, _bank([with_id(m, sid) for m in sq], 100, seed=7), sq, None, Y, 7, "square snippet", twin_models=sq, kind=nc.KIND_SQUARE)
    f = llpf_amd.EnsembleKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25, llpf_amd.MvNormal(np.array([1.0]), 0.36),
                                      100, nu=0, ny=1, seed=7)
    sol = llpf_amd.forward_trajectory(f, None, Y)
    # (forward_trajectory resets first: the filter's second draw)
    h = nc.host_run(host, sq[:1], nc.host_init(host, sq[:1], 100, 7, n_reset=1), None, Y, 40, 7, kind=nc.KIND_SQUARE)
    assert kc.bits_equal(sol.xt, h["xt"][:, 0]) and kc.bits_equal(sol.Rt, h["Rt"][:, 0]) and sol.ll == h["ll"][0], "traced callable"


@pytest.mark.parametrize("N", [2, 63, 64, 65, 255, 256, 257, 1000])
def test_ensemble_sizes_around_the_wave_and_the_workgroup(host, N):
    """2a. N around 64 and 256 (a slot with none, one or several members) at F = 3, T = 20"""
    rng = np.random.default_rng(300 + N)
    models = lg_models(rng, 3, 2, 1, 1)
    U, Y = _data(rng, 20, 1, 1, missing=(3,))
    _against_the_twin(host, _bank(models, N, seed=N), models, U, Y, N, N)


def test_chunk_edges_with_outputs_and_without(host):
    """2b. T around the 256-step chunk of the staging pipe at F = 2, N = 65; ll alone is the ll of a run with every output"""
    rng = np.random.default_rng(41)
    models = lg_models(rng, 2, 2, 1, 1)
    U, Y = _data(rng, 600, 1, 1, missing=(0, 255, 256, 599))
    b = _bank(models, 65, seed=9)
    for T in (1, 255, 256, 257, 600):
        b.seed(9)                 # the first ensemble again, the step counter at 0
        g, h = _against_the_twin(host, b, models, U[:T], Y[:T], 9, T)
        b.seed(9)
        bare, _ = _against_the_twin(host, b, models, U[:T], Y[:T], 9, (T, "ll only"), outputs=())
        assert kc.bits_equal(bare["ll"], g["ll"]), T


def test_shared_and_per_filter_inputs_split_runs_and_the_step_verbs(host):
    """2c. shared and per-filter U / Y give the same bits; run(a) then run(b) is run(a + b); correct + predict is update; reset draws
    the next ensemble and seed restores the first"""
    rng = np.random.default_rng(42)
    models = lg_models(rng, 3, 3, 2, 2)
    U, Y = _data(rng, 50, 2, 2, missing=(4,))
    b = _bank(models, 130, seed=12)
    X0 = b.get_members()
    whole, h = _against_the_twin(host, b, models, U, Y, 12, "shared")
    Xend = b.get_members()
    b.seed(12)
    assert kc.bits_equal(b.get_members(), X0), "seed restores the first ensemble"
    Up, Yp = np.broadcast_to(U, (3,) + U.shape).copy(), np.broadcast_to(Y, (3,) + Y.shape).copy()
    per = b.run(Up, Yp, True, True, outputs=OUTS)
    _same(per, whole, what="per-filter inputs")
    b.seed(12)
    first = b.run(U[:20], Y[:20], outputs=OUTS)
    second = b.run(U[20:], Y[20:], outputs=OUTS, t_index0=20.0)
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    assert kc.bits_equal(b.get_members(), Xend)
    # the step verbs against a run of one step, and against the twin's phases
    b.seed(12)
    one = b.run(U[:1], Y[:1], outputs=("e",), t_index0=0.0)
    X1 = b.get_members()
    b.seed(12)
    ll, e = b.correct(U[0], Y[0], t_index=0.0)
    hc = nc.host_run(host, models, X0, U[:1], Y[:1], 1, 12, phases=nc.CORRECT)
    assert kc.bits_equal(ll, one["ll"]) and kc.bits_equal(e, one["e"][0]) and kc.bits_equal(b.get_members(), hc["members"])
    b.predict(U[0], t_index=0.0)
    assert kc.bits_equal(b.get_members(), X1), "correct + predict is update"
    nxt = b.run(U[1:2], Y[1:2], t_index0=1.0)       # the step counter moved by one: the next step is step 1 of the whole run
    assert kc.bits_equal(nxt["ll"], whole["ll_steps"][1])
    # reset draws the next ensemble
    b.seed(12)
    b.reset()
    assert kc.bits_equal(b.get_members(), nc.host_init(host, models, 130, 12, n_reset=1)) and not kc.bits_equal(b.get_members(), X0)


def _simulated(models, N, T, seed, U, t_index0=0.0):
    """X[:, T] of llpf_bank_simulate(M = N, T + 1, seed, step0 = 0, DYNAMICS_NOISE | SAMPLE_INITIAL) on a FilterBank of the same models"""
    pf = _capi.BankHandle(cfg_of(models[0], 1024), list(models))
    X, _ = pf.simulate(N, T + 1, U, seed=seed, step0=0, flags=_capi.SIM_DYNAMICS_NOISE | _capi.SIM_SAMPLE_INITIAL, measurements=False,
                       t_index0=t_index0)
    return X[:, T]


def _box_models(mid, F):
    out = []
    for k in range(F):
        m = with_id(M.lg_test_model(), mid)
        for i, v in enumerate((0.05 + 0.01 * k, 0.1, -1.0, -2.0, 1.0, 2.0)):
            m.qt[i] = v
        out.append(m)
    return out


def test_the_members_are_the_particle_banks_draws(host):
    """3. after create(seed), T rows of Y all missing and rho = 1: the members are X[:, T] of llpf_bank_simulate with the same seed, bit
    for bit — the linear-Gaussian model, the quad-tank, and a snippet with `noise` and `initial` members of its own, for which one
    correct! from set_members is also the twin's (the snippet's measurement written in C)"""
    T, N = 7, 300
    lg = [M.lg_test_model(0.1 * (k + 1)) for k in range(3)]
    U = np.random.default_rng(1).standard_normal((T + 1, 1))
    b = _bank(lg, N, seed=31)
    b.run(U[:T], np.full((T, 1), np.nan))
    assert kc.bits_equal(b.get_members(), _simulated(lg, N, T, 31, U)), "LG"
    qt = quadtank_models(2)
    Uq, _ = M.quadtank_data(T + 1)
    b = _bank(qt, N, seed=32)
    b.run(Uq[:T], np.full((T, 2), np.nan), t_index0=1.0)
    assert kc.bits_equal(b.get_members(), _simulated(qt, N, T, 32, Uq, 1.0)), "quad-tank"
    box = _box_models(_capi.model_compile(UM.MULT_NOISE_BOX_SRC, 2, 1), 2)
    b = _bank(box, N, seed=33)
    X0 = b.get_members()
    assert np.all(np.abs(X0[..., 0]) <= 1.0) and np.all(np.abs(X0[..., 1]) <= 2.0), "the box prior"
    b.run(U[:T], np.full((T, 1), np.nan))
    X = b.get_members()
    assert kc.bits_equal(X, _simulated(box, N, T, 33, U)), "noise + initial snippet"
    y = np.array([0.3])
    ll, e = b.correct(U[T], y, t_index=float(T))
    h = nc.host_run(host, box, X, U[T:T + 1], y[None], 1, 33, step0=T, phases=nc.CORRECT, t_index0=float(T), kind=nc.KIND_LINEAR)
    assert kc.bits_equal(ll, h["ll"]) and kc.bits_equal(e, h["e"][0]) and kc.bits_equal(b.get_members(), h["members"])


def test_a_filter_alone_has_the_bits_it_has_in_a_bank(host):
    """4. filters 0, 2 and 4 of F = 5 alone with seed + f; a NaN member makes its filter NaN from that step on and leaves the neighbours'
    bits alone; set_models and set_inflation between calls equal a fresh bank"""
    rng = np.random.default_rng(44)
    models = lg_models(rng, 5, 2, 2, 1)
    U, Y = _data(rng, 30, 1, 2, missing=(9,))
    b = _bank(models, 200, seed=50)
    X0 = b.get_members()
    g = b.run(U, Y, outputs=OUTS)
    Xg = b.get_members()
    for f in (0, 2, 4):
        one = _bank([models[f]], 200, seed=50 + f)
        r = one.run(U, Y, outputs=OUTS)
        for k in OUTS:
            assert kc.bits_equal(r[k][:, 0], g[k][:, f]), (f, k)
        assert r["ll"][0] == g["ll"][f] and kc.bits_equal(one.get_members()[0], Xg[f])
    Xn = X0.copy()
    Xn[1, 17, 0] = np.nan
    b.seed(50)
    b.set_members(Xn)
    bad = b.run(U, Y, outputs=OUTS)
    assert np.isnan(bad["ll"][1]) and np.all(np.isnan(bad["xt"][:, 1])) and np.all(np.isnan(bad["ll_steps"][:9, 1])) and bad["ll_steps"][9, 1] == 0.0
    assert np.all(np.isnan(b.get_members()[1]))
    keep = [0, 2, 3, 4]
    for k in OUTS:
        assert kc.bits_equal(bad[k][:, keep], g[k][:, keep]), k
    _same(bad, nc.host_run(host, models, Xn, U, Y, 30, 50), what="NaN member vs twin")
    other = lg_models(rng, 5, 2, 2, 1)
    b.seed(50)
    b.set_models(other)
    b.set_inflation(1.25)
    got = b.run(U, Y, outputs=OUTS)
    fresh = _bank(other, 200, seed=50)
    assert not kc.bits_equal(fresh.get_members(), X0)          # (the fresh bank drew from the new d0; the old bank keeps its members)
    fresh.set_members(X0)
    fresh.set_inflation(1.25)
    _same(got, fresh.run(U, Y, outputs=OUTS), what="set_models + set_inflation vs a fresh bank")
    _same(got, nc.host_run(host, other, X0, U, Y, 30, 50, rho=1.25), what="inflation vs twin")
    L = _capi.lib()
    for rho in (0.5, float("nan"), float("inf")):
        assert L.llpf_enkf_bank_set_inflation(b.h, C.c_double(rho)) == _capi.ERR_ARG and L.llpf_last_error().decode().startswith("enkf")
    with pytest.raises(_capi.LLPFError):
        b.set_models(lg_models(rng, 5, 3, 2, 1))


def test_a_throw_and_a_refused_allocation_leave_a_usable_handle(host):
    """5. error:enkf_run is a status, a failed allocation (injected: the run's staging is chunked, so no T makes it large) is
    LLPF_ERR_ALLOC; the members are untouched by either and the handle goes on working; alloc:enkf_create frees the half-built bank"""
    rng = np.random.default_rng(45)
    models = lg_models(rng, 3, 2, 1, 1)
    U, Y = _data(rng, 10, 1, 1)
    b = _bank(models, 64, seed=1)
    X0 = b.get_members()
    with _Inject("error:enkf_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y)
    assert ei.value.code == _capi.ERR_INTERNAL and "enkf_run" in str(ei.value)
    with _Inject("alloc:enkf_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y, outputs=OUTS)
    assert ei.value.code == _capi.ERR_ALLOC
    with _Inject("alloc:enkf_create"):
        with pytest.raises(_capi.LLPFError) as ei:
            _bank(models, 64)
    assert ei.value.code == _capi.ERR_ALLOC
    assert kc.bits_equal(b.get_members(), X0)
    _against_the_twin(host, b, models, U, Y, 1, "after the throws")


def test_python_api():
    """6. from_filter_bank(...).loglik equals a loop of single filters; forward_trajectory has the documented shapes; smooth raises"""
    specs = c1_specs(3)
    rng = np.random.default_rng(3)
    U, Y = rng.standard_normal((25, 2)), rng.standard_normal((25, 2))
    pf = llpf_amd.FilterBank(256, specs, rng=9)
    bank = llpf_amd.EnsembleKalmanFilterBank.from_filter_bank(pf)
    assert bank.N == 256 and bank.seed == 9 and bank.members().shape == (3, 256, 2)
    ll = bank.loglik(U, Y)
    for k, (dy, me, df, dg, d0) in enumerate(specs):
        f = llpf_amd.EnsembleKalmanFilter(dy, me, df.cov, dg.cov, d0, 256, seed=9 + k)
        assert llpf_amd.loglik(f, U, Y) == ll[k], k
    sol = llpf_amd.forward_trajectory(f, U, Y)
    assert isinstance(sol, llpf_amd.KalmanFilteringSolution)
    assert sol.x.shape == sol.xt.shape == (25, 2) and sol.R.shape == sol.Rt.shape == (25, 2, 2) and sol.e.shape == (25, 2) and np.isfinite(sol.ll)
    assert llpf_amd.particles(f).shape == (256, 2) and llpf_amd.state(f).shape == (2,) and llpf_amd.covariance(f).shape == (2, 2)
    dy, me, df, dg, d0 = specs[0]
    f1, f2 = (llpf_amd.EnsembleKalmanFilter(dy, me, df.cov, dg.cov, d0, 256, seed=4) for _ in range(2))
    llpf_amd.reset(f1)
    llpf_amd.reset(f2)
    l1, e1 = llpf_amd.correct(f1, U[0], Y[0])
    llpf_amd.predict(f1, U[0])
    l2, e2 = llpf_amd.update(f2, U[0], Y[0])
    assert l1 == l2 and kc.bits_equal(e1, e2) and kc.bits_equal(llpf_amd.particles(f1), llpf_amd.particles(f2))
    with pytest.raises(TypeError):
        llpf_amd.smooth(f, U, Y)
    with pytest.raises(TypeError):
        bank.smooth(U, Y)
