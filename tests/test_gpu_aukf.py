"""Banks of unscented Kalman filters with augmented process noise on the device (llpf_aukf_bank_*; kernels/aukf.hpp, host/aukf.hpp): the
GPU reproduces the host build of csrc/shared/llpf_aukf.h (tests/aukf_host.c around the oracle's model functions, or around the C twins of
the two snippets that form their own noise) bit for bit, in every output and in the final state — precompiled and run-time compiled
models, with and without dynamics_w, on both sides of AUKF_POINTS_LDS (registers up to nx = 5, LDS from 6: the shapes (5, 1) and (8, 4)
below), whatever the bank, the chunking of T or the split of a run — and the Python API is the filter the CPU tests pin down."""
import ctypes as C

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import aukf_common as ac
from gpu_common import _Inject
import kalman_common as kc
from kalman_common import _data, _same
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS, lg_models, quadtank_models, with_id
import models as M
import ukf_common as uc

pytestmark = pytest.mark.gpu
W1 = ac.merwe_pair(2, 1.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ac.build_host(tmp_path_factory.mktemp("aukf_host"))


def _bank(models, w):
    return _capi.AukfBankHandle(0, list(models), w)


def _family(w):
    """the augmented unscented bank with the pair of weight sets w"""
    return kg.Family("aukf", lambda models: _bank(models, w), lambda host, models, U, Y, T, **kw: ac.host_run(host, models, w, U, Y, T, **kw),
                     lg_models, True)


def _pair(nx, k):
    """the alpha = 1 pairs and TrivialParams in turn, the small-alpha pair at k = 4"""
    return (ac.merwe_pair(nx, *uc.ALPHA1_SETS[0]), ac.merwe_pair(nx, *uc.ALPHA1_SETS[1]), ac.merwe_pair(nx, *uc.ALPHA1_SETS[2]),
            ac.trivial_pair(nx), ac.merwe_pair(nx, *uc.SMALL_ALPHA))[k % 5]


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_header_for_every_precompiled_shape(host, nx):
    """F = 130 random filters (two full workgroups and a ragged one), T = 60 with two missing rows, every output, the weight pairs in
    turn; each (nx, ny) is its own instantiation; shared and per-filter inputs give the same bits"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        fam = _family(_pair(nx, nx + ny))
        b, g, _, st, U, Y = kg.check_shape(fam, host, rng, F=130, T=60, nx=nx, ny=ny, nu=nu, missing=(7, 31), what=(nx, ny))
        assert np.isfinite(g["ll"]).all()
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]), (nx, ny, "final state")
        kg.check_broadcast_inputs(fam, b, g, U, Y, F=130, nu=nu, what=(nx, ny, "per-filter"))
        b.close()


def test_each_output_alone(host):
    kg.check_each_output_alone(_family(W1), host, seed=77, F=65, T=3, nx=2, ny=1, nu=1)


@pytest.mark.parametrize("F", [1, 63, 64, 65])
def test_bank_sizes_and_chunk_edges(host, F):
    """per-filter parameters at every bank size around the wave, T around the 256-step chunk of the staging pipe"""
    kg.check_bank_sizes_and_chunk_edges(_family(W1), host, seed=100 + F, F=F, nx=2, ny=1, nu=1, missing=(0, 255, 256), Ts=(1, 255, 256, 257))


def test_continuation_set_models_set_weights_and_state(host):
    rng, b, U, Y = kg.check_continuation(_family(ac.merwe_pair(3, 1.0, 0.0, 0.0)), host, seed=5, F=70, T=300, nx=3, ny=2, nu=2,
                                        missing=(100, 255, 256), cut=130)
    # set_models + set_weights = a fresh bank
    other = lg_models(rng, 70, 3, 2, 2)
    W2 = ac.trivial_pair(3)
    b.set_models(other)
    b.set_weights(W2)
    b.reset()
    g = b.run(U, Y, outputs=OUTS)
    _same(g, _bank(other, W2).run(U, Y, outputs=OUTS), what="set_models + set_weights")
    h, _ = ac.host_run(host, other, W2, U, Y, 300)
    _same(g, h, what="set_models + set_weights vs host")
    with pytest.raises(_capi.LLPFError):
        b.set_models(lg_models(rng, 70, 2, 2, 2))
    with pytest.raises(_capi.LLPFError):
        b.set_weights((W2[0], (1.0, 0.0, 0.0, -1.0)))


def test_per_filter_inputs_missing_rows_and_a_nan_filter_beside_healthy_ones(host):
    kg.check_per_filter_inputs_and_a_nan_filter(_family(W1), host, seed=6, F=130, T=40, nx=2, ny=1, nu=1, missing=(5, 6, 30), stride=7, row=11,
                                                nan_filter=77)


def test_a_throw_is_a_status_and_arguments_are_refused_with_the_state_untouched(host):
    """error:aukf_run is a status that leaves the state as it was; alloc:aukf_create is LLPF_ERR_ALLOC; T < 1, stray per_filter bits, a
    non-finite t_index0, a short struct_size and null inputs are LLPF_ERR_ARG under this bank's prefix; the handle runs on"""
    rng = np.random.default_rng(45)
    models = lg_models(rng, 65, 2, 1, 1)
    U, Y = _data(rng, 10, 1, 1)
    b = _bank(models, W1)
    b.run(U[:4], Y[:4])
    x0, R0 = b.get_state()
    with _Inject("error:aukf_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y)
    assert ei.value.code == _capi.ERR_INTERNAL and "aukf_run" in str(ei.value)
    with _Inject("alloc:aukf_create"):
        with pytest.raises(_capi.LLPFError) as ei:
            _bank(models, W1)
    assert ei.value.code == _capi.ERR_ALLOC
    lib = _capi.lib()
    ll = np.zeros(65)
    out = S.KalmanOutputs()
    out.struct_size = C.sizeof(S.KalmanOutputs) - 8
    run = lambda U_, Y_, T, pf, t0, o: lib.llpf_aukf_bank_run(b.h, _capi.dptr(U_), _capi.dptr(Y_), C.c_int64(T), pf, C.c_double(t0), _capi.dptr(ll), o)
    for args, word in (((U, Y, 0, 0, 0.0, None), "T must be >= 1"), ((U, Y, 10, 4, 0.0, None), "per_filter"),
                       ((U, Y, 10, 0, float("inf"), None), "t_index0 must be finite"), ((U, Y, 10, 0, float("nan"), None), "t_index0 must be finite"),
                       ((U, Y, 10, 0, 0.0, C.byref(out)), "struct_size"), ((U, None, 10, 0, 0.0, None), "Y is null"),
                       ((None, Y, 10, 0, 0.0, None), "U is null")):
        assert run(*args) == _capi.ERR_ARG, word
        msg = lib.llpf_last_error().decode()
        assert msg.startswith("aukf: ") and word in msg, msg
    x1, R1 = b.get_state()
    assert kc.bits_equal(x1, x0) and kc.bits_equal(R1, R0)
    g = b.run(U, Y, outputs=OUTS, t_index0=4.0)
    h, _ = ac.host_run(host, models, W1, U, Y, 10, t_index0=4.0, state=(x0, R0))
    _same(g, h, what="after the throws")


def test_quadtank_across_the_switch_time(host):
    """the built-in quad-tank (additive path: f at the 9 distinct state points) with per-filter parameters over T = 520 from
    t_index0 = 1 (tau crosses TSWITCH = 500; three chunks), three missing rows"""
    F, T = 65, 520
    models = quadtank_models(F)
    U, Y = M.quadtank_data(T)
    Y = Y.copy()
    Y[[5, 256, 510], 0] = np.nan
    for w in (ac.merwe_pair(4, 1.0, 0.0, 1.0), ac.trivial_pair(4)):
        b = _bank(models, w)
        g = b.run(U, Y, outputs=OUTS, t_index0=1.0)
        h, st = ac.host_run(host, models, w, U, Y, T, t_index0=1.0)
        _same(g, h, what="quad-tank")
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1])
        assert np.isfinite(g["ll"]).all() and len(set(g["ll"].tolist())) > 40


def test_runtime_compiled_shapes(host):
    """k_aukf from a hiprtc program of the model's own: the linear-Gaussian model above 4 states on either side of AUKF_POINTS_LDS —
    (5, 1) in registers, (8, 4) with the 132 KiB array in LDS — the two snippets with dynamics_w and per-filter parameters, and the
    multiplicative scalar as a traced Python callable of five parameters"""
    rng = np.random.default_rng(21)
    for nx, ny, nu in ((5, 1, 0), (8, 4, 1)):
        b, _, _, st, _, _ = kg.check_shape(_family(ac.merwe_pair(nx, 1.0, 0.0, 1.0)), host, rng, F=130, T=60, nx=nx, ny=ny, nu=nu, missing=(7,),
                                           what=("LG", nx, ny))
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]), ("LG", nx, ny, "final state")
    # the noisy pendulum: per-filter parameters and noise levels
    pid = _capi.model_compile(ac.NOISY_PENDULUM_SRC, 2, 1)
    pend = ac.noisy_pendulum_models(100)
    U, Y = uc.pendulum_data(300)
    Y = Y.copy()
    Y[[3, 256], 0] = np.nan
    for w in (ac.merwe_pair(2, 1.0, 0.0, 1.0), ac.trivial_pair(2), ac.merwe_pair(2, *uc.SMALL_ALPHA)):
        g = _bank([with_id(m, pid) for m in pend], w).run(U, Y, outputs=OUTS)
        h, _ = ac.host_run(host, pend, w, U, Y, 300, twin=ac.TWIN_NOISY_PENDULUM)
        _same(g, h, what=("noisy pendulum", w))
        assert np.isfinite(g["ll"]).all()
    # x' = a x (1 + w) + w^2: as a snippet with per-filter a, q, m0 and as a traced callable
    mid = _capi.model_compile(ac.MULT_SRC, 1, 1)
    mult = ac.mult_models(70)
    _, Y = ac.mult_data(80)
    w = ac.merwe_pair(1, 1.0, 0.0, 1.0)
    g = _bank([with_id(m, mid) for m in mult], w).run(None, Y, outputs=OUTS)
    h, _ = ac.host_run(host, mult, w, None, Y, 80, twin=ac.TWIN_MULT)
    _same(g, h, what="multiplicative snippet")
    assert np.isfinite(g["ll"]).all()
    h1, _ = ac.host_run(host, [ac.mult_model()], w, None, Y, 80, twin=ac.TWIN_MULT)
    kf = llpf_amd.AugmentedUnscentedKalmanFilter(lambda x, u, p, t, w: [p * x[0] * (1.0 + w[0]) + w[0] * w[0]], lambda x, u, p, t: [x[0] * x[0]],
                                                 0.04, 0.25, llpf_amd.MvNormal(np.array([2.0]), 0.3), nu=0, ny=1, p=0.9, weight_params=w)
    sol = llpf_amd.forward_trajectory(kf, None, Y)
    for k, v in (("x", sol.x), ("xt", sol.xt), ("R", sol.R), ("Rt", sol.Rt), ("e", sol.e)):
        assert kc.bits_equal(v, h1[k][:, 0]), ("traced callable", k)
    assert sol.ll == h1["ll"][0]


def test_python_api_from_filter_bank_equals_a_loop_of_single_filters(host):
    specs = kg.quadtank_specs(4)
    U, Y = M.quadtank_data(120)
    pf = llpf_amd.FilterBank(1000, specs, rng=3)
    ab = llpf_amd.AugmentedUnscentedKalmanFilterBank.from_filter_bank(pf)
    ll = ab.loglik(U, Y)
    assert ll.shape == (4,) and np.isfinite(ll).all() and len(set(ll.tolist())) == 4
    for k, (dy, me, df, dg, d0) in enumerate(specs):
        one = llpf_amd.AugmentedUnscentedKalmanFilter(dy, me, np.full(4, 0.1), np.full(2, 1e-4), d0)
        assert llpf_amd.loglik(one, U, Y) == ll[k], k
    ab2 = llpf_amd.AugmentedUnscentedKalmanFilterBank([(dy, me, np.full(4, 0.1), np.full(2, 1e-4), d0) for dy, me, df, dg, d0 in specs])
    assert kc.bits_equal(ab2.loglik(U, Y), ll)
    h, _ = ac.host_run(host, list(pf._models), ac.trivial_pair(4), U, Y, 120, t_index0=1.0)
    assert kc.bits_equal(h["ll"], ll)
    fw = ab.forward(U, Y)
    assert fw["x"].shape == (120, 4, 4) and fw["Rt"].shape == (120, 4, 4, 4) and ab.state()[0].shape == (4, 4)
    # the stepping verbs of one filter: update = correct then predict, all through the device
    one = llpf_amd.AugmentedUnscentedKalmanFilter(specs[0][0], specs[0][1], np.full(4, 0.1), np.full(2, 1e-4), specs[0][4],
                                                  weight_params=llpf_amd.MerweParams(1.0, 0.0, 1.0))
    sol = llpf_amd.forward_trajectory(one, U[:12], Y[:12])
    llpf_amd.reset(one)
    one._index = 0
    lls = []
    for t in range(12):
        if t % 2:
            lls.append(llpf_amd.update(one, U[t], Y[t])[0])
        else:
            l, e = llpf_amd.correct(one, U[t], Y[t])
            assert kc.bits_equal(llpf_amd.state(one), sol.xt[t]) and kc.bits_equal(np.tril(llpf_amd.covariance(one)), np.tril(sol.Rt[t]))
            llpf_amd.predict(one, U[t])
            lls.append(l)
    assert abs(sum(lls) - sol.ll) <= 1e-12 * abs(sol.ll)
    x_end = one.x
    llpf_amd.forward_trajectory(one, U[:12], Y[:12])
    assert kc.bits_equal(one.x, x_end), "correct + predict is update, bit for bit"


def test_bank_on_the_linear_c1_model_is_the_kalman_bank():
    """the statistical tie to the rest of the project: on the linear-Gaussian C1 model the bank's log-likelihood equals
    KalmanFilterBank's to 1e-10 relative, on the device"""
    _, U, Y = M.simulate_lg(M.lg_c1_model(0), 200)
    pf = llpf_amd.FilterBank(1000, kg.c1_specs(16), rng=1)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf).loglik(U, Y)
    for wp in (None, llpf_amd.MerweParams(1.0, 0.0, 1.0), llpf_amd.WikiParams(1.0, 0.0, 1.0)):
        ab = llpf_amd.AugmentedUnscentedKalmanFilterBank.from_filter_bank(pf, weight_params=wp).loglik(U, Y)
        assert np.all(np.abs(ab - kb) <= 1e-10 * np.abs(kb)), (wp, np.max(np.abs(ab - kb) / np.abs(kb)))
