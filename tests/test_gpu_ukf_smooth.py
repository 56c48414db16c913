"""The unscented Rauch-Tung-Striebel smoother on the device (llpf_ukf_bank_smooth; kernels/ukf.hpp: k_ukf_smooth, host/ukf.hpp: ukf_smooth):
the GPU reproduces the host build of csrc/shared/llpf_ukf.h (tests/ukf_host.c around the oracle's model
functions) bit for bit in every output — smoothed and forward, precompiled and run-time compiled models, whatever the bank, the chunking
of T or the split of a run — the state after a smooth is the state after a run, and the Python API is the smoother the CPU tests pin
down."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi
import kalman_common as kc
import models as M
import ukf_common as uc
import ukf_smooth_common as us
import user_models as UM
from kalman_common import _data, _same
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS, SOUTS, lg_models, quadtank_models, with_id
from test_gpu_ukf import W1, _bank, _family as _ukf_family

pytestmark = pytest.mark.gpu
ALL = OUTS + SOUTS + ("ll",)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return uc.build_host(tmp_path_factory.mktemp("ukf_host"))


@pytest.fixture(scope="module")
def hsmooth(tmp_path_factory):
    return us.build_host_smooth(tmp_path_factory.mktemp("ukf_smooth_host"))


def _family(w):
    """the unscented bank with the weights w, and its smoother"""
    def host_smooth(L, models, U, fw, T, per_filter=0, t_index0=0.0, state=None, twin=0):
        return us.host_smooth(L, models, w, U, fw, T, per_filter=per_filter & 1, t_index0=t_index0, twin=twin)
    return _ukf_family(w)._replace(host_smooth=host_smooth)


def _host(host, hsmooth, models, w, U, Y, T, **kw):
    """the host build of the forward pass and of the smoother over its outputs: every output of a smooth, and the final state"""
    return kg.twin(_family(w), (host, hsmooth), models, U, Y, T, **kw)


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_header_for_every_precompiled_shape(host, hsmooth, nx):
    """F = 1000 random filters, T = 200, missing rows, every output, the three alpha = 1 weight sets and the small-alpha one in turn;
    shared and per-filter inputs give the same bits"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        fam = _family((uc.merwe_set(nx, uc.ALPHA1_SETS[(nx + ny) % 3]), uc.merwe(nx, *uc.SMALL_ALPHA))[ny == 4])
        b, g, _, _, U, Y = kg.check_shape(fam, (host, hsmooth), rng, F=1000, T=200, nx=nx, ny=ny, nu=nu, missing=(50, 51, 120, 199), what=(nx, ny))
        assert not np.isnan(g["xT"]).any() and not np.isnan(g["RT"]).any()
        kg.check_broadcast_inputs(fam, b, g, U, Y, F=1000, nu=nu, what=(nx, ny, "per-filter"))
        b.close()


def test_each_output_alone(host, hsmooth):
    """every optional output asked for on its own is the column of the run with all of them: F = 65 (a full workgroup and a ragged one)"""
    kg.check_each_output_alone(_family(W1), (host, hsmooth), seed=77, F=65, T=3, nx=2, ny=1, nu=1)


def test_quadtank_across_the_switch_time(host, hsmooth):
    """the 17th precompiled shape: the built-in quad-tank with per-filter parameters, F = 1000, T = 200 with missing rows; and T = 700 from
    t_index0 = 1 (tau crosses TSWITCH = 500; three chunks): the device's RK4 in the oracle's order, forward and backward"""
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    models = quadtank_models(1000)
    U, Y = M.quadtank_data(200)
    Y = Y.copy()
    Y[[5, 77, 199], 0] = np.nan
    g = _bank(models, w).smooth(U, Y, forward=OUTS, t_index0=1.0)
    h, _ = _host(host, hsmooth, models, w, U, Y, 200, t_index0=1.0)
    _same(g, h, ALL, what="quad-tank F = 1000")
    F, T = 65, 700
    models = quadtank_models(F)
    U, Y = M.quadtank_data(T)
    Y = Y.copy()
    Y[[5, 256, 600], 0] = np.nan
    for w in (uc.merwe(4, 1.0, 0.0, 1.0), uc.merwe(4, 1.0, 0.0, -1.0)):
        g = _bank(models, w).smooth(U, Y, forward=OUTS, t_index0=1.0)
        h, _ = _host(host, hsmooth, models, w, U, Y, T, t_index0=1.0)
        _same(g, h, ALL, what="quad-tank")
        assert not np.isnan(g["xT"]).any() and not np.isnan(g["RT"]).any()


def test_runtime_compiled_shapes(host, hsmooth):
    """k_ukf_smooth from a hiprtc program of the model's own: the linear-Gaussian model above 4 states, the quad-tank as a snippet (the
    built-in quad-tank's bits), the pendulum, the x0^2 model as a snippet and as a traced Python callable"""
    rng = np.random.default_rng(21)
    for nx, ny, nu in ((5, 1, 0), (6, 3, 2), (8, 4, 1)):
        kg.check_shape(_family(uc.merwe(nx, 1.0, 0.0, 1.0)), (host, hsmooth), rng, F=130, T=60, nx=nx, ny=ny, nu=nu, missing=(7,),
                       what=("LG", nx, ny))
    # the quad-tank as a snippet
    qid = _capi.model_compile(UM.QUADTANK_SRC, 4, 2)
    models = quadtank_models(70)
    U, Y = M.quadtank_data(520)
    w = uc.merwe(4, 1.0, 0.0, 1.0)
    g = _bank([with_id(m, qid) for m in models], w).smooth(U, Y, forward=OUTS, t_index0=1.0)
    gb = _bank(models, w).smooth(U, Y, forward=OUTS, t_index0=1.0)
    _same(g, gb, ALL, what="quad-tank snippet vs built-in")
    h, _ = _host(host, hsmooth, models, w, U, Y, 520, t_index0=1.0)
    _same(g, h, ALL, what="quad-tank snippet vs host")
    # the pendulum: per-filter parameters, every weight set of the CPU test
    pid = _capi.model_compile(UM.PENDULUM_SRC, 2, 1)
    pend = kg.pendulum_models(100)
    U, Y = uc.pendulum_data(300)
    Y = Y.copy()
    Y[[3, 256], 0] = np.nan
    for w in (uc.merwe(2, 1.0, 0.0, 1.0), uc.merwe(2, 1.0, 0.0, 0.0), uc.merwe(2, *uc.SMALL_ALPHA)):
        g = _bank([with_id(m, pid) for m in pend], w).smooth(U, Y, forward=OUTS)
        h, _ = _host(host, hsmooth, pend, w, U, Y, 300, twin=uc.TWIN_PENDULUM)
        _same(g, h, ALL, what=("pendulum", w))
        assert not np.isnan(g["xT"]).any()
    # f(x) = x, g(x) = x0^2: as a snippet and as a traced Python callable
    sq = kg.square_models(64)
    Y = 3.0 + 0.5 * rng.standard_normal((80, 1))
    w = uc.merwe(1, 1.0, 0.0, 1.0)
    h, _ = _host(host, hsmooth, sq, w, None, Y, 80, twin=uc.TWIN_SQUARE)
    sid = _capi.model_compile(uc.SQUARE_SRC, 1, 1)
    g = _bank([with_id(m, sid) for m in sq], w).smooth(None, Y, forward=OUTS)
    _same(g, h, ALL, what="square snippet")
    ukf = llpf_amd.UnscentedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25,
                                         llpf_amd.MvNormal(np.array([1.0]), 0.36), nu=0, ny=1, weight_params=w)
    sol = llpf_amd.smooth(ukf, None, Y)
    for k, v in (("x", sol.x), ("xt", sol.xt), ("R", sol.R), ("Rt", sol.Rt), ("e", sol.e), ("xT", sol.xT), ("RT", sol.RT)):
        assert kc.bits_equal(v, h[k][:, 0]), ("traced callable", k)
    assert sol.ll == h["ll"][0]


@pytest.mark.parametrize("F", [1, 63, 64, 65, 1000])
def test_bank_sizes_and_chunk_edges(host, hsmooth, F):
    """per-filter parameters at every bank size around the wave, T around the 256-step chunk of the staging pipe; the state after a smooth
    is the state after a run"""
    kg.check_bank_sizes_and_chunk_edges(_family(W1), (host, hsmooth), seed=100 + F, F=F, nx=2, ny=1, nu=1, missing=(0, 255, 256, 699),
                                        Ts=(1, 255, 256, 257, 700))


def test_chunks_are_invisible(host, hsmooth):
    """T = 1000 with shared inputs (four chunks); 4000 filters with per-filter U, where the backward pipe — which stages U and the smoothed
    outputs only — cuts T into other chunks than the forward one; a prefix smoothed on its own equals the host smoother of that prefix"""
    rng = np.random.default_rng(7)
    models = lg_models(rng, 200, 3, 2, 2)
    U, Y = _data(rng, 1000, 2, 2, missing=(255, 256, 511, 999))
    W3 = uc.merwe(3, 1.0, 0.0, 1.0)
    b = _bank(models, W3)
    g = b.smooth(U, Y, forward=OUTS)
    h, _ = _host(host, hsmooth, models, W3, U, Y, 1000)
    _same(g, h, ALL, what="T = 1000")
    b.reset()
    gp = b.smooth(U[:300], Y[:300], forward=OUTS)
    hp, _ = _host(host, hsmooth, models, W3, U[:300], Y[:300], 300)
    _same(gp, hp, ALL, what="prefix")
    for k in OUTS:
        assert kc.bits_equal(gp[k], g[k][:300]), ("the forward pass of a prefix is the prefix of the forward pass", k)
    # smoothed outputs only against forward + smoothed outputs: other chunk lengths, the same bits
    b.reset()
    only = b.smooth(U, Y, outputs=("xT",))
    assert kc.bits_equal(only["xT"], g["xT"]) and kc.bits_equal(only["ll"], g["ll"])
    F = 4000
    models = lg_models(rng, F, 2, 1, 1)
    T = 600
    Up = rng.standard_normal((F, T, 1))
    _, Y = _data(rng, T, 1, 1, missing=(100, 599))
    b = _bank(models, W1)
    g = b.smooth(Up, Y, u_per_filter=True, forward=OUTS)
    h, _ = _host(host, hsmooth, models, W1, Up, Y, T, per_filter=1)
    _same(g, h, ALL, what="4000 filters, per-filter U")


def test_state_after_smooth_continuation_set_models_and_set_weights(host, hsmooth):
    """the state after smooth is the state after run; a smooth that continues a run with the matching t_index0 smooths the steps it was
    given; set_weights / set_models between calls = a fresh bank"""
    models = quadtank_models(100)
    U, Y = M.quadtank_data(620)
    W4 = uc.merwe(4, 1.0, 0.0, 1.0)
    b = _bank(models, W4)
    whole = b.smooth(U, Y, forward=OUTS, t_index0=1.0)
    xs, Rs = b.get_state()
    b.reset()
    run = b.run(U, Y, outputs=OUTS, t_index0=1.0)
    xr, Rr = b.get_state()
    assert kc.bits_equal(xs, xr) and kc.bits_equal(Rs, Rr)
    _same(whole, run, OUTS + ("ll",), what="forward outputs of smooth = run")
    b.reset()
    plain = b.smooth(U, Y, outputs=(), forward=OUTS, t_index0=1.0)          # nothing smoothed is asked for: a run
    _same(plain, run, OUTS + ("ll",), what="smooth without smoothed outputs")
    b.reset()
    b.run(U[:400], Y[:400], t_index0=1.0)
    x, R = b.get_state()
    second = b.smooth(U[400:], Y[400:], forward=OUTS, t_index0=401.0)
    h2, st = _host(host, hsmooth, models, W4, U[400:], Y[400:], 220, state=(x, R), t_index0=401.0)
    _same(second, h2, ALL, what="a smooth that continues a run")
    for k in OUTS:
        assert kc.bits_equal(second[k], whole[k][400:]), k
    x2, R2 = b.get_state()
    assert kc.bits_equal(x2, xs) and kc.bits_equal(R2, Rs) and kc.bits_equal(x2, st[0])
    # set_models / set_weights = a fresh bank
    other = quadtank_models(150)[50:]
    W2 = uc.merwe(4, 1.0, 0.0, 0.0)
    b.set_models(other)
    b.set_weights(W2)
    b.reset()
    g = b.smooth(U, Y, forward=OUTS, t_index0=1.0)
    f2 = _bank(other, W2).smooth(U, Y, forward=OUTS, t_index0=1.0)
    _same(g, f2, ALL, what="set_models + set_weights")
    h, _ = _host(host, hsmooth, other, W2, U, Y, 620, t_index0=1.0)
    _same(g, h, ALL, what="set_models + set_weights vs host")


def test_a_filters_bits_do_not_depend_on_the_bank_and_nan_stays_home(host, hsmooth):
    rng = np.random.default_rng(6)
    models = lg_models(rng, 130, 2, 1, 1)
    U = rng.standard_normal((130, 40, 1))
    Y = 2.0 * rng.standard_normal((130, 40, 1))
    Y[:, [5, 6, 30], 0] = np.nan
    Y[::7, 11, 0] = np.nan
    b = _bank(models, W1)
    x, R = b.get_state()
    ok = b.smooth(U, Y, True, True, forward=OUTS)
    h, _ = _host(host, hsmooth, models, W1, U, Y, 40, per_filter=3)
    _same(ok, h, ALL, what="per-filter inputs")
    for f in (0, 63, 64, 129):          # alone in a bank of one
        one = _bank([models[f]], W1).smooth(U[f:f + 1], Y[f:f + 1], True, True, forward=OUTS)
        for k in OUTS + SOUTS:
            assert kc.bits_equal(one[k][:, 0], ok[k][:, f]), (k, f)
    R[77] = -100.0 * np.eye(2)
    b.set_state(x, R)
    bad = b.smooth(U, Y, True, True, forward=OUTS)
    assert np.isnan(bad["ll"][77]) and np.all(np.isnan(bad["xT"][:, 77])) and np.all(np.isnan(bad["RT"][:, 77]))
    keep = [f for f in range(130) if f != 77]
    for k in OUTS + SOUTS:
        assert kc.bits_equal(bad[k][:, keep], ok[k][:, keep]), k
    hb, _ = _host(host, hsmooth, models, W1, U, Y, 40, per_filter=3, state=(x, R))
    _same(bad, hb, ALL, what="NaN filter")


def test_a_throw_and_a_refused_allocation_leave_a_usable_handle():
    # 2^40 steps: the stored posterior alone is beyond the device; refused by its allocation before any launch, the state untouched
    kg.check_throw_and_refused_allocation(_family(W1), seed=45, F=64, T=50, nx=2, ny=1, nu=0, short=10, huge=1 << 40)


def test_ukf_bank_smooth_on_the_linear_c1_model_is_the_kalman_banks():
    """the statistical tie to the rest of the project: on the linear-Gaussian C1 model the unscented bank's smoothed estimates equal
    KalmanFilterBank.smooth's to 1e-10 relative, on the device"""
    _, U, Y = M.simulate_lg(M.lg_c1_model(0), 200)
    pf = llpf_amd.FilterBank(1000, kg.c1_specs(16), rng=1)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf).smooth(U, Y)
    for wp in (None, llpf_amd.MerweParams(1.0, 0.0, 1.0), llpf_amd.WikiParams(1.0, 0.0, 1.0)):
        ub = llpf_amd.UnscentedKalmanFilterBank.from_filter_bank(pf, weight_params=wp).smooth(U, Y)
        assert set(ub) == set(kb)
        for f in range(16):
            for k in SOUTS:
                assert kc.close(ub[k][:, f], kb[k][:, f]), (wp, k, f)
        assert np.all(np.abs(ub["ll"] - kb["ll"]) <= 1e-10 * np.abs(kb["ll"]))


def test_python_api(host, hsmooth):
    """smooth(ukf, u, y) against the bank column; its forward fields bit-equal to forward_trajectory; from_filter_bank(...).smooth against
    a loop of single filters"""
    specs = kg.quadtank_specs(6)
    U, Y = M.quadtank_data(300)
    pf = llpf_amd.FilterBank(1000, specs, rng=3)
    ub = llpf_amd.UnscentedKalmanFilterBank.from_filter_bank(pf)
    r = ub.smooth(U, Y, forward=_capi.KALMAN_OUTPUTS)
    assert r["xT"].shape == (300, 6, 4) and r["RT"].shape == (300, 6, 4, 4) and r["ll"].shape == (6,)
    h, _ = _host(host, hsmooth, list(pf._models), llpf_amd.TrivialParams().weights(4), U, Y, 300)
    _same(r, h, ALL, what="from_filter_bank vs host")
    for k, (dy, me, df, dg, d0) in enumerate(specs):
        one = llpf_amd.UnscentedKalmanFilter(dy, me, np.full(4, 0.1), np.full(2, 1e-4), d0)
        s = llpf_amd.smooth(one, U, Y)
        assert isinstance(s, llpf_amd.KalmanSmoothingSolution)
        assert kc.bits_equal(s.xT, r["xT"][:, k]) and kc.bits_equal(s.RT, r["RT"][:, k]) and s.ll == r["ll"][k], k
        sol = llpf_amd.forward_trajectory(one, U, Y)
        for name in ("x", "xt", "R", "Rt", "e"):
            assert kc.bits_equal(getattr(s, name), getattr(sol, name)), (k, name)
        assert s.ll == sol.ll


def test_smoothing_lowers_the_error_on_pendulum_data():
    """on data simulated from the pendulum (the generator of uc.pendulum_data(1000, seed=0), re-run to keep the states) the smoothed
    mean-square error against the simulated states is below the filtered one, for every weight set"""
    T = 1000
    m = uc.pendulum_model()
    f, g = uc.pendulum_fg(m)
    rng = np.random.default_rng(0)
    U = 0.5 * np.sin(0.1 * np.arange(T)).reshape(T, 1)
    Y = np.zeros((T, 1))
    X = np.zeros((T, 2))
    x = np.array([1.0, 0.0])
    for k in range(T):
        X[k] = x
        Y[k] = g(x, U[k], 0.0) + 0.05 * rng.standard_normal()
        x = f(x, U[k], 0.0) + np.sqrt(np.array([1e-4, 4e-3])) * rng.standard_normal(2)
    U0, Y0 = uc.pendulum_data(T, seed=0)
    assert np.array_equal(U, U0) and np.array_equal(Y, Y0)
    pid = _capi.model_compile(UM.PENDULUM_SRC, 2, 1)
    for abk in uc.ALPHA1_SETS + (uc.SMALL_ALPHA,):
        w = uc.merwe_set(2, abk)
        r = _bank([with_id(m, pid)], w).smooth(U, Y, forward=("xt",))
        mse_f = float(np.mean((r["xt"][:, 0] - X) ** 2))
        mse_s = float(np.mean((r["xT"][:, 0] - X) ** 2))
        print("pendulum", abk, "filtered mse %.3e smoothed mse %.3e" % (mse_f, mse_s))
        assert mse_s < mse_f, (abk, mse_s, mse_f)
