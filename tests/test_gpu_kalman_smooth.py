"""The Rauch-Tung-Striebel smoother of Kalman banks on the device (llpf_kalman_bank_smooth; k_kalman_smooth in kernels/kalman.hpp,
host/kalman.hpp): the GPU reproduces the host build of csrc/shared/llpf_kalman.h bit for bit — forward outputs, ll and the smoothed xT, RT —
whatever the shape, the bank or the chunking; the handle's state after a smooth is the state after a run; and the Python API
(smooth(kf, u, y), KalmanFilterBank.smooth) computes the reference's smoother."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi
import kalman_common as kc
from kalman_common import _data, _same
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS, SOUTS
import kalman_smooth_common as ks
import models as M
from test_gpu_kalman import _bank, _family as _kalman_family

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kalman_host"))


@pytest.fixture(scope="module")
def hsmooth(tmp_path_factory):
    return ks.build_host_smooth(tmp_path_factory.mktemp("kalman_smooth_host"))


def _family(D):
    """the Kalman bank over random systems, filter k with a direct term where D(k), and its smoother"""
    def host_smooth(L, systems, U, fw, T, per_filter=0, state=None):
        return ks.host_smooth(L, systems, U, fw, T, per_filter=per_filter & 1)
    return _kalman_family(D)._replace(host_smooth=host_smooth)


@pytest.mark.parametrize("nx", range(1, 9))
def test_bit_identical_to_the_host_header_for_every_shape(host, hsmooth, nx):
    """F = 1000 random filters, T = 200, missing rows: xT, RT, ll and every forward output; shared and per-filter inputs give the same bits"""
    fam = _family(lambda k: k % 5 != 0)
    for ny in range(1, 5):
        rng = np.random.default_rng(1000 + 10 * nx + ny)
        nu = int(rng.integers(0, 4))
        b, g, _, _, U, Y = kg.check_shape(fam, (host, hsmooth), rng, F=1000, T=200, nx=nx, ny=ny, nu=nu, missing=(50, 51, 120, 199), what=(nx, ny))
        kg.check_broadcast_inputs(fam, b, g, U, Y, F=1000, nu=nu, what=(nx, ny, "per-filter"))
        b.close()


def test_each_output_alone(host, hsmooth):
    """every optional output asked for on its own is the column of the run with all of them: F = 65 (a full workgroup and a ragged one)"""
    kg.check_each_output_alone(_family(lambda k: k % 5 != 0), (host, hsmooth), seed=77, F=65, T=3, nx=2, ny=1, nu=1)


def test_chunks_are_invisible(host, hsmooth):
    rng = np.random.default_rng(41)
    base = [kc.random_system(rng, 4, 2, 2, k % 3) for k in range(300)]
    # shared inputs, T = 1000: four forward and four backward chunks of at most 256 steps
    systems = base[:1000] * 4
    U, Y = _data(rng, 1000, 2, 2, missing=(255, 256, 600, 999))
    b = _bank(systems)
    g = b.smooth(U, Y, forward=("xt", "Rt"))
    h, _ = kc.host_run(host, base, U, Y, 1000)
    h.update(ks.host_smooth(hsmooth, base, U, h, 1000))
    for k in ("xt", "Rt", "xT", "RT"):
        for j in range(4):
            assert kc.bits_equal(g[k][:, j * 300:(j + 1) * 300], h[k]), k
    assert kc.bits_equal(g["ll"][:300], h["ll"])
    # a prefix is a short smooth of its own: the stored posterior of the long run is the short run's
    b.reset()
    short = b.smooth(U[:300], Y[:300], forward=("xt",))
    assert kc.bits_equal(short["xt"], g["xt"][:300])
    hs = ks.host_smooth(hsmooth, base, U[:300], {"xt": h["xt"][:300], "Rt": h["Rt"][:300]}, 300)
    assert kc.bits_equal(short["xT"][:, :300], hs["xT"]) and kc.bits_equal(short["RT"][:, :300], hs["RT"])
    b.close()
    # per-filter inputs of their own for 4000 filters: backward chunks of 95 steps against forward chunks of 256
    F = 4000
    systems = [base[k % 300] for k in range(F)]
    U = rng.standard_normal((F, 1000, 2))
    Y = rng.standard_normal((F, 1000, 2))
    Y[::7, 400, 0] = np.nan
    b = _bank(systems)
    g = b.smooth(U, Y, True, True)
    pick = np.sort(rng.choice(F, 48, replace=False))
    sub = [systems[k] for k in pick]
    h, _ = kc.host_run(host, sub, U[pick], Y[pick], 1000, per_filter=3)
    hs = ks.host_smooth(hsmooth, sub, np.ascontiguousarray(U[pick]), h, 1000, per_filter=1)
    assert kc.bits_equal(g["ll"][pick], h["ll"])
    assert kc.bits_equal(g["xT"][:, pick], hs["xT"]) and kc.bits_equal(g["RT"][:, pick], hs["RT"])
    b.close()


def test_the_state_after_smooth_is_the_state_after_run():
    rng = np.random.default_rng(42)
    systems = [kc.random_system(rng, 3, 2, 1, k % 3) for k in range(500)]
    U, Y = _data(rng, 300, 1, 2, missing=(7,))
    a, b = _bank(systems), _bank(systems)
    sa = a.smooth(U[:200], Y[:200], forward=OUTS)
    rb = b.run(U[:200], Y[:200], outputs=OUTS)
    _same(sa, rb, OUTS + ("ll",), "forward")
    xa, Ra = a.get_state()
    xb, Rb = b.get_state()
    assert kc.bits_equal(xa, xb) and kc.bits_equal(Ra, Rb)
    _same(a.run(U[200:], Y[200:], outputs=OUTS), b.run(U[200:], Y[200:], outputs=OUTS), OUTS + ("ll",), "continued")
    # a smooth that continues a run smooths the steps it was given, from the state it found
    a.reset(); b.reset()
    a.run(U[:100], Y[:100])
    b.run(U[:100], Y[:100])
    s2 = a.smooth(U[100:], Y[100:], forward=("xt",))
    r2 = b.run(U[100:], Y[100:], outputs=("xt",))
    assert kc.bits_equal(s2["xt"], r2["xt"]) and kc.bits_equal(s2["ll"], r2["ll"]) and kc.bits_equal(a.get_state()[0], b.get_state()[0])
    assert kc.bits_equal(s2["xT"][-1], r2["xt"][-1])


def test_a_filters_bits_do_not_depend_on_the_bank_and_nan_stays_home(host, hsmooth):
    rng = np.random.default_rng(43)
    systems = [kc.random_system(rng, 3, 2, 1, k % 3) for k in range(1000)]
    U, Y = _data(rng, 60, 1, 2)
    full = _bank(systems)
    g = full.smooth(U, Y, forward=OUTS)
    pick = [999, 0, 517, 64, 63, 65]
    sub = _bank([systems[k] for k in pick][::-1]).smooth(U, Y, forward=OUTS)
    for j, k in enumerate(pick[::-1]):
        for key in OUTS + SOUTS:
            assert kc.bits_equal(sub[key][:, j], g[key][:, k]), (k, key)
    # filter 77 starts from an indefinite covariance: NaN in every output of its own, nothing else changes
    full.reset()
    x, R = full.get_state()
    R[77] = -100.0 * np.eye(3)
    full.set_state(x, R)
    bad = full.smooth(U, Y, forward=OUTS)
    assert np.all(np.isnan(bad["xT"][:, 77])) and np.all(np.isnan(bad["RT"][:, 77])) and np.isnan(bad["ll"][77])
    keep = [f for f in range(1000) if f != 77]
    for key in OUTS + SOUTS:
        assert kc.bits_equal(bad[key][:, keep], g[key][:, keep]), key
    h, _ = kc.host_run(host, systems, U, Y, 60, state=(x, R))
    h.update(ks.host_smooth(hsmooth, systems, U, h, 60))
    _same(bad, h, OUTS + SOUTS + ("ll",), "NaN filter")


def _simulate_states(rng, mats, T):
    A, B, Cm, D = mats["A"], mats["B"], mats["C"], mats["D"]
    nx, nu, ny = A.shape[0], B.shape[1], Cm.shape[0]
    U = rng.standard_normal((T, nu))
    X, Y = np.empty((T, nx)), np.empty((T, ny))
    x = mats["x0"] + np.linalg.cholesky(mats["P0"]) @ rng.standard_normal(nx)
    L1, L2 = np.linalg.cholesky(mats["R1"]), np.linalg.cholesky(mats["R2"])
    for t in range(T):
        X[t] = x
        Y[t] = Cm @ x + D @ U[t] + L2 @ rng.standard_normal(ny)
        x = A @ x + B @ U[t] + L1 @ rng.standard_normal(nx)
    return X, U, Y


def test_python_api():
    rng = np.random.default_rng(44)
    m, D = kc.random_system(rng, 3, 1, 1, 2)
    mt = kc.matrices(m, D)
    X, U, Y = _simulate_states(rng, mt, 400)
    Y[9, 0] = np.nan
    kf = llpf_amd.KalmanFilter(mt["A"], mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]))
    sol = llpf_amd.smooth(kf, U, Y)
    assert isinstance(sol, llpf_amd.KalmanSmoothingSolution) and isinstance(sol, llpf_amd.KalmanFilteringSolution)
    assert sol.xT.shape == (400, 3) and sol.RT.shape == (400, 3, 3) and sol.x.shape == (400, 3) and np.isscalar(sol.ll)
    fw = llpf_amd.forward_trajectory(kf, U, Y)
    for k in ("x", "xt", "R", "Rt", "e"):
        assert kc.bits_equal(getattr(sol, k), getattr(fw, k)), k
    assert sol.ll == fw.ll
    xT, RT = ks.numpy_smooth(mt, sol.x, sol.xt, sol.R, sol.Rt)
    assert kc.close(sol.xT, xT) and kc.close(sol.RT, RT)
    ref = kc.numpy_reference(mt, U, Y)
    assert kc.close(sol.xt, ref["xt"])
    # on data from the model, the smoothed estimate is closer to the true states than the filtered one
    err_s, err_f = np.mean((sol.xT - X) ** 2), np.mean((sol.xt - X) ** 2)
    assert err_s < err_f, (err_s, err_f)
    # the state after smooth is the state after forward_trajectory
    llpf_amd.smooth(kf, U, Y)
    x1 = kf.x
    llpf_amd.forward_trajectory(kf, U, Y)
    assert kc.bits_equal(x1, kf.x)
    # a bank: KalmanFilterBank.smooth is every filter's smooth
    kf2 = llpf_amd.KalmanFilter(mt["A"] * 0.5, mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]))
    kb = llpf_amd.KalmanFilterBank([kf, kf2])
    r = kb.smooth(U, Y, forward=("xt",))
    assert r["xT"].shape == (400, 2, 3) and r["RT"].shape == (400, 2, 3, 3) and r["ll"].shape == (2,)
    for j, f in enumerate((kf, kf2)):
        s = llpf_amd.smooth(f, U, Y)
        assert kc.bits_equal(r["xT"][:, j], s.xT) and kc.bits_equal(r["RT"][:, j], s.RT) and r["ll"][j] == s.ll
        assert kc.bits_equal(r["xt"][:, j], s.xt)
    rp = kb.smooth(np.stack([U, U]), np.stack([Y, Y]), outputs=("xT",))
    assert set(rp) == {"ll", "xT"} and kc.bits_equal(rp["xT"], r["xT"])


def test_from_filter_bank_smooths_like_each_filter():
    specs, models = [], []
    for k in range(6):
        model = M.lg_test_model(sigma_f=0.1 + 0.05 * k)
        mt = kc.matrices(model, np.zeros((1, 1)))
        specs.append((llpf_amd.LinearDynamics(mt["A"], mt["B"]), llpf_amd.LinearMeasurement(mt["C"]),
                      llpf_amd.MvNormal(np.zeros(2), mt["R1"]), llpf_amd.MvNormal(np.zeros(1), mt["R2"]),
                      llpf_amd.MvNormal(mt["x0"], mt["P0"])))
        models.append((model, mt))
    _, U, Y = M.simulate_lg(models[0][0], 80)
    pf = llpf_amd.FilterBank(1024, specs, rng=3)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf)
    r = kb.smooth(U, Y)
    for j, (model, mt) in enumerate(models):
        kf = llpf_amd.KalmanFilter(mt["A"], mt["B"], mt["C"], 0.0, mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]), Ts=model.Ts)
        s = llpf_amd.smooth(kf, U, Y)
        assert kc.bits_equal(r["xT"][:, j], s.xT) and kc.bits_equal(r["RT"][:, j], s.RT) and r["ll"][j] == s.ll, j


def test_a_throw_and_a_refused_allocation_leave_a_usable_handle():
    # 2^40 steps: the stored posterior alone is beyond the device; refused by its allocation before any launch, the state untouched
    kg.check_throw_and_refused_allocation(_family(lambda k: True), seed=45, F=64, T=50, nx=2, ny=1, nu=0, short=10, huge=1 << 40)
