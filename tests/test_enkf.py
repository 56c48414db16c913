"""Banks of ensemble Kalman filters, the part that needs no GPU: csrc/shared/llpf_enkf.h (the device order, built for the host by
tests/enkf_host.c) against a numpy restatement of the formulas, known answers (two members by hand, the order of the sum over the
ensemble, inflation), the reference's own statistical bars on the noise sweep, and the argument checks of the C ABI (llpf_enkf_bank_*)."""
import ctypes as C
import os

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import enkf_common as nc
import kalman_common as kc
import models as M
import oracle_binding as ob
import ukf_common as uc
import user_models as UM

OUTPUTS = nc.OUTPUTS


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return nc.build_host(tmp_path_factory.mktemp("enkf_host"))


def _measured(host, m, U, Y, fg, fgl, N, seed, t0, kind, what):
    """header vs restatement with the bar of tests/test_ekf.py::_measured: the restatement's own float64-against-long-double error is
    measured in the same run; the bar is 1e-10 where ten times that error is below it, otherwise ten times the measured error"""
    R1, R2 = S.gaussian_cov_matrix(m.dynamics_density), S.gaussian_cov_matrix(m.measurement_density)
    X0 = nc.host_init(host, [m], N, seed)
    a = nc.numpy_enkf(fg[0], fg[1], R1, R2, X0[0], U, Y, seed, m.Ts, t0)
    b = nc.numpy_enkf(fgl[0], fgl[1], R1, R2, X0[0], U, Y, seed, m.Ts, t0, dtype=np.longdouble)
    keys = OUTPUTS + ("ll", "members")
    own = {k: uc.rel_err(a[k], b[k]) for k in keys}
    got = nc.host_run(host, [m], X0, U, Y, Y.shape[0], seed, t_index0=t0, kind=kind)
    assert not np.isnan(got["ll"]).any() and not np.isnan(got["Rt"]).any(), what
    err = {k: uc.rel_err(got[k][:, 0], a[k]) for k in OUTPUTS}
    err["ll"] = uc.rel_err(got["ll"][0], a["ll"])
    err["members"] = uc.rel_err(got["members"][0], a["members"])
    print(what, "ll %.6f" % got["ll"][0], "restatement float64 vs long double:", {k: "%.2e" % v for k, v in own.items()})
    print(what, "header vs restatement:", {k: "%.2e" % v for k, v in err.items()})
    for k in err:
        bar = 1e-10 if 10.0 * own[k] <= 1e-10 else 10.0 * own[k]
        assert err[k] <= bar, (what, k, err[k], bar)


def test_header_equals_the_formulas_on_the_quadtank(host):
    """1a. The quad-tank, N = 200, T = 600 from t_index0 = 1 (across tau = TSWITCH), three missing rows.  The bar is derived in the
    run (printed), never copied."""
    m = M.quadtank_model()
    U, Y = M.quadtank_data(600)
    Y = Y.copy()
    Y[[5, 400, 577], 0] = np.nan
    _measured(host, m, U, Y, uc.quadtank_fg(m), uc.quadtank_fg(m, np.longdouble), 200, 21, 1.0, nc.KIND_ORACLE, "quad-tank")


def test_header_equals_the_formulas_on_the_pendulum(host):
    """1b. The pendulum through its C twin, N = 100, T = 300."""
    m = uc.pendulum_model()
    U, Y = uc.pendulum_data(300)
    _measured(host, m, U, Y, uc.pendulum_fg(m), uc.pendulum_fg(m, np.longdouble), 100, 5, 0.0, nc.KIND_PENDULUM, "pendulum")


def test_header_equals_the_formulas_on_a_linear_system(host):
    """1c. A random linear system with 3 states and 2 outputs, N = 257 (one slot of the sum holds two members)."""
    rng = np.random.default_rng(32)
    m, D = kc.random_system(rng, 3, 2, 1, D=False)
    mats = kc.matrices(m, D)
    U, Y = kc.simulate(rng, mats, 120, missing=(7,))
    _measured(host, m, U, Y, uc.linear_fg(mats), uc.linear_fg(mats, np.longdouble), 257, 9, 0.0, nc.KIND_ORACLE, "LG 3x2")


def _identity_model(r1, r2):
    g = S.make_gaussian
    return S.make_lg_model(np.eye(1), np.zeros((1, 0)), np.eye(1), g(np.zeros(1), r1), g(np.zeros(1), r2), g(np.zeros(1), 1.0))


def test_two_members_by_hand(host):
    """2a. N = 2, nx = ny = 1, f = g = identity: ll, xt and Rt by hand to 1e-13."""
    r1, r2, y, seed = 0.04, 0.25, 0.7, 3
    x = np.array([0.3, 1.5])
    got = nc.host_run(host, [_identity_model(r1, r2)], x.reshape(1, 2, 1), None, np.array([[y]]), 1, seed)
    xbar = x.mean()
    P = ((x - xbar) ** 2).sum() / 1.0
    S_ = P + r2
    e = y - xbar
    ll = -0.5 * (np.log(2 * np.pi) + np.log(S_) + e * e / S_)
    v = np.sqrt(r2) * nc.normals(seed, 0, nc.STREAM_MEASURE, 1, 2)[:, 0]
    xu = x + (P / S_) * (y - (x + v))
    assert abs(got["ll_steps"][0, 0] - ll) <= 1e-13 * abs(ll) and got["ll"][0] == got["ll_steps"][0, 0]
    assert abs(got["e"][0, 0, 0] - e) <= 1e-13 and abs(got["x"][0, 0, 0] - xbar) <= 1e-13 and abs(got["R"][0, 0, 0, 0] - P) <= 1e-13
    assert abs(got["xt"][0, 0, 0] - xu.mean()) <= 1e-13 * abs(xu.mean())
    Rt = ((xu - xu.mean()) ** 2).sum()
    assert abs(got["Rt"][0, 0, 0, 0] - Rt) <= 1e-13 * Rt
    w = np.sqrt(r1) * nc.normals(seed, 0, nc.STREAM_DYNAMICS, 1, 2)[:, 0]
    assert np.max(np.abs(got["members"][0, :, 0] - (xu + w))) <= 1e-13


def _tree(v):
    slot = [0.0] * 256
    for s in range(256):
        acc = 0.0
        for i in range(s, len(v), 256):
            acc = acc + float(v[i])
        slot[s] = acc
    n = 256
    while n > 1:
        slot = [slot[2 * j] + slot[2 * j + 1] for j in range(n // 2)]
        n //= 2
    return slot[0]


def test_the_sum_over_the_ensemble_is_the_stated_tree(host):
    """2b. 256 + 1 values between 1 and 2 (every addition rounds): llpf_enkf_sum is the tree the header states; a left-to-right sum
    and the tree of the first 256 with the last value added at the end are other bits."""
    rng = np.random.default_rng(4)
    v = rng.uniform(1.0, 2.0, 257)
    got = host.enkf_host_sum(nc._p(v), 257)
    assert got == _tree(v)
    seq = 0.0
    for z in v:
        seq = seq + float(z)
    assert got != seq and got != _tree(v[:256]) + float(v[256])
    for n in (1, 2, 255, 256):
        assert host.enkf_host_sum(nc._p(v), n) == _tree(v[:n]), n


def test_inflation(host):
    """2c. rho = 1 is the bits of no inflation; rho = 1.5 multiplies the spread by 1.5 and leaves the mean, both to rounding."""
    m = M.lg_test_model()
    X0 = nc.host_init(host, [m], 300, 8)
    U, Y = np.zeros((1, 1)), np.full((1, 1), np.nan)
    base = nc.host_run(host, [m], X0, U, Y, 1, 8)
    one = nc.host_run(host, [m], X0, U, Y, 1, 8, rho=1.0)
    assert kc.bits_equal(base["members"], one["members"])
    big = nc.host_run(host, [m], X0, U, Y, 1, 8, rho=1.5)
    xb, xb2 = base["members"][0].mean(axis=0), big["members"][0].mean(axis=0)
    assert np.max(np.abs(xb - xb2)) <= 1e-14 * np.max(np.abs(xb) + 1.0)
    d0, d1 = base["members"][0] - xb, big["members"][0] - xb2
    assert np.max(np.abs(d1 - 1.5 * d0)) <= 1e-13 * np.max(np.abs(d0))
    assert np.max(np.abs(big["state"][1][0] - 2.25 * base["state"][1][0])) <= 1e-12 * np.max(np.abs(base["state"][1][0]))


@pytest.mark.parametrize("N,bound", [(256, 20.0), (1000, 20.0)])
def test_loglik_tracks_kalman_over_the_noise_sweep(host, N, bound):
    """3. The reference's bars for the particle filter (tests/test_oracle_statistical.py) on the same sweep: 11 noise levels, T = 500,
    data from seed 0; argmax in 4..6 and max |ll_KF - ll_EnKF| < 20 for one fixed seed.  (A numpy EnKF with numpy's own generator stays
    at 1.9 (N = 256) and 0.9 (N = 1000) over 8 seeds with argmax 5: a failure here is a defect, not noise.)"""
    svec = 10.0 ** np.linspace(-2, 0, 11)
    _, U, Y = M.simulate_lg(M.lg_test_model(0.1), 500, seed=0)
    models = [M.lg_test_model(s) for s in svec]
    X0 = nc.host_init(host, models, N, 11)
    ll = nc.host_run(host, models, X0, U, Y, 500, 11, t_index0=1.0)["ll"]
    kf = np.array([ob.kalman_loglik(m, U, Y) for m in models])
    print("N = %d: max |ll_KF - ll_EnKF| = %.3f, argmax %d (KF %d)" % (N, np.max(np.abs(kf - ll)), int(np.argmax(ll)), int(np.argmax(kf))))
    assert 4 <= int(np.argmax(kf)) <= 6 and 4 <= int(np.argmax(ll)) <= 6
    assert np.max(np.abs(kf - ll)) < bound


NAMES = ["llpf_enkf_bank_" + v for v in ("create", "destroy", "reset", "seed", "set_models", "set_inflation", "run", "correct", "predict",
                                         "get_state", "get_members", "set_members")]


def test_the_symbols_are_declared_exported_and_bound():
    """4a. the twelve llpf_enkf_bank_* symbols: in include/llpf.h, in the library, in _capi.SYMBOLS; both classes exported"""
    header = open(os.path.join(nc.kh.ROOT, "include", "llpf.h")).read()
    L = _capi.lib()
    for n in NAMES:
        assert n + "(" in header and hasattr(L, n) and n in _capi.SYMBOLS, n
    assert issubclass(llpf_amd.EnsembleKalmanFilterBank, llpf_amd.api._KfBank) and issubclass(_capi.EnkfBankHandle, _capi._KfBankHandle)
    assert "EnsembleKalmanFilter" in llpf_amd.api.__all__ and "EnsembleKalmanFilterBank" in llpf_amd.api.__all__


def _create(models, N=64, seed=0):
    L = _capi.lib()
    arr = (S.Model * len(models))(*models)
    h = C.c_void_p()
    rc = L.llpf_enkf_bank_create(0, arr, len(models), N, seed, C.byref(h))
    if rc == _capi.OK:
        L.llpf_enkf_bank_destroy(h)
    return rc, L.llpf_last_error().decode()


def test_bad_arguments_are_refused_with_the_banks_name(monkeypatch):
    """4b. N < 2, N above the limit, a `loglik` model and the Rao-Blackwellized ids answer LLPF_ERR_ARG with a message that starts with
    the bank's name, with or without a device; `noise` and `initial` are admitted (past the argument checks).  The inflation is checked
    behind the handle (a null handle is the first answer of every export): its refusal by the C ABI is tested on the GPU, the Python
    classes refuse it here."""
    lg = M.lg_test_model()
    for N, word in ((1, ">= 2"), (0, ">= 2"), (65537, "65536")):
        rc, msg = _create([lg], N)
        assert rc == _capi.ERR_ARG and msg.startswith("enkf") and word in msg, (N, rc, msg)
    for mid in (S.MODEL_RB_LINEAR, S.MODEL_RB_BILINEAR):
        m = S.Model.from_buffer_copy(bytes(lg))
        m.model_id = mid
        rc, msg = _create([m])
        assert rc == _capi.ERR_ARG and "Rao-Blackwellized" in msg and msg.startswith("enkf"), (mid, rc, msg)
    monkeypatch.setenv("LLPF_JIT_COMPILE_ONLY", "1")
    m = S.Model.from_buffer_copy(bytes(lg))
    m.model_id = _capi.model_compile(UM.LAPLACE_SRC + "\n// test_enkf\n", 2, 1)
    rc, msg = _create([m])
    assert rc == _capi.ERR_ARG and "loglik" in msg and msg.startswith("enkf"), (rc, msg)
    for src in (UM.LAPLACE_NOISE_SRC, UM.MULT_NOISE_BOX_SRC):
        m.model_id = _capi.model_compile(src + "\n// test_enkf\n", 2, 1)
        rc, msg = _create([m])
        assert rc in (_capi.OK, _capi.ERR_NO_DEVICE), (rc, msg)
    rc, msg = _create([lg, M.quadtank_model()])
    assert rc == _capi.ERR_ARG and "differ from filter 0" in msg
    d0 = llpf_amd.MvNormal(np.zeros(2), 1.0)
    for rho in (0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="enkf"):
            llpf_amd.EnsembleKalmanFilter(llpf_amd.LinearDynamics(np.eye(2)), llpf_amd.LinearMeasurement(np.eye(2)), 0.1, 0.1, d0, 10, inflation=rho)
    f = llpf_amd.EnsembleKalmanFilter(llpf_amd.LinearDynamics(np.eye(2)), llpf_amd.LinearMeasurement(np.eye(2)), 0.1, 0.1, d0, 10)
    with pytest.raises(TypeError):
        llpf_amd.smooth(f, np.zeros((3, 0)), np.zeros((3, 2)))
    box = llpf_amd.EnsembleKalmanFilter(llpf_amd.UserDynamics(UM.MULT_NOISE_BOX_SRC, 2, 1, 1, A=np.eye(2), B=np.zeros((2, 1)), C=np.array([[1.0, 0.0]]),
                                                              qt=(0.1, 0.05, -1.0, -1.0, 1.0, 1.0)), llpf_amd.UserMeasurement(),
                                        llpf_amd.UserNoise(), 0.25, llpf_amd.UserInitial(), 50)
    assert box.nx == 2 and box.ny == 1 and _capi.model_traits(box._model.model_id) & _capi.TRAIT_NOISE


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_no_device_is_an_error_not_a_fallback():
    """4c. Valid arguments on a machine without a device: LLPF_ERR_NO_DEVICE."""
    for m in (M.lg_test_model(), M.quadtank_model()):
        rc, msg = _create([m])
        assert rc == _capi.ERR_NO_DEVICE, (rc, msg)
    f = llpf_amd.EnsembleKalmanFilter(llpf_amd.QuadTankDynamics(), llpf_amd.QuadTankMeasurement(), np.full(4, 0.1), np.full(2, 1e-4),
                                      llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)), 100)
    with pytest.raises(_capi.LLPFError) as ei:
        llpf_amd.loglik(f, *M.quadtank_data(5))
    assert ei.value.code == _capi.ERR_NO_DEVICE


@pytest.mark.parametrize("N", [2, 257])
def test_the_twin_as_a_stand_alone_program_under_sanitizers(tmp_path, N):
    """5. tests/enkf_host.c with its own main (-DENKF_HOST_MAIN), built with -fsanitize=address,undefined and run as a program: every
    output, a missing row and inflation at N = 2 and N = 257 without a report."""
    import shutil
    import subprocess
    cc = shutil.which("cc") or shutil.which("gcc")
    exe = str(tmp_path / "enkf_main")
    build = subprocess.run([cc, "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DENKF_HOST_MAIN",
                            "-I", nc.kh.SHARED, "-I", os.path.join(nc.kh.ROOT, "include"), "-I", os.path.join(nc.kh.ROOT, "tests"),
                            os.path.join(nc.kh.ROOT, "tests", "enkf_host.c"), "-o", exe, "-lm"], capture_output=True, text=True)
    if build.returncode != 0 and "sanitize" in build.stderr + build.stdout:
        pytest.skip("this compiler has no address / undefined-behaviour sanitizer runtime")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, str(N)], capture_output=True, text=True)
    assert run.returncode == 0 and "rc=0" in run.stdout and not run.stderr, (run.stdout, run.stderr)
