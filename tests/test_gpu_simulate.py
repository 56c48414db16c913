"""llpf_simulate / llpf_bank_simulate (include/llpf.h; kernels/simulate.hpp, host/simulate.hpp): M trajectories of the reference's
simulate(pf, T, du) (src/filtering.jl:457-477) on the device.  Trajectory m is particle m of a filter that never resamples, so the engine's
own reset! and predict! are the yardstick, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import models as M
import user_models as UM

pytestmark = pytest.mark.gpu

ALL = _capi.SIM_DYNAMICS_NOISE | _capi.SIM_MEASUREMENT_NOISE
BITS = lambda a: np.ascontiguousarray(a).view(np.uint64)


def _handle(model, N, seed):
    """a filter that never resamples (threshold 0) with N = M particles"""
    h = _capi.FilterHandle(S.make_config(model, N, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.0, seed, 0))
    h.seed(seed)
    return h


def _lg(nx, nu, ny, seed=0, kind_g=S.COV_DIAG):
    rng = np.random.default_rng(seed)
    Tr = rng.standard_normal((nx, nx))
    A = Tr @ np.diag(np.linspace(0.5, 0.95, nx)) @ np.linalg.inv(Tr)
    B = rng.standard_normal((nx, nu))
    Cm = rng.standard_normal((ny, nx))
    df = S.make_gaussian(np.zeros(nx), np.linspace(0.05, 0.2, nx))
    if kind_g == S.COV_SCAL:
        dg = S.make_gaussian(np.zeros(ny), 0.3)
    elif kind_g == S.COV_DIAG:
        dg = S.make_gaussian(np.zeros(ny), np.linspace(0.2, 0.5, ny))
    else:
        G = rng.standard_normal((ny, ny))
        dg = S.make_gaussian(np.zeros(ny), G @ G.T + 0.5 * np.eye(ny))
    d0 = S.make_gaussian(rng.standard_normal(nx), 2.0)
    return S.make_lg_model(A, B, Cm, df, dg, d0, 1.0)


def _mats(model):
    nx, nu, ny = model.nx, model.nu, model.ny
    A = np.array(model.A[:nx * nx]).reshape(nx, nx)
    B = np.array(model.B[:nx * nu]).reshape(nx, nu)
    Cm = np.array(model.C[:ny * nx]).reshape(ny, nx)
    return A, B, Cm


def _user_model(src, base, qt):
    m = S.Model.from_buffer_copy(bytes(base))
    m.model_id = _capi.model_compile(src, m.nx, m.ny)
    for i, v in enumerate(qt):
        m.qt[i] = v
    return m


def _mult_noise_box():
    box = [-1.0, 0.5, 3.0, 2.5]
    return _user_model(UM.MULT_NOISE_BOX_SRC, M.lg_test_model(), [0.1, 0.25] + box)


def _case(name):
    if name == "lg_2x2":
        return M.lg_c1_model(), 0.0
    if name == "lg_6x3":
        return _lg(6, 2, 3, seed=4), 0.0
    if name == "quadtank":
        return M.quadtank_model(), 495.0          # tau crosses the t > 500 switch of the outflow coefficient
    return _mult_noise_box(), 0.0


@pytest.mark.parametrize("name", ["lg_2x2", "lg_6x3", "quadtank", "user_noise_hook"])
def test_states_are_the_engines_own_predict_bit_for_bit(name):
    model, ti0 = _case(name)
    Mtr, T, seed = 1500, 10, 1234
    rng = np.random.default_rng(1)
    U = (0.3 + 0.1 * rng.random((T, model.nu))) if name == "quadtank" else rng.standard_normal((T, model.nu))
    h = _handle(model, Mtr, seed)
    for k in range(2):                      # the step counter is 2 when the comparison starts
        h.predict(U[0], 0.0)
    step0 = 2
    X, Y = h.simulate(Mtr, T, U, t_index0=ti0, seed=seed, step0=step0, flags=ALL)
    assert X.shape == (T, Mtr, model.nx) and Y.shape == (T, Mtr, model.ny)
    x0 = np.array(S.gaussian_mean(model.initial_density))
    assert np.array_equal(BITS(X[0]), BITS(np.broadcast_to(x0, (Mtr, model.nx))))
    h.set_particles(np.broadcast_to(x0, (Mtr, model.nx)).copy())
    for t in range(T - 1):
        h.predict(U[t], (ti0 + t) * model.Ts)
        assert np.array_equal(BITS(h.particles()), BITS(X[t + 1])), "step %d" % t
    assert h.resample_count() == 0 and not h.last_resampled()
    assert np.std(X[-1][:, 0]) > 0


@pytest.mark.parametrize("name", ["lg_2x2", "user_initial_hook"])
def test_sample_initial_is_the_draw_of_reset(name):
    model = M.lg_c1_model() if name == "lg_2x2" else _mult_noise_box()
    Mtr, seed = 3000, 77
    h = _handle(model, Mtr, seed)
    X, _ = h.simulate(Mtr, 3, np.zeros((3, model.nu)), seed=seed, flags=ALL | _capi.SIM_SAMPLE_INITIAL, measurements=False)
    h.seed(seed)
    h.reset()
    assert np.array_equal(BITS(h.particles()), BITS(X[0]))
    assert np.std(X[0][:, 0]) > 0.3


@pytest.mark.parametrize("kind", [S.COV_SCAL, S.COV_DIAG, S.COV_FULL])
def test_measurements_and_their_noise(kind):
    model = _lg(3, 1, 2, seed=2, kind_g=kind)
    A, B, Cm = _mats(model)
    Mtr, T, seed, step0 = 2000, 6, 5, 9
    U = np.random.default_rng(3).standard_normal((T, 1))
    h = _handle(model, 256, seed)
    X, Yn = h.simulate(Mtr, T, U, seed=seed, step0=step0, flags=_capi.SIM_DYNAMICS_NOISE)
    X2, Y = h.simulate(Mtr, T, U, seed=seed, step0=step0, flags=ALL)
    assert np.array_equal(BITS(X), BITS(X2))                    # the measurement noise has a stream of its own
    ref = (Cm[:, 0] * X[..., :1] + Cm[:, 1] * X[..., 1:2]) + Cm[:, 2] * X[..., 2:3]      # C x in the kernel's order
    assert np.all(np.abs(Yn - ref) <= 1e-15 * (np.abs(X) @ np.abs(Cm).T))
    L = np.linalg.cholesky(S.gaussian_cov_matrix(model.measurement_density))
    for t in range(T):
        e = _capi.selftest_normals(seed, step0 + t, 4, 2, Mtr)
        assert np.max(np.abs((Y[t] - Yn[t]) - e @ L.T)) <= 1e-14 * max(1.0, np.max(np.abs(e @ L.T)))


def test_quadtank_measurement_is_the_level_pair():
    model = M.quadtank_model()
    U = np.full((5, 2), 0.25)
    X, Y = _handle(model, 256, 3).simulate(700, 5, U, seed=3, flags=_capi.SIM_DYNAMICS_NOISE)
    assert np.array_equal(BITS(Y), BITS(X[:, :, :2]))


def test_sample_moments_are_the_closed_form_prior():
    model = M.lg_c1_model()
    A, B, Cm = _mats(model)
    Q = S.gaussian_cov_matrix(model.dynamics_density)
    R = S.gaussian_cov_matrix(model.measurement_density)
    Mtr, T = 100_000, 21
    U = np.random.default_rng(8).standard_normal((T, model.nu))
    X, Y = _handle(model, 256, 11).simulate(Mtr, T, U, seed=11, flags=ALL | _capi.SIM_SAMPLE_INITIAL)
    m = np.array(S.gaussian_mean(model.initial_density))
    P = S.gaussian_cov_matrix(model.initial_density)
    for t in range(T):
        if t in (0, 1, 5, 20):
            for data, mean, cov in ((X[t], m, P), (Y[t], Cm @ m, Cm @ P @ Cm.T + R)):
                se = np.sqrt(np.diag(cov) / Mtr)
                assert np.all(np.abs(data.mean(0) - mean) < 5 * se), (t, data.mean(0), mean)
                d = np.diag(cov)
                se_c = np.sqrt((np.outer(d, d) + cov ** 2) / Mtr)
                assert np.all(np.abs(np.cov(data.T) - cov) < 5 * se_c), (t, np.cov(data.T), cov)
        m = A @ m + B @ U[t]
        P = A @ P @ A.T + Q


def test_bank_slice_is_the_single_filter_with_seed_plus_k():
    models = [_lg(2, 1, 2, seed=s) for s in (1, 2, 3)]
    Mtr, T, seed = 700, 12, 40
    U = np.random.default_rng(4).standard_normal((3, Mtr, T, 1))
    bank = _capi.BankHandle(S.make_config(models[0], 1024, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 0, 0), models)
    flags = ALL | _capi.SIM_SAMPLE_INITIAL
    XB, YB = bank.simulate(Mtr, T, U, u_per_trajectory=True, t_index0=2.0, seed=seed, step0=3, flags=flags)
    assert XB.shape == (3, T, Mtr, 2) and YB.shape == (3, T, Mtr, 2)
    for k in range(3):
        X, Y = _handle(models[k], 1024, 0).simulate(Mtr, T, U[k], u_per_trajectory=True, t_index0=2.0, seed=seed + k, step0=3, flags=flags)
        assert np.array_equal(BITS(XB[k]), BITS(X)) and np.array_equal(BITS(YB[k]), BITS(Y))
    assert not np.array_equal(XB[0], XB[1])


def test_chunks_a_long_run_has_the_short_run_as_prefix():
    # M = 64, LG 2 x 2 with X and Y: 2 KiB per step, so the chunk rule gives chunks of 256 steps: 700 steps are three chunks,
    # 300 end inside the second
    model = M.lg_c1_model()
    Mtr, TL, TS = 64, 700, 300
    U = np.random.default_rng(5).standard_normal((Mtr, TL, model.nu))
    h = _handle(model, 256, 9)
    flags = ALL | _capi.SIM_SAMPLE_INITIAL
    XL, YL = h.simulate(Mtr, TL, U, u_per_trajectory=True, seed=21, step0=1, flags=flags)
    XS, YS = h.simulate(Mtr, TS, U[:, :TS].copy(), u_per_trajectory=True, seed=21, step0=1, flags=flags)
    assert np.array_equal(BITS(XL[:TS]), BITS(XS)) and np.array_equal(BITS(YL[:TS]), BITS(YS))
    XL2, YL2 = h.simulate(Mtr, TL, U, u_per_trajectory=True, seed=21, step0=1, flags=flags)
    assert np.array_equal(BITS(XL), BITS(XL2)) and np.array_equal(BITS(YL), BITS(YL2))
    assert np.all(np.isfinite(XL)) and np.std(XL[-1]) > 0
    _, Yonly = h.simulate(Mtr, TL, U, u_per_trajectory=True, seed=21, step0=1, flags=flags, states=False)
    assert np.array_equal(BITS(Yonly), BITS(YL))               # Y alone: the same numbers
    Xonly, _ = h.simulate(Mtr, TL, U, u_per_trajectory=True, seed=21, step0=1, flags=flags, measurements=False)
    assert np.array_equal(BITS(Xonly), BITS(XL))               # and X alone


@pytest.mark.parametrize("per_trajectory", [False, True], ids=["shared_u", "per_trajectory_u"])
def test_chunks_limited_by_bytes_with_a_ragged_tail(per_trajectory):
    # M = 2^15, LG 2 x 2 with X and Y: 1 MiB per step, so the 64 MiB staging limit gives chunks of 64 steps: 200 steps are
    # chunks of 64, 64, 64 and 8 (both staging slots are used twice, the last chunk is short), 130 end inside the third
    model = M.lg_c1_model()
    Mtr, TL, TS = 1 << 15, 200, 130
    U = np.random.default_rng(6).standard_normal((Mtr, TL, model.nu) if per_trajectory else (TL, model.nu))
    h = _handle(model, 256, 9)
    sim = lambda m, T, u, **kw: h.simulate(m, T, np.ascontiguousarray(u), u_per_trajectory=per_trajectory, seed=33, step0=2,
                                           flags=ALL | _capi.SIM_SAMPLE_INITIAL, **kw)
    XL, YL = sim(Mtr, TL, U)
    XS, YS = sim(Mtr, TS, U[..., :TS, :])
    assert np.array_equal(BITS(XL[:TS]), BITS(XS)) and np.array_equal(BITS(YL[:TS]), BITS(YS))
    # trajectory m depends on m and the seed only: the first 64 of 2^15 are the 64 of a small run (one chunk of 200 steps)
    X64, Y64 = sim(64, TL, U[:64] if per_trajectory else U)
    assert np.array_equal(BITS(XL[:, :64]), BITS(X64)) and np.array_equal(BITS(YL[:, :64]), BITS(Y64))
    assert np.all(np.isfinite(XL)) and np.std(XL[-1]) > 0 and np.std(YL[-1]) > 0
    # one output alone (0.5 MiB per step: chunks of 128 and 72) sits at offset 0 of the staging
    _, Yonly = sim(Mtr, TL, U, states=False)
    assert np.array_equal(BITS(Yonly), BITS(YL))
    Xonly, _ = sim(Mtr, TL, U, measurements=False)
    assert np.array_equal(BITS(Xonly), BITS(XL))


def test_the_handle_is_untouched():
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 40)
    cfg = S.make_config(model, 5000, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 13, 0)
    a, b = _capi.FilterHandle(cfg), _capi.FilterHandle(cfg)
    for h in (a, b):
        h.reset()
        h.run(U, Y, 0.0)
    a.simulate(3000, 50, U[:1].repeat(50, 0), seed=13, flags=ALL | _capi.SIM_SAMPLE_INITIAL)
    ra, rb = a.run(U, Y, 0.0, ll_steps=True), b.run(U, Y, 0.0, ll_steps=True)
    assert np.array_equal(BITS(ra["ll_steps"]), BITS(rb["ll_steps"]))
    for get in ("particles", "weights", "ancestors"):
        assert np.array_equal(getattr(a, get)(), getattr(b, get)())
    assert a.resample_count() == b.resample_count() and a.index() == b.index()


def test_arguments_are_checked():
    model = M.lg_test_model()
    h = _handle(model, 256, 1)
    L = _capi.lib()
    U = np.zeros((4, 1))
    X = np.zeros((4, 8, 2))
    Y = np.zeros((4, 8, 1))

    def call(Mtr=8, T=4, u=U, flags=ALL, x=X, y=Y, upt=0):
        return L.llpf_simulate(h.h, C.c_int64(Mtr), C.c_int64(T), _capi.dptr(u), upt, 0.0, 1, 0, flags, _capi.dptr(x), _capi.dptr(y))

    assert call() == _capi.OK
    for kw in (dict(Mtr=0), dict(T=0), dict(x=None, y=None), dict(flags=8), dict(flags=-1), dict(u=None), dict(upt=2),
               dict(Mtr=1 << 31), dict(Mtr=(1 << 31) - 1, T=1 << 40)):
        assert call(**kw) == _capi.ERR_ARG, kw
        assert L.llpf_last_error()
    assert call() == _capi.OK                                    # and the handle goes on working
    rb = _capi.FilterHandle(S.make_config(M.lg_test_model(), 256, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 1, 0))
    assert rb.simulate(4, 4, U)[0].shape == (4, 4, 2)


def test_rao_blackwellized_kinds_are_refused():
    import rbfull_models as RM
    m = RM.quadtank_case()
    h = _capi.FilterHandle(S.make_config(m, 512, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 1, 0))
    with pytest.raises(_capi.LLPFError) as ei:
        h.simulate(4, 4, np.zeros((4, m.nu)))
    assert ei.value.code == _capi.ERR_ARG and "Rao-Blackwellized" in str(ei.value)


# ---- through Python ---------------------------------------------------------------------------------------------------------------
def _pendulum_objects():
    import llpf_amd
    dyn = llpf_amd.UserDynamics(UM.PENDULUM_SRC, 2, 1, 1, qt=[9.81, 0.3])
    df = llpf_amd.MvNormal(np.zeros(2), 0.01)
    dg = llpf_amd.MvNormal(np.zeros(1), 0.04)
    d0 = llpf_amd.MvNormal(np.array([0.5, 0.0]), 0.1)
    return dyn, df, dg, d0


def test_device_only_models_through_python():
    import llpf_amd
    dyn, df, dg, d0 = _pendulum_objects()
    pf = llpf_amd.ParticleFilter(1000, dyn, llpf_amd.UserMeasurement(), df, dg, d0, Ts=0.05)
    du = llpf_amd.MvNormal(np.zeros(1), 0.1)
    with pytest.raises(TypeError):
        llpf_amd.simulate(pf, 20, du)                         # no host version of the snippet
    x, u, y = llpf_amd.simulate_batch(pf, 20, 500, du, seed=3)
    assert x.shape == (20, 500, 2) and u.shape == (20, 1) and y.shape == (20, 500, 1)
    assert np.all(np.isfinite(x)) and np.std(x[-1, :, 0]) > 0
    # a model with its own process noise and initial density (UserNoise / UserInitial)
    lg = M.lg_test_model()
    A, B, Cm = _mats(lg)
    qt = [0.1, 0.25, -1.0, 0.5, 3.0, 2.5]
    dyn2 = llpf_amd.UserDynamics(UM.MULT_NOISE_BOX_SRC, 2, 1, 1, A=A, B=B, C=Cm, qt=qt)
    pf2 = llpf_amd.ParticleFilter(1000, dyn2, llpf_amd.UserMeasurement(), llpf_amd.UserNoise(), dg, llpf_amd.UserInitial(), rng=4)
    with pytest.raises((TypeError, AttributeError)):
        llpf_amd.simulate(pf2, 20, du)
    x2, _, y2 = llpf_amd.simulate_batch(pf2, 20, 800, du, seed=4, sample_initial=True)
    assert np.all(x2[0] >= [-1.0, 0.5]) and np.all(x2[0] < [3.0, 2.5])            # the uniform box of the snippet's `initial`
    pf2._h.seed(4)
    pf2._h.reset()
    x3, _, _ = llpf_amd.simulate_batch(pf2, 20, 1000, du, seed=4, sample_initial=True)
    assert np.array_equal(BITS(x3[0]), BITS(pf2._h.particles()))


def test_a_traced_callable_simulates_the_same_through_both_paths():
    import llpf_amd
    A, B, Cm = _mats(M.lg_test_model())

    def f(x, u, p, t):
        return [A[0, 0] * x[0] + A[0, 1] * x[1] + B[0, 0] * u[0], A[1, 0] * x[0] + A[1, 1] * x[1] + 0.05 * llpf_amd.tracing.exp(0.1 * x[0])]

    def g(x, u, p, t):
        return [x[1] * x[1] + x[0]]

    df = llpf_amd.MvNormal(np.zeros(2), 0.01)
    dg = llpf_amd.MvNormal(np.zeros(1), 1.0)
    d0 = llpf_amd.MvNormal(np.array([0.3, -0.5]), 4.0)
    pf = llpf_amd.ParticleFilter(1000, f, g, df, dg, d0, nu=1)
    u = np.random.default_rng(6).standard_normal((30, 1))
    xh, _, yh = llpf_amd.simulate(pf, u, dynamics_noise=False, measurement_noise=False)
    xd, _, yd = llpf_amd.simulate_batch(pf, u, 3, dynamics_noise=False, measurement_noise=False)
    for m in range(3):
        assert np.allclose(xd[:, m], xh, rtol=1e-12, atol=1e-12) and np.allclose(yd[:, m], yh, rtol=1e-12, atol=1e-12)


def test_bank_data_filtered_by_the_bank_tracks_the_states():
    import llpf_amd
    specs = []
    for k, a in enumerate((0.9, 0.95, 0.8)):
        A = np.array([[a, 0.1], [-0.1, a]])
        specs.append((llpf_amd.LinearDynamics(A, np.array([[0.5], [0.0]])), llpf_amd.LinearMeasurement(np.eye(2)),
                      llpf_amd.MvNormal(np.zeros(2), 0.05), llpf_amd.MvNormal(np.zeros(2), 0.1), llpf_amd.MvNormal(np.zeros(2), 1.0)))
    bank = llpf_amd.FilterBank(20000, specs, rng=5)
    T = 100
    x, u, y = bank.simulate(T, 1, llpf_amd.MvNormal(np.zeros(1), 1.0), seed=1000, sample_initial=True)
    assert x.shape == (3, T, 1, 2) and y.shape == (3, T, 1, 2) and u.shape == (T, 1)
    bank._h.reset()
    r = bank._h.run_multi(np.broadcast_to(u, (3, T, 1)).copy(), y[:, :, 0, :].copy(), t_index0=0.0, xmean=True)
    for k in range(3):
        A = specs[k][0].A
        P = np.eye(2)
        for _ in range(200):
            P = A @ P @ A.T + 0.05 * np.eye(2)
        rmse = np.sqrt(np.mean((r["xmean"][10:, k, :] - x[k, 10:, 0, :]) ** 2))
        assert rmse < np.sqrt(np.mean(np.diag(P))), (k, rmse, P)
