"""Banks of square-root extended Kalman filters on the device (llpf_sqekf_bank_*; kernels/sqekf.hpp, host/sqekf.hpp): the GPU
reproduces the host build of csrc/shared/llpf_sqekf.h (tests/sqekf_host.c) bit for bit in every output and in (x, R, L) — precompiled and
run-time compiled models, whatever the bank, the chunking of T or the split of a run, on the systems where the extended bank turns NaN
as well — and the Python API (SqExtendedKalmanFilter, SqExtendedKalmanFilterBank) is that filter at the extended bank's times."""
import ctypes as C

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import kalman_common as kc
from kalman_common import _data, _same
from gpu_common import _Inject
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS, lg_models, quadtank_models, with_id
import models as M
import sqekf_common as qc
import ukf_common as uc

pytestmark = pytest.mark.gpu

FAM = qc.FAMILY
_bank = qc.bank


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return qc.build_host(tmp_path_factory.mktemp("sqekf_host"))


def _state_is(b, st, what):
    """get_state of the bank — x, R and the factor L — is the twin's final (x, R, L)"""
    x, R, L = b.get_state(factor=True)
    assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]) and kc.bits_equal(L, st[2]), (what, "final state")


@pytest.mark.parametrize("nx", range(1, 5))
def test_lingauss_bit_identical_to_the_host_header_for_every_precompiled_shape(host, nx):
    """16 of the 17 precompiled shapes: F = 130 (two full waves and a tail of 2) random filters, T = 40, rows 7, 8 and 39 missing, nu
    drawn in 0..3, every output and the final (x, R, L)"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        b, g, _, st, _, _ = kg.check_shape(FAM, host, rng, F=130, T=40, nx=nx, ny=ny, nu=nu, missing=(7, 8, 39), what=(nx, ny))
        assert np.isfinite(g["ll"]).all()
        _state_is(b, st, (nx, ny))
        b.close()


@pytest.mark.parametrize("F", [1, 63, 64, 65])
def test_bank_sizes_and_chunk_edges(host, F):
    """(2, 1), nu = 1 around the wave of 64 and the pipe's chunk of 256 steps: T in {1, 255, 256, 257}, the final x and R against the twin"""
    kg.check_bank_sizes_and_chunk_edges(FAM, host, seed=100 + F, F=F, nx=2, ny=1, nu=1, missing=(0, 254, 255, 256), Ts=(1, 255, 256, 257))


def test_each_output_alone(host):
    """every optional output asked for on its own is the column of the run with all of them (R and Rt are formed only where they are
    asked for): F = 65 (a full workgroup and a ragged one), T = 3"""
    kg.check_each_output_alone(FAM, host, seed=77, F=65, T=3, nx=2, ny=1, nu=1)


def test_quadtank_precompiled_shape_across_the_switch_time(host):
    """the 17th shape: the built-in quad-tank, F = 65 with per-filter parameters, T = 60 from t_index0 = 470 (tau crosses TSWITCH = 500)
    with a missing row: the device's RK4 and its Jacobian in the shared header's order under the two triangularisations"""
    models = quadtank_models(65)
    U, Y = M.quadtank_data(60)
    Y = Y.copy()
    Y[31, 0] = np.nan
    b = _bank(models)
    g = b.run(U, Y, outputs=OUTS, t_index0=470.0)
    h, st = qc.host_run(host, models, U, Y, 60, t_index0=470.0)
    _same(g, h, what="quad-tank across the switch")
    assert np.isfinite(g["ll"]).all() and len(set(g["ll"].tolist())) > 40
    _state_is(b, st, "quad-tank")
    b.close()


def test_runtime_compiled_shapes(host):
    """k_sqekf from a hiprtc program of the model's own: the linear-Gaussian model above 4 states at (5, 1) and (8, 4) (the largest
    pre-array, 144 doubles), F = 65, T = 20; the pendulum snippet at F = 65, T = 60; x0^2 as a snippet, bit for bit"""
    rng = np.random.default_rng(21)
    for nx, ny, nu in ((5, 1, 0), (8, 4, 1)):
        b, _, _, st, _, _ = kg.check_shape(FAM, host, rng, F=65, T=20, nx=nx, ny=ny, nu=nu, missing=(7,), what=("LG", nx, ny))
        _state_is(b, st, ("LG", nx, ny))
        b.close()
    pid = _capi.model_compile(ec.PENDULUM_JAC_SRC, 2, 1)
    pend = kg.pendulum_models(65)
    U, Y = uc.pendulum_data(60)
    Y = Y.copy()
    Y[3, 0] = np.nan
    g = _bank([with_id(m, pid) for m in pend]).run(U, Y, outputs=OUTS)
    h, _ = qc.host_run(host, pend, U, Y, 60, kind=ec.KIND_PENDULUM)
    _same(g, h, what="pendulum")
    assert np.isfinite(g["ll"]).all()
    sq = kg.square_models(65)
    Y = 3.0 + 0.5 * rng.standard_normal((40, 1))
    h, _ = qc.host_run(host, sq, None, Y, 40, kind=ec.KIND_SQUARE)
    sid = _capi.model_compile(ec.SQUARE_JAC_SRC, 1, 1)
    g = _bank([with_id(m, sid) for m in sq]).run(None, Y, outputs=OUTS)
    _same(g, h, what="square snippet")


def test_square_model_as_a_snippet_and_as_a_traced_callable_through_the_python_filter(host):
    """x0^2 through SqExtendedKalmanFilter: the snippet with hand-written members is the twin bit for bit; the traced callable
    (forward-mode Jacobians, another operation order) is the twin to 1e-10"""
    rng = np.random.default_rng(3)
    Ys = 3.0 + 0.5 * rng.standard_normal((40, 1))
    d1 = llpf_amd.MvNormal(np.array([1.0]), 0.36)
    h, _ = qc.host_run(host, [ec.square_model(1.0, 0.36)], None, Ys, 40, kind=ec.KIND_SQUARE)
    snip = llpf_amd.SqExtendedKalmanFilter(llpf_amd.UserDynamics(ec.SQUARE_JAC_SRC, 1, 0, 1), llpf_amd.UserMeasurement(), 0.1, 0.25, d1)
    tr_ = llpf_amd.SqExtendedKalmanFilter(lambda x, u, p, t: [x[0]], lambda x, u, p, t: [x[0] * x[0]], 0.1, 0.25, d1, nu=0, ny=1)
    ss, st = llpf_amd.forward_trajectory(snip, None, Ys), llpf_amd.forward_trajectory(tr_, None, Ys)
    for k in ("x", "xt", "R", "Rt", "e"):
        assert kc.bits_equal(getattr(ss, k), h[k][:, 0]), ("snippet", k)
        assert kc.close(getattr(st, k), h[k][:, 0]), ("traced", k)
    assert ss.ll == h["ll"][0] and abs(st.ll - h["ll"][0]) <= 1e-10 * abs(h["ll"][0])
    assert isinstance(snip._h, _capi.SqekfBankHandle)


def test_continuation_through_the_factor_set_state_and_set_models(host):
    """halves of T = 300 cut at 150 (a chunk edge inside the first half's neighbour), F = 70, (3, 2, 2): run(a) then run(b) is
    run(a + b); the second half against the twin from get_state's factor; get_state(factor=True) -> set_state(x, L=L) keeps every bit;
    set_state(x, R=R) factors as the twin does and refuses an indefinite R, both and neither; set_models is a fresh bank"""
    rng = np.random.default_rng(5)
    F, T, cut = 70, 300, 150
    models = lg_models(rng, F, 3, 2, 2)
    U, Y = _data(rng, T, 2, 2, missing=(149, 150, 256, 299))
    b = _bank(models)
    whole = b.run(U, Y, outputs=OUTS)
    b.reset()
    first = b.run(U[:cut], Y[:cut], outputs=OUTS)
    x, R, L = b.get_state(factor=True)
    assert np.array_equal(L, np.tril(L))
    second = b.run(U[cut:], Y[cut:], outputs=OUTS, t_index0=float(cut))
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    h2, st2 = qc.host_run(host, models, U[cut:], Y[cut:], T - cut, t_index0=float(cut), factor=(x, L))
    _same(second, h2, what="second half")
    _state_is(b, st2, "second half")
    fresh = _bank(models)
    fresh.set_state(x, L=L)
    xs, Rs, Ls = fresh.get_state(factor=True)
    assert kc.bits_equal(xs, x) and kc.bits_equal(Ls, L) and kc.bits_equal(Rs, R)
    _same(fresh.run(U[cut:], Y[cut:], outputs=OUTS, t_index0=float(cut)), second, what="set_state(L)")
    b.reset()
    assert kc.bits_equal(b.run(U, Y)["ll"], whole["ll"])          # ll only: nothing is staged per step
    fresh.set_state(x, R=R)                                       # through R: llpf_kf_chol of R, as the twin factors it
    viaR = fresh.run(U[cut:], Y[cut:], outputs=OUTS, t_index0=float(cut))
    hR, stR = qc.host_run(host, models, U[cut:], Y[cut:], T - cut, t_index0=float(cut), state=(x, R))
    _same(viaR, hR, what="set_state(R)")
    _state_is(fresh, stR, "set_state(R)")
    Rbad = R.copy()
    Rbad[33] = -np.eye(3)
    with pytest.raises(_capi.LLPFError) as ei:
        fresh.set_state(x, R=Rbad)
    assert ei.value.code == _capi.ERR_ARG and str(ei.value).endswith("sqekf: filter 33: R is not positive definite")
    for kw in (dict(), dict(R=R, L=L)):                           # neither, or both
        with pytest.raises(_capi.LLPFError) as ei:
            fresh.set_state(x, **kw)
        assert ei.value.code == _capi.ERR_ARG and "exactly one of R and L" in str(ei.value)
    _state_is(fresh, stR, "after the refused calls")
    other = lg_models(rng, F, 3, 2, 2)
    b.set_models(other)
    b.reset()
    g = b.run(U, Y, outputs=OUTS)
    ho, sto = qc.host_run(host, other, U, Y, T)
    _same(g, ho, what="set_models")
    _state_is(b, sto, "set_models")
    with pytest.raises(_capi.LLPFError):
        b.set_models(lg_models(rng, F, 2, 2, 2))


def test_per_filter_inputs_and_a_nan_filter(host):
    """per-filter U and Y at F = 130, T = 40, (2, 1, 1), rows 5, 6 and 30 missing for every filter and row 12 for every seventh; then
    filter 78 gets a NaN in its x through set_state: NaN in its own columns, every other filter's bits unmoved, the whole equal to the
    twin's"""
    rng = np.random.default_rng(6)
    F, T = 130, 40
    models = lg_models(rng, F, 2, 1, 1)
    U = rng.standard_normal((F, T, 1))
    Y = 2.0 * rng.standard_normal((F, T, 1))
    Y[:, [5, 6, 30], 0] = np.nan
    Y[::7, 12, 0] = np.nan
    b = _bank(models)
    x, _, L = b.get_state(factor=True)
    ok = b.run(U, Y, True, True, outputs=OUTS)
    assert np.all(ok["ll_steps"][[5, 6, 30]] == 0.0) and np.all(np.isnan(ok["e"][[5, 6, 30]]))
    h, _ = qc.host_run(host, models, U, Y, T, per_filter=3)
    _same(ok, h, what="per-filter inputs")
    x[78, 0] = np.nan
    b.set_state(x, L=L)
    bad = b.run(U, Y, True, True, outputs=OUTS)
    assert np.isnan(bad["ll"][78]) and np.all(np.isnan(bad["xt"][:, 78])) and np.all(np.isnan(bad["e"][:, 78]))
    assert np.all(np.isfinite(bad["R"][:, 78])), "the factor of a linear model does not see the state"
    keep = [f for f in range(F) if f != 78]
    for k in OUTS:
        assert kc.bits_equal(bad[k][:, keep], ok[k][:, keep]), k
    hb, _ = qc.host_run(host, models, U, Y, T, per_filter=3, factor=(x, L))
    _same(bad, hb, what="NaN filter")


def test_covariances_of_a_linear_model_are_the_square_root_kalman_banks_bits():
    """LG (3, 2) on the same descriptors: R and Rt of every step are SqkfBankHandle's bits on the device, the other outputs within 1e-10"""
    rng = np.random.default_rng(9)
    models = lg_models(rng, 65, 3, 2, 1)
    U, Y = _data(rng, 40, 1, 2, missing=(4,))
    g = _bank(models).run(U, Y, outputs=OUTS)
    s = _capi.SqkfBankHandle(0, models, None).run(U, Y, outputs=OUTS)
    for k in ("R", "Rt"):
        assert kc.bits_equal(g[k], s[k]), k
    for k in ("x", "xt", "e", "ll_steps"):
        assert kc.close(g[k], s[k]), k
    assert np.all(np.abs(g["ll"] - s["ll"]) <= 1e-10 * np.abs(s["ll"]))


@pytest.mark.parametrize("case", [0, 1])
def test_ill_conditioned_systems_on_the_device(host, case):
    """F = 64 copies of sqkf_common.ill_conditioned(case) with perturbed noise levels (sqekf_common.ill_conditioned_bank), T = 50: the
    extended bank's ll is NaN for every one of them; this bank's ll is finite and every output the twin's bits"""
    models, Y = qc.ill_conditioned_bank(case, 64)
    plain = _capi.EkfBankHandle(0, models).run(None, Y)["ll"]
    assert np.all(np.isnan(plain))                        # the condition on the inputs: the covariance form fails here
    b = _bank(models)
    g = b.run(None, Y, outputs=OUTS)
    h, st = qc.host_run(host, models, None, Y, 50)
    _same(g, h, what=("ill-conditioned", case))
    for k in OUTS + ("ll",):
        assert np.all(np.isfinite(g[k])), k
    _state_is(b, st, ("ill-conditioned", case))


def test_a_throw_is_a_status_and_arguments_are_refused_with_the_state_untouched(host):
    """error:sqekf_run is a status that leaves the state as it was; alloc:sqekf_create is LLPF_ERR_ALLOC; T < 1, stray per_filter bits, a
    non-finite t_index0, a short struct_size and a null Y are LLPF_ERR_ARG under this bank's prefix; the handle runs on"""
    rng = np.random.default_rng(45)
    models = lg_models(rng, 65, 2, 1, 1)
    U, Y = _data(rng, 10, 1, 1)
    b = _bank(models)
    b.run(U[:4], Y[:4])
    x0, _, L0 = b.get_state(factor=True)
    with _Inject("error:sqekf_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y)
    assert ei.value.code == _capi.ERR_INTERNAL and "sqekf_run" in str(ei.value)
    with _Inject("alloc:sqekf_create"):
        with pytest.raises(_capi.LLPFError) as ei:
            _bank(models)
    assert ei.value.code == _capi.ERR_ALLOC
    lib = _capi.lib()
    ll = np.zeros(65)
    out = S.KalmanOutputs()
    out.struct_size = C.sizeof(S.KalmanOutputs) - 8
    run = lambda U_, Y_, T, pf, t0, o: lib.llpf_sqekf_bank_run(b.h, _capi.dptr(U_), _capi.dptr(Y_), C.c_int64(T), pf, C.c_double(t0), _capi.dptr(ll), o)
    for args, word in (((U, Y, 0, 0, 0.0, None), "T must be >= 1"), ((U, Y, 10, 4, 0.0, None), "per_filter"),
                       ((U, Y, 10, 0, float("inf"), None), "t_index0 must be finite"), ((U, Y, 10, 0, float("nan"), None), "t_index0 must be finite"),
                       ((U, Y, 10, 0, 0.0, C.byref(out)), "struct_size"), ((U, None, 10, 0, 0.0, None), "Y is null"),
                       ((None, Y, 10, 0, 0.0, None), "U is null")):
        assert run(*args) == _capi.ERR_ARG, word
        msg = lib.llpf_last_error().decode()
        assert msg.startswith("sqekf: ") and word in msg, msg
    x1, _, L1 = b.get_state(factor=True)
    assert kc.bits_equal(x1, x0) and kc.bits_equal(L1, L0)
    g = b.run(U, Y, outputs=OUTS, t_index0=4.0)
    h, _ = qc.host_run(host, models, U, Y, 10, t_index0=4.0, factor=(x0, L0))
    _same(g, h, what="after the throws")


def test_python_bank_against_the_twin_at_the_extended_banks_times(host):
    """SqExtendedKalmanFilterBank over six quad-tanks: loglik is the twin's from t_index0 = 1, forward the twin's from t_index0 = 0 — the
    times ExtendedKalmanFilterBank uses — bit for bit; from_filter_bank of a FilterBank gives the same bank; set_parameters; update twice
    is a two-step run; smooth raises"""
    pf_specs = kg.quadtank_specs(6)
    specs = [(dy, me, np.full(4, 0.1), np.full(2, 1e-4), d0) for dy, me, _, _, d0 in pf_specs]
    U, Y = M.quadtank_data(60)
    sb = llpf_amd.SqExtendedKalmanFilterBank(specs)
    assert isinstance(sb._h, _capi.SqekfBankHandle) and sb.n_filters == 6
    singles = [llpf_amd.SqExtendedKalmanFilter(*s) for s in specs]
    models = [one._model for one in singles]
    ll = sb.loglik(U, Y)
    h1, _ = qc.host_run(host, models, U, Y, 60, t_index0=1.0)
    assert kc.bits_equal(ll, h1["ll"]) and np.isfinite(ll).all() and len(set(ll.tolist())) == 6
    fw = sb.forward(U, Y)
    h0, st0 = qc.host_run(host, models, U, Y, 60, t_index0=0.0)
    _same(fw, h0, what="forward")
    x, R = sb.state()
    assert kc.bits_equal(x, st0[0]) and kc.bits_equal(R, st0[1])
    eb = llpf_amd.ExtendedKalmanFilterBank(specs)
    le = eb.loglik(U, Y)
    assert np.all(np.abs(ll - le) <= 1e-9 * np.abs(le)), "on a well-conditioned model the two banks are one filter"
    pf = llpf_amd.FilterBank(100, pf_specs, rng=1)
    assert kc.bits_equal(llpf_amd.SqExtendedKalmanFilterBank.from_filter_bank(pf).loglik(U, Y), ll)
    assert kc.bits_equal(llpf_amd.SqExtendedKalmanFilterBank(singles).loglik(U, Y), ll)
    sb.set_parameters(specs[::-1])
    assert kc.bits_equal(sb.loglik(U, Y), ll[::-1])
    one = singles[2]
    assert llpf_amd.loglik(one, U, Y) == ll[2]
    sol = llpf_amd.forward_trajectory(one, U, Y)
    assert sol.ll == h0["ll"][2] and kc.bits_equal(sol.xt, h0["xt"][:, 2]) and kc.bits_equal(sol.Rt, h0["Rt"][:, 2])
    llpf_amd.reset(one)
    one._index = 0
    steps = [llpf_amd.update(one, U[t], Y[t])[0] for t in range(2)]
    assert kc.bits_equal(np.array(steps), h0["ll_steps"][:2, 2])
    assert kc.bits_equal(llpf_amd.state(one), h0["x"][2, 2]) and kc.bits_equal(llpf_amd.covariance(one), h0["R"][2, 2])
    llpf_amd.reset(one)
    one._index = 0
    l, e = llpf_amd.correct(one, U[0], Y[0])
    assert l == h0["ll_steps"][0, 2] and kc.bits_equal(llpf_amd.state(one), h0["xt"][0, 2]) and kc.close(llpf_amd.covariance(one), h0["Rt"][0, 2])
    llpf_amd.predict(one, U[0])
    assert kc.close(llpf_amd.state(one), h0["x"][1, 2]) and kc.close(llpf_amd.covariance(one), h0["R"][1, 2])
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(one, U, Y)
    with pytest.raises(TypeError, match="no smoother"):
        sb.smooth(U, Y)
