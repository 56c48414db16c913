"""Banks of square-root Kalman filters on the device (llpf_sqkf_bank_*; kernels/sqkf.hpp, host/sqkf.hpp): the GPU reproduces the host
build of csrc/shared/llpf_sqkf.h (tests/sqkf_host.c) bit for bit, whatever the shape, the bank, the chunking of T or the split of a run,
on the two systems where the covariance form turns NaN as well; and the Python API (SqKalmanFilter, SqKalmanFilterBank) computes the
Kalman filter."""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi
import kalman_common as kc
from kalman_common import _data, _same
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS
from gpu_common import _Inject
import models as M
import sqkf_common as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return sc.build_host(tmp_path_factory.mktemp("sqkf_host"))


def _bank(systems):
    return _capi.SqkfBankHandle(0, [m for m, _ in systems], np.stack([D for _, D in systems]))


def _systems(rng, F, nx, ny, nu):
    """random systems, every fifth without a direct term"""
    return [kc.random_system(rng, nx, ny, nu, k % 3, D=k % 5 != 0) for k in range(F)]


FAM = kg.Family("sqkf", _bank, sc.host_run, _systems, False)


@pytest.mark.parametrize("nx", range(1, 9))
def test_bit_identical_to_the_host_header_for_every_shape(host, nx):
    """F = 130 (two full waves and a tail of 2), T = 60, nu drawn in 0..3, rows 0, 7 and 59 missing, every output; shared inputs handed
    over as per-filter inputs give the same bits"""
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        b, g, _, _, U, Y = kg.check_shape(FAM, host, rng, F=130, T=60, nx=nx, ny=ny, nu=nu, missing=(0, 7, 59), what=(nx, ny))
        kg.check_broadcast_inputs(FAM, b, g, U, Y, F=130, nu=nu, what=(nx, ny, "per-filter"))
        b.close()


def test_each_output_alone(host):
    """every optional output asked for on its own is the column of the run with all of them: F = 65 (a full workgroup and a ragged one)"""
    kg.check_each_output_alone(FAM, host, seed=77, F=65, T=3, nx=2, ny=1, nu=1)


@pytest.mark.parametrize("F", [1, 63, 64, 65])
def test_bank_sizes_and_chunk_edges(host, F):
    """nx = 2, ny = 1, nu = 1 around the wave of 64 and the pipe's chunk of 256 steps; the final get_state x and R against the twin"""
    kg.check_bank_sizes_and_chunk_edges(FAM, host, seed=20 + F, F=F, nx=2, ny=1, nu=1, missing=(3, 255, 256), Ts=(1, 255, 256, 257, 700))


def test_continuation_on_the_device_through_the_factor(host):
    """halves of T = 600 cut at 300, F = 70, (3, 2, 2): the halves are the whole; the second half against the twin from get_state's
    factor; a fresh bank given that state through set_state(L) produces the same bits; an ll-only run the same ll; and a state set
    through R is llpf_kf_chol of it, a set through -I refused"""
    rng = np.random.default_rng(5)
    F, T, cut = 70, 600, 300
    systems = _systems(rng, F, 3, 2, 2)
    U, Y = _data(rng, T, 2, 2, missing=(255, 256, 300, 599))
    b = _bank(systems)
    whole = b.run(U, Y, outputs=OUTS)
    b.reset()
    first = b.run(U[:cut], Y[:cut], outputs=OUTS)
    x, R, L = b.get_state(factor=True)
    assert np.array_equal(L, np.tril(L))
    second = b.run(U[cut:], Y[cut:], outputs=OUTS)
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    h2, st2 = sc.host_run(host, systems, U[cut:], Y[cut:], T - cut, factor=(x, L))
    _same(second, h2, what="second half")
    x2, R2, L2 = b.get_state(factor=True)
    assert kc.bits_equal(x2, st2[0]) and kc.bits_equal(R2, st2[1]) and kc.bits_equal(L2, st2[2])
    fresh = _bank(systems)
    fresh.set_state(x, L=L)
    xs, Rs, Ls = fresh.get_state(factor=True)
    assert kc.bits_equal(xs, x) and kc.bits_equal(Ls, L) and kc.bits_equal(Rs, R)
    again = fresh.run(U[cut:], Y[cut:], outputs=OUTS)
    _same(again, second, what="set_state(L)")
    b.reset()
    bare = b.run(U, Y)                                  # ll only: nothing is staged per step
    assert kc.bits_equal(bare["ll"], whole["ll"])
    # through R: the factor is llpf_kf_chol of R (not the factor R came from, bit for bit)
    fresh.set_state(x, R=R)
    _, _, Lc = fresh.get_state(factor=True)
    assert kc.bits_equal(Lc, np.stack([sc.host_chol(host, Rf)[1] for Rf in R]))
    viaR = fresh.run(U[cut:], Y[cut:], outputs=OUTS)
    hR, stR = sc.host_run(host, systems, U[cut:], Y[cut:], T - cut, state=(x, R))
    _same(viaR, hR, what="set_state(R)")
    Rbad = R.copy()
    Rbad[33] = -np.eye(3)
    with pytest.raises(_capi.LLPFError) as ei:
        fresh.set_state(x, R=Rbad)
    assert ei.value.code == _capi.ERR_ARG and "filter 33" in str(ei.value)
    for kw in (dict(), dict(R=R, L=L)):                 # neither, or both
        with pytest.raises(_capi.LLPFError) as ei:
            fresh.set_state(x, **kw)
        assert ei.value.code == _capi.ERR_ARG
    after, _ = sc.host_run(host, systems, U[:5], Y[:5], 5, factor=(stR[0], stR[2]))
    _same(fresh.run(U[:5], Y[:5], outputs=OUTS), after, what="after the refused calls")


def test_per_filter_inputs_and_a_nan_filter(host):
    """per-filter U and Y at F = 130, T = 40, (2, 1, 1), rows 5, 6 and 30 missing for every filter and row 12 for every seventh; then
    filter 78 gets a NaN factor entry through set_state(L): NaN in its own outputs from the first correct! on, every other filter's bits
    unmoved, the whole equal to the twin's; and a filter alone in a bank of one equals its column of the bank"""
    rng = np.random.default_rng(6)
    F, T = 130, 40
    systems = _systems(rng, F, 2, 1, 1)
    U = rng.standard_normal((F, T, 1))
    Y = 2.0 * rng.standard_normal((F, T, 1))
    Y[:, [5, 6, 30], 0] = np.nan
    Y[::7, 12, 0] = np.nan
    b = _bank(systems)
    x, _, L = b.get_state(factor=True)
    ok = b.run(U, Y, True, True, outputs=OUTS)
    assert np.all(ok["ll_steps"][[5, 6, 30]] == 0.0) and np.all(np.isnan(ok["e"][[5, 6, 30]]))
    h, _ = sc.host_run(host, systems, U, Y, T, per_filter=3)
    _same(ok, h, what="per-filter inputs")
    L[78, 0, 0] = np.nan
    b.set_state(x, L=L)
    bad = b.run(U, Y, True, True, outputs=OUTS)
    assert np.isnan(bad["ll"][78]) and np.all(np.isnan(bad["xt"][:, 78])) and np.all(np.isnan(bad["Rt"][:, 78])) and np.all(np.isnan(bad["R"][:, 78, 0, 0]))
    assert np.all(np.isnan(np.delete(bad["ll_steps"][:, 78], [5, 6, 30]))) and np.all(bad["ll_steps"][[5, 6, 30], 78] == 0.0)
    keep = [f for f in range(F) if f != 78]
    for k in OUTS:
        assert kc.bits_equal(bad[k][:, keep], ok[k][:, keep]), k
    hb, _ = sc.host_run(host, systems, U, Y, T, per_filter=3, factor=(x, L))
    _same(bad, hb, what="NaN filter")
    for f in (0, 64, 129):
        one = _bank([systems[f]]).run(U[f:f + 1], Y[f:f + 1], True, True, outputs=OUTS)
        for k in OUTS:
            assert kc.bits_equal(one[k][:, 0], ok[k][:, f]), (f, k)


@pytest.mark.parametrize("case", [0, 1])
def test_ill_conditioned_systems_on_the_device(host, case):
    """sqkf_common.ill_conditioned(case) as filters 0 and 1 of a bank padded with random filters of its shape to F = 65, T = 50: the
    device equals the twin bit for bit and the two are finite at every step; the Kalman bank on the same models returns NaN ll for them
    (what it does today on such a model) and finite ll for the padding"""
    system, Y = sc.ill_conditioned(case)
    nx, ny = system[0].nx, system[0].ny
    rng = np.random.default_rng(30 + case)
    systems = [system, system] + [kc.random_system(rng, nx, ny, 0, k % 3) for k in range(63)]
    g = _bank(systems).run(None, Y, outputs=OUTS)
    h, _ = sc.host_run(host, systems, None, Y, 50)
    _same(g, h, what=("ill-conditioned", case))
    for k in OUTS + ("ll",):
        assert np.all(np.isfinite(g[k])), k
    for k in OUTS:
        assert kc.bits_equal(g[k][:, 0], g[k][:, 1]), k
    plain = _capi.KalmanBankHandle(0, [m for m, _ in systems], None).run(None, Y)["ll"]
    assert np.all(np.isnan(plain[:2])) and np.all(np.isfinite(plain[2:]))


def test_a_throw_and_a_refused_allocation_leave_a_usable_handle(host):
    """error:sqkf_run is a status that leaves the state as it was; alloc:sqkf_create is LLPF_ERR_ALLOC and frees the half-built bank; the
    handle goes on working"""
    rng = np.random.default_rng(45)
    systems = _systems(rng, 65, 2, 1, 1)
    U, Y = _data(rng, 10, 1, 1)
    b = _bank(systems)
    b.run(U[:4], Y[:4])
    x0, _, L0 = b.get_state(factor=True)
    with _Inject("error:sqkf_run"):
        with pytest.raises(_capi.LLPFError) as ei:
            b.run(U, Y)
    assert ei.value.code == _capi.ERR_INTERNAL and "sqkf_run" in str(ei.value)
    with _Inject("alloc:sqkf_create"):
        with pytest.raises(_capi.LLPFError) as ei:
            _bank(systems)
    assert ei.value.code == _capi.ERR_ALLOC
    x1, _, L1 = b.get_state(factor=True)
    assert kc.bits_equal(x1, x0) and kc.bits_equal(L1, L0)
    g = b.run(U, Y, outputs=OUTS)
    h, _ = sc.host_run(host, systems, U, Y, 10, factor=(x0, L0))
    _same(g, h, what="after the throws")


def test_python_api():
    """SqKalmanFilterBank.from_filter_bank of the C1 bank against KalmanFilterBank: loglik and every forward output to 1e-10; the bank
    against a loop of single SqKalmanFilter: bit-equal; update twice is a two-step run; smooth raises TypeError"""
    _, U, Y = M.simulate_lg(M.lg_c1_model(0), 200)
    pf = llpf_amd.FilterBank(1000, kg.c1_specs(16), rng=1)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf)
    sb = llpf_amd.SqKalmanFilterBank.from_filter_bank(pf)
    assert isinstance(sb._h, _capi.SqkfBankHandle) and sb.n_filters == 16
    lk, ls = kb.loglik(U, Y), sb.loglik(U, Y)
    assert np.all(np.abs(ls - lk) <= 1e-10 * np.abs(lk)), np.max(np.abs(ls - lk) / np.abs(lk))
    fk, fs = kb.forward(U, Y), sb.forward(U, Y)
    for k in OUTS:
        assert kc.close(fs[k], fk[k]), k
    assert sb.state()[0].shape == (16, 2) and sb.state()[1].shape == (16, 2, 2)
    singles = []
    for k in range(16):
        mt = kc.matrices(M.lg_c1_model(seed=k), np.zeros((2, 2)))
        singles.append(llpf_amd.SqKalmanFilter(mt["A"], mt["B"], mt["C"], 0, mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"])))
    bank = llpf_amd.SqKalmanFilterBank(singles)
    assert kc.bits_equal(bank.loglik(U, Y), ls)
    assert kc.bits_equal(np.array([llpf_amd.loglik(kf, U, Y) for kf in singles]), ls)
    bank.set_parameters(singles[::-1])
    assert kc.bits_equal(bank.loglik(U, Y), ls[::-1])
    kf = singles[3]
    sol = llpf_amd.forward_trajectory(kf, U, Y)
    assert sol.ll == ls[3] and kc.bits_equal(sol.xt, fs["xt"][:, 3]) and kc.bits_equal(sol.Rt, fs["Rt"][:, 3])
    llpf_amd.reset(kf)
    steps = [llpf_amd.update(kf, U[t], Y[t])[0] for t in range(2)]
    assert kc.bits_equal(np.array(steps), fs["ll_steps"][:2, 3])
    assert kc.bits_equal(llpf_amd.state(kf), fs["x"][2, 3]) and kc.bits_equal(llpf_amd.covariance(kf), fs["R"][2, 3])
    with pytest.raises(TypeError, match="the square-root Kalman filter has no smoother"):
        llpf_amd.smooth(kf, U, Y)
    with pytest.raises(TypeError, match="the square-root Kalman filter has no smoother"):
        sb.smooth(U, Y)
