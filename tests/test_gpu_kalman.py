"""Banks of Kalman filters on the device (llpf_kalman_bank_*; kernels/kalman.hpp, host/kalman.hpp): the GPU reproduces the host build
of csrc/shared/llpf_kalman.h bit for bit, whatever the shape, the bank, the chunking of T or the split of a run; and the Python API
(KalmanFilter, KalmanFilterBank) computes the reference's Kalman filter."""
import ctypes as C

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import kalman_common as kc
from kalman_common import _data, _same
import kf_gpu_frame as kg
from kf_gpu_frame import OUTS
import models as M
import oracle_binding as ob
import ukf_common as uc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kalman_host"))


def _bank(systems):
    return _capi.KalmanBankHandle(0, [m for m, _ in systems], np.stack([D for _, D in systems]))


def _family(D):
    """the Kalman bank over random systems, filter k with a direct term where D(k)"""
    return kg.Family("kalman", _bank, kc.host_run, lambda rng, F, nx, ny, nu: [kc.random_system(rng, nx, ny, nu, k % 3, D=D(k)) for k in range(F)],
                     False)


@pytest.mark.parametrize("nx", range(1, 9))
def test_bit_identical_to_the_host_header_for_every_shape(host, nx):
    """F = 1000 random filters, T = 200, every output; shared and per-filter inputs give the same bits"""
    fam = _family(lambda k: k % 5 != 0)
    for ny in range(1, 5):
        rng = np.random.default_rng(10 * nx + ny)
        nu = int(rng.integers(0, 4))
        b, g, _, _, U, Y = kg.check_shape(fam, host, rng, F=1000, T=200, nx=nx, ny=ny, nu=nu, missing=(50, 51, 120), what=(nx, ny))
        kg.check_broadcast_inputs(fam, b, g, U, Y, F=1000, nu=nu, what=(nx, ny, "per-filter"))
        b.close()


def test_each_output_alone(host):
    """every optional output asked for on its own is the column of the run with all of them: F = 65 (a full workgroup and a ragged one)"""
    kg.check_each_output_alone(_family(lambda k: k % 5 != 0), host, seed=77, F=65, T=3, nx=2, ny=1, nu=1)


def test_per_filter_inputs_of_their_own(host):
    rng = np.random.default_rng(3)
    systems = [kc.random_system(rng, 4, 2, 2, k % 3) for k in range(300)]
    U = rng.standard_normal((300, 80, 2))
    Y = rng.standard_normal((300, 80, 2))
    Y[::7, 30, 0] = np.nan
    g = _bank(systems).run(U, Y, True, True, outputs=OUTS)
    h, _ = kc.host_run(host, systems, U, Y, 80, per_filter=3)
    _same(g, h, OUTS + ("ll",))


def test_a_filters_bits_do_not_depend_on_the_bank(host):
    rng = np.random.default_rng(4)
    systems = [kc.random_system(rng, 3, 2, 1, k % 3) for k in range(1000)]
    U, Y = _data(rng, 60, 1, 2)
    g = _bank(systems).run(U, Y, outputs=OUTS)
    pick = [999, 0, 517, 64, 63, 65]
    sub = _bank([systems[k] for k in pick][::-1]).run(U, Y, outputs=OUTS)
    for j, k in enumerate(pick[::-1]):
        for key in OUTS:
            assert kc.bits_equal(sub[key][:, j], g[key][:, k]), (k, key)
    one = _bank([systems[517]]).run(U, Y, outputs=OUTS)
    for key in OUTS:
        assert kc.bits_equal(one[key][:, 0], g[key][:, 517]), key


def test_chunks_and_continuation(host):
    rng = np.random.default_rng(5)
    systems = [kc.random_system(rng, 4, 2, 2, k % 3) for k in range(1000)]
    U, Y = _data(rng, 700, 2, 2, missing=(255, 256, 600))
    b = _bank(systems)
    long = b.run(U, Y, outputs=OUTS)                   # several chunks of at most 256 steps
    b.reset()
    short = b.run(U[:300], Y[:300], outputs=OUTS)
    for k in OUTS:
        assert kc.bits_equal(long[k][:300], short[k]), k
    h, _ = kc.host_run(host, systems, U, Y, 700)
    _same(long, h, OUTS + ("ll",), "T = 700")
    b.reset()
    bare = b.run(U, Y)                                 # shared inputs and no per-step output over three chunks: nothing is staged out
    assert kc.bits_equal(bare["ll"], h["ll"]) and kc.bits_equal(bare["ll"], long["ll"])
    b.reset()
    whole = b.run(U[:50], Y[:50], outputs=OUTS)
    b.reset()
    first = b.run(U[:25], Y[:25], outputs=OUTS)
    x, R = b.get_state()
    second = b.run(U[25:50], Y[25:50], outputs=OUTS)
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    fresh = _bank(systems)
    fresh.set_state(x, R)
    again = fresh.run(U[25:50], Y[25:50], outputs=OUTS)
    _same(again, second, OUTS + ("ll",), "set_state")
    llonly = fresh.run(U[:10], Y[:10])                 # a run without per-step outputs still continues the state
    x2, _ = fresh.get_state()
    b.set_state(x, R)
    b.run(U[25:50], Y[25:50])
    ref = b.run(U[:10], Y[:10], outputs=("ll_steps",))
    assert kc.bits_equal(llonly["ll"], ref["ll"]) and kc.bits_equal(x2, b.get_state()[0])


def test_chunks_limited_by_bytes_with_a_ragged_tail(host):
    # (nx, ny, nu) = (4, 2, 2), F = 4000, per-filter U and Y, every output: 43 + 4 doubles per filter-step, 1.5 MB per step, so the
    # 64 MiB staging limit gives chunks of 44 steps: 200 steps are chunks of 44, 44, 44, 44 and 24
    rng = np.random.default_rng(8)
    F, T = 4000, 200
    systems = [kc.random_system(rng, 4, 2, 2, k % 3) for k in range(F)]
    U = rng.standard_normal((F, T, 2))
    Y = 2.0 * rng.standard_normal((F, T, 2))
    Y[::9, 43, 0] = Y[::9, 44, 0] = Y[::11, 199, 0] = np.nan
    g = _bank(systems).run(U, Y, True, True, outputs=OUTS)
    pick = [0, 1, 63, 64, 65, 1999, 2000, 3998, 3999] + list(range(9, 4000, 99))
    h, _ = kc.host_run(host, [systems[k] for k in pick], U[pick], Y[pick], T, per_filter=3)
    for key in OUTS:
        assert kc.bits_equal(g[key][:, pick], h[key]), key
    assert kc.bits_equal(g["ll"][pick], h["ll"])
    assert np.all(np.isfinite(g["ll"])) and np.all(np.isfinite(g["R"][-1]))


def test_missing_rows_and_a_filter_that_loses_definiteness(host):
    rng = np.random.default_rng(6)
    systems = [kc.random_system(rng, 2, 1, 0, k % 3) for k in range(130)]
    U, Y = _data(rng, 40, 0, 1, missing=(5, 6, 30))
    b = _bank(systems)
    x, R = b.get_state()
    ok = b.run(None, Y, outputs=OUTS)
    assert np.all(ok["ll_steps"][[5, 6, 30]] == 0.0) and np.all(np.isnan(ok["e"][[5, 6, 30]]))
    R[77] = -100.0 * np.eye(2)
    b.set_state(x, R)
    bad = b.run(None, Y, outputs=OUTS)
    # NaN from the first step on; a missing row still adds 0 (correct! is skipped)
    assert np.all(np.isnan(np.delete(bad["ll_steps"][:, 77], [5, 6, 30]))) and np.all(bad["ll_steps"][[5, 6, 30], 77] == 0.0)
    assert np.isnan(bad["ll"][77]) and np.all(np.isnan(bad["xt"][:, 77])) and np.all(np.isnan(bad["R"][1:, 77]))
    keep = [f for f in range(130) if f != 77]
    for k in OUTS:
        assert kc.bits_equal(bad[k][:, keep], ok[k][:, keep]), k
    h, _ = kc.host_run(host, systems, None, Y, 40, state=(x, R))
    _same(bad, h, OUTS + ("ll",), "NaN filter")


@pytest.mark.parametrize("verb", ["run", "smooth"])
@pytest.mark.parametrize("kind", ["kalman", "ukf"])
def test_bad_run_arguments_on_a_live_handle_are_refused_and_leave_it_as_it_was(kind, verb):
    """llpf_{kalman,ukf}_bank_{run,smooth} on a bank that has run (linear-Gaussian, F = 65: one full workgroup of 64 and a ragged one;
    nx = 2, ny = 1, nu = 1, T = 3): T = 0, Y null, U null with nu > 0, per_filter = 4, a forward struct_size one byte short and, for the
    unscented bank, t_index0 = inf and nan are each LLPF_ERR_ARG under the bank's own prefix; the state keeps its bits, and the run that
    follows is the run of a bank that never saw them."""
    F, T = 65, 3
    rng = np.random.default_rng(11)
    systems = [kc.random_system(rng, 2, 1, 1, k % 3, D=kind == "kalman") for k in range(F)]
    U, Y = _data(rng, T, 1, 1)

    def bank():
        return _bank(systems) if kind == "kalman" else _capi.UkfBankHandle(0, [m for m, _ in systems], uc.merwe(2, 1.0, 0.0, 1.0))

    fresh = bank()
    fresh.run(U, Y)
    ref = fresh.run(U, Y, outputs=OUTS)
    b = bank()
    b.run(U, Y)
    x0, R0 = b.get_state()
    L = _capi.lib()
    fn = getattr(L, "llpf_%s_bank_%s" % (kind, verb))
    ll, xT = np.empty(F), np.empty((T, F, 2))
    sm = S.KalmanSmoothOutputs()
    sm.struct_size = C.sizeof(S.KalmanSmoothOutputs)
    sm.xT = _capi.dptr(xT)
    short = S.KalmanOutputs()
    short.struct_size = C.sizeof(S.KalmanOutputs) - 1

    def call(U=U, Y=Y, T=T, per_filter=0, t_index0=0.0, fwd=None):
        times = (t_index0,) if kind == "ukf" else ()
        tail = (None if fwd is None else C.byref(fwd),) + ((C.byref(sm),) if verb == "smooth" else ())
        return fn(b.h, _capi.dptr(U), _capi.dptr(Y), T, per_filter, *times, _capi.dptr(ll), *tail)

    cases = [dict(T=0), dict(Y=None), dict(U=None), dict(per_filter=4), dict(fwd=short)]
    if kind == "ukf":
        cases += [dict(t_index0=np.inf), dict(t_index0=np.nan)]
    for case in cases:
        assert call(**case) == _capi.ERR_ARG, case
        assert L.llpf_last_error().startswith(kind.encode() + b": "), (case, L.llpf_last_error())
        x, R = b.get_state()
        assert kc.bits_equal(x, x0) and kc.bits_equal(R, R0), case
    _same(b.run(U, Y, outputs=OUTS), ref, what="after the refused calls")


def test_python_api():
    rng = np.random.default_rng(7)
    m, D = kc.random_system(rng, 3, 2, 1, 2)
    mt = kc.matrices(m, D)
    U, Y = kc.simulate(rng, mt, 50, missing=(9,))
    kf = llpf_amd.KalmanFilter(mt["A"], mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]))
    assert kf._handle is None
    sol = llpf_amd.forward_trajectory(kf, U, Y)
    assert sol.x.shape == (50, 3) and sol.xt.shape == (50, 3) and sol.R.shape == (50, 3, 3) and sol.Rt.shape == (50, 3, 3)
    assert sol.e.shape == (50, 2) and np.isscalar(sol.ll) and sol.t.shape == (50,)
    ref = kc.numpy_reference(mt, U, Y)
    for k in ("x", "xt", "R", "Rt", "e"):
        assert kc.close(getattr(sol, k), ref[k]), k
    assert abs(sol.ll - ref["ll"]) <= 1e-10 * abs(ref["ll"])
    assert llpf_amd.loglik(kf, U, Y) == sol.ll
    llpf_amd.reset(kf)
    lls = [llpf_amd.update(kf, U[t], Y[t])[0] for t in range(50)]
    assert kc.close(np.array(lls), ref["ll_steps"]) and lls[9] == 0.0
    assert np.allclose(llpf_amd.state(kf), kf.x) and kc.close(kf.x[None], (mt["A"] @ ref["xt"][-1] + mt["B"] @ U[-1])[None])
    assert llpf_amd.covariance(kf).shape == (3, 3)
    # log_likelihood_fun with a factory that returns a KalmanFilter
    from scipy import stats
    fac = lambda th: llpf_amd.KalmanFilter(mt["A"] * th[0], mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]))
    f = llpf_amd.log_likelihood_fun(fac, [stats.uniform(0.5, 1.0)], U, Y)
    assert abs(f(np.array([1.0])) - (stats.uniform(0.5, 1.0).logpdf(1.0) + sol.ll)) < 1e-9
    assert f(np.array([0.8])) != f(np.array([1.0])) and f(np.array([3.0])) == -np.inf
    # a bank of the same filter and of others: loglik with shared and per-filter arrays
    kb = llpf_amd.KalmanFilterBank([kf, (mt["A"] * 0.5, mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]))])
    ll = kb.loglik(U, Y)
    assert ll[0] == sol.ll
    assert kc.bits_equal(kb.loglik(np.stack([U, U]), np.stack([Y, Y])), ll)
    kb.set_parameters([(mt["A"] * 0.5, mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]))] * 2)
    ll2 = kb.loglik(U, Y)
    assert ll2[0] == ll2[1] == ll[1]
    fw = kb.forward(U, Y)
    assert fw["x"].shape == (50, 2, 3) and kb.state()[0].shape == (2, 3)


def test_from_filter_bank_agrees_with_the_oracle_and_the_particle_filter():
    specs, models = [], []
    for k in range(8):
        model = M.lg_test_model(sigma_f=0.1 + 0.05 * k)
        mt = kc.matrices(model, np.zeros((1, 1)))
        specs.append((llpf_amd.LinearDynamics(mt["A"], mt["B"]), llpf_amd.LinearMeasurement(mt["C"]),
                      llpf_amd.MvNormal(np.zeros(2), mt["R1"]), llpf_amd.MvNormal(np.zeros(1), mt["R2"]),
                      llpf_amd.MvNormal(mt["x0"], mt["P0"])))
        models.append(model)
    _, U, Y = M.simulate_lg(models[0], 100)
    pf = llpf_amd.FilterBank(100000, specs, rng=11)
    kb = llpf_amd.KalmanFilterBank.from_filter_bank(pf)
    ll = kb.loglik(U, Y)
    for k, model in enumerate(models):
        o = ob.kalman_loglik(model, U, Y)
        assert abs(ll[k] - o) <= 1e-10 * abs(o), (k, ll[k], o)
    llpf = pf.loglik(U, Y)
    assert np.all(np.abs(llpf - ll) < 0.5), (llpf, ll)


def test_a_large_bank(host):
    """F = 10^5, T = 1000, (4, 2), ll only: every ll finite, 64 sampled filters equal to the host build"""
    rng = np.random.default_rng(12)
    base = [kc.random_system(rng, 4, 2, 2, k % 3) for k in range(500)]
    systems = [base[k % 500] for k in range(100000)]
    U, Y = _data(rng, 1000, 2, 2)
    b = _bank(systems)
    ll = b.run(U, Y)["ll"]
    assert np.all(np.isfinite(ll))
    pick = np.sort(rng.choice(100000, 64, replace=False))
    h, _ = kc.host_run(host, [systems[k] for k in pick], U, Y, 1000)
    assert kc.bits_equal(ll[pick], h["ll"])
