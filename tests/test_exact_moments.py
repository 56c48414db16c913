"""The oracle held to the mathematics: on a linear-Gaussian model the Kalman filter is the exact answer, and exp(ll) of a bootstrap particle
filter is unbiased for every N (tests/kalman_exact.py).  Everything else in the suite compares the engine with the oracle, which was written
from the same reading of the reference; a bias of a tenth of a nat per step passed every older check against the Kalman filter.  Here the
statistic is shown to be sound (it accepts both orders of the oracle), sharp (it refuses a Kalman filter whose model is off by 1 %) and to
refuse the two recursions that are NOT unbiased — the auxiliary filter and the coupled Rao-Blackwellized filter, both as the reference has
them.  tests/test_gpu_exact_moments.py asks the same of the engine, at sizes only the device affords."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import kalman_common as KC
import kalman_exact as KE
import models as M
import oracle_binding as ob
from kalman_exact import Z_MAX
from llpf_amd import _structs as S

STRATEGIES = [S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED, S.RESAMPLE_RESIDUAL]
NAMES = {S.RESAMPLE_SYSTEMATIC: "systematic", S.RESAMPLE_STRATIFIED: "stratified", S.RESAMPLE_RESIDUAL: "residual"}
SEED0 = 1000


def replicas(cfg, U, Y, F, order=ob.ORDER_DEVICE, aux=None, threads=16):
    """F independent runs of the oracle, replica k with the Philox key SEED0 + k (what filter k of a replica bank uses): ll_steps [T, F] and
    xmean [T, F, nx]: seed, reset!, run, as tests/test_gpu_exact_moments.py drives the bank, so replica k here has the bits of replica k there.
    Every replica is a filter of its own — a Rao-Blackwellized filter keeps its inner Kalman filter across reset!, as the reference does —
    and the replicas are spread over `threads` host threads (the oracle keeps no state outside its handles)."""
    T = len(Y)
    nx = ob.OracleFilter(cfg, order).nx
    lls, xm = np.zeros((T, F)), np.zeros((T, F, nx))

    def work(j):
        for k in range(j, F, threads):
            o = ob.OracleFilter(cfg, order)
            o.seed(SEED0 + k); o.reset()
            if aux is None:
                r = o.run(U, Y, 0.0, ll_steps=True, xmean=True)
                xm[:, k] = r["xmean"]
            else:
                r = o.run_aux(U, Y, aux, ll_steps=True)
            lls[:, k] = r["ll_steps"]
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(work, range(threads)))
    return lls, xm


def _lg_case(T=20):
    m = M.lg_test_model(0.1)
    _, U, Y = M.simulate_lg(m, T, seed=3)
    return m, U, Y, KE.kalman(KE.model_matrices(m), U, Y)


# ---- the long double filter itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("system", ["lg_test", "lg_c1", "random_422", "random_422_D"])
def test_long_double_kalman_equals_the_restatements(system):
    """three statements of the same filter: long double in Joseph form (kalman_exact), the reference's literal formulas in numpy
    (kalman_common.numpy_reference) and the oracle's C (orc_kalman_loglik, which has no feedthrough D): 1e-10 relative"""
    rng = np.random.default_rng(17)
    if system == "lg_test":
        m, D = M.lg_test_model(0.1), np.zeros((1, 1))
    elif system == "lg_c1":
        m, D = M.lg_c1_model(), np.zeros((2, 2))
    else:
        m, D = KC.random_system(rng, 4, 2, 2, kind=1, D=system.endswith("_D"))
    mats = KC.matrices(m, D)
    U, Y = KC.simulate(rng, mats, 40, missing=(7, 8))
    k = KE.kalman(KE.model_matrices(m, D), U, Y)
    ref = KC.numpy_reference(mats, U, Y)
    assert k["ll_steps"][7] == 0.0 and k["ll_steps"][8] == 0.0 and np.all(k["ll_steps"][:7] != 0.0)
    assert KC.close(k["ll_steps"], ref["ll_steps"]) and KC.close(k["xt"], ref["xt"]) and KC.close(k["Rt"], ref["Rt"])
    assert abs(k["ll"] - ref["ll"]) <= 1e-10 * abs(ref["ll"])
    if not np.any(D):
        assert abs(k["ll"] - ob.kalman_loglik(m, U, Y)) <= 1e-10 * abs(k["ll"])


# ---- the statistic accepts the oracle, in both orders -------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ob.ORDER_DEVICE, ob.ORDER_REFERENCE], ids=["device", "reference"])
@pytest.mark.parametrize("strategy,kind,thr", [(S.RESAMPLE_SYSTEMATIC, S.PARTICLE_FILTER, 0.5), (S.RESAMPLE_STRATIFIED, S.ADVANCED_PARTICLE_FILTER, 1.0),
                                               (S.RESAMPLE_RESIDUAL, S.PARTICLE_FILTER, 0.0)], ids=["systematic", "stratified", "residual"])
def test_oracle_is_unbiased(order, strategy, kind, thr):
    m, U, Y, kf = _lg_case()
    lls, xm = replicas(S.make_config(m, 256, kind, strategy, thr, SEED0, 0), U, Y, 400, order)
    zZ, zX = KE.z_likelihood(lls, kf["ll_steps"]), KE.z_state(lls, xm, kf["ll_steps"], kf["xt"])
    print("oracle %s: max|zZ| %.2f max|zX| %.2f sd(ll - ll_KF) %.3f" % (NAMES[strategy], np.abs(zZ).max(), np.abs(zX).max(), KE.sd_loglik(lls, kf["ll_steps"])))
    assert np.all(np.abs(zZ) <= Z_MAX) and np.all(np.abs(zX) <= Z_MAX)


# ---- ... and refuses a model that is slightly off ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sharp_runs():
    m, U, Y, kf = _lg_case()
    lls, xm = replicas(S.make_config(m, 1024, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, SEED0, 0), U, Y, 4096)
    return U, Y, kf, lls, xm


def test_sharp_statistic_accepts_the_true_model(sharp_runs):
    U, Y, kf, lls, xm = sharp_runs
    zZ, zX = KE.z_likelihood(lls, kf["ll_steps"]), KE.z_state(lls, xm, kf["ll_steps"], kf["xt"])
    sd = KE.sd_loglik(lls, kf["ll_steps"])
    print("oracle F = 4096, N = 1024: max|zZ| %.2f max|zX| %.2f sd(ll - ll_KF) %.3f" % (np.abs(zZ).max(), np.abs(zX).max(), sd))
    assert np.all(np.abs(zZ) <= Z_MAX) and np.all(np.abs(zX) <= Z_MAX) and sd <= KE.SD_MAX


@pytest.mark.parametrize("what", ["meas", "dyn"])
def test_sharp_statistic_refuses_a_perturbed_model(sharp_runs, what):
    """the same runs against the Kalman filter of a model whose measurement variance is 1 % larger, or whose dynamics noise standard deviation
    is 10 % larger: the smallest of {1, 2, 5, 10} % that reached |z| >= 8 when this test was written (EXPERIMENTS.md)"""
    U, Y, kf, lls, _ = sharp_runs
    wrong = KE.kalman(KE.model_matrices(KE.perturbed_lg_test_model(what, KE.SENS_P[what])), U, Y)
    zZ = KE.z_likelihood(lls, wrong["ll_steps"])
    print("oracle, %s x (1 + %g): max|zZ| %.2f, ll_KF moved by %.4f" % (what, KE.SENS_P[what], np.abs(zZ).max(), wrong["ll"] - kf["ll"]))
    assert np.abs(zZ).max() > Z_MAX


# ---- resampling in isolation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [ob.ORDER_DEVICE, ob.ORDER_REFERENCE], ids=["device", "reference"])
@pytest.mark.parametrize("n", [1000, 1025])
@pytest.mark.parametrize("strategy", STRATEGIES, ids=[NAMES[s] for s in STRATEGIES])
def test_resampling_is_unbiased(strategy, n, order):
    """E[copies of i] = m we_i, seen through eight Fourier modes of the ancestor vector: S_j = mean_o cos(2 pi j anc_o / n) has the exact
    expectation sum_i we_i cos(2 pi j i / n).  Uniforms from numpy, not from Philox; n = m only (for m != n the reference's offset
    r = rand() bins[end] / N is not unbiased, which is the reference's affair)."""
    rng = np.random.default_rng(n + n)
    we = rng.exponential(size=n) ** 3
    we /= we.sum()
    R, j = 512, np.arange(1, 9)
    basis = np.cos(2 * np.pi * np.outer(j, np.arange(n)) / n)         # [8, n]
    exact = basis @ we
    urng = np.random.default_rng(12345 + strategy)
    Sj = np.empty((R, 8))
    for d in range(R):
        U = urng.uniform(size=1 if strategy == S.RESAMPLE_SYSTEMATIC else n)
        anc, _ = ob.resample(strategy, we, U, n, order)
        assert anc.min() >= 0 and anc.max() < n
        Sj[d] = basis[:, anc].mean(axis=1)
    z = (Sj.mean(axis=0) - exact) / (Sj.std(axis=0, ddof=1) / np.sqrt(R))
    print("resample %s n = %d: max|z| %.2f" % (NAMES[strategy], n, np.abs(z).max()))
    assert np.all(np.abs(z) <= Z_MAX)


# ---- the two recursions that are not unbiased ------------------------------------------------------------------------------------------
def _offsets(run):
    """offset of mean(ll) from ll_KF at N = 1024 and N = 4096 (F = 300): each more than Z_MAX standard errors from 0 and the two within Z_MAX
    combined standard errors of each other — a property of the recursion, not Monte-Carlo error.  Size and sign are printed, not asserted:
    the tree follows the reference here."""
    out = []
    for N in (1024, 4096):
        lls, ll_kf = run(N)
        off, se, steps = KE.offset(lls, ll_kf)
        print("  N = %d: mean(ll) - ll_KF = %+.4f +- %.4f; per step %s" % (N, off, se, np.array2string(steps, precision=3, max_line_width=200)))
        assert abs(off) > Z_MAX * se
        out.append((off, se))
    (o1, s1), (o2, s2) = out
    assert abs(o1 - o2) <= Z_MAX * np.hypot(s1, s2)


def test_auxiliary_filter_offset_does_not_shrink():
    """run_aux mode 1 (loglik of an AuxiliaryParticleFilter), threshold 0.1: correct! ignores y and the look-ahead weights are not divided out"""
    m, U, Y, kf = _lg_case()
    print("auxiliary filter, lg_test_model(0.1), T = 20")
    _offsets(lambda N: (replicas(S.make_config(m, N, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.1, SEED0, 0), U, Y, 300, aux=1)[0], kf["ll_steps"]))


def test_coupled_rao_blackwellized_offset_does_not_shrink():
    """the mixed 1 + 1 system with An = 0.5 against the joint Kalman filter: the reference samples xn+ with the noise of R1n where the
    marginal has An R An' + R1n"""
    rb, joint = KE.rb_mixed(0.5)
    U, Y = KE.rb_data(0.5, 30)
    kf = KE.kalman(KE.model_matrices(joint), U, Y)
    print("Rao-Blackwellized filter, An = 0.5, T = 30")
    _offsets(lambda N: (replicas(S.make_config(rb, N, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.1, SEED0, 0), U, Y, 300)[0], kf["ll_steps"]))


def test_uncoupled_rao_blackwellized_filter_is_unbiased():
    """the same system with An removed is exact in expectation: joint model A = diag(1, 0.95)"""
    rb, joint = KE.rb_mixed(None)
    U, Y = KE.rb_data(None, 30)
    kf = KE.kalman(KE.model_matrices(joint), U, Y)
    lls, _ = replicas(S.make_config(rb, 1024, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.1, SEED0, 0), U, Y, 400)
    zZ = KE.z_likelihood(lls, kf["ll_steps"])
    print("Rao-Blackwellized filter, no coupling: max|zZ| %.2f sd(ll - ll_KF) %.3f" % (np.abs(zZ).max(), KE.sd_loglik(lls, kf["ll_steps"])))
    assert np.all(np.abs(zZ) <= Z_MAX)
