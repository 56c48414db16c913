"""The engine held to the mathematics (tests/kalman_exact.py; the oracle's turn is tests/test_exact_moments.py): every case is one replica
bank — F filters of the same model on the same data, filter k with the Philox key seed + k — whose exp(ll) and exp(ll)-weighted means must
average to the Kalman filter's, with no 1/N term, within Z_MAX standard errors at every step.  F = 4096 replicas of N = 1024 particles
resolve a bias of 5 x 0.15 / 64 = 0.012 nats over the whole run; the last two tests show that on the device.

Data come from numpy (models.simulate_lg), never from the engine.  ll_steps comes from llpf_bank_run, xmean (with the ll_steps of the same
call) from llpf_bank_run_multi with U and Y broadcast to every filter.  One line per case is printed: max |zZ|, max |zX|, sd(ll - ll_KF)."""
import functools
import time

import numpy as np
import pytest

import kalman_exact as KE
import models as M
from kalman_exact import SD_MAX, Z_MAX
from llpf_amd import _capi, _structs as S

pytestmark = pytest.mark.gpu

SEED0 = 1000
KINDS = {"pf": S.PARTICLE_FILTER, "apf": S.ADVANCED_PARTICLE_FILTER}
STRATEGIES = {"systematic": S.RESAMPLE_SYSTEMATIC, "stratified": S.RESAMPLE_STRATIFIED, "residual": S.RESAMPLE_RESIDUAL}


def bank_runs(cfg, U, Y, F, multi=True):
    """ll_steps [T, F] of llpf_bank_run, and ll_steps, xmean [T, F, nx] of llpf_bank_run_multi from the same seed (None, None without `multi`)"""
    b = _capi.BankHandle(cfg, None, n_filters=F)
    b.seed(SEED0); b.reset()
    lls = b.run(U, Y, 0.0, ll_steps=True)["ll_steps"]
    if not multi:
        return lls, None, None
    T = len(Y)
    Ub = None if U is None or not b.nu else np.broadcast_to(np.asarray(U, dtype=np.float64).reshape(1, T, b.nu), (F, T, b.nu))
    Yb = np.broadcast_to(np.asarray(Y, dtype=np.float64).reshape(1, T, b.ny), (F, T, b.ny))
    b.seed(SEED0); b.reset()
    r = b.run_multi(Ub, Yb, 0.0, ll_steps=True, xmean=True)
    return lls, r["ll_steps"], r["xmean"]


def check(what, lls, kf, lls_m=None, xm=None, t0=None):
    """the assertions of every case, after its line"""
    zZ = KE.z_likelihood(lls, kf["ll_steps"])
    sd = KE.sd_loglik(lls, kf["ll_steps"])
    zX = None if xm is None else KE.z_state(lls_m, xm, kf["ll_steps"], kf["xt"])
    zZm = None if xm is None else KE.z_likelihood(lls_m, kf["ll_steps"])
    print("%s: max|zZ| %.2f max|zX| %s sd(ll - ll_KF) %.3f%s" % (what, np.abs(zZ).max(), "-" if zX is None else "%.2f" % np.abs(zX).max(), sd,
                                                                  "" if t0 is None else " (%.2f s)" % (time.perf_counter() - t0)))
    assert np.all(np.isfinite(lls)) and sd <= SD_MAX, "the case does not meet the condition the z-values rest on: sd = %g" % sd
    assert np.all(np.abs(zZ) <= Z_MAX), (what, "zZ", zZ)
    if xm is not None:
        assert np.all(np.abs(zZm) <= Z_MAX), (what, "zZ of run_multi", zZm)
        assert np.all(np.abs(zX) <= Z_MAX), (what, "zX", zX)


@functools.lru_cache(maxsize=None)
def grid_case(kind, strategy, thr, T=30, missing=()):
    """a case of the main grid: lg_test_model(0.1), N = 1024 (one tile), F = 4096"""
    m = M.lg_test_model(0.1)
    _, U, Y = M.simulate_lg(m, T, seed=3)
    for t in missing:
        Y[t] = np.nan
    kf = KE.kalman(KE.model_matrices(m), U, Y)
    t0 = time.perf_counter()
    lls, lls_m, xm = bank_runs(S.make_config(m, 1024, KINDS[kind], STRATEGIES[strategy], thr, SEED0, 0), U, Y, 4096)
    return dict(U=U, Y=Y, kf=kf, lls=lls, lls_m=lls_m, xm=xm, t0=t0)


@pytest.mark.parametrize("thr", [1.0, 0.5])
@pytest.mark.parametrize("strategy", list(STRATEGIES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_main_grid(kind, strategy, thr):
    c = grid_case(kind, strategy, thr)
    check("%s %s threshold %g" % (kind, strategy, thr), c["lls"], c["kf"], c["lls_m"], c["xm"], c["t0"])


def test_never_resampling():
    c = grid_case("pf", "systematic", 0.0, T=20)
    check("pf systematic threshold 0, T = 20", c["lls"], c["kf"], c["lls_m"], c["xm"], c["t0"])


def test_missing_measurements():
    c = grid_case("pf", "systematic", 0.5, missing=(7, 8))
    print("largest |ll_steps| of a missing row: %.3g" % np.max(np.abs(c["lls"][7:9])))
    assert np.max(np.abs(c["lls"][7:9])) < 1e-12 and np.all(c["kf"]["ll_steps"][7:9] == 0.0)      # logsumexp of normalised weights: 0 to rounding
    check("pf systematic threshold 0.5, rows 7 and 8 missing", c["lls"], c["kf"], c["lls_m"], c["xm"], c["t0"])


# ---- several tiles: the fused threshold-1 forms ----------------------------------------------------------------------------------------
def test_three_tiles_at_threshold_one():
    m = M.lg_test_model(0.1)
    _, U, Y = M.simulate_lg(m, 30, seed=3)
    kf = KE.kalman(KE.model_matrices(m), U, Y)
    t0 = time.perf_counter()
    lls, _, _ = bank_runs(S.make_config(m, 2049, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, SEED0, 0), U, Y, 1024, multi=False)
    check("N = 2049, F = 1024, threshold 1", lls, kf, t0=t0)


def test_the_lean_form_of_one_large_filter():
    """one FilterHandle at N = 70001 (69 tiles, ragged), re-seeded for 256 seeds at T = 12: the run without stored weights, ancestors, counts
    or means (last_run_form()["lean"]), which only a single filter's threshold-1 run takes"""
    m = M.lg_test_model(0.1)
    T, F = 12, 256
    _, U, Y = M.simulate_lg(m, T, seed=3)
    kf = KE.kalman(KE.model_matrices(m), U, Y)
    t0 = time.perf_counter()
    g = _capi.FilterHandle(S.make_config(m, 70001, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, SEED0, 0))
    lls = np.zeros((T, F))
    for k in range(F):
        g.seed(SEED0 + k); g.reset()
        lls[:, k] = g.run(U, Y, 0.0, ll_steps=True)["ll_steps"]
        assert g.last_run_form()["lean"], "seed %d did not take the lean form: %r" % (SEED0 + k, g.last_run_form())
    assert len(np.unique(lls.sum(axis=0))) == F
    check("N = 70001, 256 seeds, threshold 1, T = 12", lls, kf, t0=t0)


# ---- other code paths -------------------------------------------------------------------------------------------------------------------
# sd(ll - ll_KF) on the oracle at N = 1024, T = 30, threshold 0.5 is 0.48 for the (3, 2) and 0.42 for the (5, 2, 1) system, above SD_MAX; at
# N = 4096 it is 0.24 and 0.21 (EXPERIMENTS.md), so these two run 4096 particles.  F stays 1024.
@pytest.mark.parametrize("system,N", [("cov_full_32", 4096), ("lg_521", 4096)])
def test_other_linear_gaussian_systems(system, N):
    """COV_FULL for all three densities (a factor used transposed, or a covariance where its inverse belongs, shows here; the noise densities
    have means), and a dimension above the precompiled ones (compiled on demand)"""
    m = KE.cov_full_32() if system == "cov_full_32" else KE.lg_521()
    _, U, Y = M.simulate_lg(m, 30, seed=3)
    kf = KE.kalman(KE.model_matrices(m), U, Y)
    t0 = time.perf_counter()
    lls, lls_m, xm = bank_runs(S.make_config(m, N, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, SEED0, 0), U, Y, 1024)
    check("%s N = %d, F = 1024" % (system, N), lls, kf, lls_m, xm, t0)


def test_uncoupled_rao_blackwellized_bank():
    """the mixed 1 + 1 system without An against the Kalman filter of the joint model A = diag(1, 0.95); ll only"""
    rb, joint = KE.rb_mixed(None)
    U, Y = KE.rb_data(None, 30)
    kf = KE.kalman(KE.model_matrices(joint), U, Y)
    t0 = time.perf_counter()
    lls, _, _ = bank_runs(S.make_config(rb, 1024, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.1, SEED0, 0), None, Y, 1024, multi=False)
    check("Rao-Blackwellized, no coupling, N = 1024, F = 1024", lls, kf, t0=t0)


# ---- the replicas are independent, and the statistic is sharp on the device -------------------------------------------------------------
def test_replicas_are_independent():
    c = grid_case("pf", "systematic", 1.0)
    ll = c["lls"].sum(axis=0)
    F = ll.size
    assert len(np.unique(ll)) == F, "two replicas returned the same log-likelihood"
    import oracle_binding as ob
    for k in (0, 1, F - 1):            # replica k is the filter with the Philox key seed + k: the device-order oracle's bits
        o = ob.OracleFilter(S.make_config(M.lg_test_model(0.1), 1024, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, SEED0, 0), ob.ORDER_DEVICE)
        o.seed(SEED0 + k); o.reset()
        want = o.run(c["U"], c["Y"], 0.0, ll_steps=True)["ll_steps"]
        assert np.array_equal(c["lls"][:, k].view(np.uint64), want.view(np.uint64)), "replica %d is not the oracle's filter with key seed + %d" % (k, k)
        assert np.array_equal(c["lls_m"][:, k].view(np.uint64), want.view(np.uint64)), "run_multi: replica %d" % k
    for j in (1, 2, 3):
        rho = np.corrcoef(ll[:-j], ll[j:])[0, 1]
        print("correlation of ll_k with ll_{k+%d}: %+.4f (bound %.4f)" % (j, rho, Z_MAX / np.sqrt(F)))
        assert abs(rho) <= Z_MAX / np.sqrt(F)


@pytest.mark.parametrize("what", ["meas", "dyn"])
def test_a_perturbed_model_fails_the_statistic(what):
    """the first grid case against the Kalman filter of a model whose measurement variance is 1 % off, or whose dynamics noise standard
    deviation is 10 % off (the p found on the oracle, test_exact_moments.py): what the engine would look like if IT were off by that much"""
    c = grid_case("pf", "systematic", 1.0)
    wrong = KE.kalman(KE.model_matrices(KE.perturbed_lg_test_model(what, KE.SENS_P[what])), c["U"], c["Y"])
    zZ = KE.z_likelihood(c["lls"], wrong["ll_steps"])
    print("%s x (1 + %g): max|zZ| %.2f, ll_KF moved by %+.4f" % (what, KE.SENS_P[what], np.abs(zZ).max(), wrong["ll"] - c["kf"]["ll"]))
    assert np.abs(zZ).max() > Z_MAX
