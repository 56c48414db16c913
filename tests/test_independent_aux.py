"""The auxiliary particle filter and residual resampling against their second reading (oracle/independent.py: AuxiliaryParticleFilter,
reference src/filtering.jl:170-234, 367-384, src/smoothing.jl:232-236; resample_residual, src/resample.jl:63-117), in the three layers of
tests/test_independent_oracle.py: the restatement against its frozen outputs tests/golden/indep_*.npz, the C oracle in both arithmetic
orders, the HIP engine.  The residual filter's own frozen cases (pf_lg_residual*) run through that file; here are the auxiliary cases, the
sizes at which the kernels change shape and the stand-alone resampler (both computed live), the condition under which residual ancestors
can be compared at all, and restatements that misread the reference on purpose, which the frozen outputs must refuse.

Tolerances are those of test_independent_oracle.py: implementations differ in rounding only, 1e-11 per step on log-likelihoods, 1e-10 on
states and final log-weights; ancestors and resample counts identical.

Close calls.  Residual resampling decides by floor(nw_i) and by u < bins_i; a decision within rounding of its edge may fall either way
in another arithmetic, and then the ancestors differ legitimately.  That is a CONDITION on the cases, not a tolerance of the comparison:
in every frozen and live case every call is decided by the restatement alone, all margins above the slack derived in
independent.residual_slack (test_every_residual_call_is_decided_by_the_restatement_alone; no call is excused).  Measured (margin next to
its slack, the closest call of each run):
    pf_lg_residual          7 calls   integer 6.2e-04 (2.6e-13)   edge 3.5e-07 (3.5e-13)
    pf_lg_residual_thr1    60 calls   integer 6.6e-06 (7.7e-14)   edge 7.4e-08 (3.6e-13)     all 60 steps, without the missing row
    aux_lg_residual_*      59 calls   integer 5.1e-06 (5.3e-14)   edge 8.6e-09 (2.6e-13)
    live sizes              6 calls each, margin / slack >= 2.4e4 (N = 2049, the residual filter)
    stand-alone calls       the closest is (4097, 300): edge 2.1e-08 (6.1e-10), integer 3.5e-03 (4.8e-11); the others are 1e5 above their slack
    (the closest call of every run: the test's output with -s)
Uniform weights (nw_i = 1 +- 1 ulp) are the corner that cannot meet the condition: threshold 1.0 with a missing measurement, which is why
pf_lg_residual_thr1 has none; tests/test_gpu_residual.py keeps the exact test of that corner."""
import functools
import os

import numpy as np
import pytest

import independent_cases as IC
import oracle_binding as ob
from llpf_amd import _structs as S

ind = IC.ind
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
AUX = IC.aux_cases()
TOL_LL, TOL_X = 1e-11, 1e-10
ORDERS = [ob.ORDER_REFERENCE, ob.ORDER_DEVICE]
SEEN = 1e5                  # a misreading must leave the tolerance by this factor


def _golden(name):
    return np.load(os.path.join(G, "indep_%s.npz" % name))


def _agrees(h, d, case):
    """a handle (C oracle or engine) runs the case after its reset: its outputs against the restatement's, d"""
    ll, nres = IC.run_handle(h, case)
    assert np.max(np.abs(ll - d["ll_steps"])) < TOL_LL
    assert np.max(np.abs(h.particles() - d["x_final"])) < TOL_X
    assert np.array_equal(h.ancestors(), d["anc_final"]) and nres == int(d["resamples"])
    if case.get("aux") is not None:
        assert np.max(np.abs(h.weights() - d["w_final"])) < TOL_X


def _decided(calls, what):
    """every residual call's margins exceed their slack; returns the smallest margin / slack"""
    if not len(calls):
        return np.inf
    for k, (mi, si, me, se) in enumerate(calls):
        assert mi > si and me > se, "%s, residual call %d is a close call: integer margin %.3g (slack %.3g), edge margin %.3g (slack %.3g)" % (
            what, k, mi, si, me, se)
    with np.errstate(invalid="ignore"):
        return float(np.nanmin(np.concatenate([calls[:, 0] / calls[:, 1], calls[:, 2] / calls[:, 3]])))


# ---- frozen cases -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(AUX))
def test_auxiliary_restatement_reproduces_its_frozen_outputs(name):
    d, case = _golden(name), AUX[name]
    assert np.array_equal(d["U"], case["U"]) and np.array_equal(d["Y"], case["Y"], equal_nan=True)
    assert np.isnan(case["Y"]).any() and np.nanmax(np.abs(case["Y"])) > 10         # a missing look-ahead measurement and an outlier
    r = IC.run_independent(ob, case)
    assert np.max(np.abs(r["ll_steps"] - d["ll_steps"])) < 1e-12          # numpy / BLAS builds may round differently
    assert np.max(np.abs(r["x_final"] - d["x_final"])) < 1e-11 and np.max(np.abs(r["w_final"] - d["w_final"])) < 1e-11
    assert np.array_equal(r["anc_final"], d["anc_final"]) and int(r["resamples"]) == int(d["resamples"]) >= case["T"] - 1
    if case.get("advanced"):                                                # lambda is dropped: the auxiliary correct! sees uniform weights
        n = case["T"] - case["aux"]
        assert np.max(np.abs(d["ll_steps"][:n])) < 1e-12 and (case["aux"] == 0 or abs(d["ll_steps"][-1]) > 1.0)
        tsw = case["model"].qt[13]
        assert case["t0"] < tsw < case["t0"] + (case["T"] - 1) * case["model"].Ts  # the run crosses the switch time


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", list(AUX))
def test_c_oracle_agrees_with_the_auxiliary_restatement(name, order):
    d, case = _golden(name), AUX[name]
    o = IC.oracle_of(ob, case, order)
    o.reset()
    _agrees(o, d, case)
    if order == ob.ORDER_DEVICE:
        assert o.exact_steps() >= 1                                         # the outlier: a normalisation redone with the exact maximum


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(AUX))
def test_engine_agrees_with_the_auxiliary_restatement(name):
    d, case = _golden(name), AUX[name]
    g = IC.engine_of(case)
    g.reset()
    _agrees(g, d, case)


# ---- sizes at which the kernels change shape, computed live -------------------------------------------------------------------------
SIZE_CASES = [(N, "residual", None) for N in IC.SIZES] + [(N, s, m) for N in IC.SIZES for s in IC.STRATEGIES for m in IC.MODES]


def _size_id(p):
    return "%d-%s-%s" % (p[0], p[1], "filter" if p[2] is None else "aux_" + p[2])


@functools.lru_cache(maxsize=None)
def _size_reference(N, strategy, mode):
    """(case, the restatement's outputs): computed once, shared by the layers, left unchanged"""
    case = IC.size_case(N, IC.STRATEGIES[strategy], None if mode is None else IC.MODES[mode])
    return case, IC.run_independent(ob, case)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("p", SIZE_CASES, ids=_size_id)
def test_c_oracle_agrees_with_the_restatement_at_every_size(p, order):
    case, r = _size_reference(*p)
    o = IC.oracle_of(ob, case, order)
    o.reset()
    _agrees(o, r, case)
    assert int(r["resamples"]) == IC.SIZE_STEPS


@pytest.mark.gpu
@pytest.mark.parametrize("p", SIZE_CASES, ids=_size_id)
def test_engine_agrees_with_the_restatement_at_every_size(p):
    case, r = _size_reference(*p)
    g = IC.engine_of(case)
    g.reset()
    _agrees(g, r, case)


# ---- the stand-alone residual resampler -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _standalone_reference(n, m):
    we, U, j0 = IC.standalone_residual(n, m)
    j, info = ind.resample_residual(we, j0, U, m)
    s = ind.residual_slack(n, m, 1.0, info["nw_max"], info["R"])            # normalised weights: the total of the quanta's weights is 1
    assert 0 < info["num"] < m and np.all(np.diff(j[:info["num"]]) >= 0) and j.min() >= 0 and j.max() < n      # both parts are exercised
    return we, U, j0, j, np.array([[info["int_margin"], s[0], info["edge_margin"], s[1]]])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("n,m", IC.STANDALONE)
def test_c_oracle_residual_resample_is_the_restatements(n, m, order):
    we, U, j0, j, _ = _standalone_reference(n, m)
    jo, _ = ob.resample(S.RESAMPLE_RESIDUAL, we, U, m, order, j0)
    assert np.array_equal(jo, j)


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", IC.STANDALONE)
def test_engine_residual_resample_is_the_restatements(n, m):
    from llpf_amd import _capi
    we, U, j0, j, _ = _standalone_reference(n, m)
    assert np.array_equal(_capi.resample(S.RESAMPLE_RESIDUAL, we, U, m, j0), j)


def test_residual_resample_by_hand():
    """a case small enough to read: nw = (2.4, 0.8, 0.8), copies 0 0, residuals (0.4, 0.8, 0.8) / 2 -> bins 0.2, 0.6, 1.0; the third and
    fourth outputs read U[2] and U[3] (U[0], U[1] are not read); an output whose uniform is below no bin keeps its previous ancestor"""
    we = np.array([0.6, 0.2, 0.2])
    j, info = ind.resample_residual(we, np.full(4, 7), np.array([0.9, 0.9, 0.1, 0.7]), 4)
    assert list(j) == [0, 0, 0, 2] and info["num"] == 2 and info["R"] == 2
    assert abs(info["int_margin"] - 0.2) < 1e-12 and abs(info["edge_margin"] - 0.1) < 1e-12
    j, _ = ind.resample_residual(we, np.full(4, 7), np.array([0.0, 0.0, 0.59, 1.0]), 4)
    assert list(j) == [0, 0, 1, 7]
    j, info = ind.resample_residual(np.array([0.5, 0.25, 0.25]), np.full(4, 7), np.zeros(4), 4)       # num == M: no draw at all
    assert list(j) == [0, 0, 1, 2] and info["edge_margin"] == np.inf and info["int_margin"] == 0.0


# ---- the condition --------------------------------------------------------------------------------------------------------------------
def test_every_residual_call_is_decided_by_the_restatement_alone():
    """No residual call of any frozen or live case, and no stand-alone call, lies within the derived slack of an edge: the ancestors of
    all of them are the restatement's to say.  Prints the closest call of every run (pytest -s)."""
    frozen = {**IC.cases(), **AUX}
    lines = []
    for name, case in frozen.items():
        if case["strategy"] != S.RESAMPLE_RESIDUAL:
            continue
        calls = _golden(name)["residual_calls"]
        assert len(calls) == int(_golden(name)["resamples"])                # no step is left out
        lines.append("%-28s %3d calls, margin / slack >= %.1e" % (name, len(calls), _decided(calls, name)))
    for p in SIZE_CASES:
        if p[1] != "residual":
            continue
        calls = _size_reference(*p)[1]["residual_calls"]
        assert len(calls) == IC.SIZE_STEPS
        lines.append("%-28s %3d calls, margin / slack >= %.1e" % (_size_id(p), len(calls), _decided(calls, _size_id(p))))
    for n, m in IC.STANDALONE:
        lines.append("stand-alone %-16s   1 call,  margin / slack >= %.1e" % ((n, m), _decided(_standalone_reference(n, m)[4], "stand-alone %d -> %d" % (n, m))))
    print("\n" + "\n".join(lines))


def test_uniform_weights_are_refused_by_the_condition():
    """the corner the condition exists for: N = M and equal weights give nw_i = 1 within an ulp, margin 0 <= slack"""
    j, info = ind.resample_residual(np.full(400, 1.0 / 400), np.arange(400), np.zeros(400))
    assert info["int_margin"] <= ind.residual_slack(400, 400, 1.0, info["nw_max"], max(info["R"], 1))[0]


# ---- misreadings of the reference: the frozen outputs must refuse them ---------------------------------------------------------------
def _distance(name, **kw):
    """how far a variant of the restatement is from the frozen outputs of a case: (max |dll|, max |dx|, ancestors equal)"""
    cases = {**IC.cases(), **AUX}
    d, r = _golden(name), IC.run_independent(ob, cases[name], **kw)
    return np.max(np.abs(r["ll_steps"] - d["ll_steps"])), np.max(np.abs(r["x_final"] - d["x_final"])), np.array_equal(r["anc_final"], d["anc_final"])


class _ResampledLambda(ind.AuxiliaryParticleFilter):
    """lambda[j[i]] where the reference notes "unresampled lambda[i]" (src/filtering.jl:209-213)"""

    def new_weights(self, lam, j):
        return lam[j] - np.log(self.pf.N)


class _FirstMeasurementUsed(ind.AuxiliaryParticleFilter):
    """a correct! that weighs y in while no predict! has done so yet (src/filtering.jl:170-174 never reads y)"""

    def correct(self, u, y, t):
        return self.pf.correct(u, y, t) if self.pf.t == 1 else super().correct(u, y, t)


class _FromThePrediction(ind.AuxiliaryParticleFilter):
    """the advanced variant propagating the noise-free prediction again where src/filtering.jl:228 reads xprev[j]"""

    def __init__(self, pf):
        super().__init__(pf, advanced=True)

    def source(self, xprev, xpred):
        return xpred


@pytest.mark.parametrize("mode", list(IC.MODES))
@pytest.mark.parametrize("strategy", list(IC.STRATEGIES))
def test_a_resampled_lambda_is_seen(strategy, mode):
    dll, dx, _ = _distance("aux_lg_%s_%s" % (strategy, mode), wrap=_ResampledLambda)
    assert dll > SEEN * TOL_LL


@pytest.mark.parametrize("mode", list(IC.MODES))
def test_a_first_measurement_that_is_used_is_seen(mode):
    dll, dx, _ = _distance("aux_lg_systematic_%s" % mode, wrap=_FirstMeasurementUsed)
    assert dll > SEEN * TOL_LL


@pytest.mark.parametrize("mode", list(IC.MODES))
def test_an_advanced_variant_that_starts_from_the_prediction_is_seen(mode):
    dll, dx, _ = _distance("aux_quadtank_%s" % mode, wrap=_FromThePrediction)
    assert dx > SEEN * TOL_X and (mode == "forward" or dll > SEEN * TOL_LL)


@pytest.mark.parametrize("name", ["pf_lg_residual", "pf_lg_residual_thr1", "aux_lg_residual_forward", "aux_lg_residual_loglik"])
def test_residual_uniforms_counted_from_zero_are_seen(name, monkeypatch):
    """the multinomial part reading U[0], U[1], ... where output m reads U[m]"""
    right = ind.resample_residual

    def from_zero(we, jprev, U, M=None):
        num = right(we, jprev, U, M)[1]["num"]
        return right(we, jprev, np.concatenate([np.zeros(num), U]), M)

    monkeypatch.setattr(ind, "resample_residual", from_zero)
    dll, dx, same = _distance(name)
    assert dll > SEEN * TOL_LL and dx > SEEN * TOL_X
    # where the last predict! does not resample (threshold below 1: the plain filter, the wrapped update! of loglik) the final ancestors
    # are 0..N-1 either way
    assert not same or name in ("pf_lg_residual", "aux_lg_residual_loglik")
