"""A round of the level-3 output loop without its repeated work (kernels/resprop.hpp: LLPF_LR_*): the quantum taken out of the fixed-point
exp-weight, B u by one add, no padding test, the uniforms' power-of-two scalings folded (and, in builds that ask for it, the NaN count
of the exp-weights as a lane flag).
None of it may change a bit.  Every case runs under both settings of LLPF_LEAN — level 3, the kernel with these rounds, and level 2, the
same build's kernel with the rounds as they were — and both are compared against the device-order oracle and against each other (uint64
views, no tolerance): ll, the per-step log-likelihoods, final particles, weights, ancestors, the resample count and the exact redos;
last_run_form() says which kernel ran.

The cases are the ones at which such a round can go wrong: quanta of 51, 50 and 45 fraction bits with ragged last tiles; exp-weights
below 2^-33 and exactly zero (both arms of the fixed-point shift, zero quanta); a model without an input and one whose B u is -0.0 at a
step (the select that one add replaces); a step without a measurement; and NaN weights (the redo they ask for, and the status the run ends with)."""
import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import models as M
from thr1_common import FORMS, assert_form, both_forms, oracle, peaked_workload, set_form, snapshot, workload

pytestmark = pytest.mark.gpu

SWITCH = "LLPF_LEAN"
T = 12
N = 2049


def _reference(cfg, U, Y):
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    return o, snapshot(o, ro)


def _config(model, n=N):
    return S.make_config(model, n, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, 1000, 0)


def _lg_model(B):
    """the headline system (models.lg_test_model) with another input matrix, or none"""
    base = M.lg_test_model()
    A = np.array(base.A[:4]).reshape(2, 2)
    Cm = np.array(base.C[:2]).reshape(1, 2)
    g0 = S.make_gaussian
    return S.make_lg_model(A, B, Cm, g0(np.zeros(2), 0.1 ** 2), g0(np.zeros(1), np.ones(1)), g0(np.array([0.3, -0.5]), 4.0), 1.0)


@pytest.mark.parametrize("n", [1025, 2049, 70001])      # K = 51, 50 and 45; the last tile holds 1, 1 and 369 particles
def test_headline_system(n, monkeypatch):
    assert 62 - int(np.ceil(np.log2(n))) == {1025: 51, 2049: 50, 70001: 45}[n]
    cfg, U, Y = workload(n, T)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "N = %d" % n, T)


def test_peaked_weights(monkeypatch):
    """measurement noise of standard deviation 1e-4: nearly every exp-weight is below 2^-33 (the arm of the fixed-point value that has no
    high word) or exactly zero (a zero quantum); the bound test fails where the oracle's does"""
    cfg, U, Y = peaked_workload(8192, T)
    o, want = _reference(cfg, U, Y)
    got = both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "peaked weights", T)
    for form in got:
        assert int(dict(got[form])["exact_redos"][0]) == o.exact_steps(), "LLPF_LEAN %s: exact redos" % form


def test_model_without_an_input(monkeypatch):
    """nu = 0: the round adds -0.0 where the select took A x as it was"""
    model = _lg_model(None)
    assert model.nu == 0
    _, U, Y = M.simulate_lg(model, T, seed=3)
    cfg = _config(model)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "nu = 0", T)


def test_input_term_of_negative_zero(monkeypatch):
    """u = 0 at step 5 with a negative entry in B: B u is (-0.0, +0.0) there, the sign of zero the select protected"""
    B = np.array([[-0.1], [0.0]])
    model = _lg_model(B)
    _, U, Y = M.simulate_lg(model, T, seed=4)
    U = U.copy()
    U[5] = 0.0
    assert np.signbit(B[0, 0] * U[5, 0]) and not np.signbit(B[1, 0] * U[5, 0])
    cfg = _config(model)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "B u = -0.0 at step 5", T)


def test_a_step_without_a_measurement_in_mid_run(monkeypatch):
    cfg, U, Y = workload(N, T)
    Y = Y.copy()
    Y[6] = np.nan
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "no measurement at step 6", T)


def test_nan_weights_at_one_step(monkeypatch):
    """Two outputs, the second NaN at step 6 (the first decides whether a step has a measurement at all): every weight and every exp-weight
    of the launch of step 5 is NaN.  The NaN flag reaches the accumulators, the head of step 6 asks for the exact redo, and the redo finds
    the weights degenerate: the oracle raises its flag (and a NaN log-likelihood of that step), the engine sets LLPF_ERR_DEGENERATE.

    From there on the two have nothing in common: the oracle goes on resampling from the NaN weights, while the engine's filter is dead —
    every later launch returns at its head's status test (kernels/resample.hpp: res_head), so no sums reach the next head, its bound test
    fails again, and the host redoes each of the remaining steps once before the run ends with the status (host/run.hpp: run_async).  The
    redo count is therefore compared where both sides define it, over the steps up to and including the degenerate one (a run of those 7
    steps: the oracle's count), and over the whole run it must be that count plus one per remaining step.  Status, redo count and launches
    are the same under both levels in both runs.

    What this case does not tell: whether the accumulator's own NaN count (WeightAcc::bad, or the lane flag of a build with
    LLPF_LR_NANFLAG) arrives.  With every exp-weight NaN the fixed-point sum is zero and the kernel's flag on the weights themselves is
    set as well, and either alone fails the head's bound test; no measurement makes an exp-weight NaN without its weight being NaN.  The
    case holds the run's course at both levels, not that one word."""
    kd = 6
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, T)
    Y = Y.copy()
    Y[kd, 1] = np.nan
    cfg = _config(model)
    o, want = _reference(cfg, U, Y)
    ll_steps = dict(want)["ll_steps"]
    assert np.isnan(ll_steps[kd]) and np.all(np.isfinite(ll_steps[:kd]))
    assert o.L.orc_degenerate(o.h) == 1
    o7, _ = _reference(cfg, U[:kd + 1], Y[:kd + 1])
    assert o7.L.orc_degenerate(o7.h) == 1 and o7.exact_steps() == 1
    o6, _ = _reference(cfg, U[:kd], Y[:kd])
    assert o6.L.orc_degenerate(o6.h) == 0 and o6.exact_steps() == 0      # nothing fails before the NaN
    seen = {}
    for steps in (kd + 1, T):
        for form in FORMS:
            set_form(monkeypatch, SWITCH, form)
            g = _capi.FilterHandle(cfg)
            g.reset()
            with pytest.raises(_capi.DegenerateWeights) as ei:
                g.run(U[:steps], Y[:steps], 1.0, ll_steps=True)
            f = assert_form(g, SWITCH, form, "NaN measurement at step %d, %d steps" % (kd, steps))
            seen[steps, form] = (ei.value.code, f["exact_redos"], g.last_run_stats()["fused_launches"])
            print("%d steps, LLPF_LEAN %s: status %d, exact redos %d, fused launches %d" % ((steps, form) + seen[steps, form]))
    for steps in (kd + 1, T):
        assert seen[steps, "default"] == seen[steps, "0"], "%d steps, the two levels: %r" % (steps, seen)
        want_redos = o7.exact_steps() + (steps - (kd + 1))
        for form in FORMS:
            assert seen[steps, form][:2] == (4, want_redos), "%d steps, LLPF_LEAN %s: %r, %d redos expected" % (steps, form, seen[steps, form], want_redos)
