"""The fused timestep at resample_threshold 1 with the run's constants compiled in (host/run_plan.hpp: RUN_LEAN; kernels/resprop.hpp: LEAN).

A run whose fused launches store neither weights nor ancestors, which resamples systematically and wants no weighted means, takes the
kernel that holds neither the stratified counts nor the means and tests neither.  LLPF_LEAN=0 pins the kernel with the run-time tests of
the same build.  The form only drops tests and arms such a run never takes, so everything here is bit for bit (uint64 views, no
tolerance): both forms against the device-order oracle and against each other — per-step log-likelihoods, final particles, weights,
ancestors and the resample count — and last_run_form() says which kernel ran."""
import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import oracle_binding as ob
from thr1_common import (FORMS, OWN_CAP, REPORTS, SWITCHES, TILE, assert_form, assert_same, both_forms, oracle, outlier_that_fails_exactly_step,
                         peaked_workload, set_form, snapshot, workload)

pytestmark = pytest.mark.gpu

SWITCH = "LLPF_LEAN"
T = 12


def _reference(cfg, U, Y):
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    return o, snapshot(o, ro)


@pytest.mark.parametrize("N", [1025, 2049, 70001])      # two tiles, the second holds one particle; three, likewise; ragged, 69 tiles
def test_runs_equal_the_oracle_and_the_form_with_the_tests(N, monkeypatch):
    cfg, U, Y = workload(N, T)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "N = %d" % N, T)


def test_a_step_without_a_measurement(monkeypatch):
    """st.has_y stays a run-time test of the lean kernel: step 5 has no measurement, the launch of step 4 weights nothing"""
    N = 2049
    cfg, U, Y = workload(N, T)
    Y = Y.copy()
    Y[5] = np.nan
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "no measurement at step 5", T)


def test_a_tile_owns_more_outputs_than_the_owner_table_holds(monkeypatch):
    """Measurement noise of standard deviation 1e-4 on the headline system: one particle takes most of the weight and its tile owns
    more than OWN_CAP outputs — their sources come from the descent behind the owner table."""
    N = 5000
    cfg, U, Y = peaked_workload(N, T)
    beyond = 0
    for k in range(1, T):              # the ancestors of launch k - 1 (a lean one: it is not the run's last) are what a run of k steps leaves
        o = oracle(cfg)
        o.run(U[:k], Y[:k], 1.0)
        owned = np.bincount(np.asarray(o.ancestors()).astype(np.int64) // TILE)
        beyond += int(owned.max() > OWN_CAP)
    assert beyond >= 1, "in no launch does a tile own more than OWN_CAP outputs"
    o, want = _reference(cfg, U, Y)
    got = both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "peaked weights", T)
    assert int(dict(got["default"])["exact_redos"][0]) == o.exact_steps()


def test_failed_bound_test_in_mid_run(monkeypatch):
    """an outlier at step kf fails exactly that step's bound test: the exact redo (the storing kernel, as ever) is counted once and the
    launches after it are the lean kernel again"""
    N, kf = 2049, 5
    cfg, U, Y = workload(N, T)
    Yo = outlier_that_fails_exactly_step(cfg, U, Y, kf)
    o, want = _reference(cfg, U, Yo)
    assert o.exact_steps() == 1
    got = both_forms(monkeypatch, SWITCH, cfg, U, Yo, want, "outlier at step %d" % kf, T)
    for form in FORMS:
        redos = int(dict(got[form])["exact_redos"][0])
        assert redos == 1, "LLPF_LEAN %s: the exact redo was taken %d times, not once" % (form, redos)


def test_two_runs_on_one_handle(monkeypatch):
    """the second run of a shape is captured, the third replays the graph: each from a reset, each equal to the oracle's"""
    N = 2049
    cfg, U, Y = workload(N, T)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)      # (reset in the loop, as the engine's handle is: every reset! draws fresh noise)
    want = []
    for _ in range(3):
        o.reset()
        n0 = o.resample_count()
        want.append(snapshot(o, o.run(U, Y, 1.0, ll_steps=True), n0))
    traces = {}
    for form in FORMS:
        set_form(monkeypatch, SWITCH, form)
        g = _capi.FilterHandle(cfg)
        traces[form] = []
        for p in range(3):
            g.reset()
            rg = g.run(U, Y, 1.0, ll_steps=True)
            assert_form(g, SWITCH, form, "pass %d" % p)
            traces[form].append(snapshot(g, rg))
            assert_same(traces[form][p], want[p], "pass %d, LLPF_LEAN %s against the oracle:" % (p, form))
    for p in range(3):
        assert_same(traces["default"][p], traces["0"][p], "pass %d, the two forms:" % p)


@pytest.mark.parametrize("case", ["stratified", "xmean", "threshold 0.5"])
def test_dispatch(case, monkeypatch):
    """what the plan must not run lean: stratified resampling and weighted means keep the kernel with the tests (and still store neither
    weights nor ancestors); below threshold 1 nothing is skipped at all"""
    set_form(monkeypatch, SWITCH, "default")
    N = 2049
    strategy = S.RESAMPLE_STRATIFIED if case == "stratified" else S.RESAMPLE_SYSTEMATIC
    thr = 0.5 if case == "threshold 0.5" else 1.0
    cfg, U, Y = workload(N, T, strategy, thr)
    xm = case == "xmean"
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True, xmean=xm)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True, xmean=xm)
    assert g.last_run_stats()["fused_launches"] > 0, "the fused kernel did not run"
    f = g.last_run_form()
    assert not f["lean"], "%s ran lean: %r" % (case, f)
    assert f["weights_not_stored"] == (thr == 1.0), "%s: %r" % (case, f)
    assert_same(snapshot(g, rg), snapshot(o, ro), case + " against the oracle:")
    if xm:
        # the means are never fed back and are plain fp64 sums of N products x_i we_i (sum we_i = 1) that engine and oracle group
        # differently: each is within N 2^-53 max|x| of the exact sum, so the two differ by at most N 2^-52 max|x|; |x| < 100 here
        xmax = 100.0
        assert np.max(np.abs(o.particles())) < xmax
        err = np.max(np.abs(rg["xmean"] - ro["xmean"]))
        print("xmean: max difference %.3e" % err)
        assert err <= N * 2.0 ** -52 * xmax


def test_the_ladder_of_levels(monkeypatch):
    """One run under the four settings that plan levels 0, 1, 2 and 3 (host/run_plan.hpp: RunLevel): three tiles, the last of one
    particle; T = 3 is two launches that leave out what the level says and one, the run's last, that stores.  last_run_form() reports
    the level, and the four runs equal the oracle's and each other bit for bit."""
    N, steps = 2049, 3
    cfg, U, Y = workload(N, steps)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == steps
    runs = []
    for level in range(4):
        if level < 3:
            set_form(monkeypatch, SWITCHES[level], "0")      # switch i set to 0 caps the level at i
        else:
            set_form(monkeypatch, SWITCH, "default")
        g = _capi.FilterHandle(cfg)
        g.reset()
        rg = g.run(U, Y, 1.0, ll_steps=True)
        assert g.last_run_stats()["fused_launches"] >= steps, "the fused kernel did not run"
        f = g.last_run_form()
        assert tuple(f[k] for k in REPORTS) == tuple(i < level for i in range(3)), "level %d ran as %r" % (level, f)
        runs.append(snapshot(g, rg))
        assert_same(runs[level], want, "level %d against the oracle:" % level)
    for level in range(1, 4):
        assert_same(runs[level], runs[0], "levels %d and 0:" % level)
