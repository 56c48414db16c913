"""The fused timestep at resample_threshold 1 without its ancestor store between a run's steps (host/run_plan.hpp: RUN_SKIP_ANC;
kernels/resprop.hpp: SKIPA).

Every launch of such a run rewrites all N ancestors, so only those of the run's last launch reach a reader; the launches before it store
none but output M - 1's (the one entry the next launch's rounds of [c_end, M) may read; tests/test_stale_corner.py).  LLPF_SKIP_ANC=0 pins
the ancestor-storing form of the same build.  Everything here is bit for bit (uint64 views, no tolerance): both forms against the
device-order oracle and against each other — per-step log-likelihoods, final particles, weights and ancestors, the resample count.
(The entry stored behind the loop has no observer through the run API but the corner itself, which cannot be reached at will: its cover
is tests/test_stale_corner.py and the unchanged rounds of [c_end, M).)"""
import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import oracle_binding as ob
from gpu_common import assert_state_equal
from thr1_common import (FORMS, OWN_CAP, TILE, assert_form, both_forms, oracle, outlier_that_fails_exactly_step, peaked_workload, set_form,
                         snapshot, workload)

pytestmark = pytest.mark.gpu

SWITCH = "LLPF_SKIP_ANC"


_reference = {}


def _c2_reference(N, T, strategy, threads=1):
    """the oracle's run, computed once per case and left unchanged"""
    key = (N, T, strategy)
    if key not in _reference:
        cfg, U, Y = workload(N, T, strategy)
        try:
            o = oracle(cfg, threads)
            ro = o.run(U, Y, 1.0, ll_steps=True)
        finally:
            ob.set_threads(1)
        assert o.resample_count() == T
        _reference[key] = (cfg, U, Y, snapshot(o, ro))
    return _reference[key]


@pytest.mark.parametrize("T", [12, 2])                  # T = 2: one launch that skips, one that stores
@pytest.mark.parametrize("strategy", [S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED])
@pytest.mark.parametrize("N", [1025, 2048, 70001])      # two tiles, the second nearly empty; exact tiles; ragged, 69 tiles
def test_runs_equal_the_oracle_and_the_storing_form(N, strategy, T, monkeypatch):
    cfg, U, Y, want = _c2_reference(N, T, strategy)
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "N = %d, strategy %d, T = %d" % (N, strategy, T), T)


def test_all_blocks_resident(monkeypatch):
    """N = 10^6: 977 blocks, all resident together — the regime of the headline workload"""
    T = 5
    cfg, U, Y, want = _c2_reference(10 ** 6, T, S.RESAMPLE_SYSTEMATIC, threads=16)
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "N = 10^6", T)


def _trace(h, U, Y, engine, form=None):
    """a run, a single correct! + predict! straight after it (verbs that read what the run left), a second run from there"""
    out = []

    def state(tag):
        out.append((tag + " particles", h.particles()))
        out.append((tag + " weights", h.weights()))
        out.append((tag + " ancestors", np.asarray(h.ancestors()).astype(np.int64)))

    def run(tag):
        n0 = 0 if engine else h.resample_count()        # llpf_resample_count is the count of the last run; the oracle's counter runs on
        r = h.run(U, Y, 1.0, ll_steps=True)
        if engine:
            assert_form(h, SWITCH, form, tag)
        out.append((tag + " ll_steps", r["ll_steps"].copy()))
        out.append((tag + " resample_count", np.array([h.resample_count() - n0], dtype=np.int64)))
        state(tag)

    h.reset()
    run("run 1")
    out.append(("correct! ll", np.array([h.correct(U[0], Y[0], 1.0)])))
    state("correct!")
    h.predict(U[0], 1.0)
    out.append(("predict! resampled", np.array([int(h.last_resampled())], dtype=np.int64)))
    state("predict!")
    run("run 2")
    return out


def test_verbs_after_the_run_and_a_second_run(monkeypatch):
    N, T = 70001, 12
    cfg, U, Y = workload(N, T)
    want = _trace(ob.OracleFilter(cfg, ob.ORDER_DEVICE), U, Y, False)
    traces = {}
    for form in FORMS:
        set_form(monkeypatch, SWITCH, form)
        traces[form] = _trace(_capi.FilterHandle(cfg), U, Y, True, form)
        for (tag, a), (_, b) in zip(traces[form], want):
            assert_state_equal(a, b, "LLPF_SKIP_ANC %s, %s" % (form, tag))
    for (tag, a), (_, b) in zip(traces["default"], traces["0"]):
        assert_state_equal(a, b, "the two forms, " + tag)


def test_failed_bound_test_in_mid_run(monkeypatch):
    """an outlier at step kf fails exactly that step's bound test: the exact redo (the storing form, from re-formed weights) is taken
    once, and the launches after it skip again"""
    N, T, kf = 5001, 30, 11
    cfg, U, Y = workload(N, T)
    Yo = outlier_that_fails_exactly_step(cfg, U, Y, kf)
    o = oracle(cfg)
    ro = o.run(U, Yo, 1.0, ll_steps=True)
    assert o.exact_steps() == 1
    got = both_forms(monkeypatch, SWITCH, cfg, U, Yo, snapshot(o, ro), "outlier at step %d" % kf, T)
    for form in FORMS:
        redos = int(dict(got[form])["exact_redos"][0])
        assert redos == 1, "LLPF_SKIP_ANC %s: the exact redo was taken %d times, not once" % (form, redos)


def test_last_output_found_by_descent(monkeypatch):
    """Measurement noise of standard deviation 1e-4 on the C2 system: one particle takes most of the weight, its tile owns more outputs
    than the owner table holds, and the source of output M - 1 — the entry kept behind the loop — comes from the descent."""
    N, T = 5000, 12
    cfg, U, Y = peaked_workload(N, T)
    by_descent = 0
    for k in range(1, T):              # the ancestors of launch k - 1 (one that skips: it is not the run's last) are what a run of k steps leaves
        o = oracle(cfg)
        o.run(U[:k], Y[:k], 1.0)
        j = np.asarray(o.ancestors()).astype(np.int64)
        first = int(np.flatnonzero(j // TILE == j[N - 1] // TILE)[0])      # first output of the tile that owns output M - 1
        by_descent += (N - 1) - first >= OWN_CAP
    assert by_descent >= 1, "in no launch that skips is output M - 1 beyond its tile's owner table"
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    got = both_forms(monkeypatch, SWITCH, cfg, U, Y, snapshot(o, ro), "peaked weights", T)
    assert int(dict(got["default"])["exact_redos"][0]) == o.exact_steps()
