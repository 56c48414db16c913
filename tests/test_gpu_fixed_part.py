"""The fixed part of the fused timestep at level 3 (kernels/resprop.hpp: LEAN; kernels/resample.hpp: res_head / res_counts<..., LEAN>).

A level-3 launch passes its head, scan and tail with what the plan fixes for it compiled in: the head and the scan hold the argument
values of such a launch as constants and take 1 / M from the host, and the tail reduces the block's maximum, NaN flag and exp-sums behind
one barrier (block_flush).  LLPF_LEAN=0 runs the level-2 kernel of the same build, whose fixed part is the general one.  Neither form
changes a bit: both are compared against the device-order oracle and against each other (uint64 views, no tolerance) — ll, the per-step
log-likelihoods, final particles, weights, ancestors and the resample count — and last_run_form() says which kernel ran."""
import numpy as np
import pytest

from llpf_amd import _capi
import oracle_binding as ob
from thr1_common import (FORMS, OWN_CAP, REPORTS, TILE, assert_form, assert_same, both_forms, oracle, outlier_that_fails_exactly_step,
                         peaked_workload, set_form, snapshot, workload)

pytestmark = pytest.mark.gpu

SWITCH = "LLPF_LEAN"
T = 20


def _reference(cfg, U, Y):
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    return o, snapshot(o, ro)


@pytest.mark.parametrize("N", [1025, 4097, 70001])      # two tiles, the second holds one particle; five, likewise; ragged, 69 tiles
def test_runs_equal_the_oracle_and_the_general_fixed_part(N, monkeypatch):
    cfg, U, Y = workload(N, T)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "N = %d" % N, T)


def test_tiles_that_own_no_outputs(monkeypatch):
    """Measurement noise of standard deviation 1e-4 on the headline system: one tile owns more outputs than the owner table holds and
    tiles behind it own none (c_start == c_end).  Such a block goes through the one-barrier tail with nothing accumulated: the maximum
    -Inf, no NaN flag, zero sums."""
    N = 8192
    cfg, U, Y = peaked_workload(N, T)
    empty = beyond = 0
    for k in range(1, T):              # the ancestors of launch k - 1 (a level-3 one: it is not the run's last) are what a run of k steps leaves
        o = oracle(cfg)
        o.run(U[:k], Y[:k], 1.0)
        owned = np.bincount(np.asarray(o.ancestors()).astype(np.int64) // TILE, minlength=N // TILE)
        empty += int(owned.min() == 0)
        beyond += int(owned.max() > OWN_CAP)
    assert empty >= 1, "in no launch does a tile own no outputs (c_start == c_end)"
    assert beyond >= 1, "in no launch does a tile own more than OWN_CAP outputs"
    o, want = _reference(cfg, U, Y)
    got = both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "peaked weights", T)
    assert int(dict(got["default"])["exact_redos"][0]) == o.exact_steps()


def test_a_step_without_a_measurement_in_mid_run(monkeypatch):
    """step 10 has no measurement: the launch of step 9 weights nothing and its tail accumulates the prior alone"""
    N = 4097
    cfg, U, Y = workload(N, T)
    Y = Y.copy()
    Y[10] = np.nan
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    both_forms(monkeypatch, SWITCH, cfg, U, Y, want, "no measurement at step 10", T)


def test_failed_bound_test_in_mid_run(monkeypatch):
    """an outlier at step kf fails exactly that step's bound test: the head that notices reads the sums the tail of launch kf - 1
    accumulated, and the exact redo is taken once"""
    N, kf = 4097, 9
    cfg, U, Y = workload(N, T)
    Yo = outlier_that_fails_exactly_step(cfg, U, Y, kf)
    o, want = _reference(cfg, U, Yo)
    assert o.exact_steps() == 1
    got = both_forms(monkeypatch, SWITCH, cfg, U, Yo, want, "outlier at step %d" % kf, T)
    for form in FORMS:
        redos = int(dict(got[form])["exact_redos"][0])
        assert redos == 1, "LLPF_LEAN %s: the exact redo was taken %d times, not once" % (form, redos)


def test_two_runs_on_one_handle(monkeypatch):
    """the second run goes on from where the first left the handle: T = 20 is no multiple of the three accumulator slots, so its launches
    meet every slot in another role than the first run's"""
    N = 4097
    cfg, U, Y = workload(N, T)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    o.reset()
    want = []
    for _ in range(2):
        n0 = o.resample_count()        # the oracle's counter runs on, the engine's is the count of the last run
        want.append(snapshot(o, o.run(U, Y, 1.0, ll_steps=True), n0))
    traces = {}
    for form in FORMS:
        set_form(monkeypatch, SWITCH, form)
        g = _capi.FilterHandle(cfg)
        g.reset()
        traces[form] = []
        for p in range(2):
            rg = g.run(U, Y, 1.0, ll_steps=True)
            assert_form(g, SWITCH, form, "run %d" % p)
            traces[form].append(snapshot(g, rg))
            assert_same(traces[form][p], want[p], "run %d, LLPF_LEAN %s against the oracle:" % (p, form))
    for p in range(2):
        assert_same(traces["default"][p], traces["0"][p], "run %d, the two forms:" % p)


def test_last_run_form_reports_the_level(monkeypatch):
    """level 3 by default, level 2 under LLPF_LEAN=0"""
    cfg, U, Y = workload(1025, 3)
    for form, level in (("default", 3), ("0", 2)):
        set_form(monkeypatch, SWITCH, form)
        g = _capi.FilterHandle(cfg)
        g.reset()
        g.run(U, Y, 1.0)
        f = g.last_run_form()
        assert tuple(bool(f[k]) for k in REPORTS) == tuple(i < level for i in range(3)), "LLPF_LEAN %s ran as %r" % (form, f)
