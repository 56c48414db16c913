"""The fused timestep at resample_threshold 1 without its weight store (host/run_plan.hpp: RUN_SKIP_W; kernels/resprop.hpp: SKIPW).

Every step of such a run resamples, so the weights a fused launch forms are read by nobody: the run's fused launches do not store
them, and the exact redo of a failed bound test has them formed again first.  LLPF_SKIP_W=0 pins the storing form.  Everything here
is bit for bit (uint64 views, no tolerance): both forms against the device-order oracle and against each other."""
import numpy as np
import pytest

from llpf_amd import _capi
import oracle_binding as ob
from gpu_common import assert_state_equal, assert_steps_equal
from thr1_common import FORMS, assert_form, bits, oracle, outlier_that_fails_exactly_step, set_form, workload

pytestmark = pytest.mark.gpu

SWITCH = "LLPF_SKIP_W"


def _assert_run_equal(rg, g, ro, o, what):
    assert bits(rg["ll"]) == bits(ro["ll"]), "%s: ll %r against %r" % (what, rg["ll"], ro["ll"])
    assert_steps_equal(rg["ll_steps"], ro["ll_steps"], what + " ll_steps", resamples=(g.resample_count(), o.resample_count()))
    assert g.resample_count() == o.resample_count(), what
    assert_state_equal(g.particles(), o.particles(), what + " particles")
    assert_state_equal(g.weights(), o.weights(), what + " weights()")


@pytest.mark.parametrize("N", [1025, 70001, 10**6])       # one tile + 1, ragged, the headline size
def test_plain_runs_equal_the_oracle_and_the_storing_form(N, monkeypatch):
    T = 50
    cfg, U, Y = workload(N, T)
    try:
        o = oracle(cfg, 16)
        ro = o.run(U, Y, 1.0, ll_steps=True)
    finally:
        ob.set_threads(1)
    got = {}
    for form in FORMS:
        set_form(monkeypatch, SWITCH, form)
        g = _capi.FilterHandle(cfg)
        g.reset()
        rg = g.run(U, Y, 1.0, ll_steps=True)
        assert_form(g, SWITCH, form)
        assert g.last_run_stats()["fused_launches"] == T
        _assert_run_equal(rg, g, ro, o, "LLPF_SKIP_W %s" % form)
        got[form] = (rg["ll"], rg["ll_steps"].copy(), g.particles(), g.weights())
    a, b = got["default"], got["0"]
    assert bits(a[0]) == bits(b[0])
    for x, y, what in zip(a[1:], b[1:], ("ll_steps", "particles", "weights()")):
        assert_state_equal(x, y, "the two forms: " + what)


@pytest.mark.parametrize("N", [1025, 70001])
def test_failed_bound_test_in_mid_run(N, monkeypatch):
    T, kf = 60, 23
    cfg, U, Y = workload(N, T)
    Yo = outlier_that_fails_exactly_step(cfg, U, Y, kf)
    o = oracle(cfg)
    ro = o.run(U, Yo, 1.0, ll_steps=True)
    assert o.exact_steps() == 1
    got = {}
    for form in FORMS:
        set_form(monkeypatch, SWITCH, form)
        g = _capi.FilterHandle(cfg)
        g.reset()
        rg = g.run(U, Yo, 1.0, ll_steps=True)
        f = assert_form(g, SWITCH, form)
        assert f["exact_redos"] == 1, "the exact redo was not taken exactly once: %r" % (f,)
        _assert_run_equal(rg, g, ro, o, "LLPF_SKIP_W %s" % form)
        got[form] = (rg["ll_steps"].copy(), g.particles(), g.weights())
    for x, y, what in zip(got["default"], got["0"], ("ll_steps", "particles", "weights()")):
        assert_state_equal(x, y, "the two forms: " + what)


def _after_the_run_trace(h, U, Y, Yo, engine):
    """a run, single verbs straight after it, a run after those, then four passes of one shape (the engine captures the second and
    replays the third and fourth), the last three with an outlier in mid-run; everything the handle shows after each.
    llpf_resample_count is the number of resampling predict!s of the LAST RUN (include/llpf.h; single verbs after it do not move it),
    the oracle's counter runs on: of the oracle the trace records what its last run added."""
    out = []
    last_run = [0]

    def run(Yp):
        n0 = h.resample_count()
        r = h.run(U, Yp, 1.0, ll_steps=True)
        last_run[0] = h.resample_count() - n0
        return r

    def state(tag):
        out.append((tag + " particles", h.particles()))
        out.append((tag + " weights", h.weights()))
        out.append((tag + " resample_count", np.array([h.resample_count() if engine else last_run[0]], dtype=np.int64)))

    h.reset()
    r = run(Y)
    out.append(("run 1 ll_steps", r["ll_steps"].copy()))
    state("run 1")
    out.append(("correct! after run 1", np.array([h.correct(U[0], Y[0], 1.0)])))
    state("correct!")
    h.predict(U[0], 1.0)
    state("predict!")
    h.predict(U[1], 2.0)                                   # a predict! straight after a predict!
    state("predict! 2")
    r = run(Y)                                             # a second run on the handle, from where the verbs left it
    out.append(("run 2 ll_steps", r["ll_steps"].copy()))
    state("run 2")
    redos, e0 = 0, (0 if engine else h.exact_steps())
    for p, Yp in enumerate((Y, Yo, Yo, Yo)):
        h.reset()
        r = run(Yp)
        out.append(("pass %d ll_steps" % p, r["ll_steps"].copy()))
        state("pass %d" % p)
        if engine:
            redos += h.last_run_form()["exact_redos"]
    return out, (redos if engine else h.exact_steps() - e0)


def test_after_the_run(monkeypatch):
    N, T, kf = 70001, 40, 17
    cfg, U, Y = workload(N, T)
    o = oracle(cfg)
    o.run(U, Y, 1.0)
    assert o.exact_steps() == 0
    Yo = Y.copy()
    Yo[kf] += 30.0            # far outside the cloud whatever the pass's noise (every reset! draws fresh noise)
    want, n_exact = _after_the_run_trace(ob.OracleFilter(cfg, ob.ORDER_DEVICE), U, Y, Yo, False)      # (the trace resets it, as it resets the engine's handle)
    assert n_exact >= 3, "the outlier does not fail a bound test in every pass that has it"

    traces = {}
    for form in FORMS:
        set_form(monkeypatch, SWITCH, form)
        g = _capi.FilterHandle(cfg)
        traces[form], redos = _after_the_run_trace(g, U, Y, Yo, True)
        assert redos == n_exact, "exact redos: %d against the oracle's %d exact steps" % (redos, n_exact)
        assert_form(g, SWITCH, form)
        for (tag, a), (_, b) in zip(traces[form], want):
            assert_state_equal(a, b, "LLPF_SKIP_W %s, %s" % (form, tag))
    for (tag, a), (_, b) in zip(traces["default"], traces["0"]):
        assert_state_equal(a, b, "the two forms, " + tag)


@pytest.mark.parametrize("N,thr", [(70001, 0.1), (1000, 1.0)])
def test_form_is_not_selected_below_threshold_one_or_for_one_tile(N, thr, monkeypatch):
    monkeypatch.delenv("LLPF_SKIP_W", raising=False)
    cfg, U, Y = workload(N, 20, thr=thr)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True)
    assert g.last_run_stats()["fused_launches"] > 0
    assert not g.last_run_form()["weights_not_stored"]
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    _assert_run_equal(rg, g, ro, o, "N = %d, threshold %g" % (N, thr))
