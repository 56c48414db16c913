"""The fused timestep at resample_threshold 1 without the running maximum nobody reads (host/run_plan.hpp: RunKey::skip_max, RUN_NO_MAX;
kernels/resprop.hpp: NOMAX; kernels/accum.hpp: block_flush_sums; kernels/resample.hpp: res_head<..., NOMAX>).

In a level-3 run every launch that another launch with a weighting phase follows is level 4: no maximum and no NaN flag of the weights in
its rounds, no wave_max and no atomicMax in its tail, no ACC_PM load in its head, NaN published in FilterScal::mtrue and ::wmax.
LLPF_SKIP_MAX=0 keeps every launch of the same build at level 3, the form as it was.  The maximum is read by nobody, so nothing may change
a bit: every case runs under both settings, and both are compared against the device-order oracle and against each other (uint64 views,
no tolerance) — ll, the per-step log-likelihoods, final particles, weights, ancestors, the resample count, the exact redos and the fused
launches; last_run_form() says which form ran.

The cases: fewer blocks than accumulator shards and ragged last tiles; block counts that wrap 8 and 32 shards; peaked weights, whose bound
tests fail in mid-run (the exact redo is the reader a missing maximum would break: its weights and their maximum are formed again by the
weighting launch); NaN weights (the run's status, redos and launches); a step without a measurement; a model without an input; and
what a handle shows after a run — the maxw accessor, correct! and predict! as single verbs, and further runs that capture and replay
the graph."""
import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import models as M
import oracle_binding as ob
from thr1_common import assert_same, oracle, peaked_workload, snapshot, workload

pytestmark = pytest.mark.gpu

SWITCH = "LLPF_SKIP_MAX"
OTHERS = ("LLPF_SKIP_W", "LLPF_SKIP_ANC", "LLPF_LEAN", "LLPF_ABLATE")
FORMS = ("default", "0")       # the switch unset (level 4 where the plan allows) / set to 0 (level 3 throughout)
T = 12


def _set(monkeypatch, form):
    for name in OTHERS:
        monkeypatch.delenv(name, raising=False)
    if form == "default":
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, form)


def _assert_form(g, form, what):
    f = g.last_run_form()
    assert f["weights_not_stored"] and f["ancestors_not_stored"] and f["lean"], "%s: not a level-3 run: %r" % (what, f)
    assert f["no_maximum"] == (form == "default"), "%s: LLPF_SKIP_MAX %s ran as %r" % (what, form, f)
    return f


def _reference(cfg, U, Y):
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    return o, snapshot(o, ro)


def _both_forms(monkeypatch, cfg, U, Y, want, what):
    got = {}
    for form in FORMS:
        _set(monkeypatch, form)
        g = _capi.FilterHandle(cfg)
        g.reset()
        rg = g.run(U, Y, 1.0, ll_steps=True)
        f = _assert_form(g, form, what)
        launches = g.last_run_stats()["fused_launches"]
        assert launches >= len(Y), "the fused kernel did not run"
        got[form] = snapshot(g, rg)
        assert_same(got[form], want, "%s, LLPF_SKIP_MAX %s against the oracle:" % (what, form))
        got[form].append(("exact_redos", np.array([f["exact_redos"]], dtype=np.int64)))
        got[form].append(("fused_launches", np.array([launches], dtype=np.int64)))
    assert_same(got["default"], got["0"], what + ", the two forms:")
    return got


# two blocks and three (fewer than 8 shards; the last tile holds one particle); 10 blocks wrap 8 shards, 34 wrap 32; ragged, 69 tiles
@pytest.mark.parametrize("N", [1025, 2049, 9 * 1024 + 1, 33 * 1024 + 1, 70001])
def test_headline_system(N, monkeypatch):
    cfg, U, Y = workload(N, T)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    _both_forms(monkeypatch, cfg, U, Y, want, "N = %d" % N)


def test_peaked_weights(monkeypatch):
    """measurement noise of standard deviation 1e-4: bound tests fail in mid-run where the oracle's do, and each exact redo takes the
    maximum the weighting launch leaves in front of it — the level-4 launch whose weights it forms again left none"""
    cfg, U, Y = peaked_workload(8192, T)
    o, want = _reference(cfg, U, Y)
    assert o.exact_steps() >= 1, "no bound test fails: the case does not reach the exact redo"
    got = _both_forms(monkeypatch, cfg, U, Y, want, "peaked weights")
    for form in FORMS:
        assert int(dict(got[form])["exact_redos"][0]) == o.exact_steps(), "LLPF_SKIP_MAX %s: exact redos" % form


def test_nan_weights_at_one_step(monkeypatch):
    """Two outputs, the second NaN at step 6: every weight of the launch of step 5 — a level-4 launch — is NaN.  That launch keeps no NaN flag
    of the weights; their exp-weights are NaN too, so the NaN count and the zero sum stop the head of step 6, the redo finds the weights
    degenerate and the run ends with LLPF_ERR_DEGENERATE.  Status, redo count and launch count equal level 3's, in a run that ends at the
    degenerate step and in one that goes on (tests/test_gpu_lean_round.py says what the later steps do)."""
    kd = 6
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, T)
    Y = Y.copy()
    Y[kd, 1] = np.nan
    cfg = S.make_config(model, 2049, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, 1000, 0)
    o7, _ = _reference(cfg, U[:kd + 1], Y[:kd + 1])
    assert o7.L.orc_degenerate(o7.h) == 1 and o7.exact_steps() == 1
    seen = {}
    for steps in (kd + 1, T):
        for form in FORMS:
            _set(monkeypatch, form)
            g = _capi.FilterHandle(cfg)
            g.reset()
            with pytest.raises(_capi.DegenerateWeights) as ei:
                g.run(U[:steps], Y[:steps], 1.0, ll_steps=True)
            f = _assert_form(g, form, "NaN measurement at step %d, %d steps" % (kd, steps))
            seen[steps, form] = (ei.value.code, f["exact_redos"], g.last_run_stats()["fused_launches"])
            print("%d steps, LLPF_SKIP_MAX %s: status %d, exact redos %d, fused launches %d" % ((steps, form) + seen[steps, form]))
    for steps in (kd + 1, T):
        assert seen[steps, "default"] == seen[steps, "0"], "%d steps, the two forms: %r" % (steps, seen)
        want_redos = o7.exact_steps() + (steps - (kd + 1))
        for form in FORMS:
            assert seen[steps, form][:2] == (4, want_redos), "%d steps, LLPF_SKIP_MAX %s: %r, %d redos expected" % (steps, form, seen[steps, form], want_redos)


def test_a_step_without_a_measurement(monkeypatch):
    cfg, U, Y = workload(2049, T)
    Y = Y.copy()
    Y[6] = np.nan
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    _both_forms(monkeypatch, cfg, U, Y, want, "no measurement at step 6")


def test_model_without_an_input(monkeypatch):
    base = M.lg_test_model()
    A = np.array(base.A[:4]).reshape(2, 2)
    Cm = np.array(base.C[:2]).reshape(1, 2)
    g0 = S.make_gaussian
    model = S.make_lg_model(A, None, Cm, g0(np.zeros(2), 0.1 ** 2), g0(np.zeros(1), np.ones(1)), g0(np.array([0.3, -0.5]), 4.0), 1.0)
    assert model.nu == 0
    _, U, Y = M.simulate_lg(model, T, seed=3)
    cfg = S.make_config(model, 2049, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, 1000, 0)
    o, want = _reference(cfg, U, Y)
    assert o.resample_count() == T
    _both_forms(monkeypatch, cfg, U, Y, want, "nu = 0")


def _after_a_run(h, U, Y, t):
    """what a handle shows behind a run: the maxw accessor, then correct! and predict! as single verbs and the state they leave"""
    out = [("maxw after the run", np.array([h.maxw()]))]
    out.append(("ll of correct!", np.array([h.correct(U[0], Y[0], t)])))
    out.append(("maxw after correct!", np.array([h.maxw()])))
    out.append(("weights after correct!", h.weights()))
    h.predict(U[0], t)
    out.append(("maxw after predict!", np.array([h.maxw()])))
    out.append(("particles after predict!", h.particles()))
    out.append(("weights after predict!", h.weights()))
    out.append(("ancestors after predict!", np.asarray(h.ancestors()).astype(np.int64)))
    return out


def test_a_handle_after_runs(monkeypatch):
    """Three runs on one handle, each from a reset (the second captures the graph, the third replays it), and behind the last the maxw
    accessor and single verbs: the runs equal the oracle's, and everything — what the verbs behind them return included — equals what the
    form with the maximum returns.  No launch's NaN is left in FilterScal::mtrue or ::wmax: the run's last head publishes a real maximum
    and k_post_predict resets both."""
    N = 2049
    cfg, U, Y = workload(N, T)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    want = []
    for _ in range(3):
        o.reset()
        n0 = o.resample_count()
        want.append(snapshot(o, o.run(U, Y, 1.0, ll_steps=True), n0))
    traces, after = {}, {}
    for form in FORMS:
        _set(monkeypatch, form)
        g = _capi.FilterHandle(cfg)
        traces[form] = []
        for p in range(3):
            g.reset()
            rg = g.run(U, Y, 1.0, ll_steps=True)
            _assert_form(g, form, "pass %d" % p)
            traces[form].append(snapshot(g, rg))
            assert_same(traces[form][p], want[p], "pass %d, LLPF_SKIP_MAX %s against the oracle:" % (p, form))
        after[form] = _after_a_run(g, U, Y, float(T))
        for tag, v in after[form]:
            assert not np.any(np.isnan(v)), "LLPF_SKIP_MAX %s: %s is NaN" % (form, tag)
    for p in range(3):
        assert_same(traces["default"][p], traces["0"][p], "pass %d, the two forms:" % p)
    assert_same(after["default"], after["0"], "behind the runs, the two forms:")
