"""The fused timestep at resample_threshold 1 without its ancestor store between a run's steps (host/run_plan.hpp: skip_anc_run;
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
from gpu_common import assert_state_equal, assert_steps_equal
from test_gpu_skip_weight_store import _bits, _oracle, _outlier_that_fails_exactly_step

pytestmark = pytest.mark.gpu

FORMS = ("default", "0")       # LLPF_SKIP_ANC unset / LLPF_SKIP_ANC=0
OWN_CAP = 2048                 # entries of the owner table (csrc/kernels/resample.hpp); beyond it a source is found by descent
TILE = 1024


def _cfg(N, T, strategy=S.RESAMPLE_SYSTEMATIC):
    """the system of the headline workload (bench.build_workload("lg")), threshold 1, seeded as bench.py seeds it"""
    import bench
    model, U, Y, kind, _, _ = bench.build_workload("lg", N, T)
    return S.make_config(model, N, kind, strategy, 1.0, 1000, 0), U, Y


def _set_form(monkeypatch, form):
    monkeypatch.delenv("LLPF_SKIP_W", raising=False)
    if form == "default":
        monkeypatch.delenv("LLPF_SKIP_ANC", raising=False)
    else:
        monkeypatch.setenv("LLPF_SKIP_ANC", form)


def _assert_form(g, form, what=""):
    f = g.last_run_form()
    assert f["weights_not_stored"], "%s: the run stored its weights: %r" % (what, f)
    assert f["ancestors_not_stored"] == (form == "default"), "%s: LLPF_SKIP_ANC %s ran as %r" % (what, form, f)
    return f


def _snapshot(h, r, n0=0):
    """what a handle shows after a run: ll, ll_steps, particles, weights, ancestors, resamples of that run"""
    return [("ll", np.array([r["ll"]])), ("ll_steps", r["ll_steps"].copy()), ("particles", h.particles()), ("weights", h.weights()),
            ("ancestors", np.asarray(h.ancestors()).astype(np.int64)), ("resample_count", np.array([h.resample_count() - n0], dtype=np.int64))]


def _assert_same(got, want, what):
    for (tag, a), (_, b) in zip(got, want):
        if tag == "ll_steps":
            assert_steps_equal(a, b, what + " ll_steps")
        else:
            assert_state_equal(a, b, what + " " + tag)


def _both_forms(monkeypatch, cfg, U, Y, want, what, T):
    got = {}
    for form in FORMS:
        _set_form(monkeypatch, form)
        g = _capi.FilterHandle(cfg)
        g.reset()
        rg = g.run(U, Y, 1.0, ll_steps=True)
        assert g.last_run_stats()["fused_launches"] >= T, "the fused kernel did not run"
        f = _assert_form(g, form, what)
        got[form] = _snapshot(g, rg)
        _assert_same(got[form], want, "%s, LLPF_SKIP_ANC %s against the oracle:" % (what, form))
        got[form].append(("exact_redos", np.array([f["exact_redos"]], dtype=np.int64)))
    _assert_same(got["default"], got["0"], what + ", the two forms:")
    return got


_reference = {}


def _c2_reference(N, T, strategy, threads=1):
    """the oracle's run, computed once per case and left unchanged"""
    key = (N, T, strategy)
    if key not in _reference:
        cfg, U, Y = _cfg(N, T, strategy)
        try:
            o = _oracle(cfg, threads)
            ro = o.run(U, Y, 1.0, ll_steps=True)
        finally:
            ob.set_threads(1)
        assert o.resample_count() == T
        _reference[key] = (cfg, U, Y, _snapshot(o, ro))
    return _reference[key]


@pytest.mark.parametrize("T", [12, 2])                  # T = 2: one launch that skips, one that stores
@pytest.mark.parametrize("strategy", [S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED])
@pytest.mark.parametrize("N", [1025, 2048, 70001])      # two tiles, the second nearly empty; exact tiles; ragged, 69 tiles
def test_runs_equal_the_oracle_and_the_storing_form(N, strategy, T, monkeypatch):
    cfg, U, Y, want = _c2_reference(N, T, strategy)
    _both_forms(monkeypatch, cfg, U, Y, want, "N = %d, strategy %d, T = %d" % (N, strategy, T), T)


def test_all_blocks_resident(monkeypatch):
    """N = 10^6: 977 blocks, all resident together — the regime of the headline workload"""
    T = 5
    cfg, U, Y, want = _c2_reference(10 ** 6, T, S.RESAMPLE_SYSTEMATIC, threads=16)
    _both_forms(monkeypatch, cfg, U, Y, want, "N = 10^6", T)


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
            _assert_form(h, form, tag)
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
    cfg, U, Y = _cfg(N, T)
    want = _trace(ob.OracleFilter(cfg, ob.ORDER_DEVICE), U, Y, False)
    traces = {}
    for form in FORMS:
        _set_form(monkeypatch, form)
        traces[form] = _trace(_capi.FilterHandle(cfg), U, Y, True, form)
        for (tag, a), (_, b) in zip(traces[form], want):
            assert_state_equal(a, b, "LLPF_SKIP_ANC %s, %s" % (form, tag))
    for (tag, a), (_, b) in zip(traces["default"], traces["0"]):
        assert_state_equal(a, b, "the two forms, " + tag)


def test_failed_bound_test_in_mid_run(monkeypatch):
    """an outlier at step kf fails exactly that step's bound test: the exact redo (the storing form, from re-formed weights) is taken
    once, and the launches after it skip again"""
    N, T, kf = 5001, 30, 11
    cfg, U, Y = _cfg(N, T)
    Yo = _outlier_that_fails_exactly_step(cfg, U, Y, kf)
    o = _oracle(cfg)
    ro = o.run(U, Yo, 1.0, ll_steps=True)
    assert o.exact_steps() == 1
    got = _both_forms(monkeypatch, cfg, U, Yo, _snapshot(o, ro), "outlier at step %d" % kf, T)
    for form in FORMS:
        redos = int(dict(got[form])["exact_redos"][0])
        assert redos == 1, "LLPF_SKIP_ANC %s: the exact redo was taken %d times, not once" % (form, redos)


def test_last_output_found_by_descent(monkeypatch):
    """Measurement noise of standard deviation 1e-4 on the C2 system: one particle takes most of the weight, its tile owns more outputs
    than the owner table holds, and the source of output M - 1 — the entry kept behind the loop — comes from the descent."""
    import models as M
    N, T = 5000, 12
    base = M.lg_test_model()
    nx, nu, ny = base.nx, base.nu, base.ny
    A = np.array(base.A[:nx * nx]).reshape(nx, nx)
    B = np.array(base.B[:nx * nu]).reshape(nx, nu)
    Cm = np.array(base.C[:ny * nx]).reshape(ny, nx)
    g0 = S.make_gaussian
    model = S.make_lg_model(A, B, Cm, g0(np.zeros(2), 0.1 ** 2), g0(np.zeros(1), np.full(1, 1e-8)), g0(np.array([0.3, -0.5]), 4.0), 1.0)
    _, U, Y = M.simulate_lg(model, T, seed=1)
    cfg = S.make_config(model, N, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, 1000, 0)
    by_descent = 0
    for k in range(1, T):              # the ancestors of launch k - 1 (one that skips: it is not the run's last) are what a run of k steps leaves
        o = _oracle(cfg)
        o.run(U[:k], Y[:k], 1.0)
        j = np.asarray(o.ancestors()).astype(np.int64)
        first = int(np.flatnonzero(j // TILE == j[N - 1] // TILE)[0])      # first output of the tile that owns output M - 1
        by_descent += (N - 1) - first >= OWN_CAP
    assert by_descent >= 1, "in no launch that skips is output M - 1 beyond its tile's owner table"
    o = _oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    got = _both_forms(monkeypatch, cfg, U, Y, _snapshot(o, ro), "peaked weights", T)
    assert int(dict(got["default"])["exact_redos"][0]) == o.exact_steps()
