"""Shared frame of the GPU tests of the fused timestep at resample_threshold 1 (host/run_plan.hpp: RunLevel; kernels/resprop.hpp: LEVEL).

A merged fused run of filters of several tiles at threshold 1 is planned at one of four levels: its launches store weights and ancestors
(0), no weights (1), nor ancestors but output M - 1's (2), and are the kernel for systematic resampling without weighted means (3).
LLPF_SKIP_W=0, LLPF_SKIP_ANC=0 and LLPF_LEAN=0 cap the level at 0, 1 and 2.  The levels compute the same bits, so the tests compare both
settings of one switch against the device-order oracle and against each other: the helpers here take the switch's name."""
import numpy as np

from llpf_amd import _capi, _structs as S
import oracle_binding as ob
from gpu_common import assert_state_equal, assert_steps_equal

SWITCHES = ("LLPF_SKIP_W", "LLPF_SKIP_ANC", "LLPF_LEAN")              # switch i set to 0 caps the level at i
REPORTS = ("weights_not_stored", "ancestors_not_stored", "lean")      # last_run_form(): entry i is level > i
FORMS = ("default", "0")       # the switch unset / set to 0
OWN_CAP = 2048                 # entries of the owner table (csrc/kernels/resample.hpp); beyond it a source is found by descent
TILE = 1024


def workload(N, T, strategy=S.RESAMPLE_SYSTEMATIC, thr=1.0):
    """the system of the headline workload (bench.build_workload("lg"): linear-Gaussian, nx = 2), seeded as bench.py seeds it"""
    import bench
    model, U, Y, kind, _, _ = bench.build_workload("lg", N, T)
    return S.make_config(model, N, kind, strategy, thr, 1000, 0), U, Y


def peaked_workload(N, T):
    """Measurement noise of standard deviation 1e-4 on the headline system: one particle takes most of the weight, and its tile owns more
    outputs than the owner table holds"""
    import models as M
    base = M.lg_test_model()
    nx, nu, ny = base.nx, base.nu, base.ny
    A = np.array(base.A[:nx * nx]).reshape(nx, nx)
    B = np.array(base.B[:nx * nu]).reshape(nx, nu)
    Cm = np.array(base.C[:ny * nx]).reshape(ny, nx)
    g0 = S.make_gaussian
    model = S.make_lg_model(A, B, Cm, g0(np.zeros(2), 0.1 ** 2), g0(np.zeros(1), np.full(1, 1e-8)), g0(np.array([0.3, -0.5]), 4.0), 1.0)
    _, U, Y = M.simulate_lg(model, T, seed=1)
    return S.make_config(model, N, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 1.0, 1000, 0), U, Y


def oracle(cfg, threads=1):
    ob.set_threads(threads)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    o.reset()
    return o


def bits(v):
    return np.float64(v).view(np.uint64)


def snapshot(h, r, n0=0):
    """what a handle shows after a run: ll, ll_steps, particles, weights, ancestors, resamples of that run"""
    return [("ll", np.array([r["ll"]])), ("ll_steps", r["ll_steps"].copy()), ("particles", h.particles()), ("weights", h.weights()),
            ("ancestors", np.asarray(h.ancestors()).astype(np.int64)), ("resample_count", np.array([h.resample_count() - n0], dtype=np.int64))]


def assert_same(got, want, what):
    for (tag, a), (_, b) in zip(got, want):
        if tag == "ll_steps":
            assert_steps_equal(a, b, what + " ll_steps")
        else:
            assert_state_equal(a, b, what + " " + tag)


def outlier_that_fails_exactly_step(cfg, U, Y, kf):
    """Measurements with an outlier at step kf, chosen on the CPU with the device-order oracle so that the bound test of exactly that
    step fails (S < 2^-10): no exact step without the outlier, none in the steps before kf, one in the whole run."""
    o = oracle(cfg)
    o.run(U, Y, 1.0)
    assert o.exact_steps() == 0, "the plain data already fail a bound test"
    for amp in (6.0, 8.0, 10.0, 12.0, 16.0, 20.0, 30.0):
        Yo = Y.copy()
        Yo[kf] += amp
        o = oracle(cfg)
        o.run(U[:kf], Yo[:kf], 1.0)
        before = o.exact_steps()
        o = oracle(cfg)
        o.run(U[:kf + 1], Yo[:kf + 1], 1.0)
        upto = o.exact_steps()
        o = oracle(cfg)
        o.run(U, Yo, 1.0)
        if (before, upto, o.exact_steps()) == (0, 1, 1):
            return Yo
    raise AssertionError("no outlier amplitude makes exactly step %d fail" % kf)


def set_form(monkeypatch, switch, form):
    """`switch` unset (form "default") or set to `form`, the other two unset"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    if form != "default":
        monkeypatch.setenv(switch, form)


def assert_form(g, switch, form, what=""):
    """the last run left out everything below `switch`'s level, and what the switch itself decides where it was unset"""
    f = g.last_run_form()
    i = SWITCHES.index(switch)
    assert all(f[k] for k in REPORTS[:i]), "%s: the run left out less than %s needs: %r" % (what, switch, f)
    assert f[REPORTS[i]] == (form == "default"), "%s: %s %s ran as %r" % (what, switch, form, f)
    return f


def both_forms(monkeypatch, switch, cfg, U, Y, want, what, steps):
    """a run of at least `steps` fused launches under both settings of `switch`: each equal to `want` (the oracle's snapshot), and the
    two to each other; returns both snapshots, with the exact redos appended"""
    got = {}
    for form in FORMS:
        set_form(monkeypatch, switch, form)
        g = _capi.FilterHandle(cfg)
        g.reset()
        rg = g.run(U, Y, 1.0, ll_steps=True)
        assert g.last_run_stats()["fused_launches"] >= steps, "the fused kernel did not run"
        f = assert_form(g, switch, form, what)
        got[form] = snapshot(g, rg)
        assert_same(got[form], want, "%s, %s %s against the oracle:" % (what, switch, form))
        got[form].append(("exact_redos", np.array([f["exact_redos"]], dtype=np.int64)))
    assert_same(got["default"], got["0"], what + ", the two forms:")
    return got
