"""The rounds of the fused timestep's output loop (kernels/resprop.hpp: LLPF_OUTPUT_ROUNDS, LLPF_OUTPUT_LOOP, LLPF_OUTPUT_LOOP_PF).

In the merged-schedule kernels the outputs of [c_end, M) are a loop of their own behind the others, and TileSum::flush issues two
atomics instead of one flat one.  Neither changes what an output computes, so everything here is bit for bit (uint64 views, no
tolerance) against the device-order oracle: ll_steps, the final particles and weights, the ancestors accessor and the resample count.
Sizes: a second tile of one particle, of 1025, and 69 tiles with a ragged last one; threshold 1 in both forms (weights stored or not)
and threshold 0.5 (rounds of both kinds in one run); a block that runs many rounds for one source; the Rao-Blackwellized and the
auxiliary forms."""
import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import oracle_binding as ob
from gpu_common import assert_state_equal, assert_steps_equal
from thr1_common import OWN_CAP, bits, oracle, peaked_workload, set_form, workload

pytestmark = pytest.mark.gpu

T = 12


def _assert_equal(rg, g, ro, o, what):
    assert bits(rg["ll"]) == bits(ro["ll"]), "%s: ll %r against %r" % (what, rg["ll"], ro["ll"])
    assert_steps_equal(rg["ll_steps"], ro["ll_steps"], what + " ll_steps", resamples=(g.resample_count(), o.resample_count()))
    assert g.resample_count() == o.resample_count(), what
    assert_state_equal(g.particles(), o.particles(), what + " particles")
    assert_state_equal(g.weights(), o.weights(), what + " weights()")
    assert np.array_equal(g.ancestors(), o.ancestors()), what + " ancestors()"


_reference = {}


def _c2_reference(N, thr):
    """the oracle's run of the C2 system, computed once per (N, threshold) and left unchanged"""
    if (N, thr) not in _reference:
        cfg, U, Y = workload(N, T, thr=thr)
        try:
            o = oracle(cfg, 16)
            ro = o.run(U, Y, 1.0, ll_steps=True)
        finally:
            ob.set_threads(1)
        _reference[(N, thr)] = (cfg, U, Y, o, ro)
    return _reference[(N, thr)]


@pytest.mark.parametrize("form,thr", [("default", 1.0), ("0", 1.0), ("default", 0.5)])
@pytest.mark.parametrize("N", [1025, 2049, 70001])
def test_merged_runs_equal_the_oracle(N, form, thr, monkeypatch):
    cfg, U, Y, o, ro = _c2_reference(N, thr)
    set_form(monkeypatch, "LLPF_SKIP_W", form)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True)
    assert g.last_run_stats()["fused_launches"] > 0, "the fused kernel did not run"
    assert g.last_run_form()["weights_not_stored"] == (thr == 1.0 and form == "default")
    if thr == 1.0:
        assert o.resample_count() == T
    else:
        assert 0 < o.resample_count() < T, "threshold %g does not give rounds of both kinds in %d steps" % (thr, T)
    _assert_equal(rg, g, ro, o, "N = %d, threshold %g, LLPF_SKIP_W %s" % (N, thr, form))


def test_one_source_owns_more_outputs_than_the_owner_table_holds(monkeypatch):
    """Measurement noise of standard deviation 1e-4 on the C2 system: the particle nearest the measurement takes most of the weight, its
    block runs many rounds, looks sources up by descent beyond the owner table and flushes its tile sums to the global ones (the first
    step gives all 5000 outputs to one source; one later step fails its bound test and is redone in exact form)."""
    N = 5000
    cfg, U, Y = peaked_workload(N, T)
    heaviest = []
    for k in range(1, T + 1):          # the ancestors of step k are what a run of k steps leaves
        o = oracle(cfg)
        ro = o.run(U[:k], Y[:k], 1.0, ll_steps=True)
        heaviest.append(int(np.bincount(o.ancestors()).max()))
    assert sum(h > OWN_CAP for h in heaviest) >= 3, "sources own at most %r outputs" % (heaviest,)
    monkeypatch.delenv("LLPF_SKIP_W", raising=False)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True)
    assert g.last_run_stats()["fused_launches"] > 0, "the fused kernel did not run"
    _assert_equal(rg, g, ro, o, "peaked weights")


@pytest.mark.parametrize("thr", [1.0, 0.5])
def test_rao_blackwellized_form(thr):
    """RBLin<2, 1, 1> (the reference's RBPF benchmark system), three tiles, the last of one particle"""
    import bench
    model, U, Y, kind, _, _ = bench.build_workload("rbpf", 2049, T)
    cfg = S.make_config(model, 2049, kind, S.RESAMPLE_SYSTEMATIC, thr, 1000, 0)
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True)
    assert g.last_run_stats()["fused_launches"] > 0, "the fused kernel did not run"
    assert o.resample_count() == T if thr == 1.0 else 0 < o.resample_count() < T
    _assert_equal(rg, g, ro, o, "RBLin<2, 1, 1>, threshold %g" % thr)


def test_auxiliary_form():
    """the auxiliary filter's loglik loop on the C2 system: its second half is the fused kernel with the look-ahead weights as priors"""
    cfg, U, Y = workload(2049, T, thr=0.1)
    o = oracle(cfg)
    ro = o.run_aux(U, Y, 1, ll_steps=True)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run_aux(U, Y, 1, ll_steps=True)
    assert g.last_run_stats()["fused_launches"] >= T - 1, "the fused kernel did not run in every auxiliary step"
    assert o.resample_count() > 0
    _assert_equal(rg, g, ro, o, "auxiliary filter")
