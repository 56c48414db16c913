"""Wave priority by progress in the rounds of the level-3 output loop (kernels/resprop.hpp: LLPF_ROUNDS_LEFT, LLPF_ROUND_PRIO;
shared/llpf_loop_prio.h; tests/test_loop_priority_map.py pins the map itself).

At the top of each round with an owner a wave sets its priority from the rounds it still has to do, counted down in a scalar register from
(umain - o + BLOCK - 1) / BLOCK of its first lane.  The priority decides only which wave of a SIMD issues next, so no bit may change; what
can go wrong is the count itself, which also feeds a branch: a wave whose lanes lie on either side of umain, a wave with no round at all
(first lane at or beyond umain, or first == last), a block of many rounds next to blocks of none.  So everything here is bit for bit
(uint64 views, no tolerance) against the device-order oracle: ll, the per-step log-likelihoods, final particles, weights, ancestors and
the resample count, in runs that last_run_form() reports as level 3.

Sizes: N = 1025 and 2049 (a last tile of one particle: blocks of a single partial round next to full ones), N = 70001 (69 tiles, ragged),
and the peaked workload, where one tile owns more outputs than the owner table holds and runs 9 and more rounds — far above the top of
either map — while tiles behind it own none (first == last).
Not here: a run whose last tile takes rounds of [c_end, M).  That needs a resampling offset within N * 2^-53 of 1, which no seed gives at
will (tests/test_stale_corner.py, tests/test_gpu_skip_ancestor_store.py); those rounds are the loop behind the rounds with an owner, they
set no priority, and they are entered at priority 0 because every wave's last round with an owner (rounds_left 1) sets 0.
Levels 0 to 2 keep one priority for the whole loop (their code is unchanged), so there is no case at threshold 0.5."""
import numpy as np
import pytest

from llpf_amd import _capi
import oracle_binding as ob
from thr1_common import OWN_CAP, TILE, assert_same, oracle, peaked_workload, set_form, snapshot, workload

pytestmark = pytest.mark.gpu

T = 12
BLOCK = 256         # threads of a block = outputs of a round (csrc/engine.hpp)

_reference = {}


def _c2_reference(N):
    """the oracle's run of the headline system at threshold 1, computed once per N and left unchanged"""
    if N not in _reference:
        cfg, U, Y = workload(N, T)
        try:
            o = oracle(cfg, 16 if N > 10000 else 1)
            ro = o.run(U, Y, 1.0, ll_steps=True)
        finally:
            ob.set_threads(1)
        assert o.resample_count() == T
        _reference[N] = (cfg, U, Y, snapshot(o, ro))
    return _reference[N]


def _level3_run(monkeypatch, cfg, U, Y, want, what):
    set_form(monkeypatch, "LLPF_LEAN", "default")
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True)
    assert g.last_run_stats()["fused_launches"] >= T, what + ": the fused kernel did not run"
    f = g.last_run_form()
    assert f["lean"] and f["ancestors_not_stored"] and f["weights_not_stored"], "%s: not a level-3 run: %r" % (what, f)
    assert_same(snapshot(g, rg), want, what + " against the oracle:")
    return f


@pytest.mark.parametrize("N", [1025, 2049, 70001])
def test_level3_runs_equal_the_oracle(N, monkeypatch):
    cfg, U, Y, want = _c2_reference(N)
    _level3_run(monkeypatch, cfg, U, Y, want, "N = %d" % N)


def test_one_block_of_many_rounds_among_blocks_of_none(monkeypatch):
    """Measurement noise of standard deviation 1e-4 on the headline system.  In some launch one tile owns more than OWN_CAP outputs (its
    waves count down from 9 rounds and more, the map is at its top for all but the last three) and some tile owns none (first == last:
    rounds_left 0, the loop is not entered and no priority is set)."""
    N = 8192
    cfg, U, Y = peaked_workload(N, T)
    most, empty = 0, 0
    for k in range(1, T):              # the ancestors of launch k - 1 (a level-3 one: not the run's last) are what a run of k steps leaves
        o = oracle(cfg)
        o.run(U[:k], Y[:k], 1.0)
        owned = np.bincount(np.asarray(o.ancestors()).astype(np.int64) // TILE, minlength=N // TILE)
        most = max(most, int(owned.max()))
        empty += int(owned.min() == 0)
    assert most > OWN_CAP and (most + BLOCK - 1) // BLOCK >= 9, "no tile runs 9 rounds: at most %d outputs" % most
    assert empty >= 1, "in no launch does a tile own no outputs (first == last)"
    o = oracle(cfg)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    f = _level3_run(monkeypatch, cfg, U, Y, snapshot(o, ro), "peaked weights")
    assert f["exact_redos"] == o.exact_steps()
