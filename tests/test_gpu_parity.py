"""GPU parity tests: the HIP engine, called through the C ABI, against the CPU oracle.

 * against the DEVICE-ORDER oracle everything that feeds the recursion must be bit-identical
   (particles, log-weights, log-likelihoods, ancestor indices), over whole trajectories;
 * against the REFERENCE-ORDER oracle (literal restatement) floating point must agree to the stated
   tolerances and ancestor indices may differ only at ulp-level ties (counted and bounded).
"""
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import models as M
import oracle_binding as ob
from gpu_common import (TOL_LL_STEP, TOL_LL_SUM, TOL_WE_REL, assert_state_equal, assert_steps_equal, cfg_of as _cfg,
                        compare_state as _compare_state)

pytestmark = pytest.mark.gpu

INDEP_WE_BOUND = 4.0      # exp-weights against np.longdouble, in units of u scale_i (see the threshold-0.1 test below)


def test_device_math_bit_identical_to_host():
    rng = np.random.default_rng(0)
    cases = {
        0: np.concatenate([rng.uniform(-745, 1, 200000), -10.0 ** rng.uniform(-300, 2, 50000), [0.0, -0.0, -745.1, -746.0]]),
        1: np.concatenate([rng.uniform(0, 1, 200000), 10.0 ** rng.uniform(-320, 300, 50000), [1.0, 0.5, 2.0]]),
        2: 10.0 ** rng.uniform(-25, 8, 100000),
        3: rng.uniform(0, 1, 200000),
        4: rng.uniform(0, 1, 200000),
        5: 10.0 ** rng.uniform(-300, 300, 100000),
        6: 10.0 ** rng.uniform(-300, 300, 100000) * rng.choice([-1.0, 1.0], 100000),
        7: rng.uniform(0, 1, 100000) * 10.0 ** rng.uniform(-5, 5, 100000),
        8: np.concatenate([rng.uniform(-760, 0, 200000), [0.0, -745.2, -746.0, -1e9, -np.inf]]),
        9: np.concatenate([(rng.integers(0, 2 ** 53, 200000) + 1) * 2.0 ** -53, [1.0, 2.0 ** -53, 0.75]]),
        10: rng.uniform(0, 1, 200000),
        11: rng.uniform(0, 1, 200000),
        12: np.concatenate([10.0 ** rng.uniform(-6, 6, 1000000), rng.uniform(1e-3, 200.0, 1000000), [1e-3, 1.0, 4.0, 2.0 ** -600, 2.0 ** 600]]),
    }
    for which, x in cases.items():
        host = ob.math_vec(which, x)
        dev = _capi.selftest_math(which, x)
        assert np.array_equal(host.view(np.uint64), dev.view(np.uint64)), "primitive %d differs host/device" % which


def test_wave_scans_written_in_assembly():
    """kernels/reduce.hpp: 64-bit inclusive wave scan and 128-bit wave sum with the DPP modifier on the add (inline asm whose
    hazards the compiler does not see): against numpy on random bit patterns, carries across every 32-bit boundary."""
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 64, size=64 * 300, dtype=np.uint64)
    bits[:64] = np.uint64(0xFFFFFFFFFFFFFFFF)          # every add carries
    bits[64:128] = np.uint64(0xFFFFFFFF)
    x = bits.view(np.float64)
    scan = np.cumsum(bits.reshape(-1, 64), axis=1, dtype=np.uint64).reshape(-1)           # wraps mod 2^64
    lo = _capi.selftest_math(13, x); hi = _capi.selftest_math(14, x)
    assert np.array_equal(lo.astype(np.uint64), scan & np.uint64(0xFFFFFFFF))
    assert np.array_equal(hi.astype(np.uint64), scan >> np.uint64(32))
    tot = [sum((int(b) | (((int(b) << 29) | (int(b) >> 35)) & (2 ** 64 - 1)) << 64) for b in grp) % 2 ** 128 for grp in bits.reshape(-1, 64)]
    for k in range(4):
        w = _capi.selftest_math(15 + k, x).astype(np.uint64).reshape(-1, 64)
        want = np.array([(t >> (32 * k)) & 0xFFFFFFFF for t in tot], dtype=np.uint64)
        assert np.array_equal(w[:, 0], want) and np.all(w == w[:, :1])


def test_device_normals_bit_identical_to_host():
    for nd in (1, 2, 3, 4):
        host = ob.normals(12345, 17, 1, nd, 100000)
        dev = _capi.selftest_normals(12345, 17, 1, nd, 100000)
        assert np.array_equal(host.view(np.uint64), dev.view(np.uint64))
    assert abs(dev.mean()) < 0.01 and abs(dev.var() - 1.0) < 0.01


@pytest.mark.parametrize("strategy", [S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED])
@pytest.mark.parametrize("thr", [0.1, 1.0])
def test_c1_trajectory_bit_exact_vs_device_order_oracle(strategy, thr):
    """BASELINE config C1 (N=500, T=200, nx=nu=ny=2): fused on-device loop == oracle, bit for bit."""
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, 200)
    cfg = _cfg(model, 500, strategy, thr)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    _compare_state(g, o)                       # constructor draw
    g.reset(); o.reset()
    _compare_state(g, o)
    rg = g.run(U, Y, 0.0, ll_steps=True, xmean=True)
    ro = o.run(U, Y, 0.0, ll_steps=True, xmean=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    assert rg["ll"] == ro["ll"]
    np.testing.assert_allclose(rg["xmean"], ro["xmean"], rtol=1e-12, atol=1e-13)
    _compare_state(g, o)
    assert g.resample_count() == o.resample_count()
    assert g.index() == o.index() == 201
    if thr == 1.0:
        assert g.resample_count() == 200


def test_step_by_step_equals_fused_loop_and_oracle():
    """correct!/predict! as separate calls (unfused kernels) give the same bits as the fused loop."""
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, 60)
    cfg = _cfg(model, 3000, thr=0.5)
    g1, g2 = _capi.FilterHandle(cfg), _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    for h in (g1, g2, o):
        h.reset()
    r1 = g1.run(U, Y, 0.0, ll_steps=True)
    lls = []
    for k in range(60):
        ll_g = g2.correct(U[k], Y[k], k * 1.0)
        ll_o = o.correct(U[k], Y[k], k * 1.0)
        assert ll_g == ll_o
        assert g2.ess() == o.ess()
        assert g2.shouldresample() == o.shouldresample()
        if k % 20 == 3:
            _compare_state(g2, o)
            assert np.array_equal(g2.weighted_mean(), g2.weighted_mean())
            np.testing.assert_allclose(g2.weighted_mean(), o.weighted_mean(), rtol=1e-12, atol=1e-13)
        g2.predict(U[k], k * 1.0)
        o.predict(U[k], k * 1.0)
        assert g2.last_resampled() == o.last_resampled()
        lls.append(ll_g)
    assert np.array_equal(np.array(lls).view(np.uint64), r1["ll_steps"].view(np.uint64))
    _compare_state(g1, o)
    _compare_state(g2, o)


def test_c1_vs_reference_order_oracle_tolerances():
    """Against the literal (reference-order) restatement: fp within tolerance, indices equal up to ulp ties."""
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, 200)
    cfg = _cfg(model, 500, thr=0.1)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 0.0, ll_steps=True)
    ro = o.run(U, Y, 0.0, ll_steps=True)
    assert np.max(np.abs(rg["ll_steps"] - ro["ll_steps"])) <= TOL_LL_STEP
    assert abs(rg["ll"] - ro["ll"]) <= TOL_LL_SUM
    assert g.resample_count() == o.resample_count()
    mism = int(np.sum(g.ancestors() != o.ancestors()))
    assert mism == 0, "ancestor mismatches vs reference-order oracle: %d" % mism
    np.testing.assert_allclose(g.expweights(), o.expweights(), rtol=TOL_WE_REL, atol=1e-300)


@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 2047, 2048, 2049, 5000])
def test_ragged_sizes(N):
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 25)
    cfg = _cfg(model, N, thr=1.0)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    _compare_state(g, o)


@pytest.mark.parametrize("thr,strategy", [(1.0, S.RESAMPLE_SYSTEMATIC), (0.5, S.RESAMPLE_STRATIFIED), (0.1, S.RESAMPLE_SYSTEMATIC)])
def test_many_tiles_trajectory_bit_exact(thr, strategy):
    """N = 150 001 (147 tiles, ragged last tile): cross-tile output ranges, accumulator slots, fused kernel."""
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 12)
    cfg = _cfg(model, 150001, strategy, thr)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 1.0, ll_steps=True)
    ro = o.run(U, Y, 1.0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    _compare_state(g, o)
    assert g.resample_count() == o.resample_count()
    # the unfused path (history requested) gives the same bits as the fused one
    g2 = _capi.FilterHandle(cfg)
    g2.reset()
    r2 = g2.run(U[:4], Y[:4], 1.0, history=True)
    g3 = _capi.FilterHandle(cfg)
    g3.reset()
    r3 = g3.run(U[:4], Y[:4], 1.0, ll_steps=True)
    assert r2["ll"] == r3["ll"]
    assert np.array_equal(g2.particles().view(np.uint64), g3.particles().view(np.uint64))
    assert np.array_equal(g2.ancestors(), g3.ancestors())


@pytest.mark.parametrize("kind", [S.COV_SCAL, S.COV_DIAG, S.COV_FULL])
def test_covariance_kinds(kind):
    rng = np.random.default_rng(5)
    nx, nu, ny = 3, 2, 2
    A = 0.8 * np.eye(nx) + 0.05 * rng.standard_normal((nx, nx))
    B = rng.standard_normal((nx, nu)); Cm = rng.standard_normal((ny, nx))

    def cov(n):
        if kind == S.COV_SCAL:
            return 0.3
        if kind == S.COV_DIAG:
            return rng.uniform(0.1, 0.5, n)
        Q = rng.standard_normal((n, n))
        return Q @ Q.T + 0.2 * np.eye(n)
    df = S.make_gaussian(0.01 * rng.standard_normal(nx), cov(nx), kind)
    dg = S.make_gaussian(0.01 * rng.standard_normal(ny), cov(ny), kind)
    d0 = S.make_gaussian(rng.standard_normal(nx), cov(nx), kind)
    model = S.make_lg_model(A, B, Cm, df, dg, d0)
    _, U, Y = M.simulate_lg(model, 40)
    cfg = _cfg(model, 4096, thr=0.5)
    g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE); r = ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
    for h in (g, o, r):
        h.reset()
    rg = g.run(U, Y, 0.0, ll_steps=True); ro = o.run(U, Y, 0.0, ll_steps=True); rr = r.run(U, Y, 0.0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    _compare_state(g, o)
    assert np.max(np.abs(rg["ll_steps"] - rr["ll_steps"])) <= TOL_LL_STEP


def test_quadtank_bit_exact_and_tolerance():
    """BASELINE config C3 model (quad-tank, RK4 x2) at oracle-feasible size, crossing the t>500 switch."""
    model = M.quadtank_model()
    U, Y = M.quadtank_data(40)
    cfg = _cfg(model, 6000, thr=0.5, kind=S.ADVANCED_PARTICLE_FILTER)
    g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE); r = ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
    for h in (g, o, r):
        h.reset()
    t0 = 485.0      # steps 485..524: the a1 switch at t > 500 is crossed inside rk4 stages
    rg = g.run(U, Y, t0, ll_steps=True); ro = o.run(U, Y, t0, ll_steps=True); rr = r.run(U, Y, t0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    _compare_state(g, o)
    assert np.max(np.abs(rg["ll_steps"] - rr["ll_steps"])) <= 1e-9
    assert g.resample_count() == o.resample_count() > 0


@pytest.mark.parametrize("form", ["1", "0"])
def test_quadtank_both_forms_of_the_balanced_timestep_give_the_oracles_bits(form, monkeypatch):
    """Dynamics once per surviving source (k_resample_fx + k_step<MARKS>, LLPF_SOURCE_FX=1) or once per output particle (=0): a schedule,
    not a result — both the device-order oracle's bits, at a size of several tiles, with a step that does not resample in between."""
    monkeypatch.setenv("LLPF_SOURCE_FX", form)
    model = M.quadtank_model()
    U, Y = M.quadtank_data(30)
    Y[11] = np.nan
    cfg = _cfg(model, 9001, thr=0.5, kind=S.ADVANCED_PARTICLE_FILTER, seed=31)
    g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 490.0, ll_steps=True); ro = o.run(U, Y, 490.0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    _compare_state(g, o)
    assert g.last_run_stats()["source_side_timesteps"] == (30 if form == "1" else 0)


@pytest.mark.parametrize("N", [1, 63, 511, 512, 513, 1025, 2049, 70001])
@pytest.mark.parametrize("strategy,thr,sig", [(S.RESAMPLE_SYSTEMATIC, 1.0, 0.01), (S.RESAMPLE_STRATIFIED, 0.5, 0.003), (S.RESAMPLE_SYSTEMATIC, 0.5, 0.3)])
def test_source_side_form_ragged_and_degenerate(N, strategy, thr, sig, monkeypatch):
    """The source-side form pinned (LLPF_SOURCE_FX=1) where its bookkeeping is exercised hardest: ragged last tiles, a filter of one
    partly filled tile, tile counts that do not divide by the step kernel's rounds, likelihoods so peaked that one source owns the outputs
    of many tiles (run-start marks at every 512-output boundary, written by the whole wave), likelihoods so flat that most steps do not
    resample (f for ALL particles), a missing measurement, both resamplers.  The device-order oracle's bits throughout."""
    monkeypatch.setenv("LLPF_SOURCE_FX", "1")
    model = M.quadtank_model()
    model.measurement_density = S.make_gaussian(np.zeros(2), np.full(2, sig ** 2))
    T = 10
    U, Y = M.quadtank_data(T, seed=5)
    Y[6] = np.nan
    cfg = _cfg(model, N, strategy=strategy, thr=thr, kind=S.ADVANCED_PARTICLE_FILTER, seed=900 + N % 97)
    g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 497.0, ll_steps=True); ro = o.run(U, Y, 497.0, ll_steps=True)      # crosses the t > 500 switch of the model
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    _compare_state(g, o)
    assert g.resample_count() == o.resample_count()
    assert g.last_run_stats()["source_side_timesteps"] == T
    # ... and the single-step verbs on top of the state the run left (they take the per-output form: same bits)
    g.correct(U[0], Y[0], 507.0); o.correct(U[0], Y[0], 507.0)
    g.predict(U[0], 507.0); o.predict(U[0], 507.0)
    _compare_state(g, o)


def test_quadtank_handle_chooses_the_form_by_the_survivor_fraction(monkeypatch):
    """A handle's first run takes the source-side form; from then on the form follows the survivor fraction of the run before (distinct
    ancestors per predict! / N: below 5 % source-side, above 8 % per output particle).  Healthy weights (wide measurement noise): the
    second run switches; peaked weights (BASELINE C3's 1 cm noise): it stays.  Either way the oracle's bits."""
    monkeypatch.delenv("LLPF_SOURCE_FX", raising=False)
    U, Y = M.quadtank_data(25)
    for sig, stays in ((0.5, False), (0.01, True)):
        model = M.quadtank_model()
        model.measurement_density = S.make_gaussian(np.zeros(2), np.full(2, sig ** 2))
        cfg = _cfg(model, 20000, thr=0.5, kind=S.ADVANCED_PARTICLE_FILTER, seed=32)
        g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
        for run in range(2):
            g.reset(); o.reset()
            rg = g.run(U, Y, 1.0, ll_steps=True); ro = o.run(U, Y, 1.0, ll_steps=True)
            assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64)), (sig, run)
            _compare_state(g, o)
            st = g.last_run_stats()
            assert st["source_side_timesteps"] == (25 if run == 0 or stays else 0), (sig, run, st)
            assert (st["survivor_fraction"] < 0.03) == stays, (sig, run, st)


def test_missing_measurement():
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, 30)
    Y[[3, 4, 17]] = np.nan
    cfg = _cfg(model, 1000, thr=0.3)
    g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 0.0, ll_steps=True); ro = o.run(U, Y, 0.0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    _compare_state(g, o)
    # and through the single-step entry point with y = None
    assert g.correct(U[0], None, 0.0) == o.correct(U[0], None, 0.0)


def test_history_outputs_match_oracle():
    """forward_trajectory's x / w / we history (reference src/filtering.jl:357-359)."""
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, 20)
    cfg = _cfg(model, 700, thr=0.5)
    g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 0.0, history=True); ro = o.run(U, Y, 0.0, history=True)
    for k in ("x", "w", "we"):
        assert np.array_equal(rg[k].view(np.uint64), ro[k].view(np.uint64)), k
    assert np.allclose(rg["we"].sum(axis=1), 1.0, atol=1e-12)


@pytest.mark.parametrize("strategy", [S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED])
@pytest.mark.parametrize("n,m", [(10, 10), (9, 9), (1000, 1000), (5000, 5000), (4097, 300), (300, 4097)])
def test_standalone_resample_matches_oracle(strategy, n, m):
    rng = np.random.default_rng(n + m)
    we = rng.exponential(size=n) ** 3
    we /= we.sum()
    U = rng.uniform(size=1 if strategy == S.RESAMPLE_SYSTEMATIC else m)
    jg = _capi.resample(strategy, we, U, m)
    jd, _ = ob.resample(strategy, we, U, m, ob.ORDER_DEVICE)
    jr, _ = ob.resample(strategy, we, U, m, ob.ORDER_REFERENCE)
    assert np.array_equal(jg, jd)
    assert np.sum(jg != jr) <= 1          # ulp-level ties only
    assert jg.min() >= 0 and jg.max() < n
    if m <= n:      # for M > N the reference's offset r = rand()*bins[end]/N can push the last thresholds past
        assert np.all(np.diff(jg) >= 0)   # bins[N]; those outputs are never written (stay 0 here)


def test_standalone_resample_degenerate_and_stale():
    # one particle holds all the weight
    we = np.zeros(3000); we[1234] = 1.0
    for strategy in (S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED):
        U = np.full(1 if strategy == S.RESAMPLE_SYSTEMATIC else 3000, 0.37)
        assert np.all(_capi.resample(strategy, we, U) == 1234)
    # thresholds that reach bins[N]: those outputs keep their input value (reference: j[i] not written)
    we = np.full(8, 0.125)
    U = np.array([1.0 - 2.0 ** -53])
    j0 = np.full(8, 77, dtype=np.int64)
    jg = _capi.resample(S.RESAMPLE_SYSTEMATIC, we, U, 8, j0)
    jd, _ = ob.resample(S.RESAMPLE_SYSTEMATIC, we, U, 8, ob.ORDER_DEVICE, j0)
    assert np.array_equal(jg, jd)


def test_standalone_logsumexp_matches_oracle():
    rng = np.random.default_rng(3)
    for n in (10, 1000, 4096, 100001):
        w = rng.standard_normal(n) * 30
        ll_g, w_g, we_g = _capi.logsumexp(w)
        ll_d, w_d, we_d, _ = ob.logsumexp(w, ob.ORDER_DEVICE)
        ll_r, w_r, we_r, _ = ob.logsumexp(w, ob.ORDER_REFERENCE)
        assert ll_g == ll_d
        assert np.array_equal(w_g.view(np.uint64), w_d.view(np.uint64))
        assert np.array_equal(we_g.view(np.uint64), we_d.view(np.uint64))
        assert abs(ll_g - ll_r) <= 1e-12 * max(1.0, abs(ll_r))
        np.testing.assert_allclose(we_g, we_r, rtol=TOL_WE_REL, atol=1e-300)
        assert abs(we_g.sum() - 1) < 1e-12


def test_degenerate_weights_are_reported():
    model = M.lg_test_model()
    cfg = _cfg(model, 100)
    g = _capi.FilterHandle(cfg)
    with pytest.raises(_capi.DegenerateWeights):
        g.set_weights(np.full(100, -np.inf))


def test_set_state_roundtrip_and_teacher_forced_step():
    """Install an arbitrary state on both sides, take one step, compare (also vs reference order)."""
    model = M.lg_test_model()
    rng = np.random.default_rng(11)
    N = 20000
    cfg = _cfg(model, N, thr=1.0)
    g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE); r = ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
    x = rng.standard_normal((N, 2)) * 3
    w = rng.standard_normal(N) * 4
    for h in (g, o, r):
        h.set_particles(x); h.set_weights(w)
    assert np.array_equal(g.particles(), x)
    assert np.array_equal(g.weights(), w)
    np.testing.assert_allclose(g.expweights(), r.expweights(), rtol=TOL_WE_REL)
    assert g.ess() == o.ess()
    assert abs(g.ess() - r.ess()) <= 1e-9 * r.ess()
    np.testing.assert_array_equal(g.bins(), o_bins_after_predict(o, cfg))
    u = np.array([0.3])
    g.predict(u, 0.0); r.predict(u, 0.0)
    mism = int(np.sum(g.ancestors() != r.ancestors()))
    assert mism <= 2, mism
    o2 = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    o2.set_particles(x); o2.set_weights(w); o2.predict(u, 0.0)
    _compare_state(g, o2)


@pytest.mark.parametrize("N", [4, 8192])
def test_shouldresample_at_an_exact_tie(N):
    """shouldresample (src/resample.jl:5-10) is `1/sum(abs2, we) < N * threshold`; the engine tests `stot^2 < (N * threshold) * sum(e^2)` on
    its fixed-point sums, without the division.  The two can only part at a tie — exercised here: half of the particles carry equal
    weight, the others none, threshold 0.5, so that ESS == N/2 == N * threshold EXACTLY (powers of two: no rounding anywhere).  `<` is
    false on all three sides, and the predict! that follows does not resample; one particle fewer in the support and all three resample."""
    model = M.lg_test_model()
    cfg = _cfg(model, N, thr=0.5, seed=41)
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, 2))
    u = np.array([0.2])
    for support, expect in ((N // 2, False), (N // 2 - 1, True), (N // 2 + 1, False)):
        w = np.full(N, -np.inf)
        w[:support] = -1.25
        g = _capi.FilterHandle(cfg); o = ob.OracleFilter(cfg, ob.ORDER_DEVICE); r = ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
        for h in (g, o, r):
            h.set_particles(x); h.set_weights(w)
        if support == N // 2:
            assert r.ess() == N / 2 == g.ess() == o.ess()
        assert bool(g.shouldresample()) == bool(o.shouldresample()) == bool(r.shouldresample()) == expect, support
        for h in (g, o, r):
            h.predict(u, 0.0)
        assert bool(g.last_resampled()) == bool(o.last_resampled()) == bool(r.last_resampled()) == expect, support      # (resample_count is per run)
        _compare_state(g, o)


def o_bins_after_predict(o, cfg):
    """The oracle materialises bins during the resampling predict!; the GPU getter returns the bins of the
    current weights.  Run a throw-away predict on the oracle copy to obtain them."""
    o.predict(np.array([0.0]), 0.0)
    return o.bins()


def test_bank_equals_individual_filters():
    """Filter k of a bank with seed s is bit-identical to a single filter with seed s + k."""
    svec = 10.0 ** np.linspace(-2, 0, 5)
    models = [M.lg_test_model(s) for s in svec]
    _, U, Y = M.simulate_lg(models[2], 50)
    N = 3000
    base = _cfg(models[0], N, thr=0.1, seed=100)
    bank = _capi.BankHandle(base, models)
    bank.reset()
    rb = bank.run(U, Y, 1.0, ll_steps=True)
    for k, mk in enumerate(models):
        cfg = _cfg(mk, N, thr=0.1, seed=100 + k)
        g = _capi.FilterHandle(cfg)
        g.reset()
        rg = g.run(U, Y, 1.0, ll_steps=True)
        assert rg["ll"] == rb["ll"][k]
        assert np.array_equal(rg["ll_steps"].view(np.uint64), rb["ll_steps"][:, k].copy().view(np.uint64))


def test_bank_at_the_c4_share_of_one_gpu():
    """BASELINE config C4 at the size of one GPU's share (128 filters x N = 1e5, the split schedule): three filters of the
    bank are bit-identical to single filters with seed s + k, every log-likelihood is finite, and a second run of the same
    shape (replayed from the captured graph) reproduces a fresh bank's numbers for its own noise."""
    F, N, T = 128, 100000, 40
    svec = 10.0 ** np.linspace(-2, 0, F)
    models = [M.lg_test_model(s) for s in svec]
    _, U, Y = M.simulate_lg(M.lg_test_model(0.1), T)
    bank = _capi.BankHandle(_cfg(models[0], N, thr=0.1, seed=900), models)
    bank.reset()
    rb = bank.run(U, Y, 1.0, ll_steps=True)
    assert np.all(np.isfinite(rb["ll"])) and bank.resample_count() > 0
    for k in (0, 61, 127):
        g = _capi.FilterHandle(_cfg(models[k], N, thr=0.1, seed=900 + k))
        g.reset()
        rg = g.run(U, Y, 1.0, ll_steps=True)
        assert np.array_equal(rg["ll_steps"].view(np.uint64), rb["ll_steps"][:, k].copy().view(np.uint64))
    bank.reset(); r2 = bank.run(U, Y, 1.0)
    bank.reset(); r3 = bank.run(U, Y, 1.0)
    fresh = _capi.BankHandle(_cfg(models[0], N, thr=0.1, seed=900), models)
    fresh.reset(); fresh.run(U, Y, 1.0); fresh.reset(); f2 = fresh.run(U, Y, 1.0); fresh.reset(); f3 = fresh.run(U, Y, 1.0)
    assert np.array_equal(r2["ll"], f2["ll"]) and np.array_equal(r3["ll"], f3["ll"])


def test_replica_bank_equals_bank_with_explicit_models():
    """llpf_bank_create(models = NULL): one descriptor replicated on the device gives the same filters as F explicit
    copies (quad-tank and linear-Gaussian models)."""
    qt = M.quadtank_model()
    U, Y = M.quadtank_data(30, seed=2)
    cfg = _cfg(qt, 3000, thr=0.5, kind=S.ADVANCED_PARTICLE_FILTER, seed=5)
    a = _capi.BankHandle(cfg, None, 3); b = _capi.BankHandle(cfg, [qt] * 3)
    a.reset(); b.reset()
    assert np.array_equal(a.run(U, Y, 1.0)["ll"], b.run(U, Y, 1.0)["ll"])
    lg = M.lg_test_model(0.1)
    _, U2, Y2 = M.simulate_lg(lg, 30)
    cfg2 = _cfg(lg, 800, thr=0.1, seed=5)
    a = _capi.BankHandle(cfg2, None, 700); b = _capi.BankHandle(cfg2, [lg] * 700)
    a.reset(); b.reset()
    assert np.array_equal(a.run(U2, Y2, 1.0)["ll"], b.run(U2, Y2, 1.0)["ll"])


@pytest.mark.parametrize("thr,N", [(0.1, 3000), (1.0, 700), (0.5, 100000)])
def test_bank_with_inputs_of_its_own_per_filter(thr, N):
    """llpf_bank_run_multi: filter k of the bank, run on (U[k], Y[k]), is bit-identical to a single filter with seed s + k
    run on the same data — log-likelihood per step and the weighted means (fused, balanced and split schedules by size);
    a missing measurement common to all filters; mismatching missing measurements are rejected."""
    F, T = 6, 40
    models = [M.lg_test_model(0.1) for _ in range(F)]
    data = [M.simulate_lg(models[0], T, seed=20 + k) for k in range(F)]
    U = np.stack([d[1] for d in data]); Y = np.stack([d[2] for d in data])
    Y[:, 9] = np.nan
    bank = _capi.BankHandle(_cfg(models[0], N, thr=thr, seed=300), models) if thr != 1.0 else _capi.BankHandle(_cfg(models[0], N, thr=thr, seed=300), None, F)
    bank.reset()
    rb = bank.run_multi(U, Y, 0.0, ll_steps=True, xmean=True)
    for k in range(F):
        g = _capi.FilterHandle(_cfg(models[k], N, thr=thr, seed=300 + k))
        g.reset()
        rg = g.run(U[k], Y[k], 0.0, ll_steps=True, xmean=True)
        assert rg["ll"] == rb["ll"][k]
        assert np.array_equal(rg["ll_steps"].view(np.uint64), rb["ll_steps"][:, k].copy().view(np.uint64))
        assert np.allclose(rg["xmean"], rb["xmean"][:, k], rtol=1e-11, atol=1e-13)
    Y[2, 5] = np.nan
    with pytest.raises(_capi.LLPFError):
        bank.run_multi(U, Y, 0.0)


def test_python_api_mirror_smoke():
    """The mirrored reference API (names of src/LowLevelParticleFilters.jl:3) end to end."""
    rng = np.random.default_rng(0)
    A = np.array([[0.97043, -0.097368], [0.09736, 0.970437]]); B = np.array([[0.1], [0.0]]); Cm = np.array([[0.0, 1.0]])
    df = llpf_amd.MvNormal(np.zeros(2), 0.01); dg = llpf_amd.MvNormal(np.zeros(1), 1.0); d0 = llpf_amd.MvNormal(np.array([1.0, 1.0]), 4.0)
    pf = llpf_amd.ParticleFilter(1000, llpf_amd.LinearDynamics(A, B), llpf_amd.LinearMeasurement(Cm), df, dg, d0, rng=3)
    assert not llpf_amd.shouldresample(pf)                          # test/runtests.jl:274
    x, u, y = llpf_amd.simulate(pf, 100, llpf_amd.MvNormal(np.zeros(1), 1.0), rng=rng)
    ll, _ = pf(u[0], y[0])
    assert np.isfinite(ll)
    sol = llpf_amd.forward_trajectory(pf, u, y)
    assert sol.x.shape == (100, 1000, 2) and sol.w.shape == (100, 1000) and np.isfinite(sol.ll)
    xh, ll2 = llpf_amd.mean_trajectory(pf, u, y)
    assert xh.shape == (100, 2)
    assert np.mean((xh - x) ** 2) < 5
    assert abs(llpf_amd.loglik(pf, u, y) - sol.ll) < 30
    assert llpf_amd.num_particles(pf) == 1000 and llpf_amd.particles(pf).shape == (1000, 2)
    j = llpf_amd.resample(pf)
    assert j.shape == (1000,) and j.min() >= 0 and j.max() < 1000
    assert abs(llpf_amd.effective_particles(np.full(10, 0.1)) - 10) < 1e-9


def test_full_size_properties_c2():
    """BASELINE config C2 at full size (N = 1e6, T = 1000): size-independent properties instead of an oracle run.
    Reproducibility (same key -> same bits), normalisation, sorted in-range ancestors, and the particle filter's
    log-likelihood against the closed-form Kalman value (Monte-Carlo error ~ sqrt(T/N))."""
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 1000, seed=1)
    N = 1000000
    lls = []
    for rep in range(2):
        g = _capi.FilterHandle(_cfg(model, N, thr=1.0, seed=2024))
        g.reset()
        r = g.run(U, Y, 1.0, ll_steps=True)
        lls.append(r["ll_steps"].copy())
        if rep == 0:
            we = g.expweights()
            assert abs(we.sum() - 1.0) < 1e-12 and np.all(we == we[0])        # last predict! resampled: uniform
            j = g.ancestors()
            assert j.min() >= 0 and j.max() < N and np.all(np.diff(j) >= 0)
            assert g.resample_count() == 1000 and g.index() == 1001
            x = g.particles()
            assert np.all(np.isfinite(x))
    assert np.array_equal(lls[0].view(np.uint64), lls[1].view(np.uint64))
    kf = ob.kalman_loglik(model, U, Y)
    assert abs(lls[0].sum() - kf) < 0.5, (lls[0].sum(), kf)
    # a different key gives a different (but statistically equivalent) answer
    g = _capi.FilterHandle(_cfg(model, N, thr=1.0, seed=2025))
    g.reset()
    ll2 = g.run(U, Y, 1.0)["ll"]
    assert ll2 != lls[0].sum() and abs(ll2 - kf) < 0.5


def test_full_size_properties_c3_quadtank():
    """BASELINE config C3 model at N = 1e6 (T = 300 across the t > 500 switch): finite, reproducible, every step
    resamples (ESS << N), weights normalised after a correct!."""
    model = M.quadtank_model()
    U, Y = M.quadtank_data(300)
    cfg = _cfg(model, 1000000, thr=0.5, kind=S.ADVANCED_PARTICLE_FILTER, seed=5)
    g = _capi.FilterHandle(cfg)
    g.reset()
    r1 = g.run(U, Y, 350.0, ll_steps=True, xmean=True)
    assert np.all(np.isfinite(r1["ll_steps"])) and np.all(np.isfinite(r1["xmean"]))
    assert g.resample_count() == 300
    ll = g.correct(U[0], Y[0], 650.0)
    we = g.expweights()
    assert np.isfinite(ll) and abs(we.sum() - 1.0) < 1e-12 and g.ess() < 0.05 * 1000000
    g2 = _capi.FilterHandle(cfg)
    g2.reset()
    r2 = g2.run(U, Y, 350.0, ll_steps=True)
    assert np.array_equal(r1["ll_steps"].view(np.uint64), r2["ll_steps"].view(np.uint64))
    # tracks the simulated tank levels: posterior mean of the measured states close to the measurements
    assert np.max(np.abs(r1["xmean"][50:, :2] - Y[50:])) < 0.1


def test_invalid_run_arguments():
    model = M.lg_test_model()
    g = _capi.FilterHandle(_cfg(model, 100))
    with pytest.raises(_capi.LLPFError):
        g.run(np.zeros((0, 1)), np.zeros((0, 1)), 0.0)           # empty trajectory
    n = S.MAX_DIM + 1
    with pytest.raises(ValueError):                              # above LLPF_MAX_DIM: refused by the binding ...
        S.make_lg_model(np.eye(n) * 0.5, None, np.eye(n)[:2], S.make_gaussian(np.zeros(2), 1.0), S.make_gaussian(np.zeros(2), 1.0), S.make_gaussian(np.zeros(2), 1.0))
    bad = M.lg_test_model()
    bad.nx = n
    with pytest.raises(_capi.LLPFError):                         # ... and by the library
        _capi.FilterHandle(_cfg(bad, 100))
    bad = M.lg_test_model()
    bad.nu = S.MAX_INPUTS + 1
    with pytest.raises(_capi.LLPFError):
        _capi.FilterHandle(_cfg(bad, 100))


@pytest.mark.parametrize("nx,ny,nu", [(5, 2, 1), (2, 6, 0), (8, 8, 2), (12, 4, 2), (16, 8, 2)])
def test_linear_gaussian_above_the_precompiled_dimensions(nx, ny, nu):
    """The reference is generic in the state dimension (src/PFtypes.jl:65-75); the library is precompiled for nx, ny <= 4 and
    compiles LinGauss<nx, ny> on demand above that (kernels/jit.hpp: jit_builtin_lg): whole trajectories with weighted means,
    single steps, the auxiliary filter and a bank are the device-order oracle's bit for bit, the reference order's within tolerance."""
    rng = np.random.default_rng(100 + nx + ny)
    A = 0.9 * np.linalg.qr(rng.standard_normal((nx, nx)))[0]
    B = 0.2 * rng.standard_normal((nx, nu)) if nu else None
    Cm = rng.standard_normal((ny, nx))
    model = S.make_lg_model(A, B, Cm, S.make_gaussian(np.zeros(nx), 0.05), S.make_gaussian(np.zeros(ny), 0.5 + rng.random(ny)),
                            S.make_gaussian(rng.standard_normal(nx), 1.0))
    _, U, Y = M.simulate_lg(model, 30, seed=4)
    Y[11] = np.nan
    cfg = _cfg(model, 3000, thr=0.5, seed=77)
    g, o, r = _capi.FilterHandle(cfg), ob.OracleFilter(cfg, ob.ORDER_DEVICE), ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
    for h in (g, o, r):
        h.reset()
    _compare_state(g, o)
    rg, ro, rr = (h.run(U, Y, 0.0, ll_steps=True, xmean=True) for h in (g, o, r))
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64)) and o.resample_count() > 2
    np.testing.assert_allclose(rg["xmean"], ro["xmean"], rtol=1e-12, atol=1e-13)       # a plain fp64 sum: order differs, never fed back
    _compare_state(g, o)
    assert np.max(np.abs(rg["ll_steps"] - rr["ll_steps"])) <= TOL_LL_STEP
    g.reset(); o.reset()
    for k in range(8):
        assert g.update(U[k] if nu else None, Y[k], float(k)) == o.update(U[k] if nu else None, Y[k], float(k))
    _compare_state(g, o)
    g.reset(); o.reset()
    if nx <= 8:
        assert np.array_equal(g.run_aux(U, Y, 1, ll_steps=True)["ll_steps"].view(np.uint64), o.run_aux(U, Y, 1, ll_steps=True)["ll_steps"].view(np.uint64))
    else:                                          # the auxiliary filter's second half is compiled for up to 8 states: refused above, loudly
        w_before, n_before = g.weights().copy(), g.index()
        with pytest.raises(_capi.LLPFError) as ei:
            g.run_aux(U, Y, 1, ll_steps=True)
        assert ei.value.code == _capi.ERR_ARG and "8 states" in str(ei.value)      # (round 6: before anything of the handle has moved)
        assert g.index() == n_before and np.array_equal(g.weights(), w_before)
        bk = _capi.BankHandle(cfg, [model, model])
        bk.reset()
        with pytest.raises(_capi.LLPFError) as ei:
            bk.run_aux(U, Y, 1)
        assert ei.value.code == _capi.ERR_ARG
        g.reset()
        np.testing.assert_allclose(g.weighted_cov(), np.cov(g.particles().T), rtol=1e-9, atol=1e-12)      # k_wcov<16>: uniform weights after reset!
    b = _capi.BankHandle(cfg, [model, model, model])
    b.reset()
    g2 = _capi.FilterHandle(_cfg(model, 3000, thr=0.5, seed=79)); g2.reset()
    assert np.array_equal(b.run(U, Y, 0.0, ll_steps=True)["ll_steps"][:, 2].copy().view(np.uint64), g2.run(U, Y, 0.0, ll_steps=True)["ll_steps"].view(np.uint64))


def test_bank_shares_of_a_sharded_sweep_match_single_bank():
    """The 8-GPU sharding of config C4 in miniature: banks built from round-robin shards of a sweep (what each rank
    runs; partition: llpf_mbank_partition) reproduce the log-likelihoods of the whole bank."""
    svec = 10.0 ** np.linspace(-2, 0, 12)
    models = [M.lg_test_model(s) for s in svec]
    _, U, Y = M.simulate_lg(models[5], 60)
    N = 5000

    class Bank:
        def __init__(self, ms, owned):
            # a shard keeps the global filter index in its Philox key: one single-filter bank per owned filter
            self.h = [_capi.BankHandle(_cfg(m, N, thr=0.1, seed=300 + k), [m]) for m, k in zip(ms, owned)]

        def reset(self):
            for h in self.h:
                h.reset()

        def run(self, U, Y, t0):
            return {"ll": np.array([h.run(U, Y, t0)["ll"][0] for h in self.h])}
    whole = _capi.BankHandle(_cfg(models[0], N, thr=0.1, seed=300), models)
    whole.reset()
    ll_whole = whole.run(U, Y, 1.0)["ll"]
    got = np.zeros(12)
    for rank in range(4):
        own = _capi.mbank_partition(12, rank, 4)
        b = Bank([models[k] for k in own], own)
        b.reset()
        got[own] = b.run(U, Y, 1.0)["ll"]
    assert np.array_equal(got, ll_whole)


@pytest.mark.parametrize("thr", [0.1, 1.0])
@pytest.mark.parametrize("N", [500, 30000])
def test_outlier_measurements_take_the_exact_form(thr, N):
    """Measurements far outside the particle cloud make sum exp(w - bound) < 2^-10: those steps are redone in the
    exact-max form (device) / evaluated in it (oracle); every bit still agrees, and so does the reference order."""
    model = M.lg_c1_model()
    _, U, Y = M.simulate_lg(model, 60)
    Y[0] += 25.0                      # already the first correct!
    Y[20] += 40.0
    Y[21] -= 35.0                     # two consecutive steps
    Y[45] += 12.0
    cfg = _cfg(model, N, thr=thr)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    r = ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
    for h in (g, o, r):
        h.reset()
    rg = g.run(U, Y, 0.0, ll_steps=True, xmean=True)
    ro = o.run(U, Y, 0.0, ll_steps=True, xmean=True)
    rr = r.run(U, Y, 0.0, ll_steps=True)
    assert o.exact_steps() >= 3
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    np.testing.assert_allclose(rg["xmean"], ro["xmean"], rtol=1e-11, atol=1e-12)
    _compare_state(g, o)
    assert np.max(np.abs(rg["ll_steps"] - rr["ll_steps"])) <= 1e-9 * np.max(np.abs(rr["ll_steps"]))
    # single-step entry points and the history path take the same decisions
    g2 = _capi.FilterHandle(cfg)
    g2.reset()
    lls = []
    for k in range(60):
        lls.append(g2.correct(U[k], Y[k], float(k)))
        g2.predict(U[k], float(k))
    assert np.array_equal(np.array(lls).view(np.uint64), rg["ll_steps"].view(np.uint64))
    g3 = _capi.FilterHandle(cfg)
    g3.reset()
    r3 = g3.run(U, Y, 0.0, history=True)
    assert r3["ll"] == rg["ll"]
    _compare_state(g3, o)


def test_heavy_particles_beyond_the_owner_table():
    """A very informative measurement leaves a handful of particles with all the weight: the tile that holds one of them
    produces far more outputs than the fused kernel's owner table holds (2048), so the rest of its range goes through the
    descent over the cumulative counts; tiles without surviving particles produce nothing.  Every bit must still agree."""
    base = M.lg_test_model()
    A = np.array(base.A[:4]).reshape(2, 2); B = np.array(base.B[:2]).reshape(2, 1); Cm = np.array([[0.0, 1.0]])
    model = S.make_lg_model(A, B, Cm, S.make_gaussian(np.zeros(2), 0.01), S.make_gaussian(np.zeros(1), np.full(1, 1e-16)),
                            S.make_gaussian(np.array([0.3, -0.5]), 4.0), 1.0)
    _, U, Y = M.simulate_lg(base, 12)
    cfg = _cfg(model, 40000, thr=1.0)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    most = 0
    for k in range(12):
        lg_, lo_ = g.correct(U[k], Y[k], float(k)), o.correct(U[k], Y[k], float(k))
        assert np.float64(lg_).view(np.uint64) == np.float64(lo_).view(np.uint64)
        g.predict(U[k], float(k)); o.predict(U[k], float(k))
        ja = g.ancestors()
        assert np.array_equal(ja, o.ancestors())
        most = max(most, int(np.bincount(ja).max()))
    assert most > 4096
    _compare_state(g, o)
    g2 = _capi.FilterHandle(cfg)
    g2.reset()
    r2 = g2.run(U, Y, 0.0, ll_steps=True)            # the fused run loop
    _compare_state(g2, o)


def test_bank_with_one_outlier_filter():
    """In a bank only the filter whose bound test fails is redone; the others are untouched by the redo."""
    models = [M.lg_test_model(s) for s in (0.05, 0.1, 0.2, 0.4)]
    _, U, Y = M.simulate_lg(models[1], 40)
    Y[17] += 9.0                      # an outlier that is much worse for the small-noise filters
    N = 4000
    bank = _capi.BankHandle(_cfg(models[0], N, thr=0.1, seed=900), models)
    bank.reset()
    rb = bank.run(U, Y, 1.0, ll_steps=True)
    n_exact = 0
    for k, mk in enumerate(models):
        cfg = _cfg(mk, N, thr=0.1, seed=900 + k)
        o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
        o.reset()
        ro = o.run(U, Y, 1.0, ll_steps=True)
        n_exact += o.exact_steps()
        assert np.array_equal(ro["ll_steps"].view(np.uint64), rb["ll_steps"][:, k].copy().view(np.uint64)), k
    assert n_exact >= 1


@pytest.mark.parametrize("schedule", ["merged", "split"])
def test_schedules_are_bit_identical(schedule, monkeypatch):
    """The exp-sums of new weights are formed either inside the weighting phase ("merged": one launch per step) or
    by a streaming normalise launch in the same bound-offset form ("split": chosen for large banks); both must give
    the oracle's bits, including a step whose bound test fails and is redone in exact-max form."""
    monkeypatch.setenv("LLPF_SCHEDULE", schedule)
    models = [M.lg_test_model(s) for s in (0.05, 0.1, 0.2, 0.4)]
    _, U, Y = M.simulate_lg(models[1], 40)
    Y[17] += 9.0
    N = 5000
    for strategy in (0, 1):
        cfg0 = _cfg(models[0], N, thr=0.5, seed=1200)
        cfg0.resampling_strategy = strategy
        bank = _capi.BankHandle(cfg0, models)
        bank.reset()
        rb = bank.run(U, Y, 1.0, ll_steps=True)
        n_exact = 0
        for k, mk in enumerate(models):
            cfg = _cfg(mk, N, thr=0.5, seed=1200 + k)
            cfg.resampling_strategy = strategy
            o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
            o.reset()
            ro = o.run(U, Y, 1.0, ll_steps=True)
            n_exact += o.exact_steps()
            assert np.array_equal(ro["ll_steps"].view(np.uint64), rb["ll_steps"][:, k].copy().view(np.uint64)), (strategy, k)
        assert n_exact >= 1
    # single filter, final state bit-exact
    cfg = _cfg(models[2], 3000, thr=1.0, seed=77)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U, Y, 0.0, ll_steps=True, xmean=True)
    ro = o.run(U, Y, 0.0, ll_steps=True, xmean=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    np.testing.assert_allclose(rg["xmean"], ro["xmean"], rtol=1e-9, atol=1e-11)   # output-only fp64 sum, never fed back
    _compare_state(g, o)


@pytest.mark.parametrize("thr", [0.1, 0.5, 1.0])
def test_split_schedule_forms_its_quanta_in_the_fused_kernel(thr, monkeypatch):
    """Split schedule in front of the fused kernel (banks and filters beyond 3 M particles; forced here on small ones): k_norm stores
    no quanta, the fused kernel's scan forms its tile's quanta from the weights against the offset its head has just read
    (ResArgs::lazy_q), and the run leaves the quanta of the current weights behind for the verbs that follow (k_requant).  Against
    the device-order oracle, bit for bit: the run, the state after it, a second predict! straight after the run (the consumer of
    the stored quanta: resample without a correct! in between), more single steps, and a second run; for one-tile filters (the
    redo of a failed bound test inside k_norm), ragged sizes and several tiles, with an outlier that makes a bound test fail; and
    the stored form (LLPF_LAZY_Q=0) gives the same bits, as do the nontemporal and the plain form of the 16-byte loop (LLPF_NT_ID)."""
    monkeypatch.setenv("LLPF_SCHEDULE", "split")
    model = M.lg_test_model(0.1)
    _, U, Y = M.simulate_lg(model, 40)
    Y[11] += 9.0
    for N in (700, 5000, 3 * 1024 + 5):
        cfg = _cfg(model, N, thr=thr, seed=31 + N)
        lls = {}
        for lazy in ("1", "0"):
            monkeypatch.setenv("LLPF_LAZY_Q", lazy)
            monkeypatch.setenv("LLPF_NT_ID", lazy)       # the nontemporal form of the steps that do not resample (default: from 7 M particles on) / the plain form
            g = _capi.FilterHandle(cfg)
            o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
            g.reset(); o.reset()
            rg = g.run(U[:20], Y[:20], 1.0, ll_steps=True)
            ro = o.run(U[:20], Y[:20], 1.0, ll_steps=True)
            assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64)), (N, lazy)
            _compare_state(g, o)
            assert g.ess() == o.ess()
            g.predict(U[20], 21.0); o.predict(U[20], 21.0)          # predict! twice in a row: resamples from the quanta the run left
            assert g.last_resampled() == o.last_resampled()
            _compare_state(g, o)
            for k in range(21, 26):
                assert g.correct(U[k], Y[k], 1.0 + k) == o.correct(U[k], Y[k], 1.0 + k)
                g.predict(U[k], 1.0 + k); o.predict(U[k], 1.0 + k)
            _compare_state(g, o)
            rg2 = g.run(U[26:39], Y[26:39], 27.0, ll_steps=True)      # 13 steps: an even number of weighting phases (the first run: odd — its step 0 keeps the stored form)
            ro2 = o.run(U[26:39], Y[26:39], 27.0, ll_steps=True)
            assert np.array_equal(rg2["ll_steps"].view(np.uint64), ro2["ll_steps"].view(np.uint64)), (N, lazy)
            _compare_state(g, o)
            lls[lazy] = np.concatenate([rg["ll_steps"], rg2["ll_steps"]])
        assert np.array_equal(lls["1"].view(np.uint64), lls["0"].view(np.uint64))


def test_split_schedule_runs_repeat_themselves_beyond_the_resident_set():
    """The split schedule without stored quanta reads, in a resampling step, weights that the same launch replaces (two weight buffers
    keep the two apart).  Its first version had ONE buffer and raced — invisibly while every block of a launch was resident (all tests
    up to 4e6 particles passed), with three different log-likelihoods in three runs at 1.6e7.  Here: the same run four times, on fresh
    handles and on one handle, at 1.6e7 and 4.2e6 particles (15 625 and 4 102 tiles against ~1 500 resident blocks), every output
    hashed (tools/dbg/lazy_repeat.py is the longer form)."""
    import hashlib
    model = M.lg_test_model(0.1)
    for N, T, thr in ((16_000_000, 10, 0.5), (4_200_000, 24, 0.3)):
        _, U, Y = M.simulate_lg(model, T)
        cfg = _cfg(model, N, thr=thr, seed=4242)
        one = _capi.FilterHandle(cfg)
        digests = set()
        for rep in range(4):
            h = _capi.FilterHandle(cfg) if rep % 2 == 0 else one
            h.seed(4242)
            h.reset()
            r = h.run(U, Y, 1.0, ll_steps=True)
            m = hashlib.sha256()
            for a in (r["ll_steps"], h.particles(), h.weights(), h.ancestors()):
                m.update(np.ascontiguousarray(a).tobytes())
            digests.add(m.hexdigest())
        assert len(digests) == 1, (N, len(digests))
        assert one.resample_count() >= 1


@pytest.mark.parametrize("schedule", ["merged", "split"])
def test_launches_larger_than_the_resident_set(schedule, monkeypatch):
    """More workgroups than the chip holds at once (~1000-2000): blocks of a launch that start after other blocks of
    the SAME launch have finished must still read the previous step's scalars (offset, systematic uniform, ancestor
    identity flag live in per-slot entries).  A bank of 48 x 65536 particles (3072 tiles) against the same filters
    run one at a time (64 tiles each, all resident), bit for bit; and one filter of 4.2e6 particles against the
    device-order oracle."""
    monkeypatch.setenv("LLPF_SCHEDULE", schedule)
    F, N, T = 48, 65536, 24
    models = [M.lg_test_model(0.05 + 0.01 * k) for k in range(F)]
    _, U, Y = M.simulate_lg(models[5], T)
    for thr in (1.0, 0.3):
        bank = _capi.BankHandle(_cfg(models[0], N, thr=thr, seed=4100), models)
        bank.reset()
        rb = bank.run(U, Y, 1.0, ll_steps=True)
        for k in (0, 1, 17, 30, 46, 47):
            g = _capi.FilterHandle(_cfg(models[k], N, thr=thr, seed=4100 + k))
            g.reset()
            rg = g.run(U, Y, 1.0, ll_steps=True)
            assert np.array_equal(rg["ll_steps"].view(np.uint64), rb["ll_steps"][:, k].copy().view(np.uint64)), (thr, k)
    N = 4200000
    cfg = _cfg(models[3], N, thr=0.5, seed=4200)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    g.reset(); o.reset()
    rg = g.run(U[:8], Y[:8], 1.0, ll_steps=True)
    ro = o.run(U[:8], Y[:8], 1.0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    assert g.resample_count() == o.resample_count() >= 1


@pytest.mark.parametrize("case", ["fused_1.6e7", "balanced", "stratified", "residual", "threshold_half", "quadtank_source_side", "aux"])
def test_beyond_1024_tiles_bit_identical_to_the_device_order_oracle(case, monkeypatch):
    """Above 1024 tiles (N > 1 048 576) the head of every resampling kernel takes its tile prefix from k_tile_prefix (group totals +
    the prefix inside the group, kernels/resample.hpp) instead of reading every tile sum: O(tiles) like the reference's cumsum
    (src/resample.jl:19-22) where it used to be O(tiles^2).  Whole trajectories against the device-order oracle, bit for bit: the fused
    kernel at N = 1.6e7 (15 625 tiles, 16 groups; the working set is beyond the 256 MB Infinity Cache), and at N = 1.1e6 + 77 (1075
    tiles: the second group holds 51 tiles, the last tile is ragged) the balanced form, stratified and residual resampling, a threshold
    that mixes resampling and non-resampling steps, the quad-tank's source-side form and the auxiliary filter."""
    strategy, thr, N, T, kind = S.RESAMPLE_SYSTEMATIC, 1.0, 1_100_077, 6, S.PARTICLE_FILTER
    model = M.lg_test_model()
    if case == "fused_1.6e7":
        N, T = 16_000_000, 8
    elif case == "balanced":
        monkeypatch.setenv("LLPF_UNFUSED", "1")
    elif case == "stratified":
        strategy = S.RESAMPLE_STRATIFIED
    elif case == "residual":
        strategy = S.RESAMPLE_RESIDUAL
    elif case == "threshold_half":
        thr, T = 0.5, 10
    elif case == "quadtank_source_side":
        model, kind, thr, T = M.quadtank_model(), S.ADVANCED_PARTICLE_FILTER, 0.5, 5
    if case == "quadtank_source_side":
        U, Y = M.quadtank_data(T, seed=2)
    else:
        _, U, Y = M.simulate_lg(model, T, seed=1)
    cfg = S.make_config(model, N, kind, strategy, thr, 321, 0)
    ob.set_threads(16)
    try:
        o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
        o.reset()
        ro = o.run_aux(U, Y, 0, ll_steps=True) if case == "aux" else o.run(U, Y, 1.0, ll_steps=True)
    finally:
        ob.set_threads(1)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = g.run_aux(U, Y, 0, ll_steps=True) if case == "aux" else g.run(U, Y, 1.0, ll_steps=True)
    assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64))
    assert g.resample_count() == o.resample_count() >= 1
    _compare_state(g, o)
    if case == "fused_1.6e7":
        # the captured run loop (second and third run of the shape) gives what the enqueued one gave
        g.seed(321); g.reset(); r2 = g.run(U, Y, 1.0, ll_steps=True)
        g.seed(321); g.reset(); r3 = g.run(U, Y, 1.0, ll_steps=True)
        assert np.array_equal(r2["ll_steps"].view(np.uint64), r3["ll_steps"].view(np.uint64))


def test_near_maximum_particle_count():
    """3e8 particles (2.4 GB per state plane: byte offsets above 2^31, 292 969 tiles): the 32-bit offset addressing,
    the tile-sum prefix over ~3e5 tiles and the 63-bit quanta total; checked through size-independent properties
    (the per-step log-likelihood estimates the same quantity as a 1e6-particle run, to Monte-Carlo accuracy)."""
    model = M.lg_test_model(0.1)
    _, U, Y = M.simulate_lg(model, 4, seed=1)
    big = _capi.FilterHandle(_cfg(model, 300_000_000, thr=1.0, seed=11))
    big.reset()
    rb = big.run(U, Y, 1.0, ll_steps=True, xmean=True)
    small = _capi.FilterHandle(_cfg(model, 1_000_000, thr=1.0, seed=12))
    small.reset()
    rs = small.run(U, Y, 1.0, ll_steps=True, xmean=True)
    assert np.all(np.isfinite(rb["ll_steps"])) and np.all(np.isfinite(rb["xmean"]))
    assert np.max(np.abs(rb["ll_steps"] - rs["ll_steps"])) < 0.02
    assert np.max(np.abs(rb["xmean"] - rs["xmean"])) < 0.02
    assert big.resample_count() == 4
    assert abs(big.ess() - 3e8) < 1.0          # after the last resampling predict! the weights are uniform
    # linear in N (round 6: the head's tile prefix is O(tiles)): 72 B per particle-step at no less than a quarter of the HBM peak;
    # with every block reading all 292 969 tile sums a timestep took several times this bound
    big.seed(11); big.reset()
    big.run(U, Y, 1.0)
    us_per_step = 1e3 * big.last_run_ms() / 4
    print("N = 3e8: %.0f us per timestep, %.3f of the HBM roofline" % (us_per_step, 3e8 * 72 / (us_per_step * 1e-6) / 8e12))
    assert us_per_step < 3e8 * 72 / 2.0e12 * 1e6


def test_c_client_of_the_abi():
    """examples/loglik_c2.c: the boundary driven from plain C (include/llpf.h, no Python in the process): runs, and its
    log-likelihood estimate does not depend on the particle count beyond Monte-Carlo error."""
    import json, os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import shutil, tempfile
    if shutil.which("gcc") is None:
        pytest.skip("no C compiler on this box")
    libdir = os.path.join(root, "lowlevelparticlefilters.jl_amd")
    exe = os.path.join(tempfile.mkdtemp(), "loglik_c2")          # always against the current include/llpf.h (struct_size guard)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-I", os.path.join(root, "include"), os.path.join(root, "examples", "loglik_c2.c"),
                           "-L", libdir, "-lllpf_hip", "-lm", "-o", exe])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(root, "lowlevelparticlefilters.jl_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    outs = []
    for n in (20000, 200000):
        r = subprocess.run([exe, str(n), "300", "7"], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert all(np.isfinite(o["loglik"]) for o in outs)
    assert abs(outs[0]["loglik"] - outs[1]["loglik"]) < 3.0
    assert outs[1]["particle_steps_per_s"] > 1e9


def test_error_paths_of_the_newer_entry_points():
    """Invalid uses are rejected with LLPF_ERR_ARG and a message (no exception crosses the ABI, nothing is computed):
    the Rao-Blackwellized model with the auxiliary verbs, smooth with M > N or an RB model,
    RB model shapes the kernels do not cover, a quad-tank model with eps = 0."""
    model = M.lg_test_model(0.1)
    _, U, Y = M.simulate_lg(model, 10)
    g2 = _capi.FilterHandle(_cfg(model, 500))
    g2.reset()
    r = g2.run(U, Y, 0.0, history=True)
    with pytest.raises(_capi.LLPFError):
        g2.smooth(501, U, r["x"], r["w"], r["we"])
    with pytest.raises(_capi.LLPFError):
        g2.run_aux(U, Y, 2)
    gs = S.make_gaussian
    with pytest.raises(ValueError):
        S.make_rb_model(np.eye(3), None, None, np.eye(2), None, np.zeros((1, 3)), None, gs(np.zeros(3), 1.0), np.eye(2),
                        gs(np.zeros(1), 1.0), gs(np.zeros(3), 1.0), gs(np.zeros(2), 1.0))       # nxn + nxl > 4
    rb2 = S.make_rb_model(np.eye(2), None, np.ones((2, 1)), [[0.9]], None, np.ones((1, 2)), [[1.0]], gs(np.zeros(2), 0.1), [[0.1]],
                          gs(np.zeros(1), 1.0), gs(np.zeros(2), 1.0), gs(np.zeros(1), 1.0))      # An != 0 with two nonlinear states
    with pytest.raises(_capi.LLPFError):
        _capi.FilterHandle(_cfg(rb2, 100))
    qt = M.quadtank_model()
    qt.qt[S.QT_NAMES.index("eps")] = 0.0
    with pytest.raises(_capi.LLPFError):
        _capi.FilterHandle(_cfg(qt, 100, kind=S.ADVANCED_PARTICLE_FILTER))


@pytest.mark.parametrize("thr", [0.1, 1.0])
def test_repeated_runs_replay_a_captured_graph(thr):
    """loglik called again and again with the same shapes (an optimisation / MCMC loop): the second call captures the
    run loop into a hipGraph, later calls replay it.  Every pass must equal the oracle's pass (fresh noise each time:
    the Philox step base moves, the captured relative steps do not), including a pass whose outlier measurement makes
    a bound test fail in the middle of a replay, and a change of data with the same shape."""
    model = M.lg_test_model(0.1)
    _, U, Y = M.simulate_lg(model, 50, seed=9)
    Yo = Y.copy()
    Yo[31] += 12.0
    cfg = _cfg(model, 3000, thr=thr, seed=17)
    g = _capi.FilterHandle(cfg)
    o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
    n_exact = 0
    for p, Yp in enumerate([Y, Y, Y, Yo, Yo, Y, Yo]):
        g.reset(); o.reset()
        rg = g.run(U, Yp, 1.0, ll_steps=True)
        e0 = o.exact_steps()
        ro = o.run(U, Yp, 1.0, ll_steps=True)
        n_exact += o.exact_steps() - e0
        assert np.array_equal(rg["ll_steps"].view(np.uint64), ro["ll_steps"].view(np.uint64)), p
        _compare_state(g, o)
    assert n_exact >= 3


# ---- parity evidence at the BASELINE sizes themselves (oracle with OpenMP over the per-particle loops) -----------------
# Every full-length case is built as bench.py builds the run it times (bench.build_workload, seed 1000, t_index0 1.0), so the suite
# holds that very run to the device-order oracle, every step.  The oracle runs on 16 threads: its bits do not depend on them
# (tests/test_oracle_threads.py).
def _bench_case(name, N, T, thr=None):
    import bench
    model, U, Y, kind, thr0, _ = bench.build_workload(name, N, T)
    return S.make_config(model, N, kind, S.RESAMPLE_SYSTEMATIC, thr0 if thr is None else thr, 1000, 0), U, Y


def _oracle_run(cfg, U, Y, aux=False):
    ob.set_threads(16)
    try:
        o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
        o.reset()
        ro = o.run_aux(U, Y, 1, ll_steps=True) if aux else o.run(U, Y, 1.0, ll_steps=True)
    finally:
        ob.set_threads(1)
    return o, ro


def _engine_run(g, U, Y, aux=False, **kw):
    return g.run_aux(U, Y, 1, ll_steps=True, **kw) if aux else g.run(U, Y, 1.0, ll_steps=True, **kw)


def _compare_full_run(g, rg, o, ro, rb=False):
    """every step's log-likelihood, the resample count, the final particles, log-weights, exp-weights and ancestors (and, for the RB
    kinds, every particle's Kalman mean and covariance) bit for bit; a mismatch names its first timestep"""
    assert_steps_equal(rg["ll_steps"], ro["ll_steps"], resamples=(g.resample_count(), o.resample_count()))
    assert g.resample_count() == o.resample_count()
    _compare_state(g, o)
    if rb:
        xg, Rg = g.rb_linear_state()
        xo, Ro = o.rb_linear_state()
        assert_state_equal(xg, xo, "Kalman means")
        assert_state_equal(Rg, Ro, "Kalman covariances")


def _replays_repeat_the_first_run(g, U, Y, o, ro):
    """seed(1000) and two reset()s bring the handle back to where its first run started (the constructor draws with reset index 0,
    the first reset() with 1); the second run of the shape captures the run loop into a hipGraph, the third replays it.  Both must
    give the first run's bits, which are the oracle's."""
    for p in (2, 3):
        g.seed(1000); g.reset(); g.reset()
        rp = _engine_run(g, U, Y)
        assert_steps_equal(rp["ll_steps"], ro["ll_steps"], "ll_steps of run %d" % p, resamples=(g.resample_count(), o.resample_count()))
        _compare_state(g, o)


def _c2_full_length(thr):
    cfg, U, Y = _bench_case("lg", 1000000, 1000, thr)
    o, ro = _oracle_run(cfg, U, Y)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = _engine_run(g, U, Y)
    _compare_full_run(g, rg, o, ro)
    return g, U, Y, o, ro


def test_c2_full_length_bit_identical_to_the_device_order_oracle():
    """bench.py's headline workload, C2 `lg`: the 2-D linear-Gaussian ParticleFilter, N = 1e6, T = 1000, systematic resampling at
    every step (threshold 1.0).  Compared with the device-order oracle bit for bit: all 1000 per-step log-likelihoods, the resample
    count, the final particles, log-weights, exp-weights and ancestors."""
    g, _, _, _, _ = _c2_full_length(1.0)
    assert g.resample_count() == 1000


def test_c2_threshold_0_1_full_length_and_graph_replays_bit_identical_to_the_device_order_oracle():
    """C2 `lg` at `bench.py --threshold 0.1` (the reference's default: resampling and non-resampling steps mixed), N = 1e6,
    T = 1000.  Compared with the device-order oracle bit for bit: all 1000 per-step log-likelihoods, the resample count, the final
    particles, log-weights, exp-weights and ancestors; then the second and third run of the handle (hipGraph capture, then replay)
    are held to the same bits."""
    g, U, Y, o, ro = _c2_full_length(0.1)
    assert 0 < g.resample_count() < 1000
    _replays_repeat_the_first_run(g, U, Y, o, ro)


def test_c2_full_size_ancestor_mismatches_against_the_reference_order():
    """the count SURVEY 8(d) asks for: the engine's exact fixed-point bins against the reference's serial fp64 cumulative sum at
    N = 1e6, 50 teacher-forced resampling steps.  A threshold within ~1e-13 of a bin edge may fall on the other side: at most a
    handful of the 5e7 ancestor decisions differ, and every output whose ancestor agrees has bit-identical particles.  Every
    correct! is also held to an np.longdouble evaluation of the same step (gpu_common.independent_correct)."""
    from gpu_common import teacher_forced_ancestor_mismatches
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 50, seed=1)
    r = teacher_forced_ancestor_mismatches(_cfg(model, 1000000, thr=1.0, seed=1000), U, Y, 50, threads=16, independent=True)
    print("teacher-forced ancestor mismatches at N = 1e6:", r)
    assert r["resampling_steps"] == 50
    assert r["mismatches_total"] <= 50 and r["mismatches_per_step_max"] <= 8, r
    assert r["particles_equal_on_matching_ancestors"]
    # the stated fp64 tolerance at the BASELINE size: every correct! from the reference order's own state
    assert r["correct_steps"] == 50 and r["ll_abs_err_max"] <= 1e-10 and r["expweights_rel_err_max"] <= 1e-12, r
    assert r["indep_ll_abs_err_max"] <= 1e-12 and r["indep_expweights_bound_ratio_max"] <= INDEP_WE_BOUND, r


def test_c2_full_size_correct_on_non_uniform_weights_against_independent_arithmetic():
    """correct! at N = 1e6 on the non-uniform weights of threshold 0.1 (bench.py --threshold 0.1: C2 `lg`, seed 1000), 100
    teacher-forced steps: lazy normalisation, the analytic-bound fast form and the ESS from fix96 sums, against (a) the reference
    order (libm exp, pairwise sums, serial cumsum: |dll| <= 1e-10, exp-weights rel <= 1e-12) and (b) an np.longdouble evaluation of
    the same step from the same fp64 particles and log-weights (gpu_common.independent_correct), which shares no arithmetic with the
    engine: |dll| <= 1e-12, and every exp-weight within INDEP_WE_BOUND u scale_i of the long-double value (u = 2^-53).

    The bound: log we_i = w_i + logpdf_i - ll is formed in fp64 from terms of size |w_i|, |logpdf_i|, |ll|, |log we_i|, each carrying
    one or two roundings, and logpdf_i carries the cancellation in v = y - C x_i, worth |v_k| / Sigma_kk times v_k's rounding
    (|y_k| + (|C| |x_i|)_k + |mu_k|) u; exp, the product by 1 / S and the rounding of the exact fix96 sum S add ~3 u.  scale_i (see
    independent_correct) sums those sizes, so the relative error of we_i is c u scale_i with c of a few; INDEP_WE_BOUND = 4 holds
    the count of roundings to that."""
    from gpu_common import teacher_forced_ancestor_mismatches
    cfg, U, Y = _bench_case("lg", 1000000, 100, 0.1)
    r = teacher_forced_ancestor_mismatches(cfg, U, Y, 100, threads=16, independent=True)
    print("teacher-forced correct! at threshold 0.1, N = 1e6:", r)
    assert r["correct_steps"] == 100 and 0 < r["resampling_steps"] < 100, r
    assert r["ll_abs_err_max"] <= 1e-10 and r["expweights_rel_err_max"] <= 1e-12, r
    assert r["indep_ll_abs_err_max"] <= 1e-12 and r["indep_expweights_bound_ratio_max"] <= INDEP_WE_BOUND, r
    assert r["mismatches_total"] <= 50 and r["particles_equal_on_matching_ancestors"], r


def test_c4_share_bank_against_the_oracle():
    """bench.py's C4 workload, one GPU's share: 128 linear-Gaussian filters x N = 1e5, noise levels 10 ** linspace(-2, 0, 128),
    data simulate_lg(lg_test_model(0.1), 1000, seed=1), T = 1000, threshold 0.1, seed 5 (filter k keys its streams with 5 + k), run
    through a BankHandle (test_one_shard_is_the_plain_bank ties it to bench.py's MBankHandle).  The split schedule inside a bank over
    a long run: per-step log-likelihoods bit-identical to the device-order ORACLE (not to single HIP filters), all 1000 steps of
    filters 0, 63, 64 and 127 and the first 100 steps of all 128."""
    F, N, T, T_all = 128, 100000, 1000, 100
    svec = 10.0 ** np.linspace(-2, 0, F)
    models = [M.lg_test_model(s) for s in svec]
    _, U, Y = M.simulate_lg(M.lg_test_model(0.1), T, seed=1)
    bank = _capi.BankHandle(_cfg(models[0], N, thr=0.1, seed=5), models)
    bank.reset()
    rb = bank.run(U, Y, 1.0, ll_steps=True)
    assert np.all(np.isfinite(rb["ll_steps"]))
    for k in range(F):
        full = k in (0, 63, 64, 127)
        n = T if full else T_all
        o, ro = _oracle_run(_cfg(models[k], N, thr=0.1, seed=5 + k), U[:n], Y[:n])
        assert_steps_equal(rb["ll_steps"][:n, k], ro["ll_steps"], "ll_steps of filter %d" % k)


def test_c3_full_size_full_length():
    """bench.py's C3 workload as specified: quad-tank AdvancedParticleFilter (RK4 x 2), N = 1e6, T = 2000 (through the t > 500
    switch), threshold 0.5, seed 1000, t_index0 1.0.  All 2000 per-step log-likelihoods, the resample count, the final particles,
    log-weights, exp-weights and ancestors are the device-order oracle's bit for bit; the run is finite, resamples at every step and
    tracks the measured levels."""
    cfg, U, Y = _bench_case("quadtank", 1000000, 2000)
    g = _capi.FilterHandle(cfg)
    g.reset()
    r = _engine_run(g, U, Y, xmean=True)
    assert np.all(np.isfinite(r["ll_steps"])) and np.all(np.isfinite(r["xmean"]))
    assert g.resample_count() == 2000 and g.index() == 2001
    assert np.max(np.abs(r["xmean"][50:, :2] - Y[50:])) < 0.1
    o, ro = _oracle_run(cfg, U, Y)
    _compare_full_run(g, r, o, ro)


def test_c5_rbpf_full_full_length():
    """bench.py's C5 workload: the RBPF with per-particle 8x8 covariance (quad-tank levels + 8 linear states, state-dependent
    coupling), N = 2e5, T = 1000, threshold 0.1, seed 1000.  All per-step log-likelihoods, the resample count, the final particles
    ([xn; xl]), log-weights, exp-weights, ancestors and every particle's Kalman mean and covariance, bit for bit the device-order
    oracle's."""
    cfg, U, Y = _bench_case("rbpf_full", 200000, 1000)
    o, ro = _oracle_run(cfg, U, Y)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = _engine_run(g, U, Y)
    _compare_full_run(g, rg, o, ro, rb=True)
    assert g.resample_count() > 0


@pytest.mark.parametrize("thr", [1.0, 0.1])
def test_c2_beyond_the_infinity_cache_full_length(thr):
    """bench.py's C2 system at N = 1.6e7 (its `other_configs` run: a 1 GB working set, beyond the 256 MB Infinity Cache), T = 100,
    seed 1000: threshold 1.0 takes the fused kernel's nontemporal 16-byte loop; threshold 0.1 the split schedule with lazy quanta at
    its natural size, with blocks that are not all co-resident.  All 100 per-step log-likelihoods, the resample count and the final
    particles, log-weights, exp-weights and ancestors are the device-order oracle's bit for bit.  At threshold 0.1 the second and
    third run of the handle (hipGraph capture, then replay) are held to the same bits."""
    cfg, U, Y = _bench_case("lg", 16000000, 100, thr)
    o, ro = _oracle_run(cfg, U, Y)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = _engine_run(g, U, Y)
    _compare_full_run(g, rg, o, ro)
    if thr == 0.1:
        assert 0 < g.resample_count() < 100
        _replays_repeat_the_first_run(g, U, Y, o, ro)


@pytest.mark.parametrize("name", ["aux", "rbpf"])
def test_aux_and_rbpf_full_length(name):
    """bench.py's `aux` workload (the AuxiliaryParticleFilter's loglik loop on the C2 system, run_aux mode 1) and its `rbpf` workload
    (the RBPF of the reference's test/test_rbpf.jl system, constant coupling, threshold 0.1), N = 1e6, T = 1000, seed 1000.  All
    per-step log-likelihoods, the resample count, the final particles, log-weights, exp-weights and ancestors bit for bit the
    device-order oracle's."""
    aux = name == "aux"
    cfg, U, Y = _bench_case(name, 1000000, 1000)
    o, ro = _oracle_run(cfg, U, Y, aux)
    g = _capi.FilterHandle(cfg)
    g.reset()
    rg = _engine_run(g, U, Y, aux)
    _compare_full_run(g, rg, o, ro)
    assert g.resample_count() > 0


def test_weighted_cov_on_the_device():
    """weighted_cov (reference src/filtering.jl:571-581: StatsBase's corrected covariance under probability weights) of the current state as
    an accessor and per step as a run output: against numpy on the particles / exp-weights the engine returns, and the run output against
    the accessor; the xcov output does not change the run (same ll, particles, ancestors as a run without it)."""
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 25)
    cfg = S.make_config(model, 5000, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 21, 0)
    g, g2 = _capi.FilterHandle(cfg), _capi.FilterHandle(cfg)
    g.reset(); g2.reset()

    def ref_cov(x, we):
        s = we.sum()
        mu = (x * we[:, None]).sum(axis=0) / s
        d = x - mu
        n = np.count_nonzero(we)
        return (d * we[:, None]).T @ d * (n / ((n - 1) * s))

    np.testing.assert_allclose(g.weighted_cov(), ref_cov(g.particles(), g.expweights()), rtol=1e-11, atol=1e-15)      # uniform weights after reset!
    r = g.run(U, Y, 0.0, ll_steps=True, history=True, xcov=True)
    r2 = g2.run(U, Y, 0.0, ll_steps=True)
    assert np.array_equal(r["ll_steps"].view(np.uint64), r2["ll_steps"].view(np.uint64)) and np.array_equal(g.ancestors(), g2.ancestors())
    for k in range(25):
        np.testing.assert_allclose(r["xcov"][k], ref_cov(r["x"][k], r["we"][k]), rtol=1e-11, atol=1e-15)
    g.correct(U[0], Y[0], 0.0)
    np.testing.assert_allclose(g.weighted_cov(), ref_cov(g.particles(), g.expweights()), rtol=1e-11, atol=1e-15)
    c1 = g.weighted_cov()
    assert np.array_equal(c1, g.weighted_cov()) and np.array_equal(c1, c1.T)         # fixed order: the same bits again


def test_run_graphs_with_mean_and_covariance_outputs_survive_a_growing_run_length():
    """Round-4 advisor finding: the captured run loop was keyed on the xmean buffer only; a later, longer run reallocates the xcov buffer
    while the others keep their addresses, and the short run's graph then replayed launches against the freed pointer.  Short runs
    (captured the second time), a long run, the short run again: the same outputs every time."""
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 400)
    cfg = S.make_config(model, 3000, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 33, 0)
    g = _capi.FilterHandle(cfg)
    g.seed(5); g.reset()
    first = g.run(U[:400], Y[:400], 0.0, xmean=True)             # xmean (and U, Y, ll) buffers sized for the longest run up front
    short = []
    for _ in range(3):
        g.seed(5); g.reset()
        short.append(g.run(U[:20], Y[:20], 0.0, xmean=True, xcov=True))
    g.seed(5); g.reset()
    long_ = g.run(U[:400], Y[:400], 0.0, xmean=True, xcov=True)   # xcov grows: 20 -> 400 steps
    g.seed(5); g.reset()
    again = g.run(U[:20], Y[:20], 0.0, xmean=True, xcov=True)
    for r in short[1:] + [again]:
        assert np.array_equal(r["xcov"].view(np.uint64), short[0]["xcov"].view(np.uint64))
        assert np.array_equal(r["xmean"].view(np.uint64), short[0]["xmean"].view(np.uint64))
    # (with the covariance requested the mean comes from the launch that also feeds it: another fixed summation order than the
    # partial sums of the weighting kernel — equal to rounding, not to the bit)
    np.testing.assert_allclose(long_["xmean"], first["xmean"], rtol=1e-12, atol=1e-14)
    assert np.array_equal(long_["xcov"][:20].view(np.uint64), short[0]["xcov"].view(np.uint64)) and np.all(np.isfinite(long_["xcov"]))
