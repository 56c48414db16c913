"""The summary statistics a user reads — weighted_mean / xmean, weighted_cov / xcov, weighted_quantile / xquant (k_wmean, k_wcov<8>,
k_wcov<16>, the k_wq_* passes) — on states of every kind, against references that share nothing with the kernels:

 * mean and covariance against the np.longdouble reference of tests/stats_common.py, entry by entry within the bound derived there,
   (ceil(N / 256) + 32) 2^-53 times the sum of the absolute terms; from particles() / expweights(), and for states the test installs
   also from the test's own particles and the long double exp-weights of its own (gridded) log-weights;
 * the quantiles bit for bit against the device-order restatement of StatsBase's algorithm (oracle: orc_weighted_quantile_dev), one
   dimension at a time, and within 1e-10 of the spread against its reference-order restatement;
 * the run loop's outputs against the same references on the returned history, against the accessors of a handle stepped by hand,
   against runs that ask for one output only, against a run that asks for none (the outputs must not move the filter), and against
   themselves when the captured graph of the run loop is replayed.

Measured on an MI355X, the largest ratio per shape over all particle counts and states — |err| / (2^-53 sum we |x|) of weighted_mean,
|err| / (2^-53 A) of weighted_cov, expweights() against the long double in ulp (the bound is 33 at N <= 256, 306 at N = 70001):
    shape      mean   cov   expweights        shape      mean   cov   expweights
    lg1        1.63   2.33  2.54              lg5        2.10   8.33  1.91
    lg2        2.10   4.27  2.44              lg8        3.46   3.91  2.06
    lg3-scal   1.96   3.92  1.99              lg9        2.10   3.88  1.51
    lg3-diag   1.93   3.92  1.99              lg12       2.10   5.11  2.52
    lg3-full   1.85   3.92  1.99              lg16       3.23   5.29  2.43
    lg4        1.91   4.25  2.38              qt         1.94   4.25  2.38
    run loop (N = 3000 and 2, 257, 1025; all shapes, kinds, strategies and thresholds): xmean <= 2.79, xcov <= 4.82
These exclude the 24 states in which the second-order term E of the mean's rounding (stats_common.ref_cov) is the larger part of the
error: N = 2, 3, 4 with the particles offset by 1e6 and a second weight of 1e-7 and less, where the covariance itself is ~1e-7 and the
squared rounding of a mean near 1e6 is ~1e-20 — up to 1.4e7 2^-53 A there, on the device as in the same formula in numpy, all within
K 2^-53 A + E.
"""
import functools

import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
import models as M
import oracle_binding as ob
import rbfull_models as RB
import stats_common as sc
from test_quantile import P

pytestmark = pytest.mark.gpu

PP = P + [1e-300, 0.999999]          # 11 probabilities: three rounds of the WQ_QCH = 4 quantiles a pass selects
T_STATE = 8                          # the run behind state (g)
T_RUN = 12
RUN_NOISE = 0.5                      # narrower measurement noise in the run loop's cases: threshold 0.5 resamples at some steps, not at all


# ---- models -----------------------------------------------------------------------------------------------------------------------
def _lg_model(nx, ny, nu, d0_kind=S.COV_SCAL, noise=4.0):
    rng = np.random.default_rng(100 + nx + ny)
    A = 0.9 * np.linalg.qr(rng.standard_normal((nx, nx)))[0]
    B = 0.2 * rng.standard_normal((nx, nu)) if nu else None
    Cm = rng.standard_normal((ny, nx))
    mu0 = rng.standard_normal(nx)
    if d0_kind == S.COV_SCAL:
        d0 = S.make_gaussian(mu0, 1.0)
    elif d0_kind == S.COV_DIAG:
        d0 = S.make_gaussian(mu0, 0.5 + rng.random(nx))
    else:
        Q = rng.standard_normal((nx, nx))
        d0 = S.make_gaussian(mu0, Q @ Q.T / nx + 0.3 * np.eye(nx), S.COV_FULL)
    # (measurement noise wide enough that the weights of a few particles stay comparable: see _check_quantiles)
    return S.make_lg_model(A, B, Cm, S.make_gaussian(np.zeros(nx), 0.05), S.make_gaussian(np.zeros(ny), noise * nx * (0.5 + rng.random(ny))), d0)


# linear-Gaussian (nx, ny, nu): precompiled up to 4 states, compiled at run time above (the shapes tests/test_gpu_parity.py compiles, and
# 9 states: the first shape on the k_wcov<16> side of the 8 / 9 split); the covariance kinds of the initial density; the quad-tank
SHAPES = {
    "lg1": (1, 1, 1), "lg2": (2, 1, 1), "lg3-scal": (3, 2, 1), "lg3-diag": (3, 2, 1), "lg3-full": (3, 2, 1), "lg4": (4, 2, 2),
    "lg5": (5, 2, 1), "lg8": (8, 8, 2), "lg9": (9, 2, 0), "lg12": (12, 4, 2), "lg16": (16, 8, 2), "qt": None,
}
KINDS = {"lg3-diag": S.COV_DIAG, "lg3-full": S.COV_FULL}


@functools.lru_cache(maxsize=None)
def _shape(name, T, noise=4.0):
    """(model, filter kind, U, Y) with one missing measurement; noise: the scale of the measurement noise's variance"""
    if name == "qt":
        model, kind = M.quadtank_model(), S.ADVANCED_PARTICLE_FILTER
        model.measurement_density = S.make_gaussian(np.zeros(2), np.full(2, noise / 16.0))
        U, Y = M.quadtank_data(T)
    else:
        model, kind = _lg_model(*SHAPES[name], KINDS.get(name, S.COV_SCAL), noise), S.PARTICLE_FILTER
        _, U, Y = M.simulate_lg(model, T, seed=4)
    Y[T // 2 - 1] = np.nan
    return model, kind, U, Y


def _handle(name, N, thr, T=T_STATE, strategy=S.RESAMPLE_SYSTEMATIC, kind=None, seed=None, noise=4.0):
    model, k0, U, Y = _shape(name, T, noise)
    cfg = S.make_config(model, N, k0 if kind is None else kind, strategy, thr, 1000 + N % 89 if seed is None else seed, 0)
    return _capi.FilterHandle(cfg), U, Y


def _u(U, k):
    return U[k] if U.shape[1] else None


# ---- the checks -------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_moments(shape, N, where, m, c, x, we, what=""):
    """mean m and covariance c of the device against the long double reference on (x, we)"""
    bound = sc.bound_units(N)
    mr, am = sc.ref_mean(x, we)
    rm = sc.ratio(m - mr, am)
    assert rm <= bound, "%s N = %d %s: weighted_mean%s off by %.1f u sum we |x| (bound %d)" % (shape, N, where, what, rm, bound)
    if c is None:
        return rm, None
    C, A, E = sc.ref_cov(x, we, N)
    if np.count_nonzero(np.asarray(we)) == 1:      # 0 * inf in every entry (N = 1, or all the weight on one particle)
        assert np.all(np.isnan(C)) and np.all(np.isnan(c)), "%s N = %d %s: one particle with weight, weighted_cov = %r" % (shape, N, where, c)
        return rm, None
    rc = sc.ratio(c - C, A)                        # the figure reported: all of the error in units of u A
    assert sc.ratio(c - C, A, E) <= bound, "%s N = %d %s: weighted_cov%s off by %.1f u A (bound %d, second-order term %.3g u A)" % (
        shape, N, where, what, rc, bound, sc.ratio(E, A))
    return rm, rc


def _check_quantiles(shape, N, where, q, x, we):
    """q [len(PP), nx] of the device: the device-order restatement's bits, the reference-order restatement within 1e-10 of the spread.
    (The second holds where the running sums of StatsBase's fp64 formula are well conditioned.  Where one particle holds all the weight
    up to rounding they are not — 1 + 1e-20 does not exceed h = 1, so the formula steps past every particle and returns the largest
    value for EVERY p, while the device's integer sums cross at the particle next to the heavy one: v = 0, 1, 2 with w = 1, 1e-20,
    1e-20 gives 2 and 1 — which is why the models above have measurement
    noise wide enough for the weights of a few particles to stay comparable.  States of one and two weights: (f).)"""
    spread = np.ptp(x, axis=0) + 1.0
    for d in range(x.shape[1]):
        col = np.ascontiguousarray(x[:, d])
        dev = ob.weighted_quantile_dev(col, we, PP)
        assert np.array_equal(_bits(q[:, d]), _bits(dev)), "%s N = %d %s, state %d: quantiles %r against %r" % (shape, N, where, d, q[:, d], dev)
        ref = ob.weighted_quantile(col, we, P[:-1])          # (p = 1 is ill-conditioned in StatsBase's own formula: tests/test_quantile.py)
        err = np.abs(q[:len(P) - 1, d] - ref)
        assert np.all(err <= 1e-10 * spread[d]), "%s N = %d %s, state %d: %.3g of the spread" % (shape, N, where, d, np.max(err) / spread[d])


def _check_state(g, shape, N, where, own=None):
    """the three accessors on the handle's current state; own = (x, long double exp-weights) the test installed itself"""
    x, we = g.particles(), g.expweights()
    m, c = g.weighted_mean(), g.weighted_cov()
    c2 = g.weighted_cov()
    assert np.array_equal(_bits(c), _bits(c2)), "%s N = %d %s: weighted_cov differs between two calls" % (shape, N, where)
    assert np.array_equal(_bits(c), _bits(c.T)), "%s N = %d %s: weighted_cov is not symmetric to the bit" % (shape, N, where)
    rm, rc = _check_moments(shape, N, where, m, c, x, we)
    line = "%-8s N = %-6d %-22s mean %5.2f cov %s" % (shape, N, where, rm, "  NaN" if rc is None else "%5.2f" % rc)
    if own is not None:
        xo, weo = own
        assert np.array_equal(_bits(x), _bits(xo)), "%s N = %d %s: particles() is not what set_particles installed" % (shape, N, where)
        wef = weo.astype(np.float64)
        ulps = np.abs((we - weo).astype(np.float64)) / np.where(wef > 0, np.spacing(wef), 1.0)
        assert np.all((we == 0) == (weo == 0)) and np.max(ulps) <= 4.0, "%s N = %d %s: expweights() %.2f ulp from the long double" % (shape, N, where, np.max(ulps))
        rmo, rco = _check_moments(shape, N, where, m, c, xo, weo, " (own weights)")
        line += "  own weights: mean %5.2f cov %s expweights %.2f ulp" % (rmo, "  NaN" if rco is None else "%5.2f" % rco, np.max(ulps))
    print(line)
    _check_quantiles(shape, N, where, g.weighted_quantile(PP), x, we)
    return c


def _installed_state(rng, N, nx, offset):
    """particles with a third of them tied to particle 0, gridded log-weights with 30-40 % -inf; particle 0 and one particle that is not
    tied to it always carry weight, so that the weighted particles are never all one point (A = 0 bounds nothing)"""
    x = rng.standard_normal((N, nx)) * (1.0 + 0.5 * np.arange(nx)) + offset
    free = 1
    if N >= 3:
        tied = rng.integers(1, N, N // 3)
        x[tied] = x[0]
        free = int(np.setdiff1d(np.arange(1, N), tied)[0])
    lw = sc.grid_logweights(rng, N)
    for i in (0, free)[:N]:
        if np.isneginf(lw[i]):
            lw[i] = -1.5
    return x, lw, free


CASES = sorted(set(
    [(s, N) for s in ("lg2", "lg16") for N in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 70001)] +
    [(s, N) for s in SHAPES for N in (2, 257, 4097)] +
    # around N * nx = 16 + nx * nx, where the covariance of the accessor used to lie past the staging buffer (host/bank.hpp: bank_carve)
    [(s, N) for s in ("lg5", "lg8", "lg16") for N in (1, 2, 4, 7, 8, 15, 16, 17)]), key=lambda c: (list(SHAPES).index(c[0]), c[1]))


@pytest.mark.parametrize("shape,N", CASES, ids=["%s-%d" % c for c in CASES])
def test_accessors_on_states_of_every_kind(shape, N):
    """(a) reset!: the `uniform` flag; (b) one correct!: lazily normalised; (c) three update!s that never resample: the weights
    accumulate; (d) update!s that resample every step; (e) particles and weights the test installs: ties, weights of exactly zero, states
    offset by 1e6; (f) exactly two weights, and all the weight on one particle (NaN, no error, the handle goes on); (g) what a whole run
    leaves behind at threshold 1 (the lean form) and 0.1 (the balanced form)."""
    g, U, Y = _handle(shape, N, 0.0)
    nx = g.nx
    g.reset()
    _check_state(g, shape, N, "(a) reset")
    g.correct(_u(U, 0), Y[0], 0.0)
    _check_state(g, shape, N, "(b) correct")
    g.predict(_u(U, 0), 0.0)
    for k in range(1, 4):
        g.update(_u(U, k), Y[k], float(k))
        assert not g.last_resampled()
    _check_state(g, shape, N, "(c) accumulated")

    rng = np.random.default_rng(7 * N + nx)
    first = None
    for offset in (0.0, 1e6):
        x, lw, free = _installed_state(rng, N, nx, offset)
        g.set_particles(x); g.set_weights(lw)
        c = _check_state(g, shape, N, "(e) installed%s" % (" + 1e6" if offset else ""), own=(x, sc.exp_weights(lw)))
        first = (x, lw, c) if first is None else first
    if N >= 2:
        lw2 = np.full(N, -np.inf)
        lw2[0], lw2[free] = -2.25, 0.0
        g.set_weights(lw2)
        _check_state(g, shape, N, "(f) two weights", own=(x, sc.exp_weights(lw2)))
    lw1 = np.full(N, -np.inf)
    lw1[N // 2] = -3.5
    g.set_weights(lw1)
    c = _check_state(g, shape, N, "(f) one weight", own=(x, sc.exp_weights(lw1)))
    assert np.all(np.isnan(c))
    g.set_particles(first[0]); g.set_weights(first[1])          # ... and the handle goes on working: the first installed state again
    assert np.array_equal(_bits(g.weighted_cov()), _bits(first[2]))
    assert np.isfinite(g.update(_u(U, 4), Y[4], 4.0))

    g, U, Y = _handle(shape, N, 1.0)
    g.reset()
    for k in range(3):
        g.update(_u(U, k), Y[k], float(k))
        assert g.last_resampled()
    _check_state(g, shape, N, "(d) resampled")
    for thr in (1.0, 0.1):
        if thr != 1.0:
            g, U, Y = _handle(shape, N, thr)
        g.reset()
        g.run(U, Y, 0.0)
        _check_state(g, shape, N, "(g) run, threshold %.1f" % thr)


# ---- the run loop's outputs -------------------------------------------------------------------------------------------------------
PF, APF = S.PARTICLE_FILTER, S.ADVANCED_PARTICLE_FILTER
SYS, STRAT, RESID = S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED, S.RESAMPLE_RESIDUAL
RUN_CASES = (
    [("lg2", 3000, kind, strategy, thr) for kind in (PF, APF) for strategy in (SYS, STRAT, RESID) for thr in (0.1, 0.5, 1.0)] +
    [(s, 3000, None, SYS, thr) for s in ("lg1", "lg4", "lg5", "lg9", "lg16", "qt") for thr in (0.5, 1.0)] +
    [("lg2", N, PF, SYS, 0.5) for N in (2, 257, 1025)])


def _run_id(c):
    return "%s-%d-%s-%s-%.1f" % (c[0], c[1], {PF: "pf", APF: "apf", None: "own"}[c[2]], {SYS: "systematic", STRAT: "stratified", RESID: "residual"}[c[3]], c[4])


@pytest.mark.parametrize("shape,N,kind,strategy,thr", RUN_CASES, ids=[_run_id(c) for c in RUN_CASES])
def test_outputs_of_the_run_loop(shape, N, kind, strategy, thr):
    """run(history, xmean, xcov, quantiles) over 12 steps with a missing measurement: every step's outputs against the references on the
    returned history; the filter of a run without outputs; the outputs of runs that ask for one of them; the accessors of a handle
    stepped by hand; a second and a third run of the same shape (the captured graph)."""
    seed = 500 + N % 97
    hs = [_handle(shape, N, thr, T_RUN, strategy, kind, seed, RUN_NOISE)[0] for _ in range(5)]
    g, g0, gc, gq, gh = hs
    _, _, U, Y = _shape(shape, T_RUN, RUN_NOISE)
    nx = g.nx
    for h in hs:
        h.seed(seed); h.reset()
    r = g.run(U, Y, 0.0, ll_steps=True, xmean=True, history=True, xcov=True, quantiles=PP)

    # the references, step by step on the returned history
    worst_m = worst_c = 0.0
    for k in range(T_RUN):
        where = "step %d" % k
        rm, rc = _check_moments(shape, N, where, r["xmean"][k], r["xcov"][k], r["x"][k], r["we"][k], " (run)")
        worst_m, worst_c = max(worst_m, rm), max(worst_c, rc or 0.0)
        assert np.array_equal(_bits(r["xcov"][k]), _bits(r["xcov"][k].T))
        _check_quantiles(shape, N, where, r["xquant"][k].T, r["x"][k], r["we"][k])
    print("%-8s N = %-6d run %-28s xmean %5.2f xcov %5.2f" % (shape, N, _run_id((shape, N, kind, strategy, thr)), worst_m, worst_c))

    # the statistics do not move the filter
    r0 = g0.run(U, Y, 0.0, ll_steps=True)
    print("         resampled at %d of %d steps" % (g0.resample_count(), T_RUN))
    assert np.array_equal(_bits(r["ll_steps"]), _bits(r0["ll_steps"]))
    assert np.array_equal(_bits(g.particles()), _bits(g0.particles())) and np.array_equal(_bits(g.weights()), _bits(g0.weights()))
    assert np.array_equal(g.ancestors(), g0.ancestors())
    # one output alone
    assert np.array_equal(_bits(gc.run(U, Y, 0.0, xcov=True)["xcov"]), _bits(r["xcov"]))
    assert np.array_equal(_bits(gq.run(U, Y, 0.0, quantiles=PP)["xquant"]), _bits(r["xquant"]))

    # a handle stepped by hand: correct!, the accessors, predict!
    bound = sc.bound_units(N)
    for k in range(T_RUN):
        t = float(k) * g.cfg.model.Ts
        ll = gh.correct(_u(U, k), Y[k], t)
        assert _bits(np.float64(ll)) == _bits(r["ll_steps"][k]), "step %d: the run and the single steps differ" % k
        assert np.array_equal(_bits(gh.weighted_cov()), _bits(r["xcov"][k])), "xcov[%d] is not the accessor's" % k
        assert np.array_equal(_bits(gh.weighted_quantile(PP).T), _bits(r["xquant"][k])), "xquant[%d] is not the accessor's" % k
        # (the means of a run come from the launch that forms the weights: another fixed order than the accessor's — each within the
        #  bound of the reference, so within twice the bound of each other)
        am = sc.ref_mean(r["x"][k], r["we"][k])[1]
        assert sc.ratio(gh.weighted_mean() - r["xmean"][k], am) <= 2 * bound
        gh.predict(_u(U, k), t)

    # the same shape a second and a third time: captured, replayed
    for _ in range(2):
        g.seed(seed); g.reset()
        rn = g.run(U, Y, 0.0, ll_steps=True, xmean=True, history=True, xcov=True, quantiles=PP)
        assert np.array_equal(_bits(rn["xcov"]), _bits(r["xcov"])) and np.array_equal(_bits(rn["xquant"]), _bits(r["xquant"]))
        assert np.array_equal(_bits(rn["ll_steps"]), _bits(r["ll_steps"]))
    assert nx == r["xcov"].shape[1]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _state(g):
    return [g.particles(), g.weights(), g.expweights(), g.ancestors(), np.array([g.index()])]


def _refused(g, call):
    """`call` raises LLPF_ERR_ARG and leaves the handle's state as it was"""
    before = _state(g)
    with pytest.raises(_capi.LLPFError) as ei:
        call()
    assert ei.value.code == _capi.ERR_ARG, ei.value
    for a, b in zip(before, _state(g)):
        assert np.array_equal(_bits(a) if a.dtype == np.float64 else a, _bits(b) if b.dtype == np.float64 else b)


def test_refusals_leave_the_handle_untouched():
    """xcov / xquant from the auxiliary run loop, weighted_cov / weighted_quantile of LLPF_MODEL_RB_BILINEAR (the particle carries a
    covariance of its own), a probability outside [0, 1]: LLPF_ERR_ARG, nothing of the handle moves.  (A bank's run verbs take no
    output descriptor at all: the C ABI cannot ask a bank for xcov or xquant.)"""
    g, U, Y = _handle("lg2", 300, 0.5)
    g.reset()
    g.update(_u(U, 0), Y[0], 0.0)
    g.correct(_u(U, 1), Y[1], 1.0)
    _refused(g, lambda: g._run("aux_run", U, Y, 0, False, False, False, xcov=True))
    _refused(g, lambda: g._run("aux_run", U, Y, 1, True, False, False, quantiles=[0.5]))
    for bad in ([0.5, 1.5], [-1e-300], [0.5, np.nan], [1.0 + 2.0 ** -52]):
        _refused(g, lambda: g.weighted_quantile(bad))
        _refused(g, lambda: g.run(U, Y, 0.0, quantiles=bad))
    _refused(g, lambda: g.weighted_quantile(np.zeros(1025)))
    twin, _, _ = _handle("lg2", 300, 0.5)
    twin.reset()
    twin.update(_u(U, 0), Y[0], 0.0)
    twin.correct(_u(U, 1), Y[1], 1.0)
    assert np.array_equal(_bits(g.weighted_cov()), _bits(twin.weighted_cov()))
    assert np.array_equal(_bits(g.run(U, Y, 2.0, ll_steps=True)["ll_steps"]), _bits(twin.run(U, Y, 2.0, ll_steps=True)["ll_steps"]))

    model, _ = RB.linear_case(2, 2, 2)
    Ur, Yr = RB.simulate_io(model, 4)
    rb = _capi.FilterHandle(S.make_config(model, 200, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 5, 0))
    rb.reset()
    rb.correct(Ur[0] if Ur.shape[1] else None, Yr[0], 0.0)
    _refused(rb, lambda: rb.weighted_cov())
    _refused(rb, lambda: rb.weighted_quantile([0.5]))
    _refused(rb, lambda: rb.run(Ur, Yr, 0.0, xcov=True))
    _refused(rb, lambda: rb.run(Ur, Yr, 0.0, quantiles=[0.5]))
    assert np.all(np.isfinite(rb.weighted_mean()))
