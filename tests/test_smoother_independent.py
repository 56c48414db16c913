"""The FFBS particle smoother (llpf_smooth: kernels/smooth.hpp, kernels/smooth_fx.hpp, host/smooth.hpp) against an independent reference.

Every backward draw of an implementation — the C oracle in both arithmetic orders (no GPU needed), the HIP engine (`gpu`) — is checked
against oracle/independent.py: smoother_backward_step, the distribution of the draw in numpy.longdouble from the model objects of that
file, fed the implementation's own xb[t+1] (teacher forcing) and the draw's Philox uniform.  The reported index i must satisfy
cdf[i-1] - delta <= u <= cdf[i] + delta and xb[t, m] must be xf[t, i] bit for bit; delta is derived in backward_step_slack (quanta:
N 2^-K; sums to comparison: 8 * 2^-53; the fp64 rounding of the log-weights, weighted by the probabilities), not fitted.  A draw whose u
lies within delta of an edge accepts either neighbour and tests nothing ("excused"): none may be in the cases below, whose seed is chosen so.
The engine is also held bit for bit to the device-order oracle on every case.  Cases and the check: tests/smoother_cases.py.

What the sizes are for: k_smooth_draw is one block of 256 threads per trajectory; it strides over N in three sweeps, scans 1024 entries
per iteration of the third with a total carried between iterations and an early exit, and clamps the count to N - 1 — so N below, on
and above one wave, one block and one chunk, M = 1 and M = N, T = 1 (nothing runs on the device) and T = 2; hand-made histories put all
the weight where the early exit is taken in the first chunk, at its edge, in the second, or never.

Measured here with the oracle, against the long-double reference (never against the engine), over the 61 000 draws of all cases in both
orders: largest (slack the reported index needs) / delta = 0 — every index lies inside its reference interval without any slack —,
excused draws 0 (share 0), smallest distance from a uniform to an interior edge 4.9e-8, largest delta 1.2e-11 for the linear models
(N = 4097) and 2.7e-11 for the quad-tank.  The perturbed references fail as they must: the dynamics one step late or early 29 of 384
draws of the quad-tank case, the covariance used without inversion 142 of 192 of the full-covariance case.
No number in this file was measured on a GPU before the file's own first run there; delta is derived.  That run (one MI355X): every
`gpu` case passed both checks at the first attempt with the same figures (ratio 0, no excused draw); run times per test: nx = 16 1.6 s
and nx = 5 0.6 s (the run-time compilation of their kernels), the refusal of a compiled model with noise 1.0 s, every size (all M, T of
one N and one resampler) at most 0.4 s, every other case below that.  Without a GPU the 127 tests of this file that need none take 23 s, none over 1 s.

NaN in wf: settled by refusal.  The maximum of the backward weights is a chain of llpf_fmax(a, b) = a > b ? a : b, which returns b whenever
a is NaN and NaN whenever only b is: the serial chain of the oracle ends with the maximum of what follows the last NaN, a strided
block reduction with something else (test_a_nan_makes_the_maximum_depend_on_the_order).  llpf_smooth and orc_smooth refuse a wf with NaN
or +inf and a xf that is not finite; -inf log-weights stay legal and are cases here.
"""
import numpy as np
import pytest

import independent_cases as IC
import oracle_binding as ob
import smoother_cases as SC
from llpf_amd import _capi, _structs as S

ORDERS = [ob.ORDER_DEVICE, ob.ORDER_REFERENCE]


def _oracle_check(case, order, named=True, **perturb):
    xb, idx = SC.run(ob.OracleFilter(SC.config_of(case), order), case)
    st = SC.verify(case, xb, idx, ob, fixed_point=order == ob.ORDER_DEVICE, **perturb)
    print(case["name"], "order", order, {k: st[k] for k in ("draws", "wrong", "excused", "ratio_max", "edge_min", "delta_max")})
    if not perturb:
        SC.assert_verified(st, case["name"], named)
    return st, xb, idx


def _engine_check(case):
    """the engine on a case: every draw against the independent reference, and indices and samples bit for bit against the device-order oracle"""
    xg, ig = SC.run(_capi.FilterHandle(SC.config_of(case)), case)
    xo, io = SC.run(ob.OracleFilter(SC.config_of(case), ob.ORDER_DEVICE), case)
    st = SC.verify(case, xg, ig, ob)           # (the residual time-T draw is held to the oracle only)
    print(case["name"], "engine", {k: st[k] for k in ("draws", "wrong", "excused", "ratio_max", "edge_min", "delta_max")})
    SC.assert_verified(st, case["name"] + " (engine)")
    assert np.array_equal(ig, io), "%s: indices differ from the device-order oracle's" % case["name"]
    assert np.array_equal(xg.view(np.uint64), xo.view(np.uint64)), "%s: samples differ from the device-order oracle's" % case["name"]
    return xg, ig


def _facts_hold(facts, idx):
    if "only" in facts:
        assert np.all(idx[0] == facts["only"])
    if "never" in facts:
        assert not np.any((idx[0] >= facts["never"].start) & (idx[0] < facts["never"].stop)), "an index with a log-weight of -inf was drawn"


# ---- without a GPU: the reference and the case list against the C oracle in both orders ---------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("strategy", SC.STRATEGIES)
@pytest.mark.parametrize("N", SC.SIZES)
def test_oracle_draws_are_the_references_at_every_size(N, strategy, order):
    for case in SC.size_cases(N, strategy):
        _oracle_check(case, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("key", SC.DENSITY_CASES)
def test_oracle_draws_are_the_references_for_every_transition_density(key, order):
    _oracle_check(SC.density_case(key), order)


def test_a_neighbouring_index_is_refused():
    """the check is as sharp as the distribution's edges: moving every index of one time step to its neighbour fails every one of them"""
    case = SC.size_cases(257, S.RESAMPLE_STRATIFIED)[-1]                        # M = N = 257, T = 5
    xb, idx = SC.run(ob.OracleFilter(SC.config_of(case), ob.ORDER_DEVICE), case)
    for t in (0, case["T"] - 1):
        off = idx.copy()
        off[t] = np.where(idx[t] + 1 < case["N"], idx[t] + 1, idx[t] - 1)
        xo = xb.copy()
        xo[t] = case["xf"][t, off[t]]
        st = SC.verify(case, xo, off, ob)
        assert st["samples_ok"] and st["wrong"] >= case["M"]


def _uninverted(df, v):
    """the mutation: the quadratic form with Sigma where Sigma^-1 belongs"""
    return SC.ind.gaussian_logpdf_ld(SC.ind.Gaussian(df.mu, np.linalg.inv(df.Sigma)), v)


@pytest.mark.parametrize("order", ORDERS)
def test_a_covariance_used_without_inversion_is_seen(order):
    st, _, _ = _oracle_check(SC.density_case("nx3_full"), order, logpdf=_uninverted)
    assert st["wrong"] > st["draws"] // 4


@pytest.mark.parametrize("order", ORDERS)
def test_quadtank_across_its_switch_time_and_a_step_evaluated_at_the_wrong_time_is_seen(order):
    case = SC.quadtank_case()
    tsw, Ts = case["model"].qt[13], case["model"].Ts
    assert 0 < tsw / Ts < case["T"] - 2 and tsw / Ts != int(tsw / Ts)          # strictly inside the window of the backward steps
    _oracle_check(case, order)
    for shift in (1, -1):
        st, _, _ = _oracle_check(case, order, time_shift=shift)
        assert st["wrong"] > 0, "a reference evaluated %+d step off passes: the case cannot see a wrong time argument" % shift


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", SC.HANDMADE)
def test_oracle_draws_on_hand_made_histories(name, order):
    case, facts = SC.handmade_case(name)
    _, _, idx = _oracle_check(case, order)
    _facts_hold(facts, idx)
    if name.startswith("flat"):        # identical particles, equal weights: the distribution is i / N, the index ceil(u N) - 1
        u = ob.uniforms_nd(SC.SEED, 0, SC.STREAM_SMOOTH, 1, case["M"])[:, 0]
        assert np.array_equal(idx[0], np.ceil(u.astype(np.longdouble) * case["N"]).astype(np.int64) - 1)


def _fmax_chain(values, start):
    m = start
    for v in values:
        m = m if m > v else v           # llpf_fmax (csrc/shared/llpf_detmath.h)
    return m


def test_a_nan_makes_the_maximum_depend_on_the_order():
    w = [5.0, float("nan"), 1.0, 2.0]
    serial = _fmax_chain(w[1:], w[0])                                          # the oracle: m = w[0], then in index order
    lanes = [_fmax_chain(w[k::2], -np.inf) for k in range(2)]                  # the kernel: every thread its stride, then the block
    assert serial == 2.0 and _fmax_chain(lanes[1:], lanes[0]) == 5.0


def _spoiled(case, which, pos, value):
    c = dict(case)
    c[which] = case[which].copy()
    c[which].reshape(-1)[pos] = value
    return c


SPOILED = [("wf", 0, np.nan), ("wf", 700, np.nan), ("wf", -1, np.nan), ("wf", 3, np.inf), ("xf", 11, np.nan), ("xf", -1, -np.inf)]


@pytest.mark.parametrize("order", ORDERS)
def test_oracle_refuses_a_history_that_is_not_finite(order):
    case = SC.size_cases(257, S.RESAMPLE_SYSTEMATIC)[2]
    for which, pos, value in SPOILED:
        with pytest.raises(ValueError, match=r"\(-3\)"):
            SC.run(ob.OracleFilter(SC.config_of(case), order), _spoiled(case, which, pos, value))


def _noise_case():
    case = IC.cases()["pf_lg_laplace_noise"]
    T, N = 4, case["N"]
    rng = np.random.default_rng(0)
    wf = np.full((T, N), -np.log(N))
    return case, 8, case["U"][:T], rng.standard_normal((T, N, 2)), wf, np.exp(wf)


def test_oracle_refuses_a_model_with_process_noise_of_its_own():
    case, Mt, U, xf, wf, wef = _noise_case()
    with pytest.raises(ValueError, match=r"\(-2\)"):
        IC.oracle_of(ob, case, ob.ORDER_DEVICE).smooth(Mt, U, xf, wf, wef)


# ---- the same cases on the engine ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("strategy", SC.STRATEGIES)
@pytest.mark.parametrize("N", SC.SIZES)
def test_engine_draws_are_the_references_at_every_size(N, strategy):
    for case in SC.size_cases(N, strategy):
        _engine_check(case)


@pytest.mark.gpu
@pytest.mark.parametrize("key", SC.DENSITY_CASES)
def test_engine_draws_are_the_references_for_every_transition_density(key):
    _engine_check(SC.density_case(key))


@pytest.mark.gpu
def test_engine_quadtank_across_its_switch_time():
    _engine_check(SC.quadtank_case())


@pytest.mark.gpu
@pytest.mark.parametrize("name", SC.HANDMADE)
def test_engine_draws_on_hand_made_histories(name):
    case, facts = SC.handmade_case(name)
    _, idx = _engine_check(case)
    _facts_hold(facts, idx)


@pytest.mark.gpu
def test_engine_refuses_a_history_that_is_not_finite():
    case = SC.size_cases(257, S.RESAMPLE_SYSTEMATIC)[2]
    g = _capi.FilterHandle(SC.config_of(case))
    for which, pos, value in SPOILED:
        with pytest.raises(_capi.LLPFError, match=which) as e:
            SC.run(g, _spoiled(case, which, pos, value))
        assert e.value.code == _capi.ERR_ARG
    SC.run(g, case)                      # and the handle still works


@pytest.mark.gpu
def test_engine_refuses_a_model_with_process_noise_of_its_own():
    """llpf_smooth weights with logpdf(dynamics_density, .); a model with a `noise` member has a placeholder there (api.py fills in a
    standard normal) and a transition density that is not Gaussian: LLPF_ERR_ARG, naming the reason.  A `loglik` member (the measurement
    likelihood) does not enter the backward pass and stays allowed: tests/test_user_models.py smooths the pendulum."""
    case, Mt, U, xf, wf, wef = _noise_case()
    with pytest.raises(_capi.LLPFError, match="process noise of its own") as e:
        IC.engine_of(case).smooth(Mt, U, xf, wf, wef)
    assert e.value.code == _capi.ERR_ARG


@pytest.mark.gpu
def test_python_smooth_refuses_a_user_noise_density():
    import llpf_amd
    import user_models as UM
    case = IC.cases()["pf_lg_laplace_noise"]
    lg = case["model"]
    A = np.array(lg.A[:4]).reshape(2, 2); B = np.array(lg.B[:2]).reshape(2, 1); Cm = np.array(lg.C[:2]).reshape(1, 2)
    dyn = llpf_amd.UserDynamics(UM.LAPLACE_NOISE_SRC, 2, 1, 1, A=A, B=B, C=Cm, qt=case["user"][3])
    dg = llpf_amd.MvNormal(np.zeros(1), S.gaussian_cov_matrix(lg.measurement_density))
    d0 = llpf_amd.MvNormal(S.gaussian_mean(lg.initial_density), S.gaussian_cov_matrix(lg.initial_density))
    pf = llpf_amd.AdvancedParticleFilter(case["N"], dyn, llpf_amd.UserMeasurement(), llpf_amd.GaussianLikelihood(llpf_amd.UserMeasurement(), dg),
                                         llpf_amd.UserNoise(), d0, rng=IC.SEED)
    with pytest.raises(TypeError, match="UserNoise"):
        llpf_amd.smooth(pf, 8, case["U"][:4], case["Y"][:4])
    sol = llpf_amd.forward_trajectory(pf, case["U"][:4], case["Y"][:4])
    with pytest.raises(TypeError, match="UserNoise"):
        llpf_amd.smooth(pf, sol.x, sol.w, sol.we, sol.ll, 8, case["U"][:4], case["Y"][:4])
