"""The cases of the FFBS smoother's independent check and the check itself (tests/test_smoother_independent.py without a GPU,
tests/test_gpu_smoother_independent.py on the engine).

A case is a filter history (xf, wf, wef: llpf_smooth takes them from the caller), the model twice — as the llpf_model the engine and the C
oracle take and as the numpy objects of oracle/independent.py — and (M, T, strategy).  `verify` takes what an implementation returned for it,
(xb, idx), and checks every backward draw against oracle/independent.py: smoother_backward_step (long double) fed the implementation's own
xb[t+1] (teacher forcing: one borderline draw cannot spread down a trajectory), backward_step_slack for the derived slack delta, the
uniform of the draw from the Philox stream the Random123 vectors pin (tests/test_detmath.py).  Nothing in a case is frozen: the reference
is computed from the output under test.
"""
import functools

import numpy as np

import independent_cases as IC      # puts oracle/ on the path
import models as M
from llpf_amd import _structs as S

ind = IC.ind

SEED = 11
STREAM_SMOOTH, STREAM_SMOOTH_INIT = 5, 6          # LLPF_STREAM_SMOOTH, LLPF_STREAM_SMOOTH_INIT (csrc/shared/llpf_philox.h)
# one wave (64), one block (256), one chunk of the draw kernel's scan (1024), each with its neighbours; two and four chunks and one more
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)
LENGTHS = (1, 2, 5)                               # T = 1: the host-only return; T = 2: one backward step
STRATEGIES = (S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED, S.RESAMPLE_RESIDUAL)
EXCUSED_SHARE_MAX = 1e-3


def trajectories(N):
    """M of the size cases: 1 and N up to N = 257; above it 1 and 64, so that the long-double reference stays short"""
    return sorted({1, N}) if N <= 257 else [1, 64]


def _objects(model):
    if model.model_id == S.MODEL_QUADTANK_RK4:
        return IC._qt_object(model), IC._gauss(model.dynamics_density)
    return IC._lg_objects(model), IC._gauss(model.dynamics_density)


def _case(name, model, N, Mtraj, strategy, U, xf, wf, wef, kind=S.PARTICLE_FILTER):
    imodel, idf = _objects(model)
    T = wf.shape[0]
    return dict(name=name, model=model, imodel=imodel, idf=idf, N=N, M=Mtraj, T=T, strategy=strategy, kind=kind,
                U=None if model.nu == 0 else np.ascontiguousarray(U[:T]), xf=np.ascontiguousarray(xf[:T]), wf=np.ascontiguousarray(wf[:T]),
                wef=np.ascontiguousarray(wef[:T]))


def config_of(case):
    return S.make_config(case["model"], case["N"], case["kind"], case["strategy"], 0.5, SEED, 0)


@functools.lru_cache(maxsize=None)
def _history(key, N, T, strategy, kind=S.PARTICLE_FILTER):
    """a filter history of T steps from the device-order C oracle (any history would do: the smoother takes it as an argument)"""
    import oracle_binding as ob
    model, U, Y = _MODELS[key](T)
    o = ob.OracleFilter(S.make_config(model, N, kind, strategy, 0.5, SEED, 0), ob.ORDER_DEVICE)
    o.reset()
    r = o.run(U, Y, 0.0, history=True)
    return model, U, r["x"], r["w"], r["we"]


def _lg(A, B, Cm, df, d0_scale=1.0, seed=4):
    def make(T):
        nx, ny = np.atleast_2d(A).shape[0], np.atleast_2d(Cm).shape[0]
        model = S.make_lg_model(A, B, Cm, df, S.make_gaussian(np.zeros(ny), 0.5), S.make_gaussian(np.zeros(nx), d0_scale))
        _, U, Y = M.simulate_lg(model, T, seed=seed)
        return model, U, Y
    return make


def _rot(n, seed):
    return np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))[0]


def _c2(T):
    model = M.lg_test_model(0.1)                   # nx = 2, nu = 1, scalar covariance
    _, U, Y = M.simulate_lg(model, T, seed=2)
    return model, U, Y


def _quadtank(T):
    # the outflow of tank 1 doubles at t_switch = 2.5 Ts: strictly inside the smoothed window of T = 6 (backward steps at 0 .. 4 Ts), so a
    # backward step evaluated one step early or late integrates other dynamics.  Process noise of standard deviation 0.03: the change of
    # 0.04 per step in the first state is more than one standard deviation.
    df = S.make_gaussian(np.zeros(4), np.full(4, 9e-4))
    model = S.make_quadtank_model(df, S.make_gaussian(np.zeros(2), np.full(2, 1e-4)), S.make_gaussian(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1)),
                                  1.0, 2, t_switch=2.5)
    U, Y = M.quadtank_data(T)
    return model, U, Y


_R3 = _rot(3, 1)
_MODELS = {
    "c2": _c2,
    "nx1": _lg([[0.9]], [[0.5]], [[1.0]], S.make_gaussian(np.zeros(1), 0.04)),
    "nx3_diag": _lg(0.9 * _rot(3, 2), 0.3 * np.ones((3, 1)), np.eye(2, 3), S.make_gaussian(np.zeros(3), np.array([0.01, 0.09, 0.25]))),
    # eigenvalues 0.01, 0.04 and 1 along axes that are not the coordinate axes: off-diagonal terms of the size of the diagonal, and a
    # factor used transposed or without inversion weights other particles
    "nx3_full": _lg(0.9 * _rot(3, 2), 0.3 * np.ones((3, 1)), np.eye(2, 3), S.make_gaussian(np.zeros(3), _R3 @ np.diag([0.01, 0.04, 1.0]) @ _R3.T)),
    "nx5": _lg(0.9 * _rot(5, 3), 0.2 * np.ones((5, 1)), np.eye(2, 5), S.make_gaussian(np.zeros(5), 0.05)),
    "nx16": _lg(0.9 * _rot(16, 5), 0.1 * np.ones((16, 2)), np.eye(2, 16), S.make_gaussian(np.zeros(16), np.linspace(0.02, 0.2, 16))),
    "nu0": _lg(np.array([[0.97043, -0.097368], [0.09736, 0.970437]]), None, [[0.0, 1.0]], S.make_gaussian(np.zeros(2), 0.01)),
    "quadtank": _quadtank,
}
DENSITY_CASES = ("nx1", "nx3_diag", "nx3_full", "nx5", "nx16", "nu0")


def size_cases(N, strategy):
    """every (M, T) of the size sweep for one N and one resampler of the time-T draw; linear-Gaussian, nx = 2, scalar covariance"""
    model, U, xf, wf, wef = _history("c2", N, max(LENGTHS), strategy)
    return [_case("c2_N%d_M%d_T%d_s%d" % (N, Mt, T, strategy), model, N, Mt, strategy, U[:T], xf[:T], wf[:T], wef[:T])
            for Mt in trajectories(N) for T in LENGTHS]


def density_case(key):
    """the transition density: N = 300, M = 48, T = 4"""
    model, U, xf, wf, wef = _history(key, 300, 4, S.RESAMPLE_SYSTEMATIC)
    return _case(key, model, 300, 48, S.RESAMPLE_SYSTEMATIC, U, xf, wf, wef)


def quadtank_case():
    model, U, xf, wf, wef = _history("quadtank", 300, 6, S.RESAMPLE_SYSTEMATIC, S.ADVANCED_PARTICLE_FILTER)
    return _case("quadtank_switch", model, 300, 64, S.RESAMPLE_SYSTEMATIC, U, xf, wf, wef, kind=S.ADVANCED_PARTICLE_FILTER)


HANDMADE = tuple("%s_N%d" % (k, N) for N in (2049, 4097) for k in ("one_0", "one_1023", "one_1024", "one_last", "flat", "band", "all_but_one"))


def handmade_case(name):
    """histories no filter produced (T = 2: one backward step over wf[0], M = 64).  one_<n>: all weight on particle n (every other
    log-weight 2000 below it: its quantum is 0) — the draw kernel's scan leaves its loop in the first chunk (n = 0, 1023), in the second
    (1024) or never (N - 1); flat: equal weights and identical particles, the distribution is exactly i / N; band: log-weights -inf on
    [500, 1500), what a likelihood of bounded support leaves behind; all_but_one: every log-weight but one -inf.
    Returns (case, facts): facts["only"] the one index that may be drawn, facts["never"] a slice no index may fall in."""
    kind, N = name.rsplit("_N", 1)
    N = int(N)
    rng = np.random.default_rng(N + len(kind))
    model, U, _ = _c2(2)
    xf = rng.standard_normal((2, N, 2))
    wf = np.log(rng.uniform(0.1, 1.0, (2, N)))
    wf -= np.log(np.sum(np.exp(wf), axis=1, keepdims=True))
    facts = {}
    if kind.startswith("one_"):
        n0 = N - 1 if kind == "one_last" else int(kind[4:])
        wf[0] = -2000.0
        wf[0, n0] = 0.0
        facts["only"] = n0
    elif kind == "flat":
        xf[0] = xf[0, 0]
        wf[0] = -np.log(N)
    elif kind == "band":
        wf[0, 500:1500] = -np.inf
        facts["never"] = slice(500, 1500)
    elif kind == "all_but_one":
        wf[0] = -np.inf
        wf[0, 1500] = -0.25
        facts["only"] = 1500
    else:
        raise KeyError(name)
    return _case(name, model, N, 64, S.RESAMPLE_SYSTEMATIC, U, xf, wf, np.exp(wf)), facts


def run(handle, case):
    """(xb, idx) of an implementation (an OracleFilter or a FilterHandle of config_of(case)) for a case"""
    return handle.smooth(case["M"], case["U"], case["xf"], case["wf"], case["wef"])


def _bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _time_T_thresholds(case, ob):
    """the thresholds of j = resample(strategy, wef[:, T], M) over the normalised bins, from the independent restatement's formulas
    (oracle/independent.py: resample_systematic, resample_stratified), and that restatement's own indices"""
    N, Mt, T = case["N"], case["M"], case["T"]
    we = case["wef"][T - 1]
    Us = ob.uniforms_nd(SEED, T, STREAM_SMOOTH_INIT, 1, Mt)[:, 0]
    jprev = np.zeros(Mt, dtype=np.int64)
    if case["strategy"] == S.RESAMPLE_SYSTEMATIC:
        j, _ = ind.resample_systematic(we, jprev, float(Us[0]), Mt)
        s = ind.LD(Us[0]) / N + np.arange(Mt, dtype=ind.LD) / Mt
    else:
        j, _ = ind.resample_stratified(we, jprev, Us, Mt)
        s = (np.arange(Mt, dtype=ind.LD) + Us.astype(ind.LD)) / Mt
    return s, j


def verify(case, xb, idx, ob, fixed_point=True, time_shift=0, logpdf=None):
    """Every draw of (xb, idx) against the long-double reference.  fixed_point: the implementation sums quanta (the engine, the oracle in
    device order) or fp64 numbers (the oracle in reference order) — see backward_step_slack.  time_shift / logpdf perturb the REFERENCE
    (the mutation checks): the dynamics evaluated time_shift steps late, another density.
    Returns dict(draws, wrong, excused, ratio_max = the largest (slack the reported index needs) / delta, edge_min = the smallest distance
    from a uniform to an interior edge of its distribution, delta_max, samples_ok, first = a description of the first wrong draw)."""
    N, Mt, T, Ts = case["N"], case["M"], case["T"], case["model"].Ts
    xf, wf = case["xf"], case["wf"]
    st = dict(draws=0, wrong=0, excused=0, ratio_max=0.0, edge_min=np.inf, delta_max=0.0, samples_ok=True, first=None)

    def account(t, cdf, u, delta):
        need, excused, edge = ind.check_draws(cdf, u, idx[t], delta)
        bad = need > delta
        st["draws"] += Mt
        st["wrong"] += int(np.sum(bad))
        st["excused"] += int(np.sum(excused))
        st["ratio_max"] = max(st["ratio_max"], float(np.max(need / delta)))
        st["edge_min"] = min(st["edge_min"], float(np.min(edge)))
        st["delta_max"] = max(st["delta_max"], float(np.max(delta)))
        if np.any(bad) and st["first"] is None:
            m = int(np.flatnonzero(bad)[0])
            st["first"] = "t = %d, m = %d: index %d needs %.3g, delta = %.3g, u = %.17g" % (t, m, idx[t, m], need[m], np.broadcast_to(delta, (Mt,))[m], u[m])
        return excused

    rows = np.arange(Mt)
    for t in range(T):
        st["samples_ok"] = st["samples_ok"] and bool(np.all((idx[t] >= 0) & (idx[t] < N))) and _bits_equal(xb[t], xf[t, np.clip(idx[t], 0, N - 1)])
    if case["strategy"] != S.RESAMPLE_RESIDUAL:
        # time T: the bins are the running sums of wef itself.  Slack: the quanta (or the fp64 cumsum) as in backward_step_slack, the same
        # 8 roundings from sums to comparison, and |1 - sum(wef)| <= N 2^-53, by which bins[end] scales the thresholds
        we = case["wef"][T - 1].astype(ind.LD)
        cdf = (np.cumsum(we) / np.sum(we))[None, :].repeat(Mt, axis=0)
        cdf[:, -1] = 1
        s, j = _time_T_thresholds(case, ob)
        K = ind.qbits(N)
        delta = np.full(Mt, (N * 2.0 ** -K * (1 + N * 2.0 ** -K) if fixed_point else 2 * N * ind.U53) + (8 + N) * ind.U53)
        excused = account(T - 1, cdf, s, delta)
        if not np.array_equal(j[~excused], idx[T - 1][~excused]):
            st["wrong"] += 1
            st["first"] = st["first"] or "time T: indices differ from the independent resampler's"
    for t in range(T - 2, -1, -1):
        step = ind.smoother_backward_step(xf[t], wf[t], case["imodel"], case["idf"], None if case["U"] is None else case["U"][t],
                                          (t + time_shift) * Ts, xb[t + 1], **({} if logpdf is None else {"logpdf": logpdf}))
        delta = ind.backward_step_slack(step, case["imodel"], case["idf"], fixed_point)
        account(t, step["cdf"], ob.uniforms_nd(SEED, t, STREAM_SMOOTH, 1, Mt)[:, 0], delta)
    return st


def assert_verified(st, what, named=True):
    """the check's verdict; `named`: a case of the lists above, whose seed is chosen so that no draw is excused"""
    assert st["samples_ok"], "%s: xb is not xf[idx] bit for bit, or an index is out of range" % what
    assert st["wrong"] == 0, "%s: %d of %d draws are not the reference's: %s" % (what, st["wrong"], st["draws"], st["first"])
    assert st["excused"] <= (0 if named else EXCUSED_SHARE_MAX * st["draws"]), \
        "%s: %d of %d draws lie within delta of an edge and test nothing" % (what, st["excused"], st["draws"])
