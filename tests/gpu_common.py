"""Shared helpers of the GPU parity tests."""
import os

import numpy as np

from llpf_amd import _structs as S

TOL_LL_STEP = 1e-10      # per-step |ll_gpu - ll_ref_order|   
TOL_LL_SUM = 1e-8        # cumulative
TOL_WE_REL = 1e-12       # max relative error of exp-weights vs reference order


def cfg_of(model, N, strategy=S.RESAMPLE_SYSTEMATIC, thr=0.1, seed=7, kind=S.PARTICLE_FILTER):
    return S.make_config(model, N, kind, strategy, thr, seed, 0)


class _Inject:
    """with _Inject("<kind>:<site>"): the library's fault injection (LLPF_TEST_THROW) for the calls inside"""

    def __init__(self, spec):
        self.spec = spec

    def __enter__(self):
        os.environ["LLPF_TEST_THROW"] = self.spec      # os.environ assigns through putenv: the library's getenv sees it

    def __exit__(self, *a):
        del os.environ["LLPF_TEST_THROW"]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _val(v):
    return "%s (%r)" % (float(v).hex(), float(v)) if isinstance(v, (float, np.floating)) else repr(int(v))


def step_mismatch(got, want, resamples=None):
    """None if the per-step arrays (T, ...) are bit-identical.  Otherwise a message that names the first differing timestep, both
    values there (hex and decimal), how many timesteps differ and, given resamples = (got, want), both resample counts."""
    a, b = _bits(got), _bits(want)
    if a.shape != b.shape:
        return "shapes differ: %s against %s" % (a.shape, b.shape)
    rows = np.flatnonzero(np.any((a != b).reshape(len(a), -1), axis=1))
    if not rows.size:
        return None
    k = int(rows[0])
    c = int(np.flatnonzero((a[k] != b[k]).reshape(-1))[0])
    gv, wv = np.asarray(got)[k].reshape(-1)[c], np.asarray(want)[k].reshape(-1)[c]
    where = "step %d" % k if np.asarray(got)[k].size == 1 else "step %d, column %d" % (k, c)
    msg = "first difference at %s: %s against %s; %d of %d steps differ" % (where, _val(gv), _val(wv), rows.size, len(a))
    if resamples is not None:
        msg += "; resample counts %d against %d" % tuple(resamples)
    return msg


def state_mismatch(got, want):
    """None if the final-state arrays are bit-identical; otherwise how many entries differ and the index of the first one."""
    a, b = _bits(got), _bits(want)
    if a.shape != b.shape:
        return "shapes differ: %s against %s" % (a.shape, b.shape)
    d = np.flatnonzero((a != b).reshape(-1))
    if not d.size:
        return None
    i = np.unravel_index(int(d[0]), a.shape)
    return "%d of %d entries differ, the first at index %s: %s against %s" % (
        d.size, a.size, tuple(int(v) for v in i), _val(np.asarray(got)[i]), _val(np.asarray(want)[i]))


def assert_steps_equal(got, want, what="ll_steps", resamples=None):
    msg = step_mismatch(got, want, resamples)
    assert msg is None, "%s: %s" % (what, msg)


def assert_state_equal(got, want, what):
    msg = state_mismatch(got, want)
    assert msg is None, "%s differ: %s" % (what, msg)


def compare_state(g, o, exact=True, we_rtol=0.0):
    xg, xo = g.particles(), o.particles()
    wg, wo = g.weights(), o.weights()
    eg, eo = g.expweights(), o.expweights()
    if exact:
        assert_state_equal(xg, xo, "particles")
        assert_state_equal(wg, wo, "log-weights")
        assert_state_equal(eg, eo, "exp-weights")
        assert_state_equal(g.ancestors(), o.ancestors(), "ancestors")
    else:
        np.testing.assert_allclose(xg, xo, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(eg, eo, rtol=we_rtol, atol=1e-300)


EPS = np.finfo(np.float64).eps / 2         # unit roundoff of fp64
_LOG2PI = np.log(np.longdouble(2) * np.longdouble("3.14159265358979323846264338327950288"))


def independent_correct(model, x, w, y):
    """One correct! of a linear-Gaussian model (measurement C x, density N(mu, Sigma) with a scalar or diagonal Sigma) evaluated in
    np.longdouble (64-bit significand) from the fp64 particles x [N, nx], the fp64 log-weights w [N] and the model's constants: it
    shares nothing with the engine's arithmetic (csrc/shared/llpf_detmath.h, llpf_fixed.h) or with the oracle.
    Returns (ll, log_we, scale): the log-likelihood increment logsumexp(w + logpdf(y - C x)), the logs of the normalised
    exp-weights log we_i = w_i + logpdf_i - ll, and for every particle the size of what an fp64 evaluation of log we_i rounds,
        scale_i = |w_i| + |logpdf_i| + |log we_i| + |ll| + sum_k |v_k| (|y_k| + (|C| |x_i|)_k + |mu_k|) / Sigma_kk + 1,
    v = y - C x_i - mu: the terms of w_i + logpdf_i - ll, and the cancellation in v, which moves q/2 = sum v_k^2 / (2 Sigma_kk) by
    |v_k| / Sigma_kk times v_k's own rounding.  An fp64 evaluation makes |d log we_i| <= c u scale_i with a small count c of roundings
    per term (u = 2^-53); relative error of we_i = |d log we_i| to first order."""
    ld = np.longdouble
    nx, ny = model.nx, model.ny
    g = model.measurement_density
    if g.kind == S.COV_SCAL:
        var = np.full(ny, g.cov[0], dtype=ld)
    elif g.kind == S.COV_DIAG:
        var = np.array(g.cov[:ny], dtype=ld)
    else:
        raise ValueError("independent_correct: scalar or diagonal measurement covariance only")
    Cm = np.array(model.C[:ny * nx], dtype=np.float64).reshape(ny, nx)
    mu = np.array(g.mu[:ny], dtype=ld)
    yl = np.asarray(y, dtype=ld).reshape(ny)
    xl = np.asarray(x, dtype=ld)
    cx = np.zeros((len(xl), ny), dtype=ld)
    for r in range(ny):
        for c in range(nx):
            cx[:, r] += ld(Cm[r, c]) * xl[:, c]
    v = (yl - cx) - mu
    lp = -(ny * _LOG2PI + np.sum(np.log(var))) / 2 - np.sum(v * v / var, axis=1) / 2
    a = np.asarray(w, dtype=ld) + lp
    m = np.max(a)
    ll = m + np.log(np.sum(np.exp(a - m)))
    log_we = a - ll
    canc = np.sum(np.abs(v) * (np.abs(yl) + np.abs(x) @ np.abs(Cm).T + np.abs(mu)) / var, axis=1)
    scale = np.abs(np.asarray(w, dtype=ld)) + np.abs(lp) + np.abs(log_we) + abs(ll) + canc + 1
    return ll, log_we, scale.astype(np.float64)


def teacher_forced_ancestor_mismatches(cfg, U, Y, steps, t_index0=1.0, threads=None, independent=False, engine=None):
    """the engine against the REFERENCE-ORDER oracle (libm exp, pairwise sum, serial fp64 cumsum, two-pointer search:
    src/utils.jl:18-27, src/resample.jl:17-36) at full size.  A particle filter is chaotic in its ancestry, so the two are compared
    step by step from the SAME state: the reference-order state (particles, log-weights) is installed in the engine
    (llpf_set_particles / llpf_set_weights) before every correct! and again before every predict!; both sides then take that step
    with the same measurement / the same Philox draws, and the oracle alone carries the recursion on.  Compared: the log-likelihood
    increment and the normalised exp-weights of every correct! (the stated fp64 tolerance: |dll| <= 1e-10, rel <= 1e-12), the
    ancestor vectors of every resampling predict!, and the propagated particles of every output whose ancestor agrees.
    Returns dict(steps, resampling_steps, mismatches_total, mismatches_per_step_max, steps_with_mismatch,
    particles_equal_on_matching_ancestors, correct_steps, ll_abs_err_max, expweights_rel_err_max).
    threads: OpenMP threads of the reference-order oracle (its results do not depend on them; 1 again afterwards).
    independent (linear-Gaussian models, see independent_correct): every correct! is also evaluated in np.longdouble from the same
    fp64 state, which adds the keys indep_ll_abs_err_max (|ll - ll_longdouble|), indep_expweights_rel_err_max and
    indep_expweights_bound_ratio_max, the largest |we_i / we_i,longdouble - 1| / (u scale_i) over particles and steps (we_i > 1e-290).
    engine: the filter under test (default: a FilterHandle of cfg)."""
    import oracle_binding as ob
    from llpf_amd import _capi
    g = _capi.FilterHandle(cfg) if engine is None else engine
    if threads:
        ob.set_threads(threads)
    try:
        r = ob.OracleFilter(cfg, ob.ORDER_REFERENCE)
        g.reset(); r.reset()
        out = _teacher_forced(g, r, cfg, U, Y, steps, t_index0, independent)
    finally:
        if threads:
            ob.set_threads(1)
    return out


def _teacher_forced(g, r, cfg, U, Y, steps, t_index0, independent):
    Ts = cfg.model.Ts
    tot = worst = nsteps = nres = ncorr = 0
    same_x = True
    dll = dwe = 0.0
    ill = iwe = iratio = 0.0
    for k in range(steps):
        t = (t_index0 + k) * Ts
        u = U[k] if U is not None and len(U) else None
        x0, w0 = r.particles(), r.weights()
        g.set_particles(x0)                         # correct! from the same state on both sides
        g.set_weights(w0)
        ll_g = g.correct(u, Y[k], t)
        ll_r = r.correct(u, Y[k], t)
        if not np.any(np.isnan(Y[k])):
            ncorr += 1
            dll = max(dll, abs(ll_g - ll_r))
            eg, er = g.expweights(), r.expweights()
            nz = er > 1e-290
            dwe = max(dwe, float(np.max(np.abs(eg[nz] - er[nz]) / er[nz])))
            if independent:
                ll_i, lwe_i, scale = independent_correct(cfg.model, x0, w0, Y[k])
                ill = max(ill, float(abs(np.longdouble(ll_g) - ll_i)))
                we_i = np.exp(lwe_i)
                nz = we_i > 1e-290
                rel = np.abs((eg[nz] / we_i[nz]) - 1).astype(np.float64)
                iwe = max(iwe, float(np.max(rel)))
                iratio = max(iratio, float(np.max(rel / (EPS * scale[nz]))))
        g.set_weights(r.weights())                  # predict! from the same state (particles are unchanged by correct!)
        g.predict(u, t)
        r.predict(u, t)
        if not r.last_resampled():
            assert not g.last_resampled()
            continue
        nres += 1
        jg, jr = g.ancestors(), r.ancestors()
        diff = jg != jr
        m = int(np.sum(diff))
        tot += m
        worst = max(worst, m)
        nsteps += 1 if m else 0
        xg, xr = g.particles(), r.particles()
        same_x = same_x and bool(np.array_equal(xg[~diff], xr[~diff]))
    return {"steps": int(steps), "resampling_steps": int(nres), "mismatches_total": int(tot), "mismatches_per_step_max": int(worst),
            "steps_with_mismatch": int(nsteps), "particles_equal_on_matching_ancestors": same_x,
            "correct_steps": int(ncorr), "ll_abs_err_max": float(dll), "expweights_rel_err_max": float(dwe),
            **({"indep_ll_abs_err_max": ill, "indep_expweights_rel_err_max": iwe, "indep_expweights_bound_ratio_max": iratio}
               if independent else {})}
