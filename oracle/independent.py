"""oracle/independent.py — a SECOND, independent CPU restatement of the hot path, in plain numpy.

TEST INFRASTRUCTURE ONLY (imported by tests/ and tests/golden/make_independent.py; never by the product).

Why it exists.  oracle/llpf_oracle.c shares headers with the engine (csrc/shared/: the deterministic exp / log, the fixed-point
sums, Philox, and — for the Rao-Blackwellized filter with per-particle covariance — the whole Kalman recursion body
llpf_rbfull_body.h).  A wrong sign in that shared Riccati update would be bit-identical on both sides.  This file shares
NOTHING with the engine except the random numbers it is fed: plain 2-D numpy arrays, numpy.linalg.cholesky / solve, libm-grade
numpy exp / log, Python loops over particles.  It follows the reference line by line:

  particle filter      reset!              src/filtering.jl:4-14
                       correct!            src/filtering.jl:164-168 = measurement_equation! src/PFtypes.jl:107-120 + logsumexp!
                                           src/utils.jl:18-27 (sum_all_but :66-71)
                       predict!            src/filtering.jl:140-153 = shouldresample src/resample.jl:5-10, resample
                                           (systematic :17-36, stratified :38-61), propagate_particles! src/PFtypes.jl:122-139,
                                           reset_weights! src/utils.jl:73-79
                       forward_trajectory  src/filtering.jl:343-365;  loglik src/smoothing.jl:227-230
                       Gaussian logpdf     src/utils.jl:252-257;  rk4 src/utils.jl:220-237;  quad-tank examples/example_quadtank.jl:8-35
  residual resampling  resample(ResampleResidual, ...) src/resample.jl:63-117 (resample_residual): stand-alone, as a ParticleFilter's
                       strategy, and under the auxiliary filter; with the margins of its floor / u < bin decisions in numpy.longdouble
                       and how far an fp64 or fixed-point implementation may be from them (residual_slack)
  auxiliary filter     AuxiliaryParticleFilter src/PFtypes.jl:38-49: correct! src/filtering.jl:170-174, predict! :195-217 (lambda from the
                       next measurement, expnormalize! src/utils.jl:57-63, w = lambda[i] - log N), over an AdvancedParticleFilter
                       :219-234 (lambda only chooses the ancestors; propagated again from xprev[j]), forward_trajectory :367-384,
                       loglik src/smoothing.jl:232-236
  RBPF, !singleR       reset! src/rbpf.jl:146-160, predict! :163-232, correct! :235-283 with
                       correct!(kf, ...) src/filtering.jl:100-128
  FFBS smoother        one backward step of smooth, src/smoothing.jl:128-141, draw_one_categorical src/resample.jl:128-152: the
                       distribution of every draw in numpy.longdouble (smoother_backward_step) and how far an fp64 implementation
                       may be from it (backward_step_slack), at the end of this file

The reference's own random streams (Xoshiro randn, global rand()) are unpinned by its tests; the normals and uniforms are
INPUTS here (callables `normals(step, n, nd)` / `uniforms(step, n)`), supplied by the tests from the Philox generator that the
Random123 known-answer vectors pin (tests/test_detmath.py).  Rounding differs from the C oracle's reference order only through
operation order inside numpy (BLAS dot products, pairwise sums): agreement is asserted at 1e-10 per step, observed ~1e-13.
"""
import math

import numpy as np

LOG2PI = math.log(2.0 * math.pi)


# ---- Gaussian pieces (src/utils.jl:241-270) ---------------------------------------------------------------------------------
class Gaussian:
    def __init__(self, mu, Sigma):
        self.mu = np.asarray(mu, dtype=np.float64).reshape(-1)
        k = self.mu.size
        S = np.asarray(Sigma, dtype=np.float64)
        if S.ndim == 0:
            S = float(S) * np.eye(k)
        elif S.ndim == 1:
            S = np.diag(S)
        self.Sigma = S.reshape(k, k)
        self.L = np.linalg.cholesky(self.Sigma)

    def logpdf(self, x):
        """extended_logpdf(d, x) = mvnormal_c0(d) - invquad(Sigma, x - mu) / 2, src/utils.jl:252-257; x: (..., k)"""
        d = np.atleast_2d(x) - self.mu
        k = self.mu.size
        logdet = 2.0 * np.sum(np.log(np.diag(self.L)))
        z = np.linalg.solve(self.Sigma, d.T).T
        return -(k * LOG2PI + logdet) / 2.0 - np.sum(d * z, axis=1) / 2.0

    def sample(self, xi):
        """rand(rng, d) = mu + cholesky(Sigma).L * randn, src/utils.jl:260; xi: (n, k) standard normals"""
        return self.mu + np.atleast_2d(xi) @ self.L.T


class Laplace:
    """independent Laplace components of scale b: a measurement density other than a Gaussian (the reference weights with
    logpdf of any Distribution, ext/LowLevelParticleFiltersDistributionsExt.jl:80, or with a measurement_likelihood callable,
    src/PFtypes.jl:226-239)"""

    def __init__(self, b):
        self.b = float(b)

    def logpdf(self, v):
        v = np.atleast_2d(v)
        return -np.sum(np.abs(v), axis=1) / self.b - v.shape[1] * math.log(2.0 * self.b)


class StudentT:
    """independent Student-t components, nu degrees of freedom, scale sigma"""

    def __init__(self, nu, sigma):
        self.nu, self.sigma = float(nu), float(sigma)
        self.c1 = math.lgamma((self.nu + 1.0) / 2.0) - math.lgamma(self.nu / 2.0) - 0.5 * math.log(self.nu * math.pi) - math.log(self.sigma)

    def logpdf(self, v):
        v = np.atleast_2d(v)
        return np.sum(self.c1 - (self.nu + 1.0) / 2.0 * np.log1p((v / self.sigma) ** 2 / self.nu), axis=1)


# ---- process noise / initial densities other than a Gaussian ---------------------------------------------------------------
# The reference's AdvancedParticleFilter hands the noise to the user — x[i] = dynamics(xprev[j[i]], u, p, t, true) adds its own
# (src/PFtypes.jl:242-259, test/runtests.jl:553-599) — and its ParticleFilter draws from ANY dynamics_density / initial_density
# (rand!(rng, d, noise) src/PFtypes.jl:135, rand(rng, initial_density) src/filtering.jl:8).  The draws are inputs here too: per
# particle, nx standard normals xi and nx uniforms uu in [0, 1).
class MultiplicativeGaussianNoise:
    """x' = f(x) + (s0 + s1 |x|) .* xi : Gaussian noise whose standard deviation grows with the state it leaves"""

    def __init__(self, s0, s1):
        self.s0, self.s1 = float(s0), float(s1)

    def propagate(self, x, fx, xi, uu):
        return fx + (self.s0 + self.s1 * np.abs(x)) * xi


class LaplaceNoise:
    """x' = f(x) + Laplace(0, b) per component, drawn through the inverse CDF of one uniform each"""

    def __init__(self, b):
        self.b = float(b)

    def propagate(self, x, fx, xi, uu):
        v = 2.0 * uu - 1.0
        t = np.maximum(1.0 - np.abs(v), 2.0 ** -53)
        return fx + np.sign(v) * self.b * (-np.log(t))


class UniformBox:
    """initial density: independent uniforms on [lo_d, hi_d]"""

    def __init__(self, lo, hi):
        self.lo, self.hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)

    def sample_u(self, xi, uu):
        return self.lo + (self.hi - self.lo) * uu


# ---- models -------------------------------------------------------------------------------------------------------------------
class LinearModel:
    """dynamics A x + B u, measurement C x (examples/example_lineargaussian.jl:28-29)"""

    def __init__(self, A, B, C):
        self.A, self.C = np.atleast_2d(A), np.atleast_2d(C)
        self.B = np.zeros((self.A.shape[0], 0)) if B is None else np.asarray(B, dtype=np.float64).reshape(self.A.shape[0], -1)

    def f(self, x, u, t):
        out = x @ self.A.T
        if self.B.shape[1]:
            u = np.asarray(u)
            out = out + self.B @ (u if u.dtype == np.longdouble else u.astype(np.float64)).reshape(-1)
        return out

    def g(self, x, u, t):
        return x @ self.C.T


class QuadTank:
    """examples/example_quadtank.jl:8-35 through rk4(f, Ts; supersample) of src/utils.jl:220-237"""

    def __init__(self, k1=1.6, k2=1.6, g=9.81, A=(4.9, 4.9, 4.9, 4.9), a=(0.03, 0.03, 0.03, 0.03), gamma=(0.2, 0.2),
                 tswitch=500.0, a1factor=2.0, eps=1e-3, Ts=1.0, supersample=2):
        self.k1, self.k2, self.grav, self.A, self.a, self.gamma = k1, k2, g, A, a, gamma
        self.tswitch, self.a1factor, self.eps, self.Ts, self.ss = tswitch, a1factor, eps, Ts, supersample

    def rhs(self, h, u, t):
        A1, A2, A3, A4 = self.A
        a1, a2, a3, a4 = self.a
        if t > self.tswitch:
            a1 = a1 * self.a1factor
        g1, g2 = self.gamma
        s = np.sqrt(np.maximum(2.0 * self.grav * h, 0.0) + self.eps)          # ssqrt(x) = sqrt(max(x, 0) + 1e-3)
        return np.stack([
            -a1 / A1 * s[:, 0] + a3 / A1 * s[:, 2] + g1 * self.k1 / A1 * u[0],
            -a2 / A2 * s[:, 1] + a4 / A2 * s[:, 3] + g2 * self.k2 / A2 * u[1],
            -a3 / A3 * s[:, 2] + (1.0 - g2) * self.k2 / A3 * u[1],
            -a4 / A4 * s[:, 3] + (1.0 - g1) * self.k1 / A4 * u[0]], axis=1)

    def f(self, x, u, t):
        Tss = self.Ts / self.ss
        for _ in range(self.ss):
            f1 = self.rhs(x, u, t)
            f2 = self.rhs(x + Tss / 2.0 * f1, u, t + Tss / 2.0)
            f3 = self.rhs(x + Tss / 2.0 * f2, u, t + Tss / 2.0)
            f4 = self.rhs(x + Tss * f3, u, t + Tss)
            x = x + Tss / 6.0 * (f1 + 2.0 * f2 + 2.0 * f3 + f4)
            t = t + Tss
        return x

    def g(self, x, u, t):
        return x[:, :2]


# ---- logsumexp! and the resamplers --------------------------------------------------------------------------------------------
def logsumexp_inplace(w):
    """ll = logsumexp!(w, we), src/utils.jl:18-27: offset = maximum, s = sum of all but the maximum's exp(0) = 1"""
    imax = int(np.argmax(w))
    m = w[imax]
    w = w - m
    we = np.exp(w)
    we_wo = we.copy()
    we_wo[imax] -= 1.0
    s = float(np.sum(we_wo))
    we = we * (1.0 / (s + 1.0))
    w = w - math.log1p(s)
    return w, we, math.log1p(s) + m


def resample_systematic(we, jprev, U, M=None):
    """src/resample.jl:17-36: bins = cumsum(we); r = rand() * bins[end] / N; s_i = r + (i-1)/M; j[i] = first b with s_i < bins[b],
    entries whose threshold is never met keep their previous value"""
    N = we.size
    M = N if M is None else M
    bins = np.cumsum(we)
    r = U * bins[-1] / N
    s = r + np.arange(M) * (1.0 / M)
    j = np.searchsorted(bins, s, side="right")
    keep = j >= N
    j = np.where(keep, jprev[:M], j)
    return j.astype(np.int64), bins


def resample_stratified(we, jprev, Us, M=None):
    """src/resample.jl:38-61: u_i = (i - 1 + rand()) / M * bins[end]"""
    N = we.size
    M = N if M is None else M
    bins = np.cumsum(we)
    s = (np.arange(M) + Us[:M]) / M * bins[-1]
    j = np.searchsorted(bins, s, side="right")
    keep = j >= N
    j = np.where(keep, jprev[:M], j)
    return j.astype(np.int64), bins


def resample_residual(we, jprev, U, M=None):
    """src/resample.jl:63-117: we is normalised by its sum (:66-69); nw_i = we_i M; particle i is written floor(nw_i) times, in particle
    order, into j[0..num-1] (:75-84); num == M returns (:86-88); otherwise the residuals nw_i - floor(nw_i) are normalised by their sum
    (:90-98) and summed cumulatively (:100-103), and output m = num..M-1 takes the first i with U[m] < bins[i] (:105-114) — the reference
    draws one rand() per remaining output in order, and U is indexed by OUTPUT, so U[0..num-1] are never read; an output whose uniform
    is below no bin keeps jprev[m].
    Returns (j, info).  Both kinds of decision are comparisons of real numbers with an edge, and an implementation in other arithmetic
    may decide a call within rounding of its edge the other way; info says how close the calls of this resampling were, in
    numpy.longdouble from the fp64 weights:
      int_margin    min over the particles with nw_i >= 1/2 of |nw_i - round(nw_i)| (inf if there is none).  An nw_i below 1/2 has 0 as
                    its nearest integer and floors to 0 whichever way it is rounded: no call.
      edge_margin   min over the uniforms that are read of the distance to the nearest bin edge bins[0..N-1]; the last one, 1, is counted
                    too, since a uniform at or above a computed bins[N-1] = 1 - ulp keeps jprev (inf if no uniform is read).
      num, nw_max, R = M - num: what residual_slack scales with.
    A single particle is no call either: nw_0 = we_0 / we_0 M = M in any arithmetic (x / x = 1 exactly; q M / q for the quanta)."""
    we = np.asarray(we, dtype=np.float64)
    N = we.size
    M = N if M is None else M
    nw = we / np.sum(we) * M
    cnt = np.floor(nw).astype(np.int64)
    j = np.array(jprev[:M], dtype=np.int64)
    copies = np.repeat(np.arange(N), cnt)[:M]
    num = copies.size
    j[:num] = copies
    nwl = np.asarray(we, dtype=LD) / np.sum(np.asarray(we, dtype=LD)) * M
    big = nwl >= 0.5
    info = dict(num=num, R=M - num, nw_max=float(np.max(nw)), edge_margin=np.inf,
                int_margin=float(np.min(np.abs(nwl[big] - np.rint(nwl[big])))) if N > 1 and np.any(big) else np.inf)
    if num == M:
        return j, info
    res = nw - cnt
    bins = np.cumsum(res / np.sum(res))
    u = np.asarray(U, dtype=np.float64)[num:M]
    i = np.searchsorted(bins, u, side="right")
    met = i < N
    j[num:M][met] = i[met]
    resl = nwl - cnt
    binsl = np.cumsum(resl) / np.sum(resl)
    k = np.clip(np.searchsorted(binsl, u.astype(LD), side="left"), 1, N - 1) if N > 1 else np.zeros(u.size, dtype=np.int64)
    info["edge_margin"] = float(np.min(np.minimum(np.abs(binsl[k] - u), np.abs(binsl[k - 1] - u))))
    return j, info


def residual_slack(N, M, total, nw_max, R):
    """(slack_int, slack_edge): how far the numbers an fp64 or a fixed-point implementation of resample_residual decides on can lie from
    the long-double nw_i and bins_i that resample_residual's margins are measured with.  Derived, not fitted:

      quanta.  The engine replaces e_i (the exp-weights before normalisation, 0 <= e_i <= 1, sum E = `total`) by q_i = floor(e_i 2^K),
      K = qbits(N): q_i = e_i 2^K - d_i, 0 <= d_i < 1, Q = sum q_i = E 2^K - D, 0 <= D < N.  Its nw'_i = M q_i / Q is exact in integers, and
          nw'_i - nw_i = (nw_i D - M d_i) / Q   lies in (-M / Q, N nw_i / Q):   |dnw_i| <= max(M, N nw_max) / Q,  Q > E 2^K - N.
      The cumulative sums C_i of the residuals (equal copy counts: that is what int_margin > slack_int secures) then move by less than
      N M / Q (sum_i nw_i = M), and the engine keeps only K bits of each residual (rem >> ceil(log2 N), less than 2 N / Q each in units
      of nw): |dC_i| <= (N M + 2 N^2) / Q =: c for every partial sum and for their total, which is R = M - num exactly (sum nw_i = M,
      sum floor(nw_i) = num): bins_i = C_i / R <= 1 moves by at most (c + c bins_i) / (R - c) <= 2 c / (R - c).
      `total`: the engine normalises against an analytic bound of the log-weights and accepts any E >= 2^-10 (below that it repeats the
      step with the exact maximum, E >= 1); stand-alone calls are handed normalised weights, E = 1.
      fp64 (the reference order).  we_i / sum * M: the serial sum of N terms carries (N - 1) roundings, the division and the product
      one each: |dnw_i| <= (N + 2) 2^-53 nw_i.  The residuals inherit that absolutely, sum (N + 2) 2^-53 M over all particles, relative to
      their total R; the normalisation, the serial cumulative sum (N roundings on numbers <= 1) and the reciprocal add 2 N + 8 roundings.
    Terms of second order are dropped."""
    Q = total * 2.0 ** qbits(N) - N
    c = (N * M + 2.0 * N * N) / Q
    slack_int = max(M, N * nw_max) / Q + (N + 2) * U53 * nw_max
    slack_edge = (2 * c / (R - c) + (2 * (N + 2) * M / R + 2 * N + 8) * U53) if R > 0 else 0.0
    return slack_int, slack_edge


def _peak(d):
    """the largest value a measurement density takes (all densities here are unimodal about their mean, or about 0)"""
    return float(d.logpdf(d.mu if hasattr(d, "mu") else np.zeros((1, 1)))[0])


def engine_total(s1, m, off):
    """the sum E of the exp-weights the engine cuts into quanta (residual_slack's `total`) when the restatement's own normalisation found
    s1 = sum exp(w - m), m = max w: the engine subtracts the bound `off` >= m in place of m unless that leaves E < 2^-10, and then uses m.
    The bound's own rounding is covered by taking the smaller of the two near the switch."""
    Eb = s1 * math.exp(m - off) * (1.0 - 1e-9)
    return Eb if Eb >= 2.0 ** -10 * (1.0 - 1e-8) else s1


# ---- the particle filter ----------------------------------------------------------------------------------------------------
class ParticleFilter:
    def __init__(self, N, model, df, dg, d0, resample_threshold=0.1, stratified=False, Ts=1.0, residual=False):
        self.N, self.model, self.df, self.dg, self.d0 = N, model, df, dg, d0
        self.thr, self.stratified, self.residual, self.Ts = resample_threshold, stratified, residual, Ts
        self.j = np.arange(N)
        self.calls = []                     # residual resampling: info of every call, with the slack that goes with it

    def reset(self, xi, uu=None):
        self.x = self.d0.sample_u(xi, uu) if hasattr(self.d0, "sample_u") else self.d0.sample(xi)      # x_i ~ d0
        self.w = np.full(self.N, -math.log(self.N))
        self.we = np.full(self.N, 1.0 / self.N)
        self.wbound = -math.log(self.N)     # what the engine knows the log-weights to lie below (engine_total)
        self.t = 1

    def correct(self, u, y, t):
        has_y = y is not None and not np.any(np.isnan(y))        # any(ismissing, y) && return, src/PFtypes.jl:109
        if has_y:
            self.w = self.w + self.dg.logpdf(np.asarray(y, dtype=np.float64) - self.model.g(self.x, u, t))
        m = float(np.max(self.w))
        self.w, self.we, ll = logsumexp_inplace(self.w)
        if self.residual:
            self.total = engine_total(math.exp(ll - m), m, self.wbound + (_peak(self.dg) if has_y else 0.0))
            self.wbound = float(np.max(self.w))
        return ll

    def resample(self, we, U):
        """j = resample(strategy, we, j, bins), src/resample.jl:12"""
        if self.residual:
            self.j, info = resample_residual(we, self.j, U)
            s = residual_slack(self.N, self.N, self.total, info["nw_max"], info["R"])
            self.calls.append(dict(info, slack_int=s[0], slack_edge=s[1], total=self.total))
        elif self.stratified:
            self.j, self.bins = resample_stratified(we, self.j, U)
        else:
            self.j, self.bins = resample_systematic(we, self.j, float(U[0]))

    def propagate(self, xprev, u, t, xi, uu):
        if hasattr(self.df, "propagate"):                        # the model adds its own noise (PFtypes.jl:254 / any dynamics_density, :135)
            return self.df.propagate(xprev, self.model.f(xprev, u, t), xi, uu)
        return self.model.f(xprev, u, t) + self.df.sample(xi)

    def reset_weights(self):
        """src/utils.jl:73-79"""
        self.w = np.full(self.N, math.log(1.0 / self.N))
        self.we = np.full(self.N, 1.0 / self.N)
        self.wbound = math.log(1.0 / self.N)

    def predict(self, u, t, xi, U, uu=None):
        N = self.N
        ess = 1.0 / float(np.sum(self.we * self.we))
        self.resampled = self.thr == 1.0 or ess < N * self.thr
        if self.resampled:
            self.resample(self.we, U)
            xprev = self.x[self.j]
            self.reset_weights()
        else:
            self.j = np.arange(N)
            xprev = self.x
        self.x = self.propagate(xprev, u, t, xi, uu)
        self.t += 1

    def run(self, U, Y, t_index0, normals, uniforms, step0=0, user_uniforms=None):
        """T iterations of correct!(u_k, y_k, t_k); predict!(u_k, t_k), t_k = (t_index0 + k) Ts: forward_trajectory
        (t_index0 = 0) / loglik (t_index0 = 1).  normals(step, n, nd), uniforms(step, n): the draws of predict! number `step`."""
        T = len(Y)
        ll_steps = np.zeros(T)
        nres = 0
        for k in range(T):
            t = (t_index0 + k) * self.Ts
            u = U[k] if U is not None and len(U) else None
            ll_steps[k] = self.correct(u, Y[k], t)
            uu = user_uniforms(step0 + k, self.N, self.x.shape[1]) if user_uniforms is not None else None
            self.predict(u, t, normals(step0 + k, self.N, self.x.shape[1]), uniforms(step0 + k, self.N), uu)
            nres += int(self.resampled)
        return ll_steps, nres


# ---- the auxiliary particle filter ------------------------------------------------------------------------------------------
def expnormalize(w):
    """expnormalize!(w), src/utils.jl:57-63: exp(w - maximum) scaled by 1 / (1 + sum of all but the maximum's exp(0) = 1)"""
    imax = int(np.argmax(w))
    we = np.exp(w - w[imax])
    we_wo = we.copy()
    we_wo[imax] -= 1.0
    s = float(np.sum(we_wo))
    return we * (1.0 / (s + 1.0)), s + 1.0


class AuxiliaryParticleFilter:
    """AuxiliaryParticleFilter(pf), src/PFtypes.jl:38-49, over a ParticleFilter above; `advanced`: that filter's noise is the model's own
    (the AdvancedParticleFilter contract), which selects predict! of src/filtering.jl:219-234 in place of :195-217"""

    def __init__(self, pf, advanced=False):
        self.pf, self.advanced = pf, advanced

    def reset(self, xi, uu=None):
        self.pf.reset(xi, uu)

    def correct(self, u, y, t):
        """src/filtering.jl:170-174: the measurement was weighed in by the predict! before, what is left is ll = logsumexp!(w, we) —
        so u, y and t are not used, and the y of the very first call never is"""
        pf = self.pf
        pf.w, pf.we, ll = logsumexp_inplace(pf.w)
        pf.wbound = float(np.max(pf.w))
        return ll

    def new_weights(self, lam, j):
        """src/filtering.jl:209-213: "note unresampled lambda[i] instead of lambda[j[i]]" """
        return lam - math.log(self.pf.N)

    def source(self, xprev, xpred):
        """what the advanced variant propagates again, src/filtering.jl:228: propagate_particles!(pf.pf, u, j, p, t) reads xprev[j]"""
        return xprev

    def predict(self, u, y1, t, xi, U, uu=None):
        """src/filtering.jl:195-217 (over an AdvancedParticleFilter :219-234); y1: the NEXT measurement"""
        pf = self.pf
        xprev = pf.x
        xpred = pf.model.f(xprev, u, t)                          # propagate_particles!(pf.pf, u, p, t, nothing): no noise, PFtypes.jl:261-274
        has_y = y1 is not None and not np.any(np.isnan(y1))
        lam = np.zeros(pf.N)                                     # lambda .= 0; measurement_equation!(pf.pf, u, y1, p, t, lambda), :201-203
        if has_y:
            lam = lam + pf.dg.logpdf(np.asarray(y1, dtype=np.float64) - pf.model.g(xpred, u, t))
        w = pf.w + lam                                           # s.w .+= lambda, :204
        we, s1 = expnormalize(w)                                 # :205
        if pf.residual:
            m = float(np.max(w))
            pf.total = engine_total(s1, m, pf.wbound + (_peak(pf.dg) if has_y else 0.0))
        pf.resample(we, U)                                       # :206, with whatever strategy the wrapped filter has
        pf.resampled = True
        if self.advanced:                                        # lambda has chosen the ancestors and is dropped
            pf.reset_weights()                                   # :226
            pf.x = pf.propagate(self.source(xprev, xpred)[pf.j], u, t, xi, uu)      # :228, with noise and permutation
        else:
            pf.x = xpred[pf.j] + pf.df.sample(xi)                # permute_with_buffer!, src/utils.jl:81-86; add_noise!, src/PFtypes.jl:143-155
            pf.w = self.new_weights(lam, pf.j)
            pf.we = lam                                          # the reference's `we` is the buffer lambda lives in
            if pf.residual:                                      # lambda <= the density's peak: what the engine bounds these weights by
                pf.wbound = (_peak(pf.dg) if has_y else 0.0) - math.log(pf.N)
        pf.t += 1

    def run(self, U, Y, mode, normals, uniforms, t_index0=0.0, step0=0, user_uniforms=None):
        """mode 0: forward_trajectory(pf::AuxiliaryParticleFilter, u, y), src/filtering.jl:367-384: correct! at every step, predict! with
        y[k + 1] between them.  mode 1: loglik, src/smoothing.jl:232-236: T - 1 updates pf(u[k], y[k], y[k + 1]), then the WRAPPED filter's
        update! (correct! and predict!) on the last pair.  Every predict! takes one draw number, step0 + k."""
        pf = self.pf
        T = len(Y)
        ll_steps = np.zeros(T)
        nres = 0
        for k in range(T):
            t = (t_index0 + k) * pf.Ts
            u = U[k] if U is not None and len(U) else None
            nd = pf.x.shape[1]
            last = mode == 1 and k == T - 1
            ll_steps[k] = pf.correct(u, Y[k], t) if last else self.correct(u, Y[k], t)
            if not last and k == T - 1:
                break
            uu = user_uniforms(step0 + k, pf.N, nd) if user_uniforms is not None else None
            xi, Us = normals(step0 + k, pf.N, nd), uniforms(step0 + k, pf.N)
            if last:
                pf.predict(u, t, xi, Us, uu)
            else:
                self.predict(u, Y[k + 1], t, xi, Us, uu)
            nres += int(pf.resampled)
        return ll_steps, nres


# ---- Rao-Blackwellized filter, every particle its own Kalman filter ----------------------------------------------------------------
class RBPF:
    """xn' = f_n(xn, u) + An(xn) xl + wn,  xl' = Al xl + Bl u + wl,  y = g(xn) + Cl xl + e;  An(xn) = An[0] + sum_k xn[k] An[1 + k]"""

    def __init__(self, N, fn_model, An, Al, Bl, Cl, R1n, R1l, R2, d0n, d0l, resample_threshold=0.1, stratified=False, Ts=1.0):
        self.N, self.fn, self.An = N, fn_model, np.asarray(An, dtype=np.float64)
        self.Al, self.Cl = np.atleast_2d(Al), np.atleast_2d(Cl)
        self.Bl = np.zeros((self.Al.shape[0], 0)) if Bl is None else np.asarray(Bl, dtype=np.float64).reshape(self.Al.shape[0], -1)
        self.R1n, self.R1l, self.R2, self.d0n, self.d0l = R1n, np.atleast_2d(R1l), R2, d0n, d0l
        self.thr, self.stratified, self.Ts = resample_threshold, stratified, Ts
        self.j = np.arange(N)

    def coupling(self, xn):
        return self.An[0] + np.tensordot(xn, self.An[1:], axes=(0, 0))

    def reset(self, xi):
        N, nl = self.N, self.Al.shape[0]
        self.xn = self.d0n.sample(xi)
        self.xl = np.tile(self.d0l.mu, (N, 1))                   # xl = copy(pf.kf.d0.mu), R = copy(pf.kf.d0.Sigma), :151-152
        self.R = np.tile(self.d0l.Sigma, (N, 1, 1))
        self.w = np.full(N, -math.log(N))
        self.we = np.full(N, 1.0 / N)
        self.t = 1

    def correct(self, u, y, t):
        if y is not None and not np.any(np.isnan(y)):
            y = np.asarray(y, dtype=np.float64)
            yn = self.fn.g(self.xn, u, t)
            C = self.Cl
            I = np.eye(self.Al.shape[0])
            for i in range(self.N):                              # correct!(kf, u, y - yn), src/filtering.jl:100-128
                R = self.R[i]
                e = (y - yn[i]) - C @ self.xl[i]
                S = C @ R @ C.T
                S = (S + S.T) / 2.0 + self.R2.Sigma               # symmetrize(Ct R Ct') .+ R2
                Sc = np.linalg.cholesky(S)
                K = np.linalg.solve(S, (R @ C.T).T).T            # (R Ct') / S
                self.xl[i] = self.xl[i] + K @ e
                Rn = (I - K @ C) @ R
                self.R[i] = (Rn + Rn.T) / 2.0                    # symmetrize((I - K Ct) R)
                logdet = 2.0 * np.sum(np.log(np.diag(Sc)))
                self.w[i] += -(e.size * LOG2PI + logdet) / 2.0 - float(e @ np.linalg.solve(S, e)) / 2.0
        self.w, self.we, ll = logsumexp_inplace(self.w)
        return ll

    def predict(self, u, t, xi, U, uu=None):
        N = self.N
        ess = 1.0 / float(np.sum(self.we * self.we))
        self.resampled = self.thr == 1.0 or ess < N * self.thr
        if self.resampled:
            if self.stratified:
                self.j, self.bins = resample_stratified(self.we, self.j, U)
            else:
                self.j, self.bins = resample_systematic(self.we, self.j, float(U[0]))
            self.w = np.full(N, math.log(1.0 / N))
            self.we = np.full(N, 1.0 / N)
        else:
            self.j = np.arange(N)
        xn0, xl0, R0 = self.xn[self.j], self.xl[self.j], self.R[self.j]
        assert np.any(self.coupling(self.xn[0]) != 0.0), "zeroAn branch (src/rbpf.jl:175) is not restated here"
        fi = self.fn.f(xn0, u, t)
        wn = self.R1n.sample(xi)                                 # rand(pf.rng, pf.R1n)
        uu = np.zeros(0) if (u is None or self.Bl.shape[1] == 0) else np.asarray(u, dtype=np.float64).reshape(-1)
        Al = self.Al
        xn1, xl1, R1 = np.empty_like(xn0), np.empty_like(xl0), np.empty_like(R0)
        for i in range(N):                                       # src/rbpf.jl:206-221
            An = self.coupling(xn0[i])
            R = R0[i]
            Nt = An @ R @ An.T + self.R1n.Sigma
            L = np.linalg.solve(Nt.T, (Al @ R @ An.T).T).T       # Al R An' / Nt
            R1[i] = Al @ R @ Al.T + self.R1l - L @ Nt @ L.T
            Axl = An @ xl0[i]
            z = Axl + wn[i]
            xn1[i] = fi[i] + z
            xl1[i] = Al @ xl0[i] + (self.Bl @ uu if uu.size else 0.0) + L @ (z - Axl)
        self.xn, self.xl, self.R = xn1, xl1, R1
        self.t += 1

    def run(self, U, Y, t_index0, normals, uniforms, step0=0, user_uniforms=None):
        T = len(Y)
        ll_steps = np.zeros(T)
        nres = 0
        for k in range(T):
            t = (t_index0 + k) * self.Ts
            u = U[k] if U is not None and len(U) else None
            ll_steps[k] = self.correct(u, Y[k], t)
            self.predict(u, t, normals(step0 + k, self.N, self.xn.shape[1]), uniforms(step0 + k, self.N))
            nres += int(self.resampled)
        return ll_steps, nres


# ---- FFBS particle smoother: one backward step (src/smoothing.jl:128-141, draw_one_categorical src/resample.jl:128-152) -------------
# For every trajectory m the reference draws i ~ Categorical(softmax_n(wb[m, n])), wb[m, n] = wf[n, t] + logpdf(df, xb[m, t+1] -
# f(xf[n, t], u[t], p, t Ts)), by the inverse CDF of one uniform.  Restated here in numpy.longdouble (64-bit significand on x86: 2^11
# times finer than anything the engine or the C oracle compute), from the fp64 history and the model objects above; nothing is shared
# with either but the uniform.  The check is teacher forced: xb[t+1] is what the implementation under test produced itself.
LD = np.longdouble
LOG2PI_LD = np.log(LD(2) * LD("3.14159265358979323846264338327950288"))
U53 = 2.0 ** -53                 # unit roundoff of fp64


def _chol_ld(S):
    """lower Cholesky factor of S in long double (numpy.linalg has no long double)"""
    k = S.shape[0]
    L = np.zeros((k, k), dtype=LD)
    for i in range(k):
        for j in range(i + 1):
            s = LD(S[i, j]) - np.sum(L[i, :j] * L[j, :j])
            L[i, j] = np.sqrt(s) if i == j else s / L[j, j]
    return L


def gaussian_logpdf_ld(df, v):
    """Gaussian.logpdf of v [..., k] in long double: -(k log 2 pi + logdet Sigma) / 2 - v' Sigma^-1 v / 2 through the long-double Cholesky
    factor.  Returns (logpdf, g) with g = Sigma^-1 (v - mu), the gradient of the quadratic form / 2 (what backward_step_slack needs)."""
    k = df.mu.size
    L = _chol_ld(df.Sigma)
    d = np.asarray(v, dtype=LD) - df.mu.astype(LD)
    z = np.empty_like(d)
    for i in range(k):                                   # L z = d
        z[..., i] = (d[..., i] - np.sum(z[..., :i] * L[i, :i], axis=-1)) / L[i, i]
    g = np.empty_like(d)
    for i in range(k - 1, -1, -1):                       # L' g = z
        g[..., i] = (z[..., i] - np.sum(g[..., i + 1:] * L[i + 1:, i], axis=-1)) / L[i, i]
    logdet = 2 * np.sum(np.log(np.diag(L)))
    return -(k * LOG2PI_LD + logdet) / 2 - np.sum(z * z, axis=-1) / 2, g


def smoother_backward_step(xf_t, wf_t, model, df, u_t, t, xb_next, logpdf=gaussian_logpdf_ld):
    """The distribution the backward draw at time index t samples from, for every trajectory: xf_t [N, nx], wf_t [N] the filter's
    particles and log-weights, model (LinearModel / QuadTank) and df (Gaussian) the transition, u_t the input, t = index * Ts the time the
    dynamics are evaluated at, xb_next [M, nx] the smoothed samples of index t + 1.
    Returns a dict: cdf [M, N] (long double, cdf[:, -1] = 1), p [M, N] the probabilities, and what backward_step_slack takes."""
    x = np.asarray(xf_t, dtype=LD)
    fx = model.f(x, None if u_t is None else np.asarray(u_t, dtype=LD), LD(t))                  # [N, nx], long double throughout
    xq = np.asarray(xb_next, dtype=LD)
    lp, g = logpdf(df, xq[:, None, :] - fx[None, :, :])                                          # [M, N], [M, N, nx]
    wb = np.asarray(wf_t, dtype=LD)[None, :] + lp
    mx = np.max(wb, axis=1, keepdims=True)
    e = np.exp(wb - mx)
    tot = np.sum(e, axis=1, keepdims=True)
    cdf = np.cumsum(e, axis=1) / tot
    cdf[:, -1] = 1
    return dict(cdf=cdf, p=e / tot, wb=wb, mx=mx, lp=lp, g=g, fx=fx, x=x, xq=xq, u=u_t, wf=np.asarray(wf_t, dtype=LD))


def qbits(N):
    """K = 62 - ceil(log2 N): the engine adds N quanta floor(e 2^K), e <= 1, in 64 bits"""
    return 62 - int(math.ceil(math.log2(N))) if N > 1 else 62


def backward_step_slack(step, model, df, fixed_point=True):
    """delta [M]: how far the CDF an fp64 implementation draws from can lie from step["cdf"].  Derived, not fitted:

      1. quanta.  The engine replaces e_n = exp(wb_n - max wb) by floor(e_n 2^K) 2^-K, K = qbits(N): each e_n shrinks by less than
         2^-K, the largest e_n is exactly 1 so the total E is at least 1; Q_i / Q then lies in [(E_i - i 2^-K) / E, E_i / (E - N 2^-K)],
         within N 2^-K (1 + N 2^-K) of E_i / E.  An implementation that sums in fp64 instead (fixed_point=False: the reference order,
         a serial cumsum of N terms that never exceeds 1) is within (N - 1) 2^-53 on both the partial sum and the total: 2 N 2^-53.
      2. from sums to the comparison.  bins_i = fl(fl(Q_i) fl(1 / fl(Q))), s = fl(u fl(fl(Q) fl(1 / fl(Q)))): five roundings and a
         division, each relative 2^-53 on numbers <= 1 — 8 * 2^-53 covers them.
      3. the log-weights.  An absolute error d_n of wb_n multiplies e_n by (1 + d_n); a perturbation p_n -> p_n (1 + d_n) of a
         normalised distribution moves no partial sum by more than 2 sum_n p_n |d_n| (numerator and denominator).  With u = 2^-53,
         v = xq - fl(f(x_n)) and g = Sigma^-1 v:
            d_n / u <=   3 (1 + |wf_n| + |c0| + q_n / 2)          wf + (c0 - q/2): two additions and the halving
                       + |wb_n - mx| + 2                          the subtraction of the maximum; exp itself (< 1 ulp, llpf_detmath.h) and
                                                                   its quantum's truncation of the significand
                       + 2 (k + 2) cond(Sigma) q_n                the whitening L z = v and the sum of squares (backward error (k+2) u
                                                                   of a triangular solve, amplified by at most cond)
                       + sum_k |g_k| (|xq_k| + |fx_k| + c_f F_k)  the cancellation in v: q/2 moves by g . dv, dv_k = the rounding of
                                                                   the subtraction plus f's own error c_f u F_k
         F = |A| |x| + |B| |u| and c_f = nx + nu + 1 for a LinearModel (a dot product of nx + nu terms); for QuadTank (rk4, `supersample`
         substeps of four right-hand sides: about 40 operations on numbers of the size of x per substep, none cancelling) F = |x| + |fx|
         and c_f = 64 * supersample.  A common error of mx shifts every wb alike and cancels.
         Particles with p_n = 0 (a log-weight of -inf, or e_n below the long double's underflow) contribute nothing.
    Terms of second order in 2^-53 are dropped: they are 2^-40 of the first-order terms."""
    p, wb, mx, g = step["p"], step["wb"], step["mx"], step["g"]
    M, N = p.shape
    k = df.mu.size
    absx, absfx = np.abs(step["x"]), np.abs(step["fx"])
    if isinstance(model, LinearModel):
        F = absx @ np.abs(model.A).T.astype(LD)
        if model.B.shape[1]:
            F = F + np.abs(model.B).astype(LD) @ np.abs(np.asarray(step["u"], dtype=LD).reshape(-1))
        cf = model.A.shape[0] + model.B.shape[1] + 1
    else:
        F, cf = absx + absfx, 64 * model.ss
    c0s = -(k * LOG2PI + float(np.linalg.slogdet(df.Sigma)[1])) / 2.0
    c0 = abs(c0s)
    cond = float(np.linalg.cond(df.Sigma))
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.abs(2 * (LD(c0s) - step["lp"]))                                                   # v' Sigma^-1 v
        d = (3 * (1 + np.abs(step["wf"])[None, :] + c0 + q / 2) + np.abs(wb - mx) + 2 + 2 * (k + 2) * cond * q
             + np.sum(np.abs(g) * (np.abs(step["xq"])[:, None, :] + absfx[None, :, :] + cf * F[None, :, :]), axis=2))
        contrib = np.where(p > 0, p * d, 0)
    rounding = 2 * U53 * np.sum(contrib, axis=1)
    quanta = N * 2.0 ** -qbits(N) * (1 + N * 2.0 ** -qbits(N)) if fixed_point else 2 * N * U53
    return (quanta + 8 * U53 + rounding).astype(np.float64)


def check_draws(cdf, u, idx, delta):
    """The assertion of the smoother's check for M draws: index i is right iff cdf[i-1] - delta <= u <= cdf[i] + delta (cdf[-1] = 0).
    Returns (need [M], excused [M], edge [M]): need = how much slack the reported index needs (0: inside its interval), excused = u lies
    within delta of an interior edge of the distribution, where either neighbour is accepted and the draw tests nothing, edge = the
    distance from u to the nearest interior edge."""
    M, N = cdf.shape
    u = np.asarray(u, dtype=LD)
    idx = np.asarray(idx, dtype=np.int64)
    rows = np.arange(M)
    hi = cdf[rows, idx]
    lo = np.where(idx > 0, cdf[rows, np.maximum(idx - 1, 0)], LD(0))
    need = np.maximum(np.maximum(lo - u, u - hi), 0).astype(np.float64)
    edge = np.min(np.abs(cdf[:, :-1] - u[:, None]), axis=1).astype(np.float64) if N > 1 else np.full(M, np.inf)
    return need, edge <= delta, edge
