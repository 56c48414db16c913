"""The exact answer on a linear-Gaussian model and the statistics that hold a particle filter to it (test_exact_moments.py on the oracle,
test_gpu_exact_moments.py on the engine).  No GPU, no oracle arithmetic: a Kalman filter in np.longdouble written out with its own
Cholesky factorisation, so that nothing here shares code with what it judges.

The property (Del Moral 2004, Prop. 7.4.1; for adaptive resampling Whiteley, Lee, Heine 2016): a bootstrap particle filter whose
resampling is unbiased, E[copies of i] = M we_i, has for every N, every t and every phi

    E[Zhat_t] = Z_t                       E[Zhat_t sum_i W_i phi(x_i)] = Z_t E[phi(x_t) | y_1..t]

with Zhat_t = exp(sum_{s<=t} ll_steps[s]) and the weighted sum taken after correct! (what xmean is).  Neither has a 1/N term, so over
F independent replicas k, with r_{k,t} = exp(sum_{s<=t} (ll_steps[s, k] - ll_KF[s])),

    zZ_t     = (mean_k r_t - 1) / (sd_k r_t / sqrt F)
    zX_{t,d} = mean_k v / (sd_k v / sqrt F),     v_k = r_{k,t} (xmean[t, k, d] - x_KF[t, d])

are standard normal if the filter is right, and grow like sqrt F if it is not."""
import numpy as np

import kalman_common as KC
from llpf_amd import _structs as S

# The two files that use it hold at most about 2000 z-values (cases x steps x (1 + nx)).  Under the normal law P(|z| > 5) = 5.7e-7, so a
# false alarm anywhere has probability about 2000 x 5.7e-7 = 1.2e-3 — once, not per run: the seeds are fixed and the engine is
# bit-reproducible, so a case passes for ever or fails for ever.  The normal law holds for the z of a mean over F >= 256 replicas of a
# near-normal r: the cases keep sd(ll - ll_KF) <= SD_MAX, where a log-normal r has skewness 1.1 and the skewness moves the mean's z by
# about 1.1 / (6 sqrt F) < 0.02.  A z beyond 5 is therefore a finding to be examined, never a bound to be widened.
Z_MAX = 5.0
SD_MAX = 0.35

LD = np.longdouble


def _chol(S_):
    """lower Cholesky factor in long double (numpy.linalg has none); LinAlgError if S is not positive definite"""
    n = S_.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = S_[j, j] - np.dot(L[j, :j], L[j, :j])
        if not d > 0:
            raise np.linalg.LinAlgError("not positive definite")
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (S_[i, j] - np.dot(L[i, :j], L[j, :j])) / L[j, j]
    return L


def _solve_chol(L, b):
    """S^-1 b from S = L L' (b a vector or a matrix of columns)"""
    n = L.shape[0]
    b = np.array(b, dtype=LD)
    z = np.zeros_like(b)
    for i in range(n):
        z[i] = (b[i] - np.tensordot(L[i, :i], z[:i], axes=(0, 0))) / L[i, i]
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = (z[i] - np.tensordot(L[i + 1:, i], x[i + 1:], axes=(0, 0))) / L[i, i]
    return x


def model_matrices(model, D=None):
    """kalman_common.matrices(model, D) plus the means of the two noise densities (wbar, ebar), which that function leaves out"""
    mats = KC.matrices(model, np.zeros((model.ny, model.nu)) if D is None else D)
    mats["wbar"] = S.gaussian_mean(model.dynamics_density)
    mats["ebar"] = S.gaussian_mean(model.measurement_density)
    return mats


def kalman(mats, U, Y):
    """The Kalman filter of x+ = A x + B u + w, y = C x + D u + e, w ~ N(wbar, R1), e ~ N(ebar, R2), x_0 ~ N(x0, P0), in long double and
    in Joseph form.  Returns ll_steps [T], the filtered means xt [T, nx] and covariances Rt [T, nx, nx] (after the measurement update, which
    is where the particle filter's xmean is taken), all as float64; `ll_ld`: the long double sum.  A row of Y whose first element is NaN is
    missing: it contributes 0 and leaves the prediction as the filtered state."""
    A, B, Cm, D, R1, R2 = (np.asarray(mats[k], dtype=LD) for k in ("A", "B", "C", "D", "R1", "R2"))
    nx, ny = A.shape[0], Cm.shape[0]
    wbar = np.asarray(mats.get("wbar", np.zeros(nx)), dtype=LD)
    ebar = np.asarray(mats.get("ebar", np.zeros(ny)), dtype=LD)
    x, P = np.asarray(mats["x0"], dtype=LD).copy(), np.asarray(mats["P0"], dtype=LD).copy()
    Y = np.asarray(Y, dtype=np.float64).reshape(-1, ny)
    T = Y.shape[0]
    U = np.zeros((T, 0)) if B.shape[1] == 0 else np.asarray(U, dtype=np.float64).reshape(T, -1)
    lls = np.zeros(T, dtype=LD)
    xt, Rt = np.zeros((T, nx), dtype=LD), np.zeros((T, nx, nx), dtype=LD)
    log2pi = np.log(8 * np.arctan(LD(1)))
    I = np.eye(nx, dtype=LD)
    for t in range(T):
        u = U[t].astype(LD)
        if not np.isnan(Y[t, 0]):
            e = Y[t].astype(LD) - (Cm @ x + D @ u + ebar)
            Sm = Cm @ P @ Cm.T + R2
            Sm = (Sm + Sm.T) / 2
            L = _chol(Sm)
            K = _solve_chol(L, Cm @ P).T                  # K = P C' S^-1 (P and S symmetric)
            lls[t] = -(ny * log2pi + 2 * np.sum(np.log(np.diag(L))) + e @ _solve_chol(L, e)) / 2
            x = x + K @ e
            IKC = I - K @ Cm
            P = IKC @ P @ IKC.T + K @ R2 @ K.T
            P = (P + P.T) / 2
        xt[t], Rt[t] = x, P
        x = A @ x + B @ u + wbar
        P = A @ P @ A.T + R1
        P = (P + P.T) / 2
    return dict(ll_steps=lls.astype(np.float64), xt=xt.astype(np.float64), Rt=Rt.astype(np.float64), ll=float(lls.sum()), ll_ld=lls.sum())


def ratios(ll_steps, ll_kf):
    """r [T, F] = exp(sum_{s<=t} (ll_steps[s, k] - ll_KF[s])) from ll_steps [T, F] and the Kalman filter's ll_steps [T]"""
    return np.exp(np.cumsum(np.asarray(ll_steps) - np.asarray(ll_kf)[:, None], axis=0))


def _z_of_mean(v, centre=0.0):
    """(mean - centre) / standard error over the last axis"""
    F = v.shape[-1]
    return (v.mean(axis=-1) - centre) / (v.std(axis=-1, ddof=1) / np.sqrt(F))


def z_likelihood(ll_steps, ll_kf):
    """zZ [T]"""
    return _z_of_mean(ratios(ll_steps, ll_kf), 1.0)


def z_state(ll_steps, xmean, ll_kf, x_kf):
    """zX [T, nx] from ll_steps [T, F], xmean [T, F, nx] and the Kalman filter's ll_steps [T] and filtered means [T, nx]"""
    v = ratios(ll_steps, ll_kf)[:, :, None] * (np.asarray(xmean) - np.asarray(x_kf)[:, None, :])
    return _z_of_mean(np.moveaxis(v, 1, -1))


def sd_loglik(ll_steps, ll_kf):
    """sd_k (ll_k - ll_KF) of the whole run: the condition SD_MAX is set on"""
    return float(np.std(np.sum(ll_steps, axis=0) - np.sum(ll_kf), ddof=1))


def offset(ll_steps, ll_kf):
    """mean_k (ll_k - ll_KF) of the whole run, its standard error, and the per-step offsets [T]"""
    d = np.asarray(ll_steps) - np.asarray(ll_kf)[:, None]
    tot = d.sum(axis=0)
    return float(tot.mean()), float(tot.std(ddof=1) / np.sqrt(tot.size)), d.mean(axis=1)


# ---- the models of the two files ---------------------------------------------------------------------------------------------------
def perturbed_lg_test_model(what, p):
    """lg_test_model(0.1) with the measurement variance x (1 + p) (`meas`) or the dynamics noise standard deviation x (1 + p) (`dyn`): the
    WRONG model whose Kalman filter a correct particle filter of lg_test_model(0.1) must be told apart from"""
    import models as M
    if what == "dyn":
        return M.lg_test_model(0.1 * (1.0 + p))
    m = M.lg_test_model(0.1)
    m.measurement_density = S.make_gaussian(np.zeros(1), np.ones(1) * (1.0 + p))
    return m


# the smallest p of {1, 2, 5, 10} % whose zZ reaches |z| >= 8 on the device-order oracle at F = 4096, N = 1024, T = 20 (EXPERIMENTS.md)
SENS_P = {"meas": 0.01, "dyn": 0.10}


def rb_mixed(An):
    """the mixed 1 + 1 Rao-Blackwellized system of test_oracle_statistical.test_rbpf_matches_kalman_filter (reference test/test_rbpf.jl:5-31)
    with the coupling An (None: no coupling), and the joint linear-Gaussian model whose Kalman filter is its exact answer"""
    g = S.make_gaussian
    rb = S.make_rb_model([[1.0]], np.zeros((1, 0)), None if An is None else [[An]], [[0.95]], np.zeros((1, 0)), [[1.0]], [[1.0]],
                         g(np.zeros(1), np.array([[0.01]])), [[0.01]], g(np.zeros(1), np.array([[0.1]])), g(np.array([1.0]), np.array([[0.01]])),
                         g(np.array([1.0]), np.array([[1.0]])))
    a = 0.0 if An is None else An
    joint = S.make_lg_model(np.array([[1, a], [0, 0.95]]), np.zeros((2, 0)), np.array([[1.0, 1.0]]), g(np.zeros(2), np.diag([0.01, 0.01])),
                            g(np.zeros(1), np.array([[0.1]])), g(np.array([1.0, 1.0]), np.diag([0.01, 1.0])))
    return rb, joint


def rb_data(An, T, seed=1):
    """measurements of the mixed system, drawn in numpy as the test above draws them"""
    rng = np.random.default_rng(seed)
    a = 0.0 if An is None else An
    xn, xl = 1.0, 1.0
    Y = np.zeros((T, 1))
    for t in range(T):
        Y[t] = xn + xl + np.sqrt(0.1) * rng.standard_normal()
        xn, xl = xn + a * xl + 0.1 * rng.standard_normal(), 0.95 * xl + 0.1 * rng.standard_normal()
    return np.zeros((T, 0)), Y


def cov_full_32():
    """the (nx, ny) = (3, 2) system of test_gpu_parity.test_covariance_kinds with COV_FULL for all three densities"""
    kind = S.COV_FULL
    rng = np.random.default_rng(5)
    nx, nu, ny = 3, 2, 2
    A = 0.8 * np.eye(nx) + 0.05 * rng.standard_normal((nx, nx))
    B = rng.standard_normal((nx, nu)); Cm = rng.standard_normal((ny, nx))

    def cov(n):
        Q = rng.standard_normal((n, n))
        return Q @ Q.T + 0.2 * np.eye(n)
    df = S.make_gaussian(0.01 * rng.standard_normal(nx), cov(nx), kind)
    dg = S.make_gaussian(0.01 * rng.standard_normal(ny), cov(ny), kind)
    d0 = S.make_gaussian(rng.standard_normal(nx), cov(nx), kind)
    return S.make_lg_model(A, B, Cm, df, dg, d0)


def lg_521():
    """the (nx, ny, nu) = (5, 2, 1) system of test_gpu_parity.test_linear_gaussian_above_the_precompiled_dimensions (compiled on demand)"""
    nx, ny, nu = 5, 2, 1
    rng = np.random.default_rng(100 + nx + ny)
    A = 0.9 * np.linalg.qr(rng.standard_normal((nx, nx)))[0]
    B = 0.2 * rng.standard_normal((nx, nu))
    Cm = rng.standard_normal((ny, nx))
    return S.make_lg_model(A, B, Cm, S.make_gaussian(np.zeros(nx), 0.05), S.make_gaussian(np.zeros(ny), 0.5 + rng.random(ny)),
                           S.make_gaussian(rng.standard_normal(nx), 1.0))
