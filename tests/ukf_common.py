"""Shared pieces of the unscented-Kalman-bank tests (test_ukf.py, test_gpu_ukf.py) and of tools/bench_ukf.py: the host build of
csrc/shared/llpf_ukf.h (tests/ukf_host.c) around the oracle's model functions or the C twins of the test snippets, and a numpy
restatement of the textbook additive-noise unscented Kalman filter in its literal formulas (np.linalg.cholesky / inv / slogdet, dense
symmetrize) that shares nothing with the header.  The restatement also runs in np.longdouble with hand-written factorisations, which
measures its own rounding error."""
import ctypes as C

import numpy as np

from llpf_amd import _structs as S
import kf_host as kh
from kf_host import ROOT, SHARED, _dp, _p
import oracle_binding as ob

TWIN_PENDULUM, TWIN_SQUARE = 1, 2

# f(x) = x, g(x) = x_0^2: the unscented transform of a quadratic is exact (tests/ukf_host.c: square_f / square_g)
SQUARE_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    DEV void prepare(const ModelD* m, const double* u, double t) {}
    DEV void dynamics(const double* x, double* out) const { out[0] = x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
};
'''


# ---- weights: (gamma, wm0, wc0, wi), the formulas of the issue restated (api.MerweParams / WikiParams are what users call) ----
def merwe(L, alpha, beta, kappa):
    lam = alpha * alpha * (L + kappa) - L
    wm0 = lam / (L + lam)
    return (float(np.sqrt(L + lam)), wm0, wm0 + 1.0 - alpha * alpha + beta, 1.0 / (2.0 * (L + lam)))


ALPHA1_SETS = ((1.0, 0.0, 1.0), (1.0, 0.0, 0.0), (1.0, 0.0, "3-L"))      # (alpha, beta, kappa); the last has wm0 < 0 for L > 3
SMALL_ALPHA = (1e-3, 2.0, 0.0)


def merwe_set(L, abk):
    a, b, k = abk
    return merwe(L, a, b, 3.0 - L if k == "3-L" else k)


# ---- the host build of the header ----
def build_host(outdir):
    """the host build of tests/ukf_host.c in outdir (ukf_host_run and ukf_host_smooth)"""
    smooth = [C.c_int] * 3 + [C.c_void_p, C.c_int, C.POINTER(S.Model)] + [_dp] * 3 + [C.c_int64, C.c_int, C.c_double] + [_dp] * 4
    return kh.build(outdir, "ukf_host.c", {"ukf_host_run": kh.MODEL_HEAD + [_dp] * 3 + kh.RUN_TAIL, "ukf_host_smooth": smooth})


def oracle_fns():
    """the addresses of the oracle's dynamics / measurement: the device's built-in models in the device's order"""
    lib = ob.lib()
    return C.cast(lib.orc_dynamics, C.c_void_p), C.cast(lib.orc_measurement, C.c_void_p)


def host_run(L, models, w, U, Y, T, per_filter=0, t_index0=0.0, state=None, twin=0):
    """the host build of the header over the filters `models` (llpf_model descriptors; model id LINEAR_GAUSSIAN or QUADTANK_RK4 through
    the oracle's functions, anything through a twin); state = (x0 [F, nx], P0 [F, nx, nx]) or None (reset).  Returns the outputs in the
    device's layout and the final state."""
    F = len(models)
    m0 = models[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    arr = (S.Model * F)(*models)
    R1, R2, x0, P0 = kh.pack_models(models, state)
    wv = np.array(w, dtype=np.float64)
    out, outp = kh.outputs(T, F, nx, ny)
    f, g = (None, None) if twin else oracle_fns()
    rc = L.ukf_host_run(F, nx, ny, nu, f, g, twin, arr, _p(R1), _p(R2), _p(wv), _p(x0), _p(P0), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T,
                        per_filter, float(t_index0), *outp)
    assert rc == 0
    return out, (x0, P0)


# ---- the restatement ----
class Lin64:
    """float64 through numpy's LAPACK routines"""
    dtype = np.float64
    chol = staticmethod(np.linalg.cholesky)
    inv = staticmethod(np.linalg.inv)

    @staticmethod
    def logdet(S_):
        return np.linalg.slogdet(S_)[1]


class LinLong:
    """np.longdouble, hand-written (np.linalg has no long double): Cholesky, and the inverse and log-determinant from it"""
    dtype = np.longdouble

    @staticmethod
    def chol(A):
        n = A.shape[0]
        Lc = np.zeros((n, n), dtype=np.longdouble)
        for i in range(n):
            for j in range(i + 1):
                s = A[i, j] - Lc[i, :j] @ Lc[j, :j]
                if i == j:
                    if not s > 0:
                        raise np.linalg.LinAlgError("not positive definite")
                    Lc[i, i] = np.sqrt(s)
                else:
                    Lc[i, j] = s / Lc[j, j]
        return Lc

    @staticmethod
    def inv(A):
        n = A.shape[0]
        Lc = LinLong.chol(A)
        Li = np.zeros((n, n), dtype=np.longdouble)
        for c in range(n):                 # forward substitution on the identity's columns
            for r in range(c, n):
                s = (np.longdouble(1) if r == c else np.longdouble(0)) - Lc[r, c:r] @ Li[c:r, c]
                Li[r, c] = s / Lc[r, r]
        return Li.T @ Li

    @staticmethod
    def logdet(A):
        return 2 * np.sum(np.log(np.diag(LinLong.chol(A))))


def symmetrize(M):
    return (M + M.T) / 2


def numpy_ukf(f, g, R1, R2, x0, P0, w, U, Y, Ts=1.0, t_index0=0.0, lin=Lin64):
    """forward_trajectory of the additive-noise UKF in its literal formulas; f(x, u, tau), g(x, u, tau) -> arrays.  Raises LinAlgError when
    a covariance is not positive definite."""
    dt = lin.dtype
    gamma, wm0, wc0, wi = (dt(v) for v in w)
    R1, R2 = np.asarray(R1, dtype=dt), np.asarray(R2, dtype=dt)
    x, R = np.asarray(x0, dtype=dt).copy(), np.asarray(P0, dtype=dt).copy()
    nx, ny, T = x.shape[0], R2.shape[0], Y.shape[0]
    wm = np.array([wm0] + [wi] * (2 * nx), dtype=dt)
    wc = np.array([wc0] + [wi] * (2 * nx), dtype=dt)

    def points(m, P):
        Cf = lin.chol(P)
        return np.stack([m] + [m + gamma * Cf[:, i] for i in range(nx)] + [m - gamma * Cf[:, i] for i in range(nx)])

    out = dict(ll_steps=np.zeros(T, dtype=dt), x=np.empty((T, nx), dtype=dt), xt=np.empty((T, nx), dtype=dt), R=np.empty((T, nx, nx), dtype=dt),
               Rt=np.empty((T, nx, nx), dtype=dt), e=np.full((T, ny), np.nan, dtype=dt))
    for t in range(T):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        out["x"][t], out["R"][t] = x, R
        if not np.isnan(Y[t, 0]):
            X = points(x, R)
            Yp = np.stack([np.asarray(g(Xi, u, tau), dtype=dt) for Xi in X])
            yh = wm @ Yp
            dY, dX = Yp - yh, X - x
            Sm = symmetrize((dY.T * wc) @ dY) + R2
            Cxy = (dX.T * wc) @ dY
            e = np.asarray(Y[t], dtype=dt) - yh
            lin.chol(Sm)
            Si = lin.inv(Sm)
            K = Cxy @ Si
            x = x + K @ e
            R = symmetrize(R - K @ Sm @ K.T)
            out["ll_steps"][t] = -(ny * np.log(2 * dt(np.pi)) + lin.logdet(Sm) + e @ Si @ e) / 2
            out["e"][t] = e
        out["xt"][t], out["Rt"][t] = x, R
        X = points(x, R)
        Xn = np.stack([np.asarray(f(Xi, u, tau), dtype=dt) for Xi in X])
        x = wm @ Xn
        dX = Xn - x
        R = symmetrize((dX.T * wc) @ dX) + R1
    out["ll"] = out["ll_steps"].sum()
    return out


def linear_fg(mats, dtype=np.float64):
    """f, g of a linear model (kalman_common.matrices) for numpy_ukf"""
    A, B, Cm = (np.asarray(mats[k], dtype=dtype) for k in ("A", "B", "C"))
    return (lambda x, u, tau: A @ x + (B @ u if B.shape[1] else 0)), (lambda x, u, tau: Cm @ x)


def rel_err(a, b):
    """max |a - b| / (|b| + max |b| of the step's matrix / vector), the scale kalman_common.close uses; NaN patterns must agree"""
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = ~np.isnan(b)
    scale = np.abs(np.where(ok, b, 0))
    if b.ndim >= 2:
        scale = scale + np.max(scale.reshape(b.shape[0], -1), axis=1).reshape((-1,) + (1,) * (b.ndim - 1))
    return float(np.max(np.abs(a[ok] - b[ok]) / (scale[ok] + 1e-300))) if ok.any() else 0.0


# ---- the nonlinear test systems ----
def pendulum_model():
    """the descriptor of tests/user_models.py's pendulum (PENDULUM_SRC; nx = 2, nu = 1, ny = 1): qt = (g / l, damping), Ts = dt.  The
    model id is the linear-Gaussian one until a test that has a device replaces it with the compiled snippet's."""
    g = S.make_gaussian
    m = S.make_lg_model(np.eye(2), np.zeros((2, 1)), np.array([[1.0, 0.0]]), g(np.zeros(2), np.array([1e-4, 4e-3])), g(np.zeros(1), 0.05 ** 2),
                        g(np.array([0.8, 0.0]), np.array([0.3, 0.3])), Ts=0.05)
    m.qt[0], m.qt[1] = 9.81, 0.05
    return m


def pendulum_fg(m, dtype=np.float64):
    """the pendulum's f, g in their mathematical form (np.sin) for numpy_ukf, in float64 or long double"""
    gl, damp, dt_ = dtype(m.qt[0]), dtype(m.qt[1]), dtype(m.Ts)

    def f(x, u, tau):
        return np.array([x[0] + dt_ * x[1], x[1] + dt_ * (u[0] - gl * np.sin(x[0]) - damp * x[1] ** 3)], dtype=dtype)
    return f, (lambda x, u, tau: np.array([np.sin(x[0])], dtype=dtype))


def pendulum_data(T, seed=0):
    m = pendulum_model()
    f, g = pendulum_fg(m)
    rng = np.random.default_rng(seed)
    U = 0.5 * np.sin(0.1 * np.arange(T)).reshape(T, 1)
    Y = np.zeros((T, 1))
    x = np.array([1.0, 0.0])
    for k in range(T):
        Y[k] = g(x, U[k], 0.0) + 0.05 * rng.standard_normal()
        x = f(x, U[k], 0.0) + np.sqrt(np.array([1e-4, 4e-3])) * rng.standard_normal(2)
    return U, Y


def quadtank_fg(model, dtype=np.float64):
    """the quad-tank's f, g restated generically in `dtype` (llpf_amd.QuadTankDynamics computes in float64 only): the same rk4 of the same
    right-hand side, for the long-double measurement of the restatement's rounding error"""
    c = {k: dtype(v) for k, v in S.QUADTANK_DEFAULTS.items()}
    ss, Ts = int(model.supersample), dtype(model.Ts)

    def rhs(h, u, t):
        a1 = c["a1"] * (c["a1_factor"] if t > c["t_switch"] else dtype(1))
        sq = lambda z: np.sqrt(max(z, dtype(0)) + c["eps"])
        g2 = 2 * c["g"]
        return np.array([
            -a1 / c["A1"] * sq(g2 * h[0]) + c["a3"] / c["A1"] * sq(g2 * h[2]) + c["gamma1"] * c["k1"] / c["A1"] * u[0],
            -c["a2"] / c["A2"] * sq(g2 * h[1]) + c["a4"] / c["A2"] * sq(g2 * h[3]) + c["gamma2"] * c["k2"] / c["A2"] * u[1],
            -c["a3"] / c["A3"] * sq(g2 * h[2]) + (1 - c["gamma2"]) * c["k2"] / c["A3"] * u[1],
            -c["a4"] / c["A4"] * sq(g2 * h[3]) + (1 - c["gamma1"]) * c["k1"] / c["A4"] * u[0]], dtype=dtype)

    def f(x, u, t):
        x = np.asarray(x, dtype=dtype).copy()
        h = Ts / ss
        t = dtype(t)
        for _ in range(ss):
            f1 = rhs(x, u, t)
            f2 = rhs(x + h / 2 * f1, u, t + h / 2)
            f3 = rhs(x + h / 2 * f2, u, t + h / 2)
            f4 = rhs(x + h * f3, u, t + h)
            x = x + h / 6 * (f1 + 2 * f2 + 2 * f3 + f4)
            t = t + h
        return x
    return f, (lambda x, u, t: np.asarray(x, dtype=dtype)[:2].copy())
