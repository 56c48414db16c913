"""Shared pieces of the tests of the bank of unscented Kalman filters with augmented process noise (test_aukf.py, test_gpu_aukf.py) and of
tools/bench_aukf.py: the host build of csrc/shared/llpf_aukf.h (tests/aukf_host.c) around the oracle's model functions (additive) or the
C twins of the two device snippets below, which form their own noise, and a numpy restatement of the textbook augmented unscented Kalman
filter in its literal formulas — np.linalg.cholesky of the dense block-diagonal matrix of (x; w), dense sums over the 4 nx + 1 points —
that shares nothing with the header and runs in float64 and np.longdouble."""
import ctypes as C

import numpy as np

from llpf_amd import _structs as S
import kf_host as kh
from kf_host import _dp, _p
import ukf_common as uc

TWIN_NOISY_PENDULUM, TWIN_MULT = 1, 2
TWIN_SQUARE_NOISE, TWIN_MULT_ONLY = 3, 4      # x' = x + w^2 and x' = a x (1 + w): host only, the known answers of one predict!

# the pendulum of tests/ekf_common.py with its torque carrying w[0] and its damping multiplied by (1 + w[1]): the expressions of
# aukf_host.c's twin.  dynamics is dynamics_w at w = 0
NOISY_PENDULUM_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    double g_over_l, damp, dt, torque;
    DEV void prepare(const ModelD* m, const double* u, double t) {
        g_over_l = m->qt[0]; damp = m->qt[1]; dt = m->Ts; torque = (m->nu > 0 && u) ? u[0] : 0.0;
    }
    DEV void sine(const double* x, double* sn) const {
        double cs;
        const double turns = x[0] * 0.15915494309189535;            // angle / (2 pi)
        llpf_sincos2pi(turns - llpf_rint(turns) < 0.0 ? turns - llpf_rint(turns) + 1.0 : turns - llpf_rint(turns), sn, &cs);
    }
    DEV void dynamics_w(const double* x, const double* w, double* out) const {
        double sn;
        sine(x, &sn);
        out[0] = x[0] + dt * x[1];
        out[1] = x[1] + dt * ((torque + w[0]) - g_over_l * sn - damp * (1.0 + w[1]) * x[1] * x[1] * x[1]);
    }
    DEV void dynamics(const double* x, double* out) const {
        double sn;
        sine(x, &sn);
        out[0] = x[0] + dt * x[1];
        out[1] = x[1] + dt * (torque - g_over_l * sn - damp * x[1] * x[1] * x[1]);
    }
    DEV void measurement(const double* x, double* out) const { sine(x, out); }
};
'''

# x' = a x (1 + w) + w^2 with a = qt[0], g(x) = x^2 (aukf_host.c: mult_f / mult_g)
MULT_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    double a;
    DEV void prepare(const ModelD* m, const double* u, double t) { a = m->qt[0]; }
    DEV void dynamics_w(const double* x, const double* w, double* out) const { out[0] = a * x[0] * (1.0 + w[0]) + w[0] * w[0]; }
    DEV void dynamics(const double* x, double* out) const { out[0] = a * x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
};
'''


# ---- weights: the pair (measurement set at L = nx, dynamics set at L = 2 nx) ----
def merwe_pair(nx, alpha, beta, kappa):
    """Merwe (alpha, beta, kappa) at both dimensions; kappa "3-L" is 3 - L at each"""
    k = lambda L: 3.0 - L if kappa == "3-L" else kappa
    return uc.merwe(nx, alpha, beta, k(nx)), uc.merwe(2 * nx, alpha, beta, k(2 * nx))


def trivial_pair(nx):
    t = lambda L: (float(np.sqrt(L + 0.5)),) + (1.0 / (2.0 * L + 1.0),) * 3
    return t(nx), t(2 * nx)


# ---- the host build of the header ----
def build_host(outdir):
    """the host build of tests/aukf_host.c in outdir (aukf_host_run)"""
    return kh.build(outdir, "aukf_host.c", {"aukf_host_run": kh.MODEL_HEAD + [_dp] * 3 + kh.RUN_TAIL})


def host_run(L, models, w, U, Y, T, per_filter=0, t_index0=0.0, state=None, twin=0):
    """the host build of the header over the filters `models` (llpf_model descriptors; model id LINEAR_GAUSSIAN or QUADTANK_RK4 through
    the oracle's functions, taken as additive; the two snippets through their twins); w: the pair of weight sets; state = (x0 [F, nx],
    P0 [F, nx, nx]) or None (reset).  Returns the outputs in the device's layout and the final state."""
    F = len(models)
    m0 = models[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    arr = (S.Model * F)(*models)
    R1, R2, x0, P0 = kh.pack_models(models, state)
    wv = np.array(list(w[0]) + list(w[1]), dtype=np.float64)
    out, outp = kh.outputs(T, F, nx, ny)
    f, g = (None, None) if twin else uc.oracle_fns()
    rc = L.aukf_host_run(F, nx, ny, nu, f, g, twin, arr, _p(R1), _p(R2), _p(wv), _p(x0), _p(P0), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T,
                         per_filter, float(t_index0), *outp)
    assert rc == 0, rc
    return out, (x0, P0)


# ---- the restatement ----
def numpy_aukf(fw, g, R1, R2, x0, P0, w, U, Y, Ts=1.0, t_index0=0.0, lin=uc.Lin64):
    """forward_trajectory of the augmented UKF in its literal formulas; fw(x, u, tau, w), g(x, u, tau) -> arrays; w: the pair of weight
    sets.  predict! factors the dense blkdiag(R, R1) and sums over the 4 nx + 1 points of (x; 0).  Raises LinAlgError when a covariance is
    not positive definite."""
    dt = lin.dtype
    (gamma, wm0, wc0, wi), (gamma_a, wm0a, wc0a, wia) = ([dt(v) for v in s] for s in w)
    R1, R2 = np.asarray(R1, dtype=dt), np.asarray(R2, dtype=dt)
    x, R = np.asarray(x0, dtype=dt).copy(), np.asarray(P0, dtype=dt).copy()
    nx, ny, T = x.shape[0], R2.shape[0], Y.shape[0]
    wm = np.array([wm0] + [wi] * (2 * nx), dtype=dt)
    wc = np.array([wc0] + [wi] * (2 * nx), dtype=dt)
    wma = np.array([wm0a] + [wia] * (4 * nx), dtype=dt)
    wca = np.array([wc0a] + [wia] * (4 * nx), dtype=dt)
    out = dict(ll_steps=np.zeros(T, dtype=dt), x=np.empty((T, nx), dtype=dt), xt=np.empty((T, nx), dtype=dt), R=np.empty((T, nx, nx), dtype=dt),
               Rt=np.empty((T, nx, nx), dtype=dt), e=np.full((T, ny), np.nan, dtype=dt))
    for t in range(T):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        out["x"][t], out["R"][t] = x, R
        if not np.isnan(Y[t, 0]):
            Cf = lin.chol(R)
            X = np.stack([x] + [x + gamma * Cf[:, i] for i in range(nx)] + [x - gamma * Cf[:, i] for i in range(nx)])
            Yp = np.stack([np.asarray(g(Xi, u, tau), dtype=dt) for Xi in X])
            yh = wm @ Yp
            dY, dX = Yp - yh, X - x
            Sm = uc.symmetrize((dY.T * wc) @ dY) + R2
            Cxy = (dX.T * wc) @ dY
            e = np.asarray(Y[t], dtype=dt) - yh
            lin.chol(Sm)
            Si = lin.inv(Sm)
            K = Cxy @ Si
            x = x + K @ e
            R = uc.symmetrize(R - K @ Sm @ K.T)
            out["ll_steps"][t] = -(ny * np.log(2 * dt(np.pi)) + lin.logdet(Sm) + e @ Si @ e) / 2
            out["e"][t] = e
        out["xt"][t], out["Rt"][t] = x, R
        Pa = np.zeros((2 * nx, 2 * nx), dtype=dt)
        Pa[:nx, :nx], Pa[nx:, nx:] = R, R1
        Ca = lin.chol(Pa)
        xa = np.concatenate([x, np.zeros(nx, dtype=dt)])
        Xa = np.stack([xa] + [xa + gamma_a * Ca[:, i] for i in range(2 * nx)] + [xa - gamma_a * Ca[:, i] for i in range(2 * nx)])
        Xn = np.stack([np.asarray(fw(Xi[:nx], u, tau, Xi[nx:]), dtype=dt) for Xi in Xa])
        x = wma @ Xn
        dX = Xn - x
        R = uc.symmetrize((dX.T * wca) @ dX)
    out["ll"] = out["ll_steps"].sum()
    return out


def additive(fg):
    """(fw, g) of an additive model from numpy_ukf's (f, g)"""
    f, g = fg
    return (lambda x, u, tau, w: f(x, u, tau) + w), g


# ---- the two test systems ----
def noisy_pendulum_model(q_torque=0.09, q_damp=0.04):
    """the descriptor of NOISY_PENDULUM_SRC (nx = 2, nu = 1, ny = 1): qt = (g / l, damping), Ts = dt, R1 = diag(var of the torque noise,
    var of the relative jitter of the damping).  The model id is the linear-Gaussian one until a test that has a device replaces it."""
    g = S.make_gaussian
    m = S.make_lg_model(np.eye(2), np.zeros((2, 1)), np.array([[1.0, 0.0]]), g(np.zeros(2), np.array([q_torque, q_damp])), g(np.zeros(1), 0.05 ** 2),
                        g(np.array([0.8, 0.0]), np.array([0.3, 0.3])), Ts=0.05)
    m.qt[0], m.qt[1] = 9.81, 0.05
    return m


def noisy_pendulum_fg(m, dtype=np.float64):
    """the noisy pendulum's fw, g in their mathematical form (np.sin) for numpy_aukf, in float64 or long double"""
    gl, damp, dt_ = dtype(m.qt[0]), dtype(m.qt[1]), dtype(m.Ts)

    def fw(x, u, tau, w):
        return np.array([x[0] + dt_ * x[1], x[1] + dt_ * ((u[0] + w[0]) - gl * np.sin(x[0]) - damp * (1 + w[1]) * x[1] ** 3)], dtype=dtype)
    return fw, (lambda x, u, tau: np.array([np.sin(x[0])], dtype=dtype))


def noisy_pendulum_models(n):
    out = []
    for k in range(n):
        m = noisy_pendulum_model(0.09 * (1 + 0.01 * (k % 9)), 0.04 + 0.001 * (k % 5))
        m.qt[0], m.qt[1] = 9.81 * (1 + 0.002 * (k % 100)), 0.05 + 0.001 * (k % 10)
        out.append(m)
    return out


def mult_model(a=0.9, q=0.04, m0=2.0, P=0.3, r2=0.25):
    """the descriptor of MULT_SRC (nx = ny = 1, nu = 0): qt[0] = a, R1 = q, R2 = r2, d0 = N(m0, P)"""
    g = S.make_gaussian
    m = S.make_lg_model(np.eye(1), np.zeros((1, 0)), np.eye(1), g(np.zeros(1), q), g(np.zeros(1), r2), g(np.array([m0]), float(P)))
    m.qt[0] = a
    return m


def mult_fg(m, dtype=np.float64):
    a = dtype(m.qt[0])
    return (lambda x, u, tau, w: np.array([a * x[0] * (1 + w[0]) + w[0] * w[0]], dtype=dtype)), (lambda x, u, tau: np.array([x[0] * x[0]], dtype=dtype))


def mult_models(n):
    return [mult_model(0.9 - 0.002 * (k % 40), 0.04 + 0.001 * (k % 7), 2.0 + 0.01 * k) for k in range(n)]


def mult_data(T, seed=3):
    rng = np.random.default_rng(seed)
    return None, 1.2 + 0.4 * rng.standard_normal((T, 1))
