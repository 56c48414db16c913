"""Shared pieces of the extended-Kalman-bank tests (test_ekf.py, test_gpu_ekf.py) and of tools/bench_ekf.py: the host build of
csrc/shared/llpf_ekf.h and csrc/shared/llpf_quadtank_jac.h (tests/ekf_host.c), the device snippets with hand-written Jacobian members
whose C twins that file holds, and a numpy restatement of the textbook first-order extended Kalman filter in its literal formulas
(np.linalg.inv, dense symmetrize, slogdet) that shares nothing with the header and runs in float64 and np.longdouble."""
import ctypes as C

import numpy as np

from llpf_amd import _structs as S
import kf_host as kh
from kf_host import ROOT, SHARED, _dp, _p
import ukf_common as uc

KIND_LG, KIND_QUADTANK, KIND_PENDULUM, KIND_SQUARE = 0, 1, 2, 3

# the pendulum of tests/user_models.py (PENDULUM_SRC) with the two Jacobian members: the expressions of ekf_host.c's twin
PENDULUM_JAC_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    double g_over_l, damp, dt, torque;
    DEV void prepare(const ModelD* m, const double* u, double t) {
        g_over_l = m->qt[0]; damp = m->qt[1]; dt = m->Ts; torque = (m->nu > 0 && u) ? u[0] : 0.0;
    }
    DEV void sincos(const double* x, double* sn, double* cs) const {
        const double turns = x[0] * 0.15915494309189535;            // angle / (2 pi)
        llpf_sincos2pi(turns - llpf_rint(turns) < 0.0 ? turns - llpf_rint(turns) + 1.0 : turns - llpf_rint(turns), sn, cs);
    }
    DEV void dynamics(const double* x, double* out) const {
        double sn, cs;
        sincos(x, &sn, &cs);
        out[0] = x[0] + dt * x[1];
        out[1] = x[1] + dt * (torque - g_over_l * sn - damp * x[1] * x[1] * x[1]);
    }
    DEV void measurement(const double* x, double* out) const {
        double sn, cs;
        sincos(x, &sn, &cs);
        out[0] = sn;
    }
    DEV void dynamics_jac(const double* x, double* fx, double* J) const {
        double sn, cs;
        sincos(x, &sn, &cs);
        fx[0] = x[0] + dt * x[1];
        fx[1] = x[1] + dt * (torque - g_over_l * sn - damp * x[1] * x[1] * x[1]);
        J[0] = 1.0;
        J[1] = dt;
        J[2] = dt * (-(g_over_l * cs));
        J[3] = 1.0 + dt * (-(3.0 * damp * x[1] * x[1]));
    }
    DEV void measurement_jac(const double* x, double* gx, double* J) const {
        double sn, cs;
        sincos(x, &sn, &cs);
        gx[0] = sn;
        J[0] = cs;
        J[1] = 0.0;
    }
};
'''

# f(x) = x, g(x) = x_0^2 with the two members (ekf_host.c: EKF_SQUARE at nx = 1)
SQUARE_JAC_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    DEV void prepare(const ModelD* m, const double* u, double t) {}
    DEV void dynamics(const double* x, double* out) const { out[0] = x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
    DEV void dynamics_jac(const double* x, double* fx, double* J) const { fx[0] = x[0]; J[0] = 1.0; }
    DEV void measurement_jac(const double* x, double* gx, double* J) const { gx[0] = x[0] * x[0]; J[0] = x[0] + x[0]; }
};
'''
# the same model with the dynamics' member only: what a snippet that forgot one looks like
SQUARE_DYN_JAC_ONLY_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    DEV void prepare(const ModelD* m, const double* u, double t) {}
    DEV void dynamics(const double* x, double* out) const { out[0] = x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
    DEV void dynamics_jac(const double* x, double* fx, double* J) const { fx[0] = x[0]; J[0] = 1.0; }
};
'''
# the same model with an initial density of its own and no `noise`: the EKF bank's refusal of `initial` on its own
SQUARE_JAC_INITIAL_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    DEV void prepare(const ModelD* m, const double* u, double t) {}
    DEV void dynamics(const double* x, double* out) const { out[0] = x[0]; }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0] * x[0]; }
    DEV void dynamics_jac(const double* x, double* fx, double* J) const { fx[0] = x[0]; J[0] = 1.0; }
    DEV void measurement_jac(const double* x, double* gx, double* J) const { gx[0] = x[0] * x[0]; J[0] = x[0] + x[0]; }
    DEV void initial(const double* xi, const double* uu, double* out) const { out[0] = 1.0 + uu[0]; }
};
'''


def build_host(outdir):
    """the host build of tests/ekf_host.c in outdir (ekf_host_run, iekf_host_run and ekf_host_qt_jac)"""
    run = kh.MODEL_HEAD + [_dp] * 2 + kh.RUN_TAIL
    return kh.build(outdir, "ekf_host.c", {"ekf_host_run": run, "iekf_host_run": run + [C.c_int, C.c_double, C.POINTER(C.c_int32)],
                                           "ekf_host_qt_jac": (None, [C.POINTER(S.Model), _dp, C.c_double, _dp, _dp, _dp])})


def kind_of(model):
    return {S.MODEL_LINEAR_GAUSSIAN: KIND_LG, S.MODEL_QUADTANK_RK4: KIND_QUADTANK}[model.model_id]


def host_run(L, models, U, Y, T, per_filter=0, t_index0=0.0, state=None, kind=None, iterations=None):
    """the host build of the header over the filters `models` (llpf_model descriptors); kind: KIND_* (default: by the model id of the
    first); state = (x0 [F, nx], P0 [F, nx, nx]) or None (reset); iterations: None, or (maxiters, epsilon) of the iterated filter, whose
    outputs have "iters" [T, F] as well.  Returns the outputs in the device's layout and the final state."""
    F = len(models)
    m0 = models[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    kind = kind_of(m0) if kind is None else kind
    arr = (S.Model * F)(*models)
    R1, R2, x0, P0 = kh.pack_models(models, state)
    out, outp = kh.outputs(T, F, nx, ny)
    f, g = uc.oracle_fns() if kind == KIND_LG else (None, None)
    args = [F, nx, ny, nu, f, g, kind, arr, _p(R1), _p(R2), _p(x0), _p(P0), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter, float(t_index0)] + outp
    if iterations is None:
        rc = L.ekf_host_run(*args)
    else:
        out["iters"] = np.full((T, F), -1, dtype=np.int32)
        rc = L.iekf_host_run(*args, int(iterations[0]), float(iterations[1]), out["iters"].ctypes.data_as(C.POINTER(C.c_int32)))
    assert rc == 0, rc
    return out, (x0, P0)


def host_qt_jac(L, model, x, u, t):
    """(fx [4], J [4, 4]) of the shared quad-tank header at (x, u, t)"""
    x, u = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(u, dtype=np.float64)
    fx, J = np.empty(4), np.empty(16)
    L.ekf_host_qt_jac(C.byref(model), _p(u), float(t), _p(x), _p(fx), _p(J))
    return fx, J.reshape(4, 4)


# ---- the restatement ----
def numpy_ekf(f, g, fjac, gjac, R1, R2, x0, P0, U, Y, Ts=1.0, t_index0=0.0, lin=uc.Lin64):
    """forward_trajectory of the first-order EKF in its literal formulas: f(x, u, tau), g(x, u, tau) -> arrays, fjac / gjac -> their
    Jacobians at x.  K = R C' inv(S);  x += K e;  R = symmetrize((I - K C) R);  x = f(x);  R = symmetrize(A R A') + R1."""
    dt = lin.dtype
    R1, R2 = np.asarray(R1, dtype=dt), np.asarray(R2, dtype=dt)
    x, R = np.asarray(x0, dtype=dt).copy(), np.asarray(P0, dtype=dt).copy()
    nx, ny, T = x.shape[0], R2.shape[0], Y.shape[0]
    I = np.eye(nx, dtype=dt)
    out = dict(ll_steps=np.zeros(T, dtype=dt), x=np.empty((T, nx), dtype=dt), xt=np.empty((T, nx), dtype=dt), R=np.empty((T, nx, nx), dtype=dt),
               Rt=np.empty((T, nx, nx), dtype=dt), e=np.full((T, ny), np.nan, dtype=dt))
    for t in range(T):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        out["x"][t], out["R"][t] = x, R
        if not np.isnan(Y[t, 0]):
            Cm = np.asarray(gjac(x, u, tau), dtype=dt).reshape(ny, nx)
            e = np.asarray(Y[t], dtype=dt) - np.asarray(g(x, u, tau), dtype=dt)
            Sm = uc.symmetrize(Cm @ R @ Cm.T) + R2
            Si = lin.inv(Sm)
            K = R @ Cm.T @ Si
            x = x + K @ e
            R = uc.symmetrize((I - K @ Cm) @ R)
            out["ll_steps"][t] = -(ny * np.log(2 * dt(np.pi)) + lin.logdet(Sm) + e @ Si @ e) / 2
            out["e"][t] = e
        out["xt"][t], out["Rt"][t] = x, R
        A = np.asarray(fjac(x, u, tau), dtype=dt).reshape(nx, nx)
        x = np.asarray(f(x, u, tau), dtype=dt)
        R = uc.symmetrize(A @ R @ A.T) + R1
    out["ll"] = out["ll_steps"].sum()
    return out


def linear_jacs(mats, dtype=np.float64):
    A, Cm = np.asarray(mats["A"], dtype=dtype), np.asarray(mats["C"], dtype=dtype)
    return (lambda x, u, tau: A), (lambda x, u, tau: Cm)


def pendulum_jacs(m, dtype=np.float64):
    """the analytic Jacobians of ukf_common.pendulum_fg, written in numpy"""
    gl, damp, dt_ = dtype(m.qt[0]), dtype(m.qt[1]), dtype(m.Ts)
    fj = lambda x, u, tau: np.array([[1, dt_], [-dt_ * gl * np.cos(x[0]), 1 - 3 * dt_ * damp * x[1] ** 2]], dtype=dtype)
    return fj, (lambda x, u, tau: np.array([[np.cos(x[0]), 0]], dtype=dtype))


def quadtank_jacs(model, dtype=np.float64):
    """the analytic Jacobian of ukf_common.quadtank_fg: the chain rule through the RK4 stages with dense 4 x 4 matrices, in `dtype`"""
    c = {k: dtype(v) for k, v in S.QUADTANK_DEFAULTS.items()}
    ss, Ts = int(model.supersample), dtype(model.Ts)
    g2 = 2 * c["g"]

    def rhs_and_D(h, u, t):
        a1 = c["a1"] * (c["a1_factor"] if t > c["t_switch"] else dtype(1))
        s = np.array([np.sqrt(max(g2 * z, dtype(0)) + c["eps"]) for z in h], dtype=dtype)
        ds = np.array([g2 / (2 * s[i]) if g2 * h[i] > 0 else dtype(0) for i in range(4)], dtype=dtype)
        xd = np.array([
            -a1 / c["A1"] * s[0] + c["a3"] / c["A1"] * s[2] + c["gamma1"] * c["k1"] / c["A1"] * u[0],
            -c["a2"] / c["A2"] * s[1] + c["a4"] / c["A2"] * s[3] + c["gamma2"] * c["k2"] / c["A2"] * u[1],
            -c["a3"] / c["A3"] * s[2] + (1 - c["gamma2"]) * c["k2"] / c["A3"] * u[1],
            -c["a4"] / c["A4"] * s[3] + (1 - c["gamma1"]) * c["k1"] / c["A4"] * u[0]], dtype=dtype)
        D = np.zeros((4, 4), dtype=dtype)
        D[0, 0], D[0, 2] = -a1 / c["A1"] * ds[0], c["a3"] / c["A1"] * ds[2]
        D[1, 1], D[1, 3] = -c["a2"] / c["A2"] * ds[1], c["a4"] / c["A2"] * ds[3]
        D[2, 2], D[3, 3] = -c["a3"] / c["A3"] * ds[2], -c["a4"] / c["A4"] * ds[3]
        return xd, D

    def fjac(x, u, t):
        x = np.asarray(x, dtype=dtype).copy()
        h = Ts / ss
        t = dtype(t)
        I = np.eye(4, dtype=dtype)
        J = I.copy()
        for _ in range(ss):
            f1, K1 = rhs_and_D(x, u, t)
            f2, D2 = rhs_and_D(x + h / 2 * f1, u, t + h / 2)
            K2 = D2 @ (I + h / 2 * K1)
            f3, D3 = rhs_and_D(x + h / 2 * f2, u, t + h / 2)
            K3 = D3 @ (I + h / 2 * K2)
            f4, D4 = rhs_and_D(x + h * f3, u, t + h)
            K4 = D4 @ (I + h * K3)
            J = (I + h / 6 * (K1 + 2 * K2 + 2 * K3 + K4)) @ J
            x = x + h / 6 * (f1 + 2 * f2 + 2 * f3 + f4)
            t = t + h
        return J
    return fjac, (lambda x, u, t: np.eye(2, 4, dtype=dtype))


def square_model(m0, R00, r2=0.25, r1=0.1):
    g = S.make_gaussian
    return S.make_lg_model(np.eye(1), np.zeros((1, 0)), np.eye(1), g(np.zeros(1), r1), g(np.zeros(1), r2), g(np.array([m0]), float(R00)))


# ---- the quad-tank as an ordinary function (tests/test_tracing.py's, restated): what the tracer differentiates ----
def quadtank_rhs(h, u, p, t):
    """examples/example_quadtank.jl:8-27 (the tank parameters in p), in the built-in model's expression order"""
    from llpf_amd import tracing as tr
    g2 = 2.0 * p["g"]
    ss = [tr.sqrt(tr.maximum(g2 * h[i], 0.0) + p["eps"]) for i in range(4)]
    c1a = tr.ifelse(t > p["t_switch"], (-(p["a1"] * p["a1_factor"])) / p["A1"], (-p["a1"]) / p["A1"])
    return [c1a * ss[0] + (p["a3"] / p["A1"]) * ss[2] + ((p["gamma1"] * p["k1"]) / p["A1"]) * u[0],
            ((-p["a2"]) / p["A2"]) * ss[1] + (p["a4"] / p["A2"]) * ss[3] + ((p["gamma2"] * p["k2"]) / p["A2"]) * u[1],
            ((-p["a3"]) / p["A3"]) * ss[2] + (((1.0 - p["gamma2"]) * p["k2"]) / p["A3"]) * u[1],
            ((-p["a4"]) / p["A4"]) * ss[3] + (((1.0 - p["gamma1"]) * p["k1"]) / p["A4"]) * u[0]]


def quadtank_levels(h, u, p, t):
    return [h[0], h[1]]


def central_differences(fun, x, n_out):
    """d fun_r / d x_c by central differences with h = 1e-6 max(1, |x_c|): [n_out, len(x)]"""
    J = np.empty((n_out, len(x)))
    for c in range(len(x)):
        h = 1e-6 * max(1.0, abs(x[c]))
        xp, xm = list(x), list(x)
        xp[c] += h
        xm[c] -= h
        J[:, c] = (np.asarray(fun(xp), dtype=np.float64) - np.asarray(fun(xm), dtype=np.float64)) / (xp[c] - xm[c])
    return J
