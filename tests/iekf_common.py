"""Shared pieces of the iterated-extended-Kalman-bank tests (test_iekf.py, test_gpu_iekf.py) and of tools/bench_ekf.py --iterated: the
host build of the iterated filter of csrc/shared/llpf_ekf.h (tests/ekf_host.c: iekf_host_run) and a numpy restatement of the textbook
iterated extended Kalman filter (Bell & Cathey 1993) in its literal formulas (np.linalg.inv, K = R C' inv(S), (I - K C) R, slogdet) that
shares nothing with the header and runs in float64 and np.longdouble."""
import numpy as np

from llpf_amd import _structs as S
import ekf_common as ec
import ukf_common as uc

build_host = ec.build_host      # the extended twin is one library: iekf_host_run is in it


def host_run(L, models, U, Y, T, maxiters, epsilon, per_filter=0, t_index0=0.0, state=None, kind=None):
    """ekf_common.host_run for the iterated filter at (maxiters, epsilon): the outputs in the device's layout, with "iters" [T, F] (the
    linearisations each step ran, 0 at a missing row), and the final state"""
    return ec.host_run(L, models, U, Y, T, per_filter, t_index0, state, kind, iterations=(maxiters, epsilon))


def pendulum_bank_models(n, model_id=None):
    """n pendulum filters (ukf_common.pendulum_model's densities) with per-filter parameters and per-filter d0: the prior angle runs
    over 0.2 .. 1.4, so the filters of one wave need different numbers of linearisations at the first steps.  model_id: the compiled
    snippet's (default: the linear-Gaussian id the host shim ignores)"""
    g = S.make_gaussian
    out = []
    for k in range(n):
        m = S.make_lg_model(np.eye(2), np.zeros((2, 1)), np.array([[1.0, 0.0]]), g(np.zeros(2), np.array([1e-4, 4e-3])), g(np.zeros(1), 0.05 ** 2),
                            g(np.array([0.2 + 1.2 * ((k * 37) % 64) / 63.0, 0.0]), np.array([0.3, 0.3])), Ts=0.05)
        m.qt[0], m.qt[1] = 9.81 * (1 + 0.002 * k), 0.05 + 0.001 * (k % 10)
        if model_id is not None:
            m.model_id = model_id
        out.append(m)
    return out


# ---- the restatement ----
def numpy_iekf_correct(g, gjac, R2, xb, Rb, y, u, tau, maxiters, epsilon, lin=uc.Lin64):
    """one iterated correct! from the prior (xb, Rb) in the literal formulas.  From x_0 = xb, for i = 0, 1, ...:
    C = dg/dx(x_i);  r = y - g(x_i) - C (xb - x_i);  S = symmetrize(C Rb C') + R2;  K = Rb C' inv(S);  x_{i+1} = xb + K r;
    R = symmetrize((I - K C) Rb);  ll = log N(r; 0, S); until i + 1 == maxiters or not max |x_{i+1} - x_i| > epsilon.
    Returns (xt, Rt, ll, r, linearisations)."""
    dt = lin.dtype
    nx, ny = xb.shape[0], R2.shape[0]
    I = np.eye(nx, dtype=dt)
    xi = xb.copy()
    i = 0
    while True:
        Cm = np.asarray(gjac(xi, u, tau), dtype=dt).reshape(ny, nx)
        r = np.asarray(y, dtype=dt) - np.asarray(g(xi, u, tau), dtype=dt) - Cm @ (xb - xi)
        Sm = uc.symmetrize(Cm @ Rb @ Cm.T) + R2
        Si = lin.inv(Sm)
        K = Rb @ Cm.T @ Si
        xn = xb + K @ r
        Rn = uc.symmetrize((I - K @ Cm) @ Rb)
        ll = -(ny * np.log(2 * dt(np.pi)) + lin.logdet(Sm) + r @ Si @ r) / 2
        move = np.max(np.abs(xn - xi))
        xi = xn
        i += 1
        if i == maxiters or not move > epsilon:
            return xn, Rn, ll, r, i


def numpy_iekf(f, g, fjac, gjac, R1, R2, x0, P0, U, Y, maxiters, epsilon, Ts=1.0, t_index0=0.0, lin=uc.Lin64):
    """forward_trajectory of the iterated EKF: ekf_common.numpy_ekf with numpy_iekf_correct in the place of its correct!"""
    dt = lin.dtype
    R1, R2 = np.asarray(R1, dtype=dt), np.asarray(R2, dtype=dt)
    x, R = np.asarray(x0, dtype=dt).copy(), np.asarray(P0, dtype=dt).copy()
    nx, ny, T = x.shape[0], R2.shape[0], Y.shape[0]
    out = dict(ll_steps=np.zeros(T, dtype=dt), x=np.empty((T, nx), dtype=dt), xt=np.empty((T, nx), dtype=dt), R=np.empty((T, nx, nx), dtype=dt),
               Rt=np.empty((T, nx, nx), dtype=dt), e=np.full((T, ny), np.nan, dtype=dt), iters=np.zeros(T, dtype=np.int32))
    for t in range(T):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        out["x"][t], out["R"][t] = x, R
        if not np.isnan(Y[t, 0]):
            x, R, out["ll_steps"][t], out["e"][t], out["iters"][t] = numpy_iekf_correct(g, gjac, R2, x, R, Y[t], u, tau, maxiters, epsilon, lin)
        out["xt"][t], out["Rt"][t] = x, R
        A = np.asarray(fjac(x, u, tau), dtype=dt).reshape(nx, nx)
        x = np.asarray(f(x, u, tau), dtype=dt)
        R = uc.symmetrize(A @ R @ A.T) + R1
    out["ll"] = out["ll_steps"].sum()
    return out


def square_fg_jacs(dtype=np.float64):
    """f(x) = x, g(x) = x_0^2 and their Jacobians for the restatement (ekf_common.SQUARE_JAC_SRC, nx = 1)"""
    f = lambda x, u, tau: np.array([x[0]], dtype=dtype)
    g = lambda x, u, tau: np.array([x[0] * x[0]], dtype=dtype)
    return (f, g), (lambda x, u, tau: np.eye(1, dtype=dtype), lambda x, u, tau: np.array([[2 * x[0]]], dtype=dtype))


def stationarity(g, gjac, R2, xb, Rb, y, x):
    """the gradient of -log p(x | y) for the prior N(xb, Rb) and y = g(x) + e, e ~ N(0, R2), at x: -C' R2^-1 (y - g(x)) + Rb^-1 (x - xb)
    with C = dg/dx(x).  Returns (its infinity norm, the larger infinity norm of its two terms)."""
    u = np.zeros(0)
    Cm = np.asarray(gjac(x, u, 0.0), dtype=np.float64).reshape(R2.shape[0], x.shape[0])
    a = -Cm.T @ np.linalg.solve(R2, np.asarray(y, dtype=np.float64) - g(x, u, 0.0))
    b = np.linalg.solve(Rb, x - xb)
    return float(np.max(np.abs(a + b))), float(max(np.max(np.abs(a)), np.max(np.abs(b))))
