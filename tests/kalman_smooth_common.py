"""Shared pieces of the Kalman-smoother tests (test_kalman_smooth.py, test_gpu_kalman_smooth.py) and of tools/bench_kalman.py --smooth:
the host build of llpf_kf_smooth (tests/kalman_host.c), a numpy restatement of the reference's RTS smoother in its literal formulas
(src/smoothing.jl:10-102), and an oracle that shares nothing with the recursion: the conditional mean and covariance of every state under
the dense joint Gaussian of all states and all measurements."""
import numpy as np

import kalman_common as kc
import kf_host as kh
from kf_host import _p

build_host_smooth = kc.build_host      # the Kalman twin is one library: kf_host_smooth is in it


def host_smooth(L, systems, U, fw, T, per_filter=0):
    """the host build of the smoother over filters `systems` [(model, D)], applied to the forward outputs fw (kc.host_run's or the
    device's: xt [T, F, nx], Rt [T, F, nx, nx]).  Returns {"xT": [T, F, nx], "RT": [T, F, nx, nx]}."""
    F = len(systems)
    m0 = systems[0][0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    R1, R2, _, _ = kh.pack_models([m for m, _ in systems])
    out, iop = kh.smooth_io(fw, T, F, nx)
    rc = L.kf_host_smooth(F, nx, ny, nu, *map(_p, kc.stacked_matrices(systems)), _p(R1), _p(R2), _p(kh.inputs(U, nu)), T, per_filter, *iop)
    assert rc == 0
    return out


def numpy_smooth(mats, x, xt, R, Rt):
    """the reference's smooth(sol, kf, u, y) in its literal formulas over one filter's forward solution (x, R the priors, xt, Rt the
    posteriors): C = Rt[t] A' / R[t+1], xT[t] = xt[t] + C (xT[t+1] - x[t+1]), RT[t] = Rt[t] + symmetrize(C (RT[t+1] - R[t+1]) C')"""
    A = mats["A"]
    T = xt.shape[0]
    xT, RT = np.empty_like(xt), np.empty_like(Rt)
    xT[-1], RT[-1] = xt[-1], Rt[-1]
    for t in range(T - 2, -1, -1):
        Cs = np.linalg.solve(R[t + 1].T, (Rt[t] @ A.T).T).T           # (Rt A') / R[t+1]
        xT[t] = xt[t] + Cs @ (xT[t + 1] - x[t + 1])
        RT[t] = Rt[t] + kc._sym(Cs @ (RT[t + 1] - R[t + 1]) @ Cs.T)
    return xT, RT


def joint_smoother(mats, U, Y):
    """E[x_t | all y] and Cov[x_t | all y] from the dense joint Gaussian of (x_0 .. x_{T-1}, the observed y_t): x = m + H xi with
    xi = (x_0 - mean(d0), w_0, ..., w_{T-2}), xi ~ N(0, blockdiag(P0, R1, ...)); y_t = C x_t + D u_t + e_t.  Rows whose first element is
    NaN are left out.  Shares nothing with the recursion."""
    A, B, Cm, D, R1, R2 = (mats[k] for k in ("A", "B", "C", "D", "R1", "R2"))
    nx, ny = A.shape[0], Cm.shape[0]
    T = Y.shape[0]
    nu = B.shape[1]
    m = np.empty((T, nx))
    m[0] = mats["x0"]
    for t in range(T - 1):
        m[t + 1] = A @ m[t] + (B @ U[t] if nu else 0.0)
    Ap = [np.eye(nx)]
    for _ in range(T):
        Ap.append(A @ Ap[-1])
    H = np.zeros((T * nx, T * nx))
    for t in range(T):
        H[t * nx:(t + 1) * nx, 0:nx] = Ap[t]
        for s in range(t):
            H[t * nx:(t + 1) * nx, (s + 1) * nx:(s + 2) * nx] = Ap[t - 1 - s]
    Q = np.zeros((T * nx, T * nx))
    Q[:nx, :nx] = mats["P0"]
    for s in range(1, T):
        Q[s * nx:(s + 1) * nx, s * nx:(s + 1) * nx] = R1
    Sx = H @ Q @ H.T
    obs = [t for t in range(T) if not np.isnan(Y[t, 0])]
    G = np.zeros((len(obs) * ny, T * nx))
    my = np.empty(len(obs) * ny)
    yv = np.empty(len(obs) * ny)
    Re = np.zeros((len(obs) * ny, len(obs) * ny))
    for j, t in enumerate(obs):
        G[j * ny:(j + 1) * ny, t * nx:(t + 1) * nx] = Cm
        my[j * ny:(j + 1) * ny] = Cm @ m[t] + (D @ U[t] if nu else 0.0)
        yv[j * ny:(j + 1) * ny] = Y[t]
        Re[j * ny:(j + 1) * ny, j * ny:(j + 1) * ny] = R2
    Sxy = Sx @ G.T
    Sy = G @ Sxy + Re
    K = np.linalg.solve(Sy, Sxy.T).T
    mean = m.reshape(-1) + K @ (yv - my)
    cov = Sx - K @ Sxy.T
    xT = mean.reshape(T, nx)
    RT = np.stack([cov[t * nx:(t + 1) * nx, t * nx:(t + 1) * nx] for t in range(T)])
    return xT, RT
