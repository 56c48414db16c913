"""Shared pieces of the unscented-smoother tests (test_ukf_smooth.py, test_gpu_ukf_smooth.py) and of tools/bench_ukf.py --smooth: the host
build of llpf_ukf_smooth_finish (tests/ukf_host.c) around the oracle's dynamics or the C twins of the test snippets, and a numpy
restatement of the textbook additive-noise unscented Rauch-Tung-Striebel smoother (Sarkka 2008) in its literal formulas, in float64
(ukf_common.Lin64) and in np.longdouble (ukf_common.LinLong), that shares nothing with the header."""
import numpy as np

from llpf_amd import _structs as S
import kf_host as kh
from kf_host import _p
import ukf_common as uc

build_host_smooth = uc.build_host      # the unscented twin is one library: ukf_host_smooth is in it


def host_smooth(L, models, w, U, fw, T, per_filter=0, t_index0=0.0, twin=0):
    """the host build of the smoother over the filters `models` (llpf_model descriptors), applied to the forward outputs fw
    (uc.host_run's or the device's: xt [T, F, nx], Rt [T, F, nx, nx]).  Returns {"xT": [T, F, nx], "RT": [T, F, nx, nx]}."""
    F = len(models)
    m0 = models[0]
    nx, nu = m0.nx, m0.nu
    arr = (S.Model * F)(*models)
    R1 = kh.pack_models(models)[0]
    wv = np.array(w, dtype=np.float64)
    out, iop = kh.smooth_io(fw, T, F, nx)
    f = None if twin else uc.oracle_fns()[0]
    rc = L.ukf_host_smooth(F, nx, nu, f, twin, arr, _p(R1), _p(wv), _p(kh.inputs(U, nu)), T, per_filter, float(t_index0), *iop)
    assert rc == 0
    return out


def numpy_ukf_smooth(f, R1, w, U, xt, Rt, Ts=1.0, t_index0=0.0, lin=uc.Lin64):
    """the unscented RTS smoother in its literal formulas over one filter's posteriors xt [T, nx], Rt [T, nx, nx]; f(x, u, tau) -> array.
    From xT[T-1] = xt[T-1], RT[T-1] = Rt[T-1], for t = T-2 .. 0 with tau = (t_index0 + t) Ts:
        X_i the points of (xt[t], Rt[t]);  X'_i = f(X_i, u[t], tau);  x- = sum wm_i X'_i;  R- = sum wc_i dX'_i dX'_i' + R1;
        G = sum wc_i dX'_i (X_i - xt[t])';  J = G' R-^-1;  xT[t] = xt[t] + J (xT[t+1] - x-);  RT[t] = Rt[t] + J (RT[t+1] - R-) J'
    Raises LinAlgError when Rt[t] or R- is not positive definite."""
    dt = lin.dtype
    gamma, wm0, wc0, wi = (dt(v) for v in w)
    R1 = np.asarray(R1, dtype=dt)
    xt, Rt = np.asarray(xt, dtype=dt), np.asarray(Rt, dtype=dt)
    T, nx = xt.shape
    wm = np.array([wm0] + [wi] * (2 * nx), dtype=dt)
    wc = np.array([wc0] + [wi] * (2 * nx), dtype=dt)
    xT, RT = np.empty_like(xt), np.empty_like(Rt)
    xT[-1], RT[-1] = xt[-1], Rt[-1]
    for t in range(T - 2, -1, -1):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        Cf = lin.chol(Rt[t])
        X = np.stack([xt[t]] + [xt[t] + gamma * Cf[:, i] for i in range(nx)] + [xt[t] - gamma * Cf[:, i] for i in range(nx)])
        Xn = np.stack([np.asarray(f(Xi, u, tau), dtype=dt) for Xi in X])
        xm = wm @ Xn
        dXn = Xn - xm
        Rm = uc.symmetrize((dXn.T * wc) @ dXn) + R1
        G = (dXn.T * wc) @ (X - xt[t])
        lin.chol(Rm)
        J = G.T @ lin.inv(Rm)
        xT[t] = xt[t] + J @ (xT[t + 1] - xm)
        RT[t] = Rt[t] + uc.symmetrize(J @ (RT[t + 1] - Rm) @ J.T)
    return xT, RT
