"""Shared pieces of the ensemble-Kalman-bank tests (test_enkf.py, test_gpu_enkf.py) and of tools/bench_enkf.py: the host build of
csrc/shared/llpf_enkf.h (tests/enkf_host.c) and a numpy restatement of the stochastic ensemble Kalman filter in its literal formulas
(np.mean, dense covariances, np.linalg.solve, slogdet) that takes the normal draws as arrays — it shares the generator with the header and
nothing else — and runs in float64 and np.longdouble."""
import ctypes as C

import numpy as np

from llpf_amd import _capi, _structs as S
import kf_host as kh
from kf_host import _dp, _p
import oracle_binding as ob
import ukf_common as uc

KIND_ORACLE, KIND_PENDULUM, KIND_SQUARE, KIND_LINEAR = 0, 2, 3, 4
CORRECT, PREDICT = 1, 2
STREAM_INIT, STREAM_DYNAMICS, STREAM_MEASURE = 0, 1, 4
OUTPUTS = _capi.KALMAN_OUTPUTS


def build_host(outdir):
    """the host build of tests/enkf_host.c in outdir"""
    run = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.POINTER(S.Model), _dp, _dp, C.c_int, C.c_uint64, C.c_uint32, C.c_double, C.c_int,
                                              _dp, _dp, C.c_int64, C.c_int, C.c_double] + [_dp] * 9
    return kh.build(outdir, "enkf_host.c", {"enkf_host_run": run,
                                            "enkf_host_init": [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(S.Model), C.c_uint64, C.c_uint32, _dp],
                                            "enkf_host_sum": (C.c_double, [_dp, C.c_int64])})


def _gs():
    return C.cast(ob.lib().orc_gauss_sample, C.c_void_p)


def kind_of(model):
    return KIND_ORACLE if model.model_id in (S.MODEL_LINEAR_GAUSSIAN, S.MODEL_QUADTANK_RK4) else None


def host_init(L, models, N, seed, n_reset=0):
    """the members reset! number n_reset draws, [F, N, nx] (Gaussian initial densities)"""
    F, nx = len(models), models[0].nx
    X = np.empty((F, N, nx))
    rc = L.enkf_host_init(F, nx, N, _gs(), (S.Model * F)(*models), int(seed), int(n_reset), _p(X))
    assert rc == 0, rc
    return X


def host_run(L, models, X, U, Y, T, seed, step0=0, rho=1.0, phases=CORRECT | PREDICT, per_filter=0, t_index0=0.0, kind=None):
    """the host build of the header over the filters `models` from the members X [F, N, nx] (not modified).  Returns the outputs in the
    device's layout with "members" [F, N, nx] and "state" (x [F, nx], R [F, nx, nx])."""
    F = len(models)
    m0 = models[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    kind = kind_of(m0) if kind is None else kind
    X = np.array(X, dtype=np.float64).reshape(F, -1, nx)
    N = X.shape[1]
    R2 = kh.f64(np.stack([S.gaussian_cov_matrix(m.measurement_density) for m in models]))
    out, outp = kh.outputs(T, F, nx, ny)
    sx, sR = np.empty((F, nx)), np.empty((F, nx, nx))
    f, g = uc.oracle_fns() if kind == KIND_ORACLE else (None, None)
    rc = L.enkf_host_run(F, nx, ny, nu, f, g, _gs(), kind, (S.Model * F)(*models), _p(R2), _p(X), N, int(seed), int(step0), float(rho),
                         int(phases), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter, float(t_index0), *outp, _p(sx), _p(sR))
    assert rc == 0, rc
    out["members"], out["state"] = X, (sx, sR)
    return out


def normals(seed, step, stream, nd, n, dtype=np.float64):
    """the standard normals of particles 0..n-1 at (step, stream) under key `seed`, [n, nd]"""
    return np.asarray(ob.normals(seed, step, stream, nd, n), dtype=dtype).reshape(n, nd)


def numpy_enkf(f, g, R1, R2, X0, U, Y, seed, Ts=1.0, t_index0=0.0, rho=1.0, dtype=np.float64, step0=0):
    """forward_trajectory of the stochastic EnKF in its literal formulas.  f(x, u, tau), g(x, u, tau) -> arrays for one member; the
    process and measurement noise are chol(R) @ xi with xi the generator's normals.  K = Pxy inv(S); x_i += K (y + v_i... - Y_i)."""
    dt = dtype
    R1, R2 = np.atleast_2d(np.asarray(R1, dtype=dt)), np.atleast_2d(np.asarray(R2, dtype=dt))
    L1, L2 = uc.Lin64.chol(R1) if dt is np.float64 else uc.LinLong.chol(R1), uc.Lin64.chol(R2) if dt is np.float64 else uc.LinLong.chol(R2)
    lin = uc.Lin64 if dt is np.float64 else uc.LinLong
    X = np.asarray(X0, dtype=dt).copy()
    N, nx = X.shape
    ny, T = R2.shape[0], Y.shape[0]
    out = dict(ll_steps=np.zeros(T, dtype=dt), x=np.empty((T, nx), dtype=dt), xt=np.empty((T, nx), dtype=dt), R=np.empty((T, nx, nx), dtype=dt),
               Rt=np.empty((T, nx, nx), dtype=dt), e=np.full((T, ny), np.nan, dtype=dt))
    cov = lambda A, B: (A - A.mean(axis=0)).T @ (B - B.mean(axis=0)) / dt(N - 1)
    for t in range(T):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        out["x"][t], out["R"][t] = X.mean(axis=0), cov(X, X)
        if not np.isnan(Y[t, 0]):
            Yv = np.stack([np.asarray(g(X[i], u, tau), dtype=dt) for i in range(N)])
            Pxy, Sm = cov(X, Yv), cov(Yv, Yv) + R2
            e = np.asarray(Y[t], dtype=dt) - Yv.mean(axis=0)
            Si = lin.inv(Sm)
            V = normals(seed, step0 + t, STREAM_MEASURE, ny, N, dt) @ L2.T
            X = X + (np.asarray(Y[t], dtype=dt) - (Yv + V)) @ (Pxy @ Si).T
            out["ll_steps"][t] = -(ny * np.log(2 * dt(np.pi)) + lin.logdet(Sm) + e @ Si @ e) / 2
            out["e"][t] = e
        out["xt"][t], out["Rt"][t] = X.mean(axis=0), cov(X, X)
        Wn = normals(seed, step0 + t, STREAM_DYNAMICS, nx, N, dt) @ L1.T
        X = np.stack([np.asarray(f(X[i], u, tau), dtype=dt) for i in range(N)]) + Wn
        if rho != 1.0:
            xb = X.mean(axis=0)
            X = xb + dt(rho) * (X - xb)
    out["ll"] = out["ll_steps"].sum()
    out["members"] = X
    return out
