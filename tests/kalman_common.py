"""Shared pieces of the Kalman-bank tests (test_kalman.py, test_gpu_kalman.py) and of tools/bench_kalman.py: the host build of
csrc/shared/llpf_kalman.h (tests/kalman_host.c), random stable linear-Gaussian systems in every covariance kind, and a numpy
restatement of the reference's correct! / predict! in its literal formulas (src/filtering.jl, src/kalman.jl)."""
import ctypes as C

import numpy as np

from llpf_amd import _capi, _structs as S
import kf_host as kh
from kf_host import ROOT, SHARED, _dp, _p

KINDS = (S.COV_SCAL, S.COV_DIAG, S.COV_FULL)


def build_host(outdir):
    """the host build of tests/kalman_host.c in outdir (kf_host_run and kf_host_smooth)"""
    return kh.build(outdir, "kalman_host.c", {"kf_host_run": [C.c_int] * 4 + [_dp] * 8 + [_dp, _dp, C.c_int64, C.c_int] + [_dp] * 7,
                                              "kf_host_smooth": [C.c_int] * 4 + [_dp] * 6 + [_dp, C.c_int64, C.c_int] + [_dp] * 4})


def _gauss(rng, n, kind, scale=1.0, mu=None):
    """a positive definite covariance of the given storage kind, as an llpf_gaussian"""
    mu = np.zeros(n) if mu is None else mu
    if kind == S.COV_SCAL:
        return S.make_gaussian(mu, float(scale * rng.uniform(0.3, 1.5)))
    if kind == S.COV_DIAG:
        return S.make_gaussian(mu, scale * rng.uniform(0.3, 1.5, n))
    M = rng.standard_normal((n, n))
    return S.make_gaussian(mu, scale * (M @ M.T / n + 0.3 * np.eye(n)), S.COV_FULL)


def random_system(rng, nx, ny, nu, kind=0, D=True):
    """a stable random system (spectral radius 0.9) as (llpf_model, D [ny, nu]); the covariances of R1, R2, d0 cycle through the kinds"""
    A = rng.standard_normal((nx, nx))
    A *= 0.9 / max(np.max(np.abs(np.linalg.eigvals(A))), 1e-3)
    B = rng.standard_normal((nx, nu))
    Cm = rng.standard_normal((ny, nx))
    Dm = rng.standard_normal((ny, nu)) if D else np.zeros((ny, nu))
    k = [KINDS[(kind + i) % 3] for i in range(3)]
    m = S.make_lg_model(A, B, Cm, _gauss(rng, nx, k[0], 0.2), _gauss(rng, ny, k[1], 0.5), _gauss(rng, nx, k[2], 1.0, rng.standard_normal(nx)))
    return m, Dm


def matrices(m, D):
    nx, ny, nu = m.nx, m.ny, m.nu
    A = np.array(m.A[:nx * nx]).reshape(nx, nx)
    B = np.array(m.B[:nx * nu]).reshape(nx, nu)
    Cm = np.array(m.C[:ny * nx]).reshape(ny, nx)
    return dict(A=A, B=B, C=Cm, D=np.asarray(D, float).reshape(ny, nu), R1=S.gaussian_cov_matrix(m.dynamics_density),
                R2=S.gaussian_cov_matrix(m.measurement_density), x0=S.gaussian_mean(m.initial_density),
                P0=S.gaussian_cov_matrix(m.initial_density))


def stacked_matrices(systems):
    """A [F, nx, nx], B [F, nx, nu], C [F, ny, nx], D [F, ny, nu] of the filters `systems` [(model, D)], as the host twin takes them"""
    mats = [matrices(m, D) for m, D in systems]
    return [kh.f64(np.stack([mm[k] for mm in mats])) for k in ("A", "B", "C", "D")]


def simulate(rng, mats, T, missing=()):
    """data from the model (numpy), U [T, nu], Y [T, ny]; rows in `missing` get a NaN first element"""
    A, B, Cm, D = mats["A"], mats["B"], mats["C"], mats["D"]
    nx, nu, ny = A.shape[0], B.shape[1], Cm.shape[0]
    U = rng.standard_normal((T, nu))
    Y = np.empty((T, ny))
    x = mats["x0"] + np.linalg.cholesky(mats["P0"]) @ rng.standard_normal(nx)
    L1, L2 = np.linalg.cholesky(mats["R1"]), np.linalg.cholesky(mats["R2"])
    for t in range(T):
        Y[t] = Cm @ x + D @ U[t] + L2 @ rng.standard_normal(ny)
        x = A @ x + B @ U[t] + L1 @ rng.standard_normal(nx)
    for t in missing:
        Y[t, 0] = np.nan
    return U, Y


def host_run(L, systems, U, Y, T, per_filter=0, state=None):
    """the host build of the header over filters `systems` [(model, D)]; state = (x0 [F, nx], P0 [F, nx, nx]) or None (reset).
    Returns the outputs in the device's layout and the final state."""
    F = len(systems)
    m0 = systems[0][0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    ABCD = stacked_matrices(systems)
    R1, R2, x0, P0 = kh.pack_models([m for m, _ in systems], state)
    out, outp = kh.outputs(T, F, nx, ny)
    rc = L.kf_host_run(F, nx, ny, nu, *map(_p, ABCD), _p(R1), _p(R2), _p(x0), _p(P0), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter, *outp)
    assert rc == 0
    return out, (x0, P0)


def _sym(M):
    return 0.5 * (M + M.T)


def numpy_reference(mats, U, Y):
    """the reference's forward_trajectory in its literal formulas: correct! (K = (R C')/S_chol, x += K e, R = symmetrize((I - K C) R),
    ll = logpdf(MvNormal(0, S), e)), then predict! (x = A x + B u, R = symmetrize(A R A') + R1)"""
    A, B, Cm, D, R1, R2 = (mats[k] for k in ("A", "B", "C", "D", "R1", "R2"))
    nx, ny = A.shape[0], Cm.shape[0]
    T = Y.shape[0]
    x, R = mats["x0"].copy(), mats["P0"].copy()
    out = dict(ll_steps=np.zeros(T), x=np.empty((T, nx)), xt=np.empty((T, nx)), R=np.empty((T, nx, nx)), Rt=np.empty((T, nx, nx)),
               e=np.full((T, ny), np.nan))
    for t in range(T):
        u = U[t] if U.shape[1] else np.zeros(0)
        out["x"][t], out["R"][t] = x, R
        if not np.isnan(Y[t, 0]):
            e = Y[t] - (Cm @ x + D @ u)
            Sm = _sym(Cm @ R @ Cm.T) + R2
            np.linalg.cholesky(Sm)
            K = (R @ Cm.T) @ np.linalg.inv(Sm)
            x = x + K @ e
            R = _sym((np.eye(nx) - K @ Cm) @ R)
            out["ll_steps"][t] = -0.5 * (ny * np.log(2 * np.pi) + np.linalg.slogdet(Sm)[1] + e @ np.linalg.solve(Sm, e))
            out["e"][t] = e
        out["xt"][t], out["Rt"][t] = x, R
        x = A @ x + B @ u
        R = _sym(A @ R @ A.T) + R1
    out["ll"] = out["ll_steps"].sum()
    return out


def close(a, b, rtol=1e-10):
    """|a - b| <= rtol (|b| + max |b| of the trailing matrix / vector): relative to the scale of each step's quantity; NaN where b is NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(b)
    scale = np.abs(np.where(ok, b, 0.0))
    if b.ndim >= 2:
        scale = scale + np.max(scale.reshape(b.shape[0], -1), axis=1).reshape((-1,) + (1,) * (b.ndim - 1))
    return bool(np.all(np.abs(a[ok] - b[ok]) <= rtol * (scale[ok] + 1e-300)))


def bits_equal(a, b):
    """the same bits, every NaN counted as one value (a NaN's sign and payload depend on the hardware that produced it)"""
    a, b = np.array(a, dtype=np.float64), np.array(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    a[np.isnan(a)] = np.nan
    b[np.isnan(b)] = np.nan
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ------------------------------------------------------------------------------------------------
# helpers of the GPU tests of the Kalman and the unscented banks
# ------------------------------------------------------------------------------------------------
OUTS = _capi.KALMAN_OUTPUTS


def _data(rng, T, nu, ny, missing=()):
    """shared inputs U [T, nu] and measurements Y [T, ny], the first output missing (NaN) at the steps `missing`"""
    U = rng.standard_normal((T, nu))
    Y = 2.0 * rng.standard_normal((T, ny))
    for t in missing:
        Y[t, 0] = np.nan
    return U, Y


def _same(g, h, keys=OUTS + ("ll",), what=""):
    for k in keys:
        assert bits_equal(g[k], h[k]), (what, k)
