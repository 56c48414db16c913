"""Shared pieces of the IMM-bank tests (test_imm.py, test_gpu_imm.py) and of tools/bench_imm.py: the host build of
csrc/shared/llpf_imm.h (tests/imm_host.c), random IMM filters over the stable systems of kalman_common, and a numpy restatement of the
IMM step in its literal textbook formulas (Blom & Bar-Shalom 1988) that shares nothing with the header."""
import ctypes as C

import numpy as np

from llpf_amd import _capi
import kalman_common as kc
import kf_host as kh
from kf_host import _dp, _p

OUTS = _capi.IMM_OUTPUTS


def build_host(outdir):
    """the host build of tests/imm_host.c in outdir (imm_host_run, imm_host_combine)"""
    return kh.build(outdir, "imm_host.c", {"imm_host_run": [C.c_int] * 6 + [_dp] * 10 + [_dp, _dp, C.c_int64, C.c_int] + [_dp] * 8,
                                           "imm_host_combine": [C.c_int] * 3 + [_dp] * 5})


def random_P(rng, M):
    """a row-stochastic transition matrix that favours staying, every entry >= 0.02"""
    P = rng.uniform(0.2, 1.0, (M, M)) + 2.0 * np.eye(M)
    return P / P.sum(axis=1, keepdims=True)


def random_mu(rng, M):
    mu = rng.uniform(0.2, 1.0, M)
    mu /= mu.sum()
    mu[0] += 1.0 - mu.sum()
    return mu


def random_imm(rng, M, nx, ny, nu, kind=0, D=True):
    """one IMM: {"systems": [(llpf_model, D [ny, nu])] * M, "P": [M, M], "mu0": [M]} over M stable random systems of one shape"""
    return dict(systems=[kc.random_system(rng, nx, ny, nu, (kind + j) % 3, D=D) for j in range(M)], P=random_P(rng, M), mu0=random_mu(rng, M))


def bank_args(imms):
    """models [F][M], D [F, M, ny, nu], P [F, M, M], mu0 [F, M] as _capi.IMMBankHandle takes them"""
    return ([[m for m, _ in s["systems"]] for s in imms], np.stack([np.stack([D for _, D in s["systems"]]) for s in imms]),
            np.stack([s["P"] for s in imms]), np.stack([s["mu0"] for s in imms]))


def bank(imms, interact=True):
    return _capi.IMMBankHandle(0, *bank_args(imms), interact)


def initial_state(imms):
    """(mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx]) of a reset"""
    mats = [[kc.matrices(m, D) for m, D in s["systems"]] for s in imms]
    return (kh.f64(np.stack([s["mu0"] for s in imms])), kh.f64([[mm["x0"] for mm in row] for row in mats]),
            kh.f64([[mm["P0"] for mm in row] for row in mats]))


def host_run(L, imms, U, Y, T, per_filter=0, state=None, interact=True):
    """the host build of the header over the IMMs `imms`; state = (mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx]) or None (reset).
    Returns the outputs in the device's layout and the final state (mu, x_modes, R_modes)."""
    F, M = len(imms), len(imms[0]["systems"])
    m0 = imms[0]["systems"][0][0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    flat = [sys for s in imms for sys in s["systems"]]
    ABCD = kc.stacked_matrices(flat)
    R1, R2, _, _ = kh.pack_models([m for m, _ in flat])
    mu, xm, Rm = (np.array(a, dtype=np.float64) for a in (initial_state(imms) if state is None else state))
    P = kh.f64(np.stack([s["P"] for s in imms]))
    out = dict(ll=np.empty(F), ll_steps=np.empty((T, F)), x=np.empty((T, F, nx)), xt=np.empty((T, F, nx)), R=np.empty((T, F, nx, nx)),
               Rt=np.empty((T, F, nx, nx)), mu=np.empty((T, F, M)), ll_modes=np.empty((T, F, M)))
    rc = L.imm_host_run(F, M, nx, ny, nu, 1 if interact else 0, *map(_p, ABCD), _p(R1), _p(R2), _p(P), _p(mu), _p(xm), _p(Rm),
                        _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter, *[_p(out[k]) for k in ("ll",) + OUTS])
    assert rc == 0
    return out, (mu, xm, Rm)


def host_combine(L, mu, xm, Rm):
    """the combined (x [F, nx], R [F, nx, nx]) of a state, by the host build of the header"""
    mu, xm, Rm = kh.f64(mu), kh.f64(xm), kh.f64(Rm)
    F, M, nx = xm.shape
    x, R = np.empty((F, nx)), np.empty((F, nx, nx))
    assert L.imm_host_combine(F, M, nx, _p(mu), _p(xm), _p(Rm), _p(x), _p(R)) == 0
    return x, R


def same(g, h, keys=OUTS + ("ll",), what=""):
    for k in keys:
        assert kc.bits_equal(g[k], h[k]), (what, k)


def _sym(M):
    return 0.5 * (M + M.T)


def _moments(w, xs, Rs):
    """mean and covariance of the mixture sum_j w_j N(x_j, R_j)"""
    x = sum(wj * xj for wj, xj in zip(w, xs))
    R = sum(wj * (Rj + np.outer(xj - x, xj - x)) for wj, xj, Rj in zip(w, xs, Rs))
    return x, R


def numpy_reference(imm, U, Y, interact=True):
    """the IMM recursion in its literal textbook formulas, one filter: per step the combined prior, the measurement update of every
    mode (K = R C' S^-1, ll_j = logpdf(N(0, S), e)), mu_j proportional to (P' mu)_j exp(ll_j) with ll[t] the log of the normaliser, the
    combined posterior, the interaction (mu_ij = P_ij mu_i / c_j; mixed mean and covariance of every mode), the time update"""
    mats = [kc.matrices(m, D) for m, D in imm["systems"]]
    M, P = len(mats), np.asarray(imm["P"], float)
    nx, T = mats[0]["A"].shape[0], Y.shape[0]
    xs, Rs = [mm["x0"].copy() for mm in mats], [mm["P0"].copy() for mm in mats]
    mu = np.asarray(imm["mu0"], float).copy()
    out = dict(ll_steps=np.zeros(T), x=np.empty((T, nx)), xt=np.empty((T, nx)), R=np.empty((T, nx, nx)), Rt=np.empty((T, nx, nx)),
               mu=np.empty((T, M)), ll_modes=np.zeros((T, M)))
    for t in range(T):
        u = U[t] if U is not None and U.shape[1] else np.zeros(0)
        out["x"][t], out["R"][t] = _moments(mu, xs, Rs)
        cbar = P.T @ mu
        if np.isnan(Y[t, 0]):
            mu = cbar
        else:
            for j, mm in enumerate(mats):
                e = Y[t] - (mm["C"] @ xs[j] + mm["D"] @ u)
                Sm = _sym(mm["C"] @ Rs[j] @ mm["C"].T) + mm["R2"]
                K = (Rs[j] @ mm["C"].T) @ np.linalg.inv(Sm)
                xs[j] = xs[j] + K @ e
                Rs[j] = _sym((np.eye(nx) - K @ mm["C"]) @ Rs[j])
                out["ll_modes"][t, j] = -0.5 * (len(e) * np.log(2 * np.pi) + np.linalg.slogdet(Sm)[1] + e @ np.linalg.solve(Sm, e))
            lw = np.log(cbar) + out["ll_modes"][t]
            out["ll_steps"][t] = np.logaddexp.reduce(lw)
            mu = np.exp(lw - out["ll_steps"][t])
        out["mu"][t] = mu
        out["xt"][t], out["Rt"][t] = _moments(mu, xs, Rs)
        if interact:
            cbar = P.T @ mu
            mixed = [_moments(P[:, j] * mu / cbar[j], xs, Rs) for j in range(M)]
            xs, Rs = [m[0] for m in mixed], [m[1] for m in mixed]
        for j, mm in enumerate(mats):
            xs[j] = mm["A"] @ xs[j] + mm["B"] @ u
            Rs[j] = _sym(mm["A"] @ Rs[j] @ mm["A"].T) + mm["R1"]
    out["ll"] = out["ll_steps"].sum()
    return out
