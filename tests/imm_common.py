"""Shared pieces of the IMM-bank tests (test_imm.py, test_imm_ekf.py, test_gpu_imm.py, test_gpu_imm_ekf.py) and of tools/bench_imm.py:
the host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_kalman.h and over csrc/shared/llpf_ekf.h (tests/imm_ekf_host.c, which
includes imm_host.c, ekf_host.c and kalman_host.c: one library, one set of compiler flags, the six stages once in kf_host_frame.h), IMMs
over random stable systems and over the model lists of the extended-Kalman tests, and a numpy restatement of the IMM over first-order
extended Kalman filters in its literal textbook formulas (Blom & Bar-Shalom 1988; np.linalg.inv, dense matrices) that shares nothing
with the headers and runs in float64 and np.longdouble; the Kalman IMM is that restatement over linear modes.

An IMM here is {"models": [llpf_model] * M, "D": None or [M, ny, nu], "P": [M, M], "mu0": [M]}.  D is None: a mode is a first-order
extended Kalman filter and the modes are descriptors of ONE model type that differ by their parameters, R1, R2 and d0 (an extended bank).
Otherwise the modes are Kalman filters of linear-Gaussian descriptors with the feedthrough D."""
import contextlib
import ctypes as C

import numpy as np

from llpf_amd import _capi, _structs as S
import ekf_common as ec
import kalman_common as kc
import kf_gpu_frame as kg
import kf_host as kh
from kf_host import _dp, _p
import ukf_common as uc

OUTS = _capi.IMM_OUTPUTS

# the quad-tank as a snippet around the shared Jacobian header (csrc/shared/llpf_quadtank_jac.h is part of every run-time program): the
# built-in model's expressions — its coefficients formed on the device by llpf_qt_coef_set where the built-in reads the host's — so the
# two must agree to the bit
QUADTANK_JAC_SRC = r'''
struct UserModel {
    static constexpr bool RB = false;
    llpf_qt_coef c;
    double u0, u1, t0;
    DEV void prepare(const ModelD* m, const double* u, double t) {
        llpf_qt_coef_set(m->qt, m->Ts, m->supersample, &c);
        u0 = u[0];  u1 = u[1];  t0 = t;
    }
    DEV void dynamics(const double* x, double* out) const { double J[16]; llpf_qt_dynamics_jac(&c, u0, u1, t0, x, out, J); }
    DEV void measurement(const double* x, double* out) const { out[0] = x[0]; out[1] = x[1]; }
    DEV void dynamics_jac(const double* x, double* fx, double* J) const { llpf_qt_dynamics_jac(&c, u0, u1, t0, x, fx, J); }
    DEV void measurement_jac(const double* x, double* gx, double* J) const {
        gx[0] = x[0];  gx[1] = x[1];
        for (int i = 0; i < 8; ++i) J[i] = 0.0;
        J[0] = 1.0;  J[5] = 1.0;
    }
};
'''


def build_host(outdir):
    """the host build of tests/imm_ekf_host.c in outdir: imm_ekf_host_run, imm_host_run and imm_host_combine, and with them ekf_host_run
    as ekf_common.build_host binds it"""
    head, tail = [C.c_int] * 6, [_dp, _dp, C.c_int64, C.c_int]
    return kh.build(outdir, "imm_ekf_host.c", {
        "imm_ekf_host_run": head + [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(S.Model)] + [_dp] * 6 + tail + [C.c_double] + [_dp] * 8,
        "ekf_host_run": kh.MODEL_HEAD + [_dp] * 2 + kh.RUN_TAIL,
        "imm_host_run": head + [_dp] * 10 + tail + [_dp] * 8,
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


def imm(models, P=None, mu0=None, rng=None, D=None):
    """one IMM over the descriptors `models`; P, mu0 random unless given"""
    M = len(models)
    return dict(models=list(models), D=D, P=random_P(rng, M) if P is None else np.asarray(P, float),
                mu0=random_mu(rng, M) if mu0 is None else np.asarray(mu0, float))


def random_imm(rng, M, nx, ny, nu, kind=0, D=True):
    """one Kalman IMM over M stable random systems of one shape (kalman_common.random_system; D = False: zero feedthrough)"""
    systems = [kc.random_system(rng, nx, ny, nu, (kind + j) % 3, D=D) for j in range(M)]
    return imm([m for m, _ in systems], rng=rng, D=[Dj for _, Dj in systems])


def lg_imms(rng, F, M, nx, ny, nu):
    """F extended IMMs over M random stable linear-Gaussian systems each (kalman_common.random_system, D = 0)"""
    return [imm([kc.random_system(rng, nx, ny, nu, (k + j) % 3, D=False)[0] for j in range(M)], rng=rng) for k in range(F)]


def grouped(models, rng, F, M):
    """F extended IMMs of M modes from a list of F * M descriptors of one model type, in order"""
    return [imm(models[k * M:(k + 1) * M], rng=rng) for k in range(F)]


def with_id(imms, model_id):
    """the same IMMs with every descriptor's model id replaced (a compiled snippet's)"""
    return [dict(s, models=[kg.with_id(m, model_id) for m in s["models"]]) for s in imms]


def as_kalman(imms):
    """the same linear-Gaussian IMMs with zero D: what the Kalman IMM's twin and bank take"""
    return [dict(s, D=[np.zeros((m.ny, m.nu)) for m in s["models"]]) for s in imms]


def systems(s):
    """the modes of a Kalman IMM as kalman_common takes a filter: [(llpf_model, D [ny, nu])] * M"""
    return list(zip(s["models"], s["D"]))


def bank_args(imms):
    """models [F][M], D [F, M, ny, nu] or None, P [F, M, M], mu0 [F, M] as _capi.IMMBankHandle takes them"""
    D = None if imms[0]["D"] is None else np.stack([np.stack(s["D"]) for s in imms])
    return [list(s["models"]) for s in imms], D, np.stack([s["P"] for s in imms]), np.stack([s["mu0"] for s in imms])


def bank(imms, interact=True, extended=None):
    """a bank over the IMMs; extended (LLPF_IMM_EXTENDED) unless they have a D"""
    return _capi.IMMBankHandle(0, *bank_args(imms), interact, imms[0]["D"] is None if extended is None else extended)


def initial_state(imms):
    """(mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx]) of a reset"""
    return (kh.f64(np.stack([s["mu0"] for s in imms])), kh.f64([[S.gaussian_mean(m.initial_density) for m in s["models"]] for s in imms]),
            kh.f64([[S.gaussian_cov_matrix(m.initial_density) for m in s["models"]] for s in imms]))


def outputs(T, F, M, nx):
    """the outputs of a run in the device's layout, and their pointers in the order of the entry points' last eight arguments"""
    out = dict(ll=np.empty(F), ll_steps=np.empty((T, F)), x=np.empty((T, F, nx)), xt=np.empty((T, F, nx)), R=np.empty((T, F, nx, nx)),
               Rt=np.empty((T, F, nx, nx)), mu=np.empty((T, F, M)), ll_modes=np.empty((T, F, M)))
    return out, [_p(out[k]) for k in ("ll",) + OUTS]


def host_run(L, imms, U, Y, T, per_filter=0, t_index0=0.0, state=None, interact=True, kind=None):
    """the host build of the headers over the IMMs `imms`: imm_host_run where they have a D (no times: t_index0 and kind are not read),
    imm_ekf_host_run elsewhere; kind: ekf_common.KIND_* (default: by the model id of the first descriptor);
    state = (mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx]) or None (reset).  Returns the outputs in the device's layout and the
    final state (mu, x_modes, R_modes)."""
    F, M = len(imms), len(imms[0]["models"])
    flat = [m for s in imms for m in s["models"]]
    m0 = flat[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    R1, R2, _, _ = kh.pack_models(flat)
    mu, xm, Rm = (np.array(a, dtype=np.float64) for a in (initial_state(imms) if state is None else state))
    P = kh.f64(np.stack([s["P"] for s in imms]))
    out, outp = outputs(T, F, M, nx)
    common = [_p(R1), _p(R2), _p(P), _p(mu), _p(xm), _p(Rm), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter]
    if imms[0]["D"] is not None:
        ABCD = kc.stacked_matrices([sys for s in imms for sys in systems(s)])
        rc = L.imm_host_run(F, M, nx, ny, nu, 1 if interact else 0, *map(_p, ABCD), *common, *outp)
    else:
        kind = ec.kind_of(m0) if kind is None else kind
        f, g = uc.oracle_fns() if kind == ec.KIND_LG else (None, None)
        rc = L.imm_ekf_host_run(F, M, nx, ny, nu, 1 if interact else 0, f, g, kind, (S.Model * (F * M))(*flat), *common, float(t_index0), *outp)
    assert rc == 0, rc
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


# ---- the restatement ----
def _moments(w, xs, Rs):
    """mean and covariance of the mixture sum_j w_j N(x_j, R_j)"""
    x = sum(wj * xj for wj, xj in zip(w, xs))
    R = sum(wj * (Rj + np.outer(xj - x, xj - x)) for wj, xj, Rj in zip(w, xs, Rs))
    return x, R


def numpy_imm(modes, P, mu0, U, Y, Ts=1.0, t_index0=0.0, interact=True, lin=uc.Lin64):
    """the IMM over first-order extended Kalman filters in its literal textbook formulas, one filter.  modes: per mode a dict of
    f, g (x, u, tau) -> arrays, fjac, gjac -> their Jacobians at x, and R1, R2, x0, P0.  Per step: the combined prior; the measurement
    update of every mode linearised at its own prior (K = R C' inv(S), ll_j = logpdf(N(0, S), e)); mu_j proportional to
    (P' mu)_j exp(ll_j) with ll[t] the log of the normaliser; the combined posterior; the interaction (mu_ij = P_ij mu_i / c_j, the mixed
    mean and covariance of every mode); the time update of every mode linearised at its mixed mean."""
    dt = lin.dtype
    M = len(modes)
    P = np.asarray(P, dtype=dt)
    R1s, R2s = [np.asarray(m["R1"], dtype=dt) for m in modes], [np.asarray(m["R2"], dtype=dt) for m in modes]
    xs, Rs = [np.asarray(m["x0"], dtype=dt).copy() for m in modes], [np.asarray(m["P0"], dtype=dt).copy() for m in modes]
    mu = np.asarray(mu0, dtype=dt).copy()
    nx, ny, T = xs[0].shape[0], R2s[0].shape[0], Y.shape[0]
    I = np.eye(nx, dtype=dt)
    out = dict(ll_steps=np.zeros(T, dtype=dt), x=np.empty((T, nx), dtype=dt), xt=np.empty((T, nx), dtype=dt), R=np.empty((T, nx, nx), dtype=dt),
               Rt=np.empty((T, nx, nx), dtype=dt), mu=np.empty((T, M), dtype=dt), ll_modes=np.zeros((T, M), dtype=dt))
    for t in range(T):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        out["x"][t], out["R"][t] = _moments(mu, xs, Rs)
        cbar = P.T @ mu
        if np.isnan(Y[t, 0]):
            mu = cbar
        else:
            for j, m in enumerate(modes):
                Cm = np.asarray(m["gjac"](xs[j], u, tau), dtype=dt).reshape(ny, nx)
                e = np.asarray(Y[t], dtype=dt) - np.asarray(m["g"](xs[j], u, tau), dtype=dt)
                Sm = uc.symmetrize(Cm @ Rs[j] @ Cm.T) + R2s[j]
                Si = lin.inv(Sm)
                K = Rs[j] @ Cm.T @ Si
                xs[j] = xs[j] + K @ e
                Rs[j] = uc.symmetrize((I - K @ Cm) @ Rs[j])
                out["ll_modes"][t, j] = -(ny * np.log(2 * dt(np.pi)) + lin.logdet(Sm) + e @ Si @ e) / 2
            lw = np.log(cbar) + out["ll_modes"][t]
            top = np.max(lw)
            out["ll_steps"][t] = top + np.log(np.sum(np.exp(lw - top)))
            mu = np.exp(lw - out["ll_steps"][t])
        out["mu"][t] = mu
        out["xt"][t], out["Rt"][t] = _moments(mu, xs, Rs)
        if interact:
            cbar = P.T @ mu
            mixed = [_moments(P[:, j] * mu / cbar[j], xs, Rs) for j in range(M)]
            xs, Rs = [m_[0] for m_ in mixed], [m_[1] for m_ in mixed]
        for j, m in enumerate(modes):
            A = np.asarray(m["fjac"](xs[j], u, tau), dtype=dt).reshape(nx, nx)
            xs[j] = np.asarray(m["f"](xs[j], u, tau), dtype=dt)
            Rs[j] = uc.symmetrize(A @ Rs[j] @ A.T) + R1s[j]
    out["ll"] = out["ll_steps"].sum()
    return out


def numpy_reference(s, U, Y, interact=True):
    """the restatement over the modes of one Kalman IMM"""
    return numpy_imm([linear_mode(m, D) for m, D in systems(s)], s["P"], s["mu0"], U, Y, interact=interact)


def _densities(m):
    return dict(R1=S.gaussian_cov_matrix(m.dynamics_density), R2=S.gaussian_cov_matrix(m.measurement_density),
                x0=S.gaussian_mean(m.initial_density), P0=S.gaussian_cov_matrix(m.initial_density))


def linear_mode(m, D, dtype=np.float64):
    """a linear-Gaussian descriptor and its feedthrough as a mode of the restatement: f = A x + B u, g = C x + D u, constant Jacobians"""
    A, B, Cm, Dm = (np.asarray(kc.matrices(m, D)[k], dtype=dtype) for k in ("A", "B", "C", "D"))
    return dict(f=lambda x, u, tau: A @ x + B @ u, g=lambda x, u, tau: Cm @ x + Dm @ u, fjac=lambda x, u, tau: A, gjac=lambda x, u, tau: Cm,
                **_densities(m))


def pendulum_mode(m, dtype=np.float64):
    """a pendulum descriptor as a mode of the restatement (ukf_common.pendulum_fg, ekf_common.pendulum_jacs)"""
    f, g = uc.pendulum_fg(m, dtype)
    fjac, gjac = ec.pendulum_jacs(m, dtype)
    return dict(f=f, g=g, fjac=fjac, gjac=gjac, **_densities(m))


@contextlib.contextmanager
def _quadtank_constants(m):
    """ukf_common.quadtank_fg and ekf_common.quadtank_jacs copy the tank constants from _structs.QUADTANK_DEFAULTS when they are called:
    inside this block that table holds the descriptor's own constants (a mode's gamma1, a1)"""
    old = dict(S.QUADTANK_DEFAULTS)
    S.QUADTANK_DEFAULTS.update({name: float(m.qt[i]) for i, name in enumerate(S.QT_NAMES)})
    try:
        yield
    finally:
        S.QUADTANK_DEFAULTS.clear()
        S.QUADTANK_DEFAULTS.update(old)


def quadtank_mode(m, dtype=np.float64):
    """a quad-tank descriptor as a mode of the restatement, with the descriptor's own constants"""
    with _quadtank_constants(m):
        f, g = uc.quadtank_fg(m, dtype)
        fjac, gjac = ec.quadtank_jacs(m, dtype)
    return dict(f=f, g=g, fjac=fjac, gjac=gjac, **_densities(m))


def square_mode(m, dtype=np.float64):
    """f(x) = x, g(x) = x_0^2 at nx = 1"""
    return dict(f=lambda x, u, tau: np.asarray(x, dtype=dtype), g=lambda x, u, tau: np.array([x[0] * x[0]], dtype=dtype),
                fjac=lambda x, u, tau: np.eye(1, dtype=dtype), gjac=lambda x, u, tau: np.array([[2 * x[0]]], dtype=dtype), **_densities(m))
