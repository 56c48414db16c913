"""Shared pieces of the tests of the IMM bank over extended Kalman filter modes (test_imm_ekf.py, test_gpu_imm_ekf.py) and of
tools/bench_imm.py --extended: the host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_ekf.h (tests/imm_ekf_host.c, which also
holds ekf_host.c's and imm_host.c's entry points), IMMs over the model lists of the extended-Kalman tests, and a numpy restatement of
the IMM over first-order extended Kalman filters in its literal textbook formulas (np.linalg.inv, dense matrices) that shares nothing
with the headers and runs in float64 and np.longdouble.

An IMM here is {"models": [llpf_model] * M, "P": [M, M], "mu0": [M]}: the modes are descriptors of ONE model type that differ by their
parameters, R1, R2 and d0."""
import contextlib
import ctypes as C

import numpy as np

from llpf_amd import _capi, _structs as S
import ekf_common as ec
import imm_common as ic
import kalman_common as kc
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
random_P, random_mu, same, host_combine = ic.random_P, ic.random_mu, ic.same, ic.host_combine


def build_host(outdir):
    """the host build of tests/imm_ekf_host.c in outdir: imm_ekf_host_run, and with it ekf_host_run, imm_host_run and imm_host_combine
    as ekf_common.build_host and imm_common.build_host bind them (one library, one set of compiler flags)"""
    run = kh.MODEL_HEAD + [_dp] * 2 + kh.RUN_TAIL
    return kh.build(outdir, "imm_ekf_host.c", {
        "imm_ekf_host_run": [C.c_int] * 6 + [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(S.Model)] + [_dp] * 6 + [_dp, _dp, C.c_int64, C.c_int, C.c_double] + [_dp] * 8,
        "ekf_host_run": run,
        "imm_host_run": [C.c_int] * 6 + [_dp] * 10 + [_dp, _dp, C.c_int64, C.c_int] + [_dp] * 8,
        "imm_host_combine": [C.c_int] * 3 + [_dp] * 5})


def imm(models, P=None, mu0=None, rng=None):
    """one IMM over the descriptors `models`; P, mu0 random (imm_common's) unless given"""
    M = len(models)
    return dict(models=list(models), P=random_P(rng, M) if P is None else np.asarray(P, float), mu0=random_mu(rng, M) if mu0 is None else np.asarray(mu0, float))


def lg_imms(rng, F, M, nx, ny, nu):
    """F IMMs over M random stable linear-Gaussian systems each (kalman_common.random_system, D = 0)"""
    return [imm([kc.random_system(rng, nx, ny, nu, (k + j) % 3, D=False)[0] for j in range(M)], rng=rng) for k in range(F)]


def grouped(models, rng, F, M):
    """F IMMs of M modes from a list of F * M descriptors of one model type, in order"""
    return [imm(models[k * M:(k + 1) * M], rng=rng) for k in range(F)]


def with_id(imms, model_id):
    """the same IMMs with every descriptor's model id replaced (a compiled snippet's)"""
    return [dict(s, models=[_with_id(m, model_id) for m in s["models"]]) for s in imms]


def _with_id(m, model_id):
    c = S.Model.from_buffer_copy(bytes(m))
    c.model_id = model_id
    return c


def as_kalman(imms):
    """linear-Gaussian IMMs in imm_common's form ({"systems": [(llpf_model, D)]}, D = 0): what the Kalman IMM's twin and bank take"""
    return [dict(systems=[(m, np.zeros((m.ny, m.nu))) for m in s["models"]], P=s["P"], mu0=s["mu0"]) for s in imms]


def bank_args(imms):
    """models [F][M], D (None), P [F, M, M], mu0 [F, M] as _capi.IMMBankHandle takes them"""
    return [list(s["models"]) for s in imms], None, np.stack([s["P"] for s in imms]), np.stack([s["mu0"] for s in imms])


def bank(imms, interact=True):
    """an extended bank (LLPF_IMM_EXTENDED) over the IMMs"""
    return _capi.IMMBankHandle(0, *bank_args(imms), interact, True)


def initial_state(imms):
    """(mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx]) of a reset"""
    return (kh.f64(np.stack([s["mu0"] for s in imms])), kh.f64([[S.gaussian_mean(m.initial_density) for m in s["models"]] for s in imms]),
            kh.f64([[S.gaussian_cov_matrix(m.initial_density) for m in s["models"]] for s in imms]))


def host_run(L, imms, U, Y, T, per_filter=0, t_index0=0.0, state=None, interact=True, kind=None):
    """the host build of the two headers over the IMMs `imms`; kind: ekf_common.KIND_* (default: by the model id of the first descriptor);
    state = (mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx]) or None (reset).  Returns the outputs in the device's layout and the
    final state (mu, x_modes, R_modes)."""
    F, M = len(imms), len(imms[0]["models"])
    flat = [m for s in imms for m in s["models"]]
    m0 = flat[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    kind = ec.kind_of(m0) if kind is None else kind
    arr = (S.Model * (F * M))(*flat)
    R1, R2, _, _ = kh.pack_models(flat)
    mu, xm, Rm = (np.array(a, dtype=np.float64) for a in (initial_state(imms) if state is None else state))
    P = kh.f64(np.stack([s["P"] for s in imms]))
    out = dict(ll=np.empty(F), ll_steps=np.empty((T, F)), x=np.empty((T, F, nx)), xt=np.empty((T, F, nx)), R=np.empty((T, F, nx, nx)),
               Rt=np.empty((T, F, nx, nx)), mu=np.empty((T, F, M)), ll_modes=np.empty((T, F, M)))
    f, g = uc.oracle_fns() if kind == ec.KIND_LG else (None, None)
    rc = L.imm_ekf_host_run(F, M, nx, ny, nu, 1 if interact else 0, f, g, kind, arr, _p(R1), _p(R2), _p(P), _p(mu), _p(xm), _p(Rm),
                            _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter, float(t_index0), *[_p(out[k]) for k in ("ll",) + OUTS])
    assert rc == 0, rc
    return out, (mu, xm, Rm)


# ---- the restatement ----
def _moments(w, xs, Rs):
    """mean and covariance of the mixture sum_j w_j N(x_j, R_j)"""
    x = sum(wj * xj for wj, xj in zip(w, xs))
    R = sum(wj * (Rj + np.outer(xj - x, xj - x)) for wj, xj, Rj in zip(w, xs, Rs))
    return x, R


def numpy_imm_ekf(modes, P, mu0, U, Y, Ts=1.0, t_index0=0.0, interact=True, lin=uc.Lin64):
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


def _densities(m):
    return dict(R1=S.gaussian_cov_matrix(m.dynamics_density), R2=S.gaussian_cov_matrix(m.measurement_density),
                x0=S.gaussian_mean(m.initial_density), P0=S.gaussian_cov_matrix(m.initial_density))


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
