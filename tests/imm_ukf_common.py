"""Shared pieces of the tests of the IMM bank over unscented Kalman filter modes (test_imm_ukf.py, test_gpu_imm_ukf.py) and of
tools/bench_imm.py --unscented: the host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_ukf.h (tests/imm_ukf_host.c, which includes
ukf_host.c, imm_host.c and kalman_host.c: one library, one set of compiler flags, the six stages once in kf_host_frame.h), the bank and
the twin over imm_common's IMMs with the bank's one set of weights w = (gamma, wm0, wc0, wi), and a numpy restatement of the IMM over
additive-noise unscented Kalman filters in its literal textbook formulas that shares nothing with the headers and runs in float64 and
np.longdouble.

An IMM is imm_common's {"models": [llpf_model] * M, "D": None, "P": [M, M], "mu0": [M]}: descriptors of ONE model type."""
import ctypes as C

import numpy as np

import llpf_amd
from llpf_amd import _capi, _structs as S
import imm_common as ic
from imm_common import OUTS, bank_args, host_combine, initial_state, outputs, same      # noqa: F401  (the frame's names, as they are)
import kalman_common as kc
import kf_host as kh
from kf_host import _dp, _p
import ukf_common as uc


def build_host(outdir):
    """the host build of tests/imm_ukf_host.c in outdir: imm_ukf_host_run, imm_host_run and imm_host_combine as imm_common binds them, and
    ukf_host_run as ukf_common.build_host binds it"""
    head, tail = [C.c_int] * 6, [_dp, _dp, C.c_int64, C.c_int]
    return kh.build(outdir, "imm_ukf_host.c", {
        "imm_ukf_host_run": head + [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(S.Model)] + [_dp] * 7 + tail + [C.c_double] + [_dp] * 8,
        "ukf_host_run": kh.MODEL_HEAD + [_dp] * 3 + kh.RUN_TAIL,
        "imm_host_run": head + [_dp] * 10 + tail + [_dp] * 8,
        "imm_host_combine": [C.c_int] * 3 + [_dp] * 5})


def bank(imms, w, interact=True):
    """a bank of unscented modes over the IMMs with the weights w"""
    models, _, P, mu0 = bank_args(imms)
    return _capi.IMMBankHandle(0, models, None, P, mu0, interact, unscented=True, weights=w)


def host_run(L, imms, w, U, Y, T, per_filter=0, t_index0=0.0, state=None, interact=True, twin=0):
    """the host build of the headers over the IMMs `imms` with the weights w (imm_ukf_host_run); twin: 0 (the oracle's functions: the
    linear-Gaussian model, the quad-tank) or ukf_common.TWIN_*; state = (mu [F, M], x_modes [F, M, nx], R_modes [F, M, nx, nx]) or None
    (reset).  Returns the outputs in the device's layout and the final state (mu, x_modes, R_modes)."""
    F, M = len(imms), len(imms[0]["models"])
    flat = [m for s in imms for m in s["models"]]
    m0 = flat[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    R1, R2, _, _ = kh.pack_models(flat)
    mu, xm, Rm = (np.array(a, dtype=np.float64) for a in (initial_state(imms) if state is None else state))
    P = kh.f64(np.stack([s["P"] for s in imms]))
    wv = np.array(w, dtype=np.float64)
    out, outp = outputs(T, F, M, nx)
    f, g = (None, None) if twin else uc.oracle_fns()
    rc = L.imm_ukf_host_run(F, M, nx, ny, nu, 1 if interact else 0, f, g, twin, (S.Model * (F * M))(*flat), _p(R1), _p(R2), _p(wv), _p(P),
                            _p(mu), _p(xm), _p(Rm), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter, float(t_index0), *outp)
    assert rc == 0, rc
    return out, (mu, xm, Rm)


# ---- the precompiled cases of test_gpu_imm_ukf.py's test a, which test_imm_ukf.py runs on the twin first ----
SHAPES = ((1, 1, 0), (2, 1, 1), (3, 2, 1), (4, 4, 2))
SHAPE_F, SHAPE_T, SHAPE_MISSING = 70, 40, (5, 6, 39)


def shape_weights(nx):
    """the two weight sets of a shape: TrivialParams, and Merwe (1, 0, 1), both of whose wc0 are positive"""
    return tuple(float(v) for v in llpf_amd.TrivialParams().weights(nx)), uc.merwe(nx, 1.0, 0.0, 1.0)


def shape_rng(nx, ny, nu, M, wi):
    return np.random.default_rng(100000 * wi + 10000 * M + 100 * nx + 10 * ny + nu)


def shape_case(nx, ny, nu, M, wi):
    """(imms, U, Y, Uf, Yf) of a case as imm_gpu_frame.check_shape draws them from shape_rng, in its order"""
    rng = shape_rng(nx, ny, nu, M, wi)
    imms = ic.lg_imms(rng, SHAPE_F, M, nx, ny, nu)
    U, Y = kc._data(rng, SHAPE_T, nu, ny, missing=SHAPE_MISSING)
    Uf = rng.standard_normal((SHAPE_F, SHAPE_T, nu))
    Yf = 2.0 * rng.standard_normal((SHAPE_F, SHAPE_T, ny))
    Yf[::3, 11, 0] = Yf[1::4, 12, 0] = Yf[:, 20, 0] = np.nan
    return imms, U, Y, Uf, Yf


class Bound:
    """imm_common's interface as tests/imm_gpu_frame.py uses it (bank, host_run, same, host_combine, initial_state, bank_args), over
    unscented modes with the weights and the twin selector bound: the frame's bodies run on an unscented bank through
    monkeypatch.setattr(imm_gpu_frame, "ic", Bound(w, twin)).  What the frame's functions take from `ic`, all of it here: check_shape
    bank, host_run, same, host_combine; check_continuation bank, host_run, same; check_a_nan_imm bank, initial_state, host_run, same;
    check_a_mode_without_mass bank, host_run, same; check_set_models bank, bank_args, same.  A name the frame comes to use and this class
    lacks is an AttributeError in the GPU test, not another bank."""
    same, host_combine, initial_state, bank_args = staticmethod(same), staticmethod(host_combine), staticmethod(initial_state), staticmethod(bank_args)

    def __init__(self, w, twin=0):
        self.w, self.twin = tuple(w), twin

    def bank(self, imms, interact=True):
        return bank(imms, self.w, interact)

    def host_run(self, L, imms, U, Y, T, **kw):
        return host_run(L, imms, self.w, U, Y, T, twin=self.twin, **kw)


# ---- the restatement ----
def numpy_imm_ukf(modes, w, P, mu0, U, Y, Ts=1.0, t_index0=0.0, interact=True, lin=uc.Lin64):
    """the IMM over additive-noise unscented Kalman filters in its literal textbook formulas, one filter.  modes: per mode a dict of
    f, g (x, u, tau) -> arrays and R1, R2, x0, P0 (imm_common.pendulum_mode, square_mode: their Jacobians are not read); w = (gamma, wm0,
    wc0, wi).  Per step: the combined prior; the unscented measurement update of every mode from the sigma points of its own prior
    (yh = sum wm Y_i, S = sum wc dY dY' + R2, Cxy = sum wc dX dY', K = Cxy inv(S), ll_j = logpdf(N(0, S), y - yh)); mu_j proportional
    to (P' mu)_j exp(ll_j) with ll[t] the log of the normaliser; the combined posterior; the interaction (mu_ij = P_ij mu_i / c_j, the
    mixed mean and covariance of every mode); the unscented time update of every mode from the sigma points of its mixed moments."""
    dt = lin.dtype
    gamma, wm0, wc0, wi = (dt(v) for v in w)
    M = len(modes)
    P = np.asarray(P, dtype=dt)
    R1s, R2s = [np.asarray(m["R1"], dtype=dt) for m in modes], [np.asarray(m["R2"], dtype=dt) for m in modes]
    xs, Rs = [np.asarray(m["x0"], dtype=dt).copy() for m in modes], [np.asarray(m["P0"], dtype=dt).copy() for m in modes]
    mu = np.asarray(mu0, dtype=dt).copy()
    nx, ny, T = xs[0].shape[0], R2s[0].shape[0], Y.shape[0]
    wm = np.array([wm0] + [wi] * (2 * nx), dtype=dt)
    wc = np.array([wc0] + [wi] * (2 * nx), dtype=dt)

    def points(m, Pm):
        Cf = lin.chol(Pm)
        return np.stack([m] + [m + gamma * Cf[:, i] for i in range(nx)] + [m - gamma * Cf[:, i] for i in range(nx)])

    def moments(wts, xl, Rl):
        x = sum(wj * xj for wj, xj in zip(wts, xl))
        return x, sum(wj * (Rj + np.outer(xj - x, xj - x)) for wj, xj, Rj in zip(wts, xl, Rl))

    out = dict(ll_steps=np.zeros(T, dtype=dt), x=np.empty((T, nx), dtype=dt), xt=np.empty((T, nx), dtype=dt), R=np.empty((T, nx, nx), dtype=dt),
               Rt=np.empty((T, nx, nx), dtype=dt), mu=np.empty((T, M), dtype=dt), ll_modes=np.zeros((T, M), dtype=dt))
    for t in range(T):
        u = np.asarray(U[t], dtype=dt) if U is not None and U.shape[1] else np.zeros(0, dtype=dt)
        tau = (t_index0 + t) * Ts
        out["x"][t], out["R"][t] = moments(mu, xs, Rs)
        cbar = P.T @ mu
        if np.isnan(Y[t, 0]):
            mu = cbar
        else:
            for j, m in enumerate(modes):
                X = points(xs[j], Rs[j])
                Yp = np.stack([np.asarray(m["g"](Xi, u, tau), dtype=dt) for Xi in X])
                yh = wm @ Yp
                dY, dX = Yp - yh, X - xs[j]
                Sm = uc.symmetrize((dY.T * wc) @ dY) + R2s[j]
                Si = lin.inv(Sm)
                K = ((dX.T * wc) @ dY) @ Si
                e = np.asarray(Y[t], dtype=dt) - yh
                xs[j] = xs[j] + K @ e
                Rs[j] = uc.symmetrize(Rs[j] - K @ Sm @ K.T)
                out["ll_modes"][t, j] = -(ny * np.log(2 * dt(np.pi)) + lin.logdet(Sm) + e @ Si @ e) / 2
            lw = np.log(cbar) + out["ll_modes"][t]
            top = np.max(lw)
            out["ll_steps"][t] = top + np.log(np.sum(np.exp(lw - top)))
            mu = np.exp(lw - out["ll_steps"][t])
        out["mu"][t] = mu
        out["xt"][t], out["Rt"][t] = moments(mu, xs, Rs)
        if interact:
            cbar = P.T @ mu
            mixed = [moments(P[:, j] * mu / cbar[j], xs, Rs) for j in range(M)]
            xs, Rs = [m_[0] for m_ in mixed], [m_[1] for m_ in mixed]
        for j, m in enumerate(modes):
            Xn = np.stack([np.asarray(m["f"](Xi, u, tau), dtype=dt) for Xi in points(xs[j], Rs[j])])
            xs[j] = wm @ Xn
            dX = Xn - xs[j]
            Rs[j] = uc.symmetrize((dX.T * wc) @ dX) + R1s[j]
    out["ll"] = out["ll_steps"].sum()
    return out
