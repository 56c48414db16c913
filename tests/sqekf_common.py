"""Shared pieces of the square-root extended Kalman bank's tests (test_sqekf.py, test_gpu_sqekf.py) and of tools/bench_sqekf.py: the
host build of csrc/shared/llpf_sqekf.h (tests/sqekf_host.c) over ekf_host.c's model kinds, the bank as kf_gpu_frame sees it, and the
ill-conditioned cases on which the covariance form of the extended filter turns NaN."""
import ctypes as C

import numpy as np

from llpf_amd import _capi, _structs as S
import ekf_common as ec
import kf_gpu_frame as kg
import kf_host as kh
from kf_host import _dp, _p
import sqkf_common as sc
import ukf_common as uc


def build_host(outdir):
    """the host build of tests/sqekf_host.c in outdir (sqekf_host_run; ekf_host.c's entry points come with it: ekf_host_run)"""
    run = kh.MODEL_HEAD + [_dp] * 2 + kh.RUN_TAIL
    return kh.build(outdir, "sqekf_host.c", {"sqekf_host_run": run + [C.c_int, _dp], "ekf_host_run": run})


def _args(models, U, Y, T, per_filter, t_index0, state, kind):
    F = len(models)
    m0 = models[0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    kind = ec.kind_of(m0) if kind is None else kind
    arr = (S.Model * F)(*models)
    R1, R2, x0, P0 = kh.pack_models(models, state)
    out, outp = kh.outputs(T, F, nx, ny)
    f, g = uc.oracle_fns() if kind == ec.KIND_LG else (None, None)
    keep = (arr, R1, R2)
    return out, x0, P0, keep, [F, nx, ny, nu, f, g, kind, arr, _p(R1), _p(R2), _p(x0), _p(P0), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter,
                               float(t_index0)] + outp


def host_run(L, models, U, Y, T, per_filter=0, t_index0=0.0, state=None, factor=None, kind=None):
    """the host build of the header over the filters `models` (llpf_model descriptors) in ekf_common.host_run's form.  The state:
    state = (x, R), factored as set_state(x, R) factors it; factor = (x, L), taken as set_state(x, L=L) takes it; neither: reset.
    Returns the outputs in the device's layout and the final state (x, R, L)."""
    out, x0, P0, _keep, args = _args(models, U, Y, T, per_filter, t_index0, state if factor is None else factor, kind)
    Rfin = np.empty_like(P0)
    rc = L.sqekf_host_run(*args, 0 if factor is None else 1, _p(Rfin))
    assert rc == 0, rc
    return out, (x0, Rfin, P0)


def ekf_host_run(L, models, U, Y, T, t_index0=0.0, kind=None):
    """the covariance-form twin (tests/ekf_host.c's ekf_host_run, as this library carries it) on the same arguments: its outputs"""
    out, _x0, _P0, _keep, args = _args(models, U, Y, T, 0, t_index0, None, kind)
    rc = L.ekf_host_run(*args)
    assert rc == 0, rc
    return out


def bank(models):
    return _capi.SqekfBankHandle(0, list(models))


FAMILY = kg.Family("sqekf", bank, host_run, kg.lg_models, True)


def ill_conditioned_models(case):
    """sqkf_common.ill_conditioned(case) as a model with Jacobians: (the system, its llpf_model, Y)"""
    system, Y = sc.ill_conditioned(case)
    return system, system[0], Y


def ill_conditioned_bank(case, F):
    """F copies of sqkf_common.ill_conditioned(case) with perturbed noise levels: copy k has R1 and R2 scaled by 1 + k / 1000.  Returns
    (the models, Y)"""
    (m, _), Y = sc.ill_conditioned(case)
    r1, r2 = S.gaussian_cov_matrix(m.dynamics_density)[0, 0], S.gaussian_cov_matrix(m.measurement_density)[0, 0]
    out = []
    for k in range(F):
        c = S.Model.from_buffer_copy(bytes(m))
        c.dynamics_density = S.make_gaussian(np.zeros(m.nx), float(r1 * (1.0 + k / 1000.0)))
        c.measurement_density = S.make_gaussian(np.zeros(m.ny), float(r2 * (1.0 + k / 1000.0)))
        out.append(c)
    return out, Y


def diffuse_pendulum():
    """the pendulum with a diffuse prior and a near-exact sensor: cov(d0) = 1e10 I, R2 = 1e-10, R1 = 1e-14 I; Y the sine of a slow swing,
    T = 50.  Returns (model, U, Y)."""
    m = uc.pendulum_model()
    g = S.make_gaussian
    m.dynamics_density, m.measurement_density = g(np.zeros(2), 1e-14), g(np.zeros(1), 1e-10)
    m.initial_density = g(np.array([0.3, 0.0]), 1e10)
    T = 50
    t = np.arange(T)
    Y = np.sin(0.3 * np.cos(0.15 * t)).reshape(T, 1)
    return m, np.zeros((T, m.nu)), Y
