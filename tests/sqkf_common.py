"""Shared pieces of the square-root Kalman bank's tests (test_sqkf.py, test_gpu_sqkf.py): the host build of
csrc/shared/llpf_sqkf.h (tests/sqkf_host.c) and the two ill-conditioned systems on which the covariance form loses definiteness."""
import ctypes as C

import numpy as np

from llpf_amd import _structs as S
import kalman_common as kc
import kf_host as kh
from kf_host import _dp, _p


def build_host(outdir):
    """the host build of tests/sqkf_host.c in outdir (sqkf_host_run and sqkf_host_chol)"""
    return kh.build(outdir, "sqkf_host.c", {"sqkf_host_run": [C.c_int] * 4 + [_dp] * 8 + [_dp, _dp, C.c_int64, C.c_int, C.c_int] + [_dp] * 8,
                                            "sqkf_host_chol": [C.c_int, _dp, _dp]})


def host_run(L, systems, U, Y, T, per_filter=0, state=None, factor=None):
    """the host build of the header over filters `systems` [(model, D)], in kalman_common.host_run's form.  The state: state = (x, R),
    factored as set_state(x, R) factors it; factor = (x, L), taken as set_state(x, L=L) takes it; neither: reset.  Returns the outputs in
    the device's layout and the final state (x, R, L)."""
    F = len(systems)
    m0 = systems[0][0]
    nx, ny, nu = m0.nx, m0.ny, m0.nu
    ABCD = kc.stacked_matrices(systems)
    R1, R2, x0, P0 = kh.pack_models([m for m, _ in systems], state if factor is None else factor)
    out, outp = kh.outputs(T, F, nx, ny)
    Rfin = np.empty((F, nx, nx))
    rc = L.sqkf_host_run(F, nx, ny, nu, *map(_p, ABCD), _p(R1), _p(R2), _p(x0), _p(P0), _p(kh.inputs(U, nu)), _p(kh.f64(Y)), T, per_filter,
                         0 if factor is None else 1, _p(Rfin), *outp)
    assert rc == 0, rc
    return out, (x0, Rfin, P0)


def host_chol(L, R):
    """llpf_kf_chol of the dense covariance R [n, n]: (positive definite, the dense lower factor)"""
    R = kh.f64(R)
    out = np.empty_like(R)
    ok = L.sqkf_host_chol(R.shape[0], _p(R), _p(out))
    return bool(ok), out


# ------------------------------------------------------------------------------------------------
# the two systems with a diffuse prior and a near-perfect measurement
# ------------------------------------------------------------------------------------------------
def _ill(A, Cm, r1, r2, p0):
    A, Cm = np.array(A, float), np.array(Cm, float)
    nx, ny = A.shape[0], Cm.shape[0]
    m = S.make_lg_model(A, np.zeros((nx, 0)), Cm, S.make_gaussian(np.zeros(nx), float(r1)), S.make_gaussian(np.zeros(ny), float(r2)),
                        S.make_gaussian(np.zeros(nx), float(p0)))
    return m, np.zeros((ny, 0))


def ill_conditioned(case):
    """case 0: the double integrator, R1 = 1e-14 I, R2 = 1e-10, P0 = 1e10 I; case 1: nx = 3, ny = 2, R1 = 1e-12 I, R2 = 1e-9 I,
    P0 = 1e9 I.  Returns the system (model, D) and Y = default_rng(1).standard_normal((50, ny)); there are no inputs."""
    if case == 0:
        sysm = _ill([[1, 1], [0, 1]], [[1, 0]], 1e-14, 1e-10, 1e10)
    else:
        sysm = _ill([[1, 1, .5], [0, 1, 1], [0, 0, 1]], [[1, 0, 0], [0, 1, 0]], 1e-12, 1e-9, 1e9)
    return sysm, np.random.default_rng(1).standard_normal((50, sysm[0].ny))
