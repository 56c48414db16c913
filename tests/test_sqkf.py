"""Banks of square-root Kalman filters (llpf_sqkf_bank_*), the checks that need no GPU: the host build of csrc/shared/llpf_sqkf.h — the
definition the device reproduces bit for bit (tests/test_gpu_sqkf.py) — computes the Kalman filter on well-conditioned systems, stays
finite and accurate on two systems where the covariance form loses positive definiteness, and continues a run bit for bit; the ABI is
declared, exported, bound and mirrored in Julia; arguments are refused before a device is looked for."""
import ctypes as C
import os
import re

import mpmath as mp
import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import kalman_common as kc
import sqkf_common as sc

ROOT = kc.ROOT
ARITY = {"llpf_sqkf_bank_create": 5, "llpf_sqkf_bank_destroy": 1, "llpf_sqkf_bank_reset": 1, "llpf_sqkf_bank_set_models": 3,
         "llpf_sqkf_bank_run": 7, "llpf_sqkf_bank_get_state": 4, "llpf_sqkf_bank_set_state": 4}


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("sqkf_host")
    return kc.build_host(d), sc.build_host(d)


# ------------------------------------------------------------------------------------------------
# 1. well-conditioned systems: the Kalman filter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", range(1, 9))
def test_host_header_is_the_kalman_filter_on_well_conditioned_systems(hosts, nx):
    """every ny 1..4, F = 20 random systems in the three covariance kinds with D != 0, T = 100, rows 0, 50 and 99 missing: every output
    of the square-root twin within kc.close (rtol 1e-10) of the Kalman twin, ll within 1e-10 relative; R and Rt exactly symmetric"""
    hk, hs = hosts
    for ny in range(1, 5):
        rng = np.random.default_rng(1000 + 10 * nx + ny)
        nu = int(rng.integers(0, 4))
        systems = [kc.random_system(rng, nx, ny, nu, k % 3) for k in range(20)]
        U, Y = kc._data(rng, 100, nu, ny, missing=(0, 50, 99))
        ref, _ = kc.host_run(hk, systems, U, Y, 100)
        got, _ = sc.host_run(hs, systems, U, Y, 100)
        for k in _capi.KALMAN_OUTPUTS:
            assert kc.close(got[k], ref[k]), (nx, ny, k)
        assert np.all(np.abs(got["ll"] - ref["ll"]) <= 1e-10 * np.abs(ref["ll"])), (nx, ny)
        assert np.all(got["ll_steps"][[0, 50, 99]] == 0.0) and np.all(np.isnan(got["e"][[0, 50, 99]]))
        for k in ("R", "Rt"):
            assert np.array_equal(got[k], np.swapaxes(got[k], -1, -2)), (nx, ny, k)


# ------------------------------------------------------------------------------------------------
# 2. the two ill-conditioned systems
# ------------------------------------------------------------------------------------------------
def _mp_reference(mats, Y):
    """the covariance form at 60 digits: ll, xt [T, nx], Rt [T, nx, nx] rounded to doubles"""
    mp.mp.dps = 60
    M = lambda a: mp.matrix(np.asarray(a, float).tolist())
    A, Cm, R1, R2 = M(mats["A"]), M(mats["C"]), M(mats["R1"]), M(mats["R2"])
    x, R = M(mats["x0"].reshape(-1, 1)), M(mats["P0"])
    nx, ny = mats["A"].shape[0], mats["C"].shape[0]
    ll = mp.mpf(0)
    xt, Rt = [], []
    for y in Y:
        e = M(y.reshape(-1, 1)) - Cm * x
        Sm = Cm * R * Cm.T + R2
        K = R * Cm.T * mp.inverse(Sm)
        x = x + K * e
        R = R - K * Cm * R
        R = (R + R.T) / 2
        ll += -(ny * mp.log(2 * mp.pi) + mp.log(mp.det(Sm)) + (e.T * mp.inverse(Sm) * e)[0]) / 2
        xt.append([float(x[i]) for i in range(nx)])
        Rt.append([[float(R[i, j]) for j in range(nx)] for i in range(nx)])
        x = A * x
        R = A * R * A.T + R1
    return float(ll), np.array(xt), np.array(Rt)


def _lq(pre):
    """the lower-triangular factor of pre pre' with a diagonal >= 0, on LAPACK's QR"""
    L = np.linalg.qr(pre.T, mode="r").T
    return L * np.sign(np.where(np.diag(L) == 0.0, 1.0, np.diag(L)))


def _qr_square_root_filter(mats, Y):
    """the yardstick: an independent fp64 square-root filter, the same array form on np.linalg.qr"""
    A, Cm = mats["A"], mats["C"]
    nx, ny = A.shape[0], Cm.shape[0]
    L1, L2, Lr = (np.linalg.cholesky(mats[k]) for k in ("R1", "R2", "P0"))
    x = mats["x0"].copy()
    ll, xt, Rt = 0.0, [], []
    for y in Y:
        Lf = _lq(np.block([[L2, Cm @ Lr], [np.zeros((nx, ny)), Lr]]))
        Ls, Kb, Lr = Lf[:ny, :ny], Lf[ny:, :ny], Lf[ny:, ny:]
        z = np.linalg.solve(Ls, y - Cm @ x)
        x = x + Kb @ z
        ll += -0.5 * ny * np.log(2 * np.pi) - np.log(np.prod(np.diag(Ls))) - 0.5 * z @ z
        xt.append(x)
        Rt.append(Lr @ Lr.T)
        x = A @ x
        Lr = _lq(np.hstack([A @ Lr, L1]))[:, :nx]
    return ll, np.array(xt), np.array(Rt)


def _errors(ll, xt, Rt, ref):
    """maximum relative errors against the 60-digit run: ll relative to itself; xt and Rt per step relative to the largest magnitude of
    that step's vector / matrix (the scale kc.close uses)"""
    rll, rxt, rRt = ref
    ex = np.max(np.max(np.abs(xt - rxt), axis=1) / np.max(np.abs(rxt), axis=1))
    eR = np.max(np.max(np.abs(Rt - rRt), axis=(1, 2)) / np.max(np.abs(rRt), axis=(1, 2)))
    return dict(ll=abs(ll - rll) / abs(rll), xt=float(ex), Rt=float(eR))


@pytest.mark.parametrize("case", [0, 1])
def test_ill_conditioned_systems_stay_finite_and_accurate(hosts, case):
    """sqkf_common.ill_conditioned: the double integrator (R1 = 1e-14 I, R2 = 1e-10, P0 = 1e10 I) and the nx = 3, ny = 2 chain
    (R1 = 1e-12 I, R2 = 1e-9 I, P0 = 1e9 I), Y = default_rng(1).standard_normal((50, ny)), both with P0 as given (no factor of 10 was
    needed).  The Kalman twin's ll is NaN on both (S indefinite at step 3 and at step 1).  The square-root twin is finite at every
    step with min eig(Rt) >= 0, and its maximum relative errors against a 60-digit mpmath run of the covariance form are at most 8 times
    those of an independent fp64 square-root filter on np.linalg.qr, plus 1e-13 (two Householder orderings of one backward-stable
    algorithm differ by small constants; a wrong update is off by orders of magnitude).
    Measured (twin / yardstick):  case 0: ll 1.7e-09 / 5.4e-08, xt 1.4e-06 / 7.9e-06, Rt 9.4e-07 / 4.6e-06;
                                  case 1: ll 4.8e-09 / 3.6e-09, xt 5.2e-07 / 3.9e-07, Rt 1.9e-07 / 1.4e-07."""
    hk, hs = hosts
    system, Y = sc.ill_conditioned(case)
    plain, _ = kc.host_run(hk, [system], None, Y, 50)
    assert np.isnan(plain["ll"][0])                       # the condition on the inputs: the covariance form fails here
    got, _ = sc.host_run(hs, [system], None, Y, 50)
    for k in ("ll", "ll_steps", "x", "xt", "R", "Rt", "e"):
        assert np.all(np.isfinite(got[k])), k
    assert min(np.linalg.eigvalsh(R).min() for R in got["Rt"][:, 0]) >= 0.0
    mats = kc.matrices(*system)
    ref = _mp_reference(mats, Y)
    mine = _errors(got["ll"][0], got["xt"][:, 0], got["Rt"][:, 0], ref)
    yard = _errors(*_qr_square_root_filter(mats, Y), ref)
    print("case %d: twin %s, yardstick %s" % (case, mine, yard))
    for k in ("ll", "xt", "Rt"):
        assert mine[k] <= 8.0 * yard[k] + 1e-13, (k, mine[k], yard[k])


# ------------------------------------------------------------------------------------------------
# 3. continuation and state, through the twin
# ------------------------------------------------------------------------------------------------
def test_host_header_continues_through_the_factor_bit_for_bit(hosts):
    """run(a) then run(b) from the factor the first run left is run(a + b); per-filter copies of shared inputs give the same bits; a state
    given as a covariance starts from llpf_kf_chol of it"""
    _, hs = hosts
    rng = np.random.default_rng(8)
    systems = [kc.random_system(rng, 3, 2, 2, k) for k in range(5)]
    U = rng.standard_normal((30, 2))
    Y = rng.standard_normal((30, 2))
    whole, (xw, Rw, Lw) = sc.host_run(hs, systems, U, Y, 30)
    per, _ = sc.host_run(hs, systems, np.broadcast_to(U, (5, 30, 2)), np.broadcast_to(Y, (5, 30, 2)), 30, per_filter=3)
    for k in whole:
        assert kc.bits_equal(whole[k], per[k]), k
    a, (xa, Ra, La) = sc.host_run(hs, systems, U[:12], Y[:12], 12)
    assert np.array_equal(La, np.tril(La)) and np.all(np.diagonal(La, axis1=1, axis2=2) >= 0.0)
    b, (xb, Rb, Lb) = sc.host_run(hs, systems, U[12:], Y[12:], 18, factor=(xa, La))
    for k in _capi.KALMAN_OUTPUTS:
        assert kc.bits_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    assert kc.bits_equal(xb, xw) and kc.bits_equal(Lb, Lw) and kc.bits_equal(Rb, Rw)
    assert kc.bits_equal(b["R"][0], Ra)                  # the final R is llpf_sq_cov of the final factor: the next run's first prior
    facs = np.stack([sc.host_chol(hs, R)[1] for R in Ra])
    viaR, _ = sc.host_run(hs, systems, U[12:], Y[12:], 18, state=(xa, Ra))
    viaL, _ = sc.host_run(hs, systems, U[12:], Y[12:], 18, factor=(xa, facs))
    for k in _capi.KALMAN_OUTPUTS:
        assert kc.bits_equal(viaR[k], viaL[k]), k
    assert kc.close(viaR["xt"], b["xt"], rtol=1e-9)      # ... and that is the same filter to rounding, not to the bit
    ok, _ = sc.host_chol(hs, -np.eye(3))
    assert not ok


# ------------------------------------------------------------------------------------------------
# 4. the surface
# ------------------------------------------------------------------------------------------------
def test_header_binding_library_and_julia_name_the_same_exports():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "capi.hip")).read()
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    L = _capi.lib()
    declared = sorted(set(re.findall(r"\b(llpf_sqkf_[a-z_]+)\s*\(", hdr)))
    assert declared == sorted(ARITY)
    assert sorted(n for n in _capi.SYMBOLS if n.startswith("llpf_sqkf_")) == declared
    assert sorted(set(re.findall(r"ccall\(\(:(llpf_sqkf_[a-z_]+), LIB\)", jl))) == declared
    for name in declared:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert len(m.group(1).split(",")) == ARITY[name], name
        assert hasattr(L, name) and len(_capi.SYMBOLS[name]) == ARITY[name], name
        assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % name, capi, re.M) and "LLPF_GUARD(%s)" % name in capi, name
        j = re.search(r"ccall\(\(:%s, LIB\),\s*\w+,\s*\((.*?)\),\s" % name, jl, re.S).group(1)
        assert len([a for a in re.sub(r"\{[^}]*\}", "", j).split(",") if a.strip()]) == ARITY[name], (name, j)
    exported = re.search(r"^export (.*?)\n\n", jl, re.S | re.M).group(1)
    for name in ("GPUSqKalmanFilter", "GPUSqKalmanFilterBank", "sqkf_run"):
        assert re.search(r"\b%s\b" % name, exported), name
    for name in ("SqKalmanFilter", "SqKalmanFilterBank"):
        assert name in llpf_amd.api.__all__ and hasattr(llpf_amd, name)
    assert issubclass(llpf_amd.SqKalmanFilter, llpf_amd.KalmanFilter)
    ma, mi = C.c_int32(), C.c_int32()
    L.llpf_version(C.byref(ma), C.byref(mi))
    assert (ma.value, mi.value) == (0, 7)


def test_pack_errors_are_refused_before_a_device_is_looked_for():
    L = _capi.lib()
    h = C.c_void_p()
    rng = np.random.default_rng(1)

    def create(models):
        arr = (S.Model * len(models))(*models)
        return L.llpf_sqkf_bank_create(0, arr, None, len(models), C.byref(h))

    m, _ = kc.random_system(rng, 3, 2, 1)
    indefinite = {3: np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]), 2: np.array([[1.0, 2.0], [2.0, 1.0]])}
    for field, n, word in (("dynamics_density", 3, b"R1"), ("measurement_density", 2, b"R2"), ("initial_density", 3, b"cov(d0)")):
        bad = S.Model.from_buffer_copy(m)
        setattr(bad, field, S.make_gaussian(np.zeros(n), indefinite[n], S.COV_FULL))
        assert create([m, bad]) == _capi.ERR_ARG, field
        msg = L.llpf_last_error()
        assert msg.startswith(b"sqkf: filter 1: ") and word in msg and b"positive definite" in msg, msg
    bad = S.Model.from_buffer_copy(m)
    bad.dynamics_density = S.make_gaussian(np.zeros(3), np.array([1.0, 0.0, 1.0]))        # a singular R1 is a Kalman filter's, not this one's
    assert create([bad]) == _capi.ERR_ARG and b"R1" in L.llpf_last_error()
    m2, _ = kc.random_system(rng, 3, 1, 1)
    assert create([m, m2]) == _capi.ERR_ARG and L.llpf_last_error().startswith(b"sqkf: filter 1: ")      # dimensions differ
    bad = S.Model.from_buffer_copy(m)
    bad.measurement_density = S.make_gaussian(np.zeros(3), 1.0)                          # a density of the wrong dimension
    assert create([bad]) == _capi.ERR_ARG and b"dimension" in L.llpf_last_error()
    bad = S.Model.from_buffer_copy(m)
    bad.model_id = S.MODEL_QUADTANK_RK4
    assert create([bad]) == _capi.ERR_ARG and b"LLPF_MODEL_LINEAR_GAUSSIAN" in L.llpf_last_error()
    assert L.llpf_sqkf_bank_create(0, None, None, 1, C.byref(h)) == _capi.ERR_ARG
    assert not h.value


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_create_without_a_gpu_is_no_device():
    rng = np.random.default_rng(2)
    m, D = kc.random_system(rng, 2, 2, 1)
    with pytest.raises(_capi.LLPFError) as ei:
        _capi.SqkfBankHandle(0, [m], D[None])
    assert ei.value.code == _capi.ERR_NO_DEVICE
    kf = llpf_amd.SqKalmanFilter(np.eye(2) * 0.5, np.ones((2, 1)), np.ones((1, 2)), 0.3, np.eye(2), np.eye(1),
                                 llpf_amd.MvNormal(np.zeros(2), np.eye(2)))
    assert kf._handle is None
    with pytest.raises(_capi.LLPFError):
        llpf_amd.loglik(kf, np.zeros((5, 1)), np.zeros((5, 1)))


def test_python_classes_refuse_what_the_filter_does_not_do():
    A, B, Cm = np.eye(2) * 0.9, np.ones((2, 1)), np.ones((1, 2))
    d0 = llpf_amd.MvNormal(np.zeros(2), np.eye(2))
    sq = llpf_amd.SqKalmanFilter(A, B, Cm, 0, np.eye(2), np.eye(1), d0)
    with pytest.raises(TypeError, match="the square-root Kalman filter has no smoother"):
        llpf_amd.smooth(sq, np.zeros((3, 1)), np.zeros((3, 1)))
    with pytest.raises(TypeError, match="the square-root Kalman filter has no smoother"):
        llpf_amd.SqKalmanFilterBank.smooth(None, None, None)
    with pytest.raises(TypeError, match="SqKalmanFilter"):
        llpf_amd.IMM([sq, sq], np.full((2, 2), 0.5), np.full(2, 0.5))
    dyn = llpf_amd.LinearDynamics(np.eye(1) * 0.8, np.ones((1, 1)))
    nlm = llpf_amd.RBMeasurementModel(llpf_amd.LinearMeasurement(np.ones((1, 1))), np.eye(1), 1)
    with pytest.raises(TypeError, match="SqKalmanFilter"):
        llpf_amd.RBPF(100, sq, dyn, nlm, np.eye(1), llpf_amd.MvNormal(np.zeros(1), np.eye(1)))
