"""Banks of Kalman filters (llpf_kalman_bank_*), the checks that need no GPU: the ABI is declared, exported, bound, guarded and mirrored
in Julia; arguments are refused before a device is looked for; and the host build of csrc/shared/llpf_kalman.h — the definition the
device reproduces bit for bit (tests/test_gpu_kalman.py) — computes the reference's Kalman filter."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import kalman_common as kc
import oracle_binding as ob

ROOT = kc.ROOT
SYMS = ["llpf_kalman_bank_create", "llpf_kalman_bank_destroy", "llpf_kalman_bank_reset", "llpf_kalman_bank_set_models",
        "llpf_kalman_bank_run", "llpf_kalman_bank_get_state", "llpf_kalman_bank_set_state"]
ARITY = {"llpf_kalman_bank_create": 5, "llpf_kalman_bank_destroy": 1, "llpf_kalman_bank_reset": 1, "llpf_kalman_bank_set_models": 3,
         "llpf_kalman_bank_run": 7, "llpf_kalman_bank_get_state": 3, "llpf_kalman_bank_set_state": 3}


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kalman_host"))


def test_symbols_are_declared_exported_bound_and_guarded():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "capi.hip")).read()
    L = _capi.lib()
    for name in SYMS:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert m, name
        assert len(m.group(1).split(",")) == ARITY[name], name
        assert hasattr(L, name) and name in _capi.SYMBOLS and len(_capi.SYMBOLS[name]) == ARITY[name], name
        assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % name, capi, re.M) and "LLPF_GUARD(%s)" % name in capi, name
    assert C.sizeof(S.KalmanOutputs) == 56
    ma, mi = C.c_int32(), C.c_int32()
    L.llpf_version(C.byref(ma), C.byref(mi))
    assert (ma.value, mi.value) == (0, 7)


def test_julia_wrapper_calls_every_symbol_with_its_arity():
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    for name in SYMS:
        m = re.search(r"ccall\(\(:%s, LIB\),\s*\w+,\s*\((.*?)\),\s*" % name, jl, re.S)
        assert m, name
        depth, n, cur = 0, 0, ""
        for ch in m.group(1):
            depth += ch in "({"
            depth -= ch in ")}"
            if ch == "," and depth == 0:
                n, cur = n + 1, ""
            else:
                cur += ch
        assert n + (1 if cur.strip() else 0) == ARITY[name], name
    exported = re.search(r"^export (.*?)\n\n", jl, re.S | re.M).group(1)
    assert "GPUKalmanFilter" in exported and "GPUKalmanFilterBank" in exported
    assert not re.search(r"\bKalmanFilter\b", exported.replace("GPUKalmanFilter", ""))
    assert "KalmanFilteringSolution(kf, u, y," in jl


def test_null_handles_and_bad_arguments_are_refused():
    L = _capi.lib()
    for name in ("llpf_kalman_bank_reset", "llpf_kalman_bank_destroy"):
        if name == "llpf_kalman_bank_destroy":
            assert getattr(L, name)(None) == _capi.OK          # destroy(NULL) is a no-op, like llpf_bank_destroy
        else:
            assert getattr(L, name)(None) == _capi.ERR_ARG
    assert L.llpf_kalman_bank_set_models(None, None, None) == _capi.ERR_ARG
    assert L.llpf_kalman_bank_run(None, None, None, 1, 0, None, None) == _capi.ERR_ARG
    assert L.llpf_kalman_bank_get_state(None, None, None) == _capi.ERR_ARG
    assert L.llpf_kalman_bank_set_state(None, None, None) == _capi.ERR_ARG
    h = C.c_void_p()
    rng = np.random.default_rng(1)

    def create(models, D=None):
        arr = (S.Model * len(models))(*models)
        return L.llpf_kalman_bank_create(0, arr, None if D is None else D.ctypes.data_as(C.POINTER(C.c_double)), len(models), C.byref(h))

    assert L.llpf_kalman_bank_create(0, None, None, 1, C.byref(h)) == _capi.ERR_ARG
    assert L.llpf_kalman_bank_create(0, (S.Model * 1)(kc.random_system(rng, 2, 1, 1)[0]), None, 1, None) == _capi.ERR_ARG
    for nx, ny, nu in ((9, 1, 0), (2, 5, 0), (2, 1, 9)):
        m = S.make_lg_model(np.eye(nx) * 0.5, np.zeros((nx, min(nu, 8))), np.ones((ny, nx)), S.make_gaussian(np.zeros(nx), 1.0),
                            S.make_gaussian(np.zeros(ny), 1.0), S.make_gaussian(np.zeros(nx), 1.0))
        m.nu = nu
        assert create([m]) == _capi.ERR_ARG, (nx, ny, nu)
    m, _ = kc.random_system(rng, 3, 2, 1)
    bad = S.Model.from_buffer_copy(m)
    bad.measurement_density = S.make_gaussian(np.zeros(2), np.array([[1.0, 2.0], [2.0, 1.0]]), S.COV_FULL)     # indefinite R2
    assert create([m, bad]) == _capi.ERR_ARG and b"R2" in L.llpf_last_error()
    bad = S.Model.from_buffer_copy(m)
    bad.initial_density = S.make_gaussian(np.zeros(3), np.array([1.0, 0.0, 1.0]))                            # singular P0
    assert create([bad]) == _capi.ERR_ARG
    bad = S.Model.from_buffer_copy(m)
    bad.dynamics_density = S.make_gaussian(np.full(3, 0.1), 1.0)                                            # non-zero noise mean
    assert create([bad]) == _capi.ERR_ARG and b"zero mean" in L.llpf_last_error()
    bad = S.Model.from_buffer_copy(m)
    bad.model_id = S.MODEL_QUADTANK_RK4
    assert create([bad]) == _capi.ERR_ARG
    m2, _ = kc.random_system(rng, 3, 1, 1)
    assert create([m, m2]) == _capi.ERR_ARG                                                               # dimensions differ
    assert not h.value


@pytest.mark.skipif(_capi.device_count() > 0, reason="this check is for machines without a GPU")
def test_create_without_a_gpu_is_no_device():
    rng = np.random.default_rng(2)
    m, D = kc.random_system(rng, 2, 2, 1)
    with pytest.raises(_capi.LLPFError) as ei:
        _capi.KalmanBankHandle(0, [m], D[None])
    assert ei.value.code == _capi.ERR_NO_DEVICE
    kf = llpf_amd.KalmanFilter(np.eye(2) * 0.5, np.ones((2, 1)), np.ones((1, 2)), 0.3, np.eye(2), np.eye(1),
                               llpf_amd.MvNormal(np.zeros(2), np.eye(2)))
    with pytest.raises(_capi.LLPFError):
        llpf_amd.loglik(kf, np.zeros((5, 1)), np.zeros((5, 1)))


@pytest.mark.parametrize("nx", range(1, 9))
def test_host_header_is_the_references_kalman_filter(host, nx):
    """every ny 1..4, the three covariance kinds, D != 0, missing rows: the header against the literal formulas, to 1e-10"""
    rng = np.random.default_rng(100 + nx)
    for ny in range(1, 5):
        for kind in range(3):
            nu = int(rng.integers(0, 4))
            m, D = kc.random_system(rng, nx, ny, nu, kind)
            mats = kc.matrices(m, D)
            U, Y = kc.simulate(rng, mats, 40, missing=(3, 17, 18))
            h, _ = kc.host_run(host, [(m, D)], U, Y, 40)
            ref = kc.numpy_reference(mats, U, Y)
            for k in _capi.KALMAN_OUTPUTS:
                assert kc.close(h[k][:, 0], ref[k]), (nx, ny, kind, k)
            assert abs(h["ll"][0] - ref["ll"]) <= 1e-10 * abs(ref["ll"]), (nx, ny, kind)
            assert np.all(h["ll_steps"][[3, 17, 18], 0] == 0.0) and np.all(np.isnan(h["e"][[3, 17, 18], 0]))
            assert np.array_equal(h["R"], np.swapaxes(h["R"], -1, -2))


def test_host_header_matches_the_oracle_kalman_loglik(host):
    rng = np.random.default_rng(7)
    for nx, ny in ((1, 1), (2, 1), (3, 2), (4, 2), (4, 4), (6, 3), (8, 4)):
        for kind in range(3):
            m, D = kc.random_system(rng, nx, ny, 2, kind, D=False)
            U, Y = kc.simulate(rng, kc.matrices(m, D), 60, missing=(10,))
            h, _ = kc.host_run(host, [(m, D)], U, Y, 60)
            o = ob.kalman_loglik(m, U, Y)
            assert abs(h["ll"][0] - o) <= 1e-10 * abs(o), (nx, ny, kind, h["ll"][0], o)


def test_host_header_per_filter_inputs_and_continuation(host):
    rng = np.random.default_rng(8)
    systems = [kc.random_system(rng, 3, 2, 2, k) for k in range(5)]
    U = rng.standard_normal((30, 2))
    Y = rng.standard_normal((30, 2))
    shared, _ = kc.host_run(host, systems, U, Y, 30)
    per, _ = kc.host_run(host, systems, np.broadcast_to(U, (5, 30, 2)), np.broadcast_to(Y, (5, 30, 2)), 30, per_filter=3)
    for k in shared:
        assert kc.bits_equal(shared[k], per[k]), k
    a, st = kc.host_run(host, systems, U[:12], Y[:12], 12)
    b, _ = kc.host_run(host, systems, U[12:], Y[12:], 18, state=st)
    for k in _capi.KALMAN_OUTPUTS:
        assert kc.bits_equal(np.concatenate([a[k], b[k]]), shared[k]), k


def test_a_non_positive_definite_S_turns_only_that_filter_nan(host):
    rng = np.random.default_rng(9)
    systems = [kc.random_system(rng, 2, 1, 0, 2) for _ in range(3)]
    Y = rng.standard_normal((10, 1))
    x0 = np.stack([kc.matrices(*s)["x0"] for s in systems])
    P0 = np.stack([kc.matrices(*s)["P0"] for s in systems])
    ok, _ = kc.host_run(host, systems, None, Y, 10, state=(x0.copy(), P0.copy()))
    P0[1] = -100.0 * np.eye(2)                      # C P0 C' + R2 < 0 for filter 1
    bad, _ = kc.host_run(host, systems, None, Y, 10, state=(x0.copy(), P0))
    assert np.all(np.isnan(bad["ll_steps"][:, 1])) and np.all(np.isnan(bad["x"][1:, 1])) and np.isnan(bad["ll"][1])
    for f in (0, 2):
        assert kc.bits_equal(bad["ll_steps"][:, f], ok["ll_steps"][:, f])


def test_kalman_filter_descriptor_in_the_rbpf_is_unchanged():
    A, B, Cm = np.eye(2) * 0.9, np.ones((2, 1)), np.ones((1, 2))
    kf = llpf_amd.KalmanFilter(A, B, Cm, 0, np.eye(2), np.eye(1), llpf_amd.MvNormal(np.zeros(2), np.eye(2)))
    assert kf._handle is None                        # building the descriptor touches no GPU
    assert kf.A.shape == (2, 2) and kf.R1.shape == (2, 2) and kf.R2.shape == (1, 1) and kf.D == 0
    kfd = llpf_amd.KalmanFilter(A, B, Cm, np.ones((1, 1)), np.eye(2), np.eye(1), llpf_amd.MvNormal(np.zeros(2), np.eye(2)))
    assert kfd._handle is None
    dyn = llpf_amd.LinearDynamics(np.eye(1) * 0.8, np.ones((1, 1)))
    nlm = llpf_amd.RBMeasurementModel(llpf_amd.LinearMeasurement(np.ones((1, 1))), np.eye(1), 1)
    with pytest.raises(NotImplementedError):
        llpf_amd.RBPF(100, kfd, dyn, nlm, np.eye(1), llpf_amd.MvNormal(np.zeros(1), np.eye(1)))
    if _capi.device_count() < 1:
        with pytest.raises(_capi.LLPFError) as ei:
            llpf_amd.RBPF(100, kf, dyn, nlm, np.eye(1), llpf_amd.MvNormal(np.zeros(1), np.eye(1)))
        assert ei.value.code == _capi.ERR_NO_DEVICE
    for name in ("KalmanFilter", "KalmanFilterBank", "KalmanFilteringSolution", "covariance"):
        assert name in llpf_amd.api.__all__ and hasattr(llpf_amd, name)
