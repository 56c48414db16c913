"""The Rauch-Tung-Striebel smoother of the Kalman bank (llpf_kf_smooth, llpf_kalman_bank_smooth), the checks that need no GPU: the host build
of the header's backward step — the definition the device reproduces bit for bit (tests/test_gpu_kalman_smooth.py) — is the reference's
smoother and the conditional law of the states under the joint Gaussian; the ABI is declared, exported, bound, guarded and mirrored in
Julia; arguments are refused before a device is looked for."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import kalman_common as kc
import kalman_smooth_common as ks

ROOT = kc.ROOT
NAME = "llpf_kalman_bank_smooth"


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("kalman_host"))


@pytest.fixture(scope="module")
def hsmooth(tmp_path_factory):
    return ks.build_host_smooth(tmp_path_factory.mktemp("kalman_smooth_host"))


@pytest.mark.parametrize("nx", range(1, 9))
def test_host_smoother_is_the_references_literal_formulas(host, hsmooth, nx):
    """every ny 1..4, the three covariance kinds, D != 0, missing rows (the last one included): the header's backward step over the host
    forward outputs against C = Rt A' / R[t+1] (solve) and symmetrize(), to 1e-10 relative"""
    rng = np.random.default_rng(200 + nx)
    for ny in range(1, 5):
        for kind in range(3):
            nu = int(rng.integers(0, 4))
            m, D = kc.random_system(rng, nx, ny, nu, kind)
            mats = kc.matrices(m, D)
            U, Y = kc.simulate(rng, mats, 40, missing=(3, 17, 18, 39))
            fw, _ = kc.host_run(host, [(m, D)], U, Y, 40)
            h = ks.host_smooth(hsmooth, [(m, D)], U, fw, 40)
            xT, RT = ks.numpy_smooth(mats, fw["x"][:, 0], fw["xt"][:, 0], fw["R"][:, 0], fw["Rt"][:, 0])
            assert kc.close(h["xT"][:, 0], xT), (nx, ny, kind)
            assert kc.close(h["RT"][:, 0], RT), (nx, ny, kind)
            assert kc.bits_equal(h["xT"][-1], fw["xt"][-1]) and kc.bits_equal(h["RT"][-1], fw["Rt"][-1])
            assert np.array_equal(h["RT"], np.swapaxes(h["RT"], -1, -2))
            # smoothing never adds uncertainty: tr RT[t] <= tr Rt[t]
            assert np.all(np.trace(h["RT"][:, 0], axis1=1, axis2=2) <= np.trace(fw["Rt"][:, 0], axis1=1, axis2=2) * (1 + 1e-12))


def test_host_smoother_is_the_conditional_law_of_the_joint_gaussian(host, hsmooth):
    """nx <= 3, T <= 30: E[x_t | y_1..y_T] and Cov[x_t | y_1..y_T] of the dense joint Gaussian, an oracle that shares nothing with the
    recursion, to 1e-8 relative"""
    rng = np.random.default_rng(31)
    for nx in (1, 2, 3):
        for ny in (1, 2, 3):
            for kind in range(3):
                nu = int(rng.integers(0, 3))
                T = int(rng.integers(5, 31))
                m, D = kc.random_system(rng, nx, ny, nu, kind)
                mats = kc.matrices(m, D)
                U, Y = kc.simulate(rng, mats, T, missing=(1, T - 2))
                fw, _ = kc.host_run(host, [(m, D)], U, Y, T)
                h = ks.host_smooth(hsmooth, [(m, D)], U, fw, T)
                jx, jR = ks.joint_smoother(mats, U, Y)
                assert kc.close(h["xT"][:, 0], jx, 1e-8), (nx, ny, kind, T)
                assert kc.close(h["RT"][:, 0], jR, 1e-8), (nx, ny, kind, T)


def test_host_smoother_per_filter_inputs(host, hsmooth):
    rng = np.random.default_rng(32)
    systems = [kc.random_system(rng, 3, 2, 2, k) for k in range(5)]
    U = rng.standard_normal((30, 2))
    Y = rng.standard_normal((30, 2))
    fw, _ = kc.host_run(host, systems, U, Y, 30)
    shared = ks.host_smooth(hsmooth, systems, U, fw, 30)
    per = ks.host_smooth(hsmooth, systems, np.ascontiguousarray(np.broadcast_to(U, (5, 30, 2))), fw, 30, per_filter=1)
    for k in ("xT", "RT"):
        assert kc.bits_equal(shared[k], per[k]), k
    for f, (m, D) in enumerate(systems):
        one = ks.host_smooth(hsmooth, [(m, D)], U, {"xt": fw["xt"][:, f:f + 1], "Rt": fw["Rt"][:, f:f + 1]}, 30)
        assert kc.bits_equal(one["xT"][:, 0], shared["xT"][:, f]) and kc.bits_equal(one["RT"][:, 0], shared["RT"][:, f])


def test_a_filter_that_loses_definiteness_is_nan_only_in_its_own_outputs(host, hsmooth):
    rng = np.random.default_rng(33)
    systems = [kc.random_system(rng, 2, 1, 1, 2) for _ in range(3)]
    U = rng.standard_normal((12, 1))
    Y = rng.standard_normal((12, 1))
    fw, _ = kc.host_run(host, systems, U, Y, 12)
    ok = ks.host_smooth(hsmooth, systems, U, fw, 12)
    bad = {k: fw[k].copy() for k in ("xt", "Rt")}
    bad["Rt"][6, 1] = -100.0 * np.eye(2)            # R[8] = A Rt[7] A' + R1 is no longer positive definite (1-based)
    sm = ks.host_smooth(hsmooth, systems, U, bad, 12)
    assert np.all(np.isnan(sm["xT"][:7, 1])) and np.all(np.isnan(sm["RT"][:7, 1]))
    assert kc.bits_equal(sm["xT"][7:, 1], ok["xT"][7:, 1]) and kc.bits_equal(sm["RT"][7:, 1], ok["RT"][7:, 1])
    for f in (0, 2):
        assert kc.bits_equal(sm["xT"][:, f], ok["xT"][:, f]) and kc.bits_equal(sm["RT"][:, f], ok["RT"][:, f])


def test_the_symbol_is_declared_exported_bound_and_guarded():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "capi.hip")).read()
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % NAME, hdr, re.S)
    assert m and len(m.group(1).split(",")) == 8
    L = _capi.lib()
    assert hasattr(L, NAME) and len(_capi.SYMBOLS[NAME]) == 8
    assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % NAME, capi, re.M) and "LLPF_GUARD(%s)" % NAME in capi
    body = re.search(r"typedef struct llpf_kalman_smooth_outputs \{(.*?)\} llpf_kalman_smooth_outputs;", hdr, re.S).group(1)
    names = [n.strip().lstrip("*") for d in body.split(";") if d.strip() for n in re.sub(r"^\s*\w+[\s*]+", "", d.strip()).split(",")]
    assert names == [f[0] for f in S.KalmanSmoothOutputs._fields_] == ["struct_size", "pad", "xT", "RT"]
    assert C.sizeof(S.KalmanSmoothOutputs) == 24 and C.sizeof(S.KalmanOutputs) == 56
    ma, mi = C.c_int32(), C.c_int32()
    L.llpf_version(C.byref(ma), C.byref(mi))
    assert (ma.value, mi.value) == (0, 7)
    # the fault-injection site of the call: kalman_smooth names it, kf_smooth (host/kfbank.hpp) reads it
    host = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "host")
    assert 'out, "kalman_smooth",' in open(os.path.join(host, "kalman.hpp")).read()
    assert "test_throw(site);\n    if (!w) return forward(nullptr);" in open(os.path.join(host, "kfbank.hpp")).read()


def test_julia_mirror_struct_offsets_and_arity():
    import test_julia_struct_mirror as jm
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    structs = jm._parse_structs(jl)
    assert "CKalmanSmoothOutputs" in structs
    got = jm._offsets("CKalmanSmoothOutputs", structs)
    want = [(f[0], getattr(S.KalmanSmoothOutputs, f[0]).offset, getattr(S.KalmanSmoothOutputs, f[0]).size) for f in S.KalmanSmoothOutputs._fields_]
    assert got == want and jm._size_align("CKalmanSmoothOutputs", structs)[0] == C.sizeof(S.KalmanSmoothOutputs)
    m = re.search(r"ccall\(\(:%s, LIB\),\s*\w+,\s*\((.*?)\),\s*" % NAME, jl, re.S)
    assert m
    depth, n, cur = 0, 0, ""
    for ch in m.group(1):
        depth += ch in "({"
        depth -= ch in ")}"
        if ch == "," and depth == 0:
            n, cur = n + 1, ""
        else:
            cur += ch
    assert n + (1 if cur.strip() else 0) == 8
    imp = re.search(r"^import LowLevelParticleFilters:(.*?)\n\n", jl, re.S | re.M).group(1)
    assert "KalmanSmoothingSolution" in re.findall(r"[\w!]+", imp)                 # imported, not redefined
    assert not re.search(r"^(mutable )?struct KalmanSmoothingSolution", jl, re.M)
    exported = re.search(r"^export (.*?)\n\n", jl, re.S | re.M).group(1)
    assert "KalmanSmoothingSolution" not in exported and not re.search(r"\bsmooth\b", exported)
    assert re.search(r"^function LowLevelParticleFilters\.smooth\(kf::GPUKalmanFilter, u, y, p = NullParameters\(\)\)", jl, re.M)
    assert re.search(r"^function smooth\(b::GPUKalmanFilterBank, u, y\)", jl, re.M)
    assert "KalmanSmoothingSolution(sol, " in jl


def test_bad_arguments_are_refused_before_any_device_lookup():
    L = _capi.lib()
    out = S.KalmanSmoothOutputs()
    out.struct_size = C.sizeof(S.KalmanSmoothOutputs)
    y = np.zeros(4)
    yp = y.ctypes.data_as(C.POINTER(C.c_double))
    assert L.llpf_kalman_bank_smooth(None, None, yp, 4, 0, None, None, C.byref(out)) == _capi.ERR_ARG
    assert b"null handle" in L.llpf_last_error()
    if _capi.device_count() < 1:
        return
    rng = np.random.default_rng(34)
    m, D = kc.random_system(rng, 2, 1, 0)
    h = _capi.KalmanBankHandle(0, [m], D[None])
    assert L.llpf_kalman_bank_smooth(h.h, None, yp, 0, 0, None, None, C.byref(out)) == _capi.ERR_ARG
    assert L.llpf_kalman_bank_smooth(h.h, None, None, 4, 0, None, None, C.byref(out)) == _capi.ERR_ARG
    small = S.KalmanSmoothOutputs()
    small.struct_size = 8
    assert L.llpf_kalman_bank_smooth(h.h, None, yp, 4, 0, None, None, C.byref(small)) == _capi.ERR_ARG
    assert b"struct_size" in L.llpf_last_error()
    h.close()


def test_kalman_smooth_dispatch_needs_the_device():
    """smooth(kf, u, y) is the Kalman smoother, not the particle smoother's argument unpacking (which raised ValueError before)"""
    kf = llpf_amd.KalmanFilter(np.eye(2) * 0.5, np.ones((2, 1)), np.ones((1, 2)), 0.3, np.eye(2), np.eye(1),
                               llpf_amd.MvNormal(np.zeros(2), np.eye(2)))
    assert "KalmanSmoothingSolution" in llpf_amd.api.__all__ and issubclass(llpf_amd.KalmanSmoothingSolution, llpf_amd.KalmanFilteringSolution)
    if _capi.device_count() > 0:
        sol = llpf_amd.smooth(kf, np.zeros((5, 1)), np.zeros((5, 1)))
        assert isinstance(sol, llpf_amd.KalmanSmoothingSolution) and sol.xT.shape == (5, 2) and sol.RT.shape == (5, 2, 2)
    else:
        with pytest.raises(_capi.LLPFError) as ei:
            llpf_amd.smooth(kf, np.zeros((5, 1)), np.zeros((5, 1)))
        assert ei.value.code == _capi.ERR_NO_DEVICE
