"""The IMM filter of csrc/shared/llpf_imm.h on the host (tests/imm_host.c: the six stages of tests/kf_host_frame.h over the Kalman family,
the build the device is held to in test_gpu_imm.py): it is the textbook recursion (a numpy restatement in literal formulas), it degenerates to the Kalman filter of tests/kalman_host.c bit for bit
where it must (one mode, no interaction, P = I), it keeps its corner rules, and the C ABI refuses what it cannot run.  No GPU needed."""
import ctypes as C
from fractions import Fraction
import os
import re

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import imm_common as ic
import kalman_common as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 0), (2, 1, 1), (4, 2, 2), (8, 4, 2)]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ic.build_host(tmp_path_factory.mktemp("imm_host"))


@pytest.fixture(scope="module")
def khost(tmp_path_factory):
    return kc.build_host(tmp_path_factory.mktemp("imm_kalman_host"))


def _case(seed, M, nx, ny, nu, T, F=1, missing=()):
    rng = np.random.default_rng(seed)
    imms = [ic.random_imm(rng, M, nx, ny, nu, k) for k in range(F)]
    U, Y = kc.simulate(rng, kc.matrices(*ic.systems(imms[0])[0]), T, missing=missing)
    return imms, U, Y


@pytest.mark.parametrize("M", [2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_host_build_is_the_textbook_recursion(host, M, shape):
    nx, ny, nu = shape
    T, missing = 60, (7, 8, 31)
    imms, U, Y = _case(100 * M + nx, M, nx, ny, nu, T, F=2, missing=missing)
    for interact in (True, False):
        h, _ = ic.host_run(host, imms, U, Y, T, interact=interact)
        for f, imm in enumerate(imms):
            ref = ic.numpy_reference(imm, U, Y, interact)
            for k in ic.OUTS:
                assert kc.close(h[k][:, f], ref[k]), (interact, f, k)
            assert abs(h["ll"][f] - ref["ll"]) <= 1e-10 * abs(ref["ll"]), (interact, f)
        assert np.all(h["ll_steps"][list(missing)] == 0.0) and np.all(h["ll_modes"][list(missing)] == 0.0)
        # the probabilities: a distribution at every step
        assert np.all(h["mu"] >= 0.0) and np.all(np.abs(h["mu"].sum(axis=2) - 1.0) <= 1e-12)


@pytest.mark.parametrize("shape", SHAPES)
def test_one_mode_is_the_kalman_filter_bit_for_bit(host, khost, shape):
    nx, ny, nu = shape
    T = 60
    imms, U, Y = _case(7 + nx, 1, nx, ny, nu, T, F=3, missing=(5, 40))
    for imm in imms:
        imm["P"], imm["mu0"] = np.ones((1, 1)), np.ones(1)
    h, (mu, xm, Rm) = ic.host_run(host, imms, U, Y, T)
    k, (xk, Rk) = kc.host_run(khost, [ic.systems(s)[0] for s in imms], U, Y, T)
    for key in ("ll", "ll_steps", "x", "xt", "R", "Rt"):
        assert kc.bits_equal(h[key], k[key]), key
    assert kc.bits_equal(h["ll_modes"][:, :, 0], k["ll_steps"]) and np.all(h["mu"] == 1.0)
    assert kc.bits_equal(xm[:, 0], xk) and kc.bits_equal(Rm[:, 0], Rk)


def _modes_are_the_kalman_filters(khost, imms, h, final, U, Y, T):
    """every mode's ll and final state are those of the Kalman twin of that mode alone; returns the twins' totals LL [F, M]"""
    M = len(imms[0]["models"])
    LL = np.empty((len(imms), M))
    for j in range(M):
        k, (xk, Rk) = kc.host_run(khost, [ic.systems(s)[j] for s in imms], U, Y, T)
        assert kc.bits_equal(h["ll_modes"][:, :, j], k["ll_steps"]), j
        assert kc.bits_equal(final[1][:, j], xk) and kc.bits_equal(final[2][:, j], Rk), j
        LL[:, j] = k["ll"]
    return LL


@pytest.mark.parametrize("M", [2, 3, 4])
def test_without_interaction_the_modes_are_independent_kalman_filters(host, khost, M):
    T = 60
    imms, U, Y = _case(40 + M, M, 3, 2, 1, T, F=3, missing=(11,))
    h, final = ic.host_run(host, imms, U, Y, T, interact=False)
    _modes_are_the_kalman_filters(khost, imms, h, final, U, Y, T)
    # ... and with P = I the mode probabilities telescope: sum_t ll[t] = log sum_j mu0_j exp(LL_j)
    for imm in imms:
        imm["P"] = np.eye(M)
    h, final = ic.host_run(host, imms, U, Y, T, interact=False)
    LL = _modes_are_the_kalman_filters(khost, imms, h, final, U, Y, T)
    mu0 = np.stack([s["mu0"] for s in imms])
    want = np.logaddexp.reduce(np.log(mu0) + LL, axis=1)
    assert np.all(np.abs(h["ll_steps"].sum(axis=0) - want) <= 1e-10 * np.abs(want))
    assert np.all(np.abs(h["ll"] - want) <= 1e-10 * np.abs(want))


@pytest.mark.parametrize("M", [2, 4])
def test_mixing_under_the_identity_transition_changes_nothing(host, khost, M):
    T = 60
    imms, U, Y = _case(50 + M, M, 4, 2, 2, T, F=2, missing=(3,))
    for imm in imms:
        imm["P"] = np.eye(M)
    h, final = ic.host_run(host, imms, U, Y, T, interact=True)
    _modes_are_the_kalman_filters(khost, imms, h, final, U, Y, T)
    off, _ = ic.host_run(host, imms, U, Y, T, interact=False)
    ic.same(h, off, what="P = I: interact on and off")


def test_a_missing_row(host):
    T = 12
    imms, U, Y = _case(61, 3, 2, 1, 1, T, missing=(4,))
    h, _ = ic.host_run(host, imms, U, Y, T)
    assert h["ll_steps"][4, 0] == 0.0 and np.all(h["ll_modes"][4, 0] == 0.0)
    # mu <- c, as formed from the posterior probabilities of the step before, without normalisation
    P, mu = imms[0]["P"], h["mu"][3, 0]
    c = np.zeros(3)
    for j in range(3):
        for i in range(3):
            c[j] = float(Fraction(P[i, j]) * Fraction(mu[i]) + Fraction(c[j]))      # one rounding: the fma
    assert kc.bits_equal(h["mu"][4, 0], c)
    # no mode corrected: the combined posterior of the step is the mixture of the uncorrected modes under the new mu
    assert not kc.bits_equal(h["xt"][4], h["x"][4]) and np.all(np.isfinite(h["xt"][4]))


def test_a_mode_without_mass_enters_no_sum_and_is_not_mixed(host, khost):
    T, M = 40, 3
    imms, U, Y = _case(62, M, 3, 2, 1, T, F=2, missing=(9,))
    for imm in imms:
        imm["P"] = np.eye(M)
        imm["mu0"] = np.array([0.25, 0.0, 0.75])
    h, final = ic.host_run(host, imms, U, Y, T)
    assert np.all(h["mu"][:, :, 1] == 0.0) and not np.any(np.signbit(h["mu"][:, :, 1]))
    assert np.all(np.isfinite(h["ll_steps"])) and np.all(np.isfinite(h["xt"]))
    # mode 1 keeps its own state: the Kalman filter of that mode alone
    _modes_are_the_kalman_filters(khost, imms, h, final, U, Y, T)
    # ... and everything else is the IMM of the two modes that have mass, bit for bit
    two = [ic.imm([s["models"][0], s["models"][2]], P=np.eye(2), mu0=np.array([0.25, 0.75]), D=[s["D"][0], s["D"][2]]) for s in imms]
    h2, _ = ic.host_run(host, two, U, Y, T)
    for k in ("ll", "ll_steps", "x", "xt", "R", "Rt"):
        assert kc.bits_equal(h[k], h2[k]), k
    assert kc.bits_equal(h["mu"][:, :, [0, 2]], h2["mu"])


@pytest.mark.parametrize("interact", [True, False])
def test_an_indefinite_mode_makes_the_whole_imm_nan_and_nothing_else(host, interact):
    T, M = 20, 3
    imms, U, Y = _case(63, M, 2, 1, 0, T, F=3, missing=(6, 15))
    ok, _ = ic.host_run(host, imms, U, Y, T, interact=interact)
    mu, xm, Rm = ic.initial_state(imms)
    Rm[1, 2] = -100.0 * np.eye(2)
    bad, final = ic.host_run(host, imms, U, Y, T, state=(mu, xm, Rm), interact=interact)
    steps = np.delete(np.arange(T), [6, 15])
    assert np.all(np.isnan(bad["ll_steps"][steps, 1])) and np.all(bad["ll_steps"][[6, 15], 1] == 0.0) and np.isnan(bad["ll"][1])
    assert np.all(np.isnan(bad["mu"][:, 1])) and np.all(np.isnan(bad["xt"][:, 1])) and np.all(np.isnan(bad["Rt"][:, 1]))
    assert np.all(np.isnan(bad["x"][1:, 1])) and np.all(np.isnan(bad["ll_modes"][steps][1:, 1]))
    assert np.all(np.isnan(final[0][1])) and np.all(np.isnan(final[1][1])) and np.all(np.isnan(final[2][1]))
    for k in ic.OUTS:
        assert kc.bits_equal(bad[k][:, [0, 2]], ok[k][:, [0, 2]]), k
    assert kc.bits_equal(bad["ll"][[0, 2]], ok["ll"][[0, 2]])


def test_the_first_steps_of_a_run_are_a_shorter_run(host):
    T, T1 = 50, 17
    imms, U, Y = _case(64, 4, 4, 2, 2, T, F=2, missing=(10,))
    h, _ = ic.host_run(host, imms, U, Y, T)
    h1, st = ic.host_run(host, imms, U[:T1], Y[:T1], T1)
    for k in ic.OUTS:
        assert kc.bits_equal(h[k][:T1], h1[k]), k
    # ... and the rest is a run from the state between; the combined estimate is a pure function of that state
    h2, _ = ic.host_run(host, imms, U[T1:], Y[T1:], T - T1, state=st)
    for k in ic.OUTS:
        assert kc.bits_equal(h[k][T1:], h2[k]), k
    x, R = ic.host_combine(host, *st)
    assert kc.bits_equal(x, h["x"][T1]) and kc.bits_equal(R, h["R"][T1])


def _create(imms, M=None, P=None, mu0=None):
    models, D, P0, m0 = ic.bank_args(imms)
    flat = [m for row in models for m in row]
    arr = (S.Model * len(flat))(*flat)
    M = len(models[0]) if M is None else M
    P, mu0 = _capi.f64(P0 if P is None else P), _capi.f64(m0 if mu0 is None else mu0)
    h = C.c_void_p()
    L = _capi.lib()
    rc = L.llpf_imm_bank_create(0, arr, _capi.dptr(_capi.f64(D)), _capi.dptr(P), _capi.dptr(mu0), len(models), M, 1, C.byref(h))
    assert not h.value or rc == _capi.OK
    if h.value:
        L.llpf_imm_bank_destroy(h)
    return rc, L.llpf_last_error().decode()


def test_arguments_that_cannot_run_are_refused():
    rng = np.random.default_rng(65)
    imms = [ic.random_imm(rng, 3, 2, 1, 1, k) for k in range(2)]
    for M in (0, 5):
        rc, msg = _create(imms, M=M)
        assert rc == _capi.ERR_ARG and "n_modes" in msg, (M, rc, msg)
    P = np.stack([s["P"] for s in imms])
    bad = P.copy()
    bad[1, 2, 0] += 1e-9
    rc, msg = _create(imms, P=bad)
    assert rc == _capi.ERR_ARG and "filter 1" in msg and "row 2" in msg, msg
    bad = P.copy()
    bad[0, 1, 0], bad[0, 1, 1] = -0.1, bad[0, 1, 1] + bad[0, 1, 0] + 0.1
    rc, msg = _create(imms, P=bad)
    assert rc == _capi.ERR_ARG and "filter 0" in msg and "negative" in msg, msg
    mu = np.stack([s["mu0"] for s in imms])
    mu[1, 0] += 1e-6
    rc, msg = _create(imms, mu0=mu)
    assert rc == _capi.ERR_ARG and "filter 1" in msg and "mu0" in msg, msg
    other = [ic.random_imm(rng, 3, 2, 1, 1), ic.random_imm(rng, 3, 2, 1, 1)]
    other[1]["models"][2], other[1]["D"][2] = kc.random_system(rng, 3, 1, 1)
    rc, msg = _create(other)
    assert rc == _capi.ERR_ARG and "filter 1, mode 2" in msg and "dimensions" in msg, msg
    # what the Kalman bank refuses, per mode: a noise density with a mean
    m = other[0]["models"][1]
    m.dynamics_density.mu[0] = 0.5
    other[1]["models"][2], other[1]["D"][2] = kc.random_system(rng, 2, 1, 1)
    rc, msg = _create(other)
    assert rc == _capi.ERR_ARG and "filter 0, mode 1" in msg and "zero mean" in msg, msg
    # the arguments themselves are fine: without a device the create gets as far as asking for one
    rc, msg = _create(imms)
    assert rc == (_capi.OK if _capi.device_count() > 0 else _capi.ERR_NO_DEVICE), (rc, msg)


def test_header_binding_and_julia_wrapper_name_the_exports():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    names = ["llpf_imm_bank_" + v for v in ("create", "destroy", "reset", "set_models", "run", "get_state", "set_state")]
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    L = _capi.lib()
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _capi.SYMBOLS and hasattr(L, n), n
        assert "(:%s, LIB)" % n in jl, n
    body = re.search(r"typedef struct llpf_imm_outputs \{(.*?)\} llpf_imm_outputs;", hdr, re.S).group(1)
    fields = re.findall(r"\*?(\w+)\s*[,;]", body)
    assert fields == [f[0] for f in S.ImmOutputs._fields_], fields
    assert C.sizeof(S.ImmOutputs) == 8 + 7 * 8 and _capi.IMM_OUTPUTS == tuple(fields[2:])


def test_there_is_no_smoother():
    rng = np.random.default_rng(66)
    mt = kc.matrices(*kc.random_system(rng, 2, 1, 1))
    kf = lambda s: llpf_amd.KalmanFilter(mt["A"] * s, mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"]))
    imm = llpf_amd.IMM([kf(1.0), kf(0.5)], [[0.9, 0.1], [0.2, 0.8]], [0.5, 0.5])
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.smooth(imm, np.zeros((3, 1)), np.zeros((3, 1)))
    assert imm._handle is None
    with pytest.raises(TypeError, match="no smoother"):
        llpf_amd.IMMBank.smooth(object.__new__(llpf_amd.IMMBank), None, None)
