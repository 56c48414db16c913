"""Banks of IMM filters on the device (llpf_imm_bank_*; kernels/imm.hpp, host/imm.hpp): the GPU reproduces the host build of
csrc/shared/llpf_imm.h (tests/imm_host.c) bit for bit, whatever the number of modes, the shape, the bank, the chunking of T or the split
of a run; and the Python API (IMM, IMMBank) is that bank.  The bodies this file shares with test_gpu_imm_ekf.py are in imm_gpu_frame.py."""
import numpy as np
import pytest

import llpf_amd
import imm_common as ic
from imm_common import OUTS
import imm_gpu_frame as ig
import kalman_common as kc
from kalman_common import _data

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 0), (3, 2, 1), (4, 2, 2), (5, 1, 1), (8, 4, 2)]
# the D != 0 systems: four IMMs of five have a feedthrough
FAM = ig.ImmFamily(lambda rng, F, M, nx, ny, nu: [ic.random_imm(rng, M, nx, ny, nu, k % 3, D=k % 5 != 0) for k in range(F)], None)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return ic.build_host(tmp_path_factory.mktemp("imm_host"))


@pytest.mark.parametrize("M", [1, 2, 3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_bit_identical_to_the_host_header(host, M, shape):
    """F = 70 (a ragged last wave at every G, two workgroups at G = 4), T = 40 with missing rows, every output; shared inputs, the same
    as per-filter inputs, per-filter inputs of their own whose missing rows differ between the filters of a wave; interact on and off"""
    nx, ny, nu = shape
    ig.check_shape(FAM, host, np.random.default_rng(1000 * M + 10 * nx + ny), F=70, T=40, M=M, nx=nx, ny=ny, nu=nu, missing=(5, 6, 30),
                   what=(M, shape))


@pytest.mark.parametrize("M", [2, 3])
def test_a_filters_bits_do_not_depend_on_the_bank(M):
    rng = np.random.default_rng(4 + M)
    imms = FAM.imms(rng, 70, M, 3, 2, 1)
    U, Y = _data(rng, 30, 1, 2, missing=(7,))
    g = ic.bank(imms).run(U, Y, outputs=OUTS)
    pick = [69, 0, 37, 16, 15, 17, 32, 31]
    sub = ic.bank([imms[k] for k in pick][::-1]).run(U, Y, outputs=OUTS)
    for j, k in enumerate(pick[::-1]):
        for key in OUTS:
            assert kc.bits_equal(sub[key][:, j], g[key][:, k]), (k, key)
    one = ic.bank([imms[37]]).run(U, Y, outputs=OUTS)
    for key in OUTS:
        assert kc.bits_equal(one[key][:, 0], g[key][:, 37]), key


def test_chunks_and_continuation(host):
    rng = np.random.default_rng(5)
    imms = FAM.imms(rng, 70, 3, 4, 2, 2)
    U, Y = _data(rng, 300, 2, 2, missing=(255, 256, 280))
    b = ic.bank(imms)
    long = b.run(U, Y, outputs=OUTS)                   # two chunks: 256 steps and 44
    h, _ = ic.host_run(host, imms, U, Y, 300)
    ic.same(long, h, what="T = 300")
    b.reset()
    bare = b.run(U, Y)                                 # no per-step output: nothing is staged out, nothing is combined
    assert kc.bits_equal(bare["ll"], long["ll"])
    end = ig.final(b)
    b.reset()
    b.run(U, Y, outputs=OUTS)
    ig.same_final(b, end, "with and without per-step outputs")
    ig.check_continuation(FAM, host, imms, U[:50], Y[:50], cut=25)


def test_a_nan_imm_leaves_its_neighbours_in_the_wave_alone(host):
    rng = np.random.default_rng(6)
    imms = FAM.imms(rng, 70, 3, 2, 1, 0)
    _, Y = _data(rng, 30, 0, 1, missing=(5, 6, 20))
    for interact in (True, False):
        ig.check_a_nan_imm(FAM, host, imms, None, Y, interact=interact, missing=(5, 6, 20), nan_filter=13, nan_mode=1)


def test_a_mode_without_mass_on_the_device(host):
    rng = np.random.default_rng(8)
    imms = FAM.imms(rng, 70, 4, 3, 2, 1)
    U, Y = _data(rng, 30, 1, 2, missing=(9,))
    ig.check_a_mode_without_mass(FAM, host, imms, U, Y, mu0=[0.5, 0.0, 0.25, 0.25])


def test_set_parameters_is_a_fresh_bank():
    rng = np.random.default_rng(9)
    old, new = FAM.imms(rng, 70, 2, 3, 2, 1), FAM.imms(rng, 70, 2, 3, 2, 1)
    U, Y = _data(rng, 20, 1, 2, missing=(3,))
    ig.check_set_models(FAM, old, new, U, Y)


def test_python_api():
    rng = np.random.default_rng(7)
    M, T = 3, 40
    mts = [kc.matrices(*kc.random_system(rng, 3, 2, 1, j)) for j in range(M)]
    kfs = [llpf_amd.KalmanFilter(mt["A"], mt["B"], mt["C"], mt["D"], mt["R1"], mt["R2"], llpf_amd.MvNormal(mt["x0"], mt["P0"])) for mt in mts]
    P, mu0 = ic.random_P(rng, M), ic.random_mu(rng, M)
    U, Y = kc.simulate(rng, mts[0], T, missing=(9,))
    imm = llpf_amd.IMM(kfs, P, mu0)
    assert imm._handle is None
    sol = llpf_amd.forward_trajectory(imm, U, Y)
    assert sol.x.shape == (T, 3) and sol.Rt.shape == (T, 3, 3) and sol.mu.shape == (T, M) and sol.ll_modes.shape == (T, M)
    assert sol.e is None and np.isscalar(sol.ll) and sol.t.shape == (T,)
    systems = [kf._model() for kf in kfs]
    ref = ic.numpy_reference(ic.imm([m for m, _ in systems], P=P, mu0=mu0, D=[D for _, D in systems]), U, Y)
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        assert kc.close(getattr(sol, k), ref[k]), k
    assert abs(sol.ll - ref["ll"]) <= 1e-10 * abs(ref["ll"])
    assert llpf_amd.loglik(imm, U, Y) == sol.ll
    llpf_amd.reset(imm)
    assert kc.bits_equal(imm.mu, mu0)
    lls = [llpf_amd.update(imm, U[t], Y[t])[0] for t in range(T)]
    assert kc.close(np.array(lls), ref["ll_steps"]) and lls[9] == 0.0
    assert np.allclose(llpf_amd.state(imm), imm.x) and llpf_amd.covariance(imm).shape == (3, 3) and abs(imm.mu.sum() - 1.0) <= 1e-12
    # a bank: row for row the single filters
    other = llpf_amd.IMM(kfs[::-1], P.T / P.T.sum(axis=1, keepdims=True), mu0[::-1])
    bank = llpf_amd.IMMBank([imm, other, (kfs, P, mu0)])
    ll = bank.loglik(U, Y)
    assert ll[0] == sol.ll and ll[2] == sol.ll and ll[1] == llpf_amd.loglik(other, U, Y)
    fw = bank.forward(U, Y)
    for k in ("x", "xt", "R", "Rt", "mu", "ll_modes"):
        assert kc.bits_equal(fw[k][:, 0], getattr(sol, k)), k
    x, R, mu = bank.state()
    assert x.shape == (3, 3) and R.shape == (3, 3, 3) and mu.shape == (3, M)
    bank.set_parameters([other, other, other])
    ll2 = bank.loglik(U, Y)
    assert ll2[0] == ll2[1] == ll2[2] == ll[1]
    bank.reset()
    with pytest.raises(TypeError, match="no smoother"):
        bank.smooth(U, Y)
    # one mode: the Kalman filter
    one = llpf_amd.IMM([kfs[0]], [[1.0]], [1.0])
    s1, sk = llpf_amd.forward_trajectory(one, U, Y), llpf_amd.forward_trajectory(kfs[0], U, Y)
    for k in ("x", "xt", "R", "Rt"):
        assert kc.bits_equal(getattr(s1, k), getattr(sk, k)), k
    assert s1.ll == sk.ll and np.all(s1.mu == 1.0)
