"""Shared frame of the GPU tests of the IMM banks (test_gpu_imm.py, test_gpu_imm_ekf.py), beside kf_gpu_frame.py and in its style.

Both banks run F IMMs of M modes over T steps behind _capi.IMMBankHandle, and their GPU tests hold the device to one C twin
(imm_common.host_run, which picks the entry point by the IMMs' D) bit for bit.  The bodies the two files had in common are here once.  A
file says what differs with an `ImmFamily`; the bodies take every size of their case as an argument, or the IMMs and the data the file
made, and they end where the files stop agreeing: what a file asserts beyond the common part stays in the file, after the call."""
from collections import namedtuple

import numpy as np

import imm_common as ic
from imm_common import OUTS
import kalman_common as kc
from kalman_common import _data

ImmFamily = namedtuple("ImmFamily", "imms t0")
ImmFamily.__doc__ = """One kind of IMM to the shared bodies.  imms(rng, F, M, nx, ny, nu): F IMMs of M modes of one shape in imm_common's
form (with a D: a Kalman bank; without: an extended one).  t0: the t_index0 of a run from a reset, or None where a run is given no time
(the Kalman IMM takes none; an extended bank then starts at 0)."""


def at(fam, steps=0):
    """the time arguments of a run, and of the twin's, that starts `steps` after the family's t0"""
    return {} if fam.t0 is None else {"t_index0": fam.t0 + steps}


def final(b):
    """(mu, x_modes, R_modes) of a bank"""
    return b.get_modes()[2:]


def same_final(b, st, what=""):
    for a, s in zip(final(b), st):
        assert kc.bits_equal(a, s), (what, "final state")


def check_shape(fam, host, rng, *, F, T, M, nx, ny, nu, missing, what):
    """F IMMs of one shape over T steps, interact on and off: every output and the final (mu, x_modes, R_modes) against the twin,
    get_state's combined estimate against host_combine, zeros at the missing rows, mu a distribution; the shared inputs handed per filter;
    per-filter inputs of their own whose missing rows differ between the filters of a wave"""
    imms = fam.imms(rng, F, M, nx, ny, nu)
    U, Y = _data(rng, T, nu, ny, missing=missing)
    Uf = rng.standard_normal((F, T, nu))
    Yf = 2.0 * rng.standard_normal((F, T, ny))
    Yf[::3, 11, 0] = Yf[1::4, 12, 0] = Yf[:, 20, 0] = np.nan
    for interact in (True, False):
        w = what + (interact,)
        b = ic.bank(imms, interact)
        g = b.run(U, Y, outputs=OUTS, **at(fam))
        h, st = ic.host_run(host, imms, U, Y, T, interact=interact, **at(fam))
        ic.same(g, h, what=w)
        same_final(b, st, w)
        x, R = b.get_state()
        xh, Rh = ic.host_combine(host, *st)
        assert kc.bits_equal(x, xh) and kc.bits_equal(R, Rh), w
        assert np.all(g["ll_steps"][list(missing)] == 0.0) and np.all(g["ll_modes"][list(missing)] == 0.0), w
        assert np.all(np.isfinite(g["ll"])) and np.all(g["mu"] >= 0.0) and np.all(np.abs(g["mu"].sum(axis=2) - 1.0) <= 1e-12), w
        b.reset()
        gp = b.run(np.broadcast_to(U, (F,) + U.shape), np.broadcast_to(Y, (F,) + Y.shape), nu > 0, True, outputs=OUTS, **at(fam))
        ic.same(gp, g, what=w + ("shared inputs given per filter",))
        b.reset()
        gf = b.run(Uf, Yf, nu > 0, True, outputs=OUTS, **at(fam))
        hf, _ = ic.host_run(host, imms, Uf, Yf, T, per_filter=3, interact=interact, **at(fam))
        ic.same(gf, hf, what=w + ("per-filter inputs",))
        b.close()


def check_continuation(fam, host, imms, U, Y, *, cut):
    """run(a) then run(b) is run(a + b), cut after `cut` steps, in every output and in the final state; the second half against the twin
    from the state between; set_state on a fresh bank; ll alone: the same ll, the same final state"""
    T = Y.shape[0]
    b = ic.bank(imms)
    whole = b.run(U, Y, outputs=OUTS, **at(fam))
    end = final(b)
    b.reset()
    first = b.run(U[:cut], Y[:cut], outputs=OUTS, **at(fam))
    st = final(b)
    second = b.run(U[cut:], Y[cut:], outputs=OUTS, **at(fam, cut))
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    same_final(b, end, "two runs")
    h2, _ = ic.host_run(host, imms, U[cut:], Y[cut:], T - cut, state=st, **at(fam, cut))
    ic.same(second, h2, what="second half")
    fresh = ic.bank(imms)
    fresh.set_state(*st)
    for a, s in zip(final(fresh), st):
        assert kc.bits_equal(np.tril(a) if a.ndim == 4 else a, np.tril(s) if s.ndim == 4 else s)
    again = fresh.run(U[cut:], Y[cut:], outputs=OUTS, **at(fam, cut))
    ic.same(again, second, what="set_state")
    b.reset()
    bare = b.run(U, Y, **at(fam))                       # ll only: nothing is staged per step, nothing is combined
    assert kc.bits_equal(bare["ll"], whole["ll"])
    same_final(b, end, "ll alone")


def check_a_nan_imm(fam, host, imms, U, Y, *, interact, missing, nan_filter, nan_mode):
    """IMM `nan_filter` from an indefinite covariance of its mode `nan_mode`: NaN in its own outputs from that step on (0 at the rows
    `missing`) and in its final state, the other filters' bits unmoved, and the twin's bits.  Returns the bank and its outputs of the run
    from a reset."""
    F, T, nx = len(imms), Y.shape[0], imms[0]["models"][0].nx
    b = ic.bank(imms, interact)
    ok = b.run(U, Y, outputs=OUTS, **at(fam))
    mu, xm, Rm = ic.initial_state(imms)
    Rm[nan_filter, nan_mode] = -100.0 * np.eye(nx)
    b.set_state(mu, xm, Rm)
    bad = b.run(U, Y, outputs=OUTS, **at(fam))
    n, steps = nan_filter, np.delete(np.arange(T), list(missing))
    assert np.all(np.isnan(bad["ll_steps"][steps, n])) and np.all(bad["ll_steps"][list(missing), n] == 0.0) and np.isnan(bad["ll"][n])
    assert np.all(np.isnan(bad["mu"][:, n])) and np.all(np.isnan(bad["xt"][:, n])) and np.all(np.isnan(bad["x"][1:, n]))
    assert all(np.all(np.isnan(a[n])) for a in final(b))
    keep = [f for f in range(F) if f != n]
    for k in OUTS:
        assert kc.bits_equal(bad[k][:, keep], ok[k][:, keep]), (interact, k)
    assert kc.bits_equal(bad["ll"][keep], ok["ll"][keep])
    hb, _ = ic.host_run(host, imms, U, Y, T, state=(mu, xm, Rm), interact=interact, **at(fam))
    ic.same(bad, hb, what=("NaN IMM", interact))
    return b, ok


def check_a_mode_without_mass(fam, host, imms, U, Y, *, mu0):
    """every second IMM gets P = I and the initial probabilities `mu0`, whose mode 1 has none: the twin's bits in every output and in the
    final state, that mode's probability exactly 0 throughout"""
    for k, s in enumerate(imms):
        if k % 2:
            s["P"], s["mu0"] = np.eye(len(mu0)), np.array(mu0)
    b = ic.bank(imms)
    g = b.run(U, Y, outputs=OUTS, **at(fam))
    h, st = ic.host_run(host, imms, U, Y, Y.shape[0], **at(fam))
    ic.same(g, h, what="a mode without mass")
    same_final(b, st, "a mode without mass")
    assert np.all(g["mu"][:, 1::2, 1] == 0.0) and np.all(np.isfinite(g["ll"]))


def check_set_models(fam, old, new, U, Y):
    """a bank of `old` that has run, after set_models(new) and a reset, is a fresh bank of `new`.  Returns the bank and its outputs."""
    b = ic.bank(old)
    b.run(U, Y)
    b.set_models(*ic.bank_args(new))
    b.reset()
    g = b.run(U, Y, outputs=OUTS, **at(fam))
    ic.same(g, ic.bank(new).run(U, Y, outputs=OUTS, **at(fam)), what="set_models")
    return b, g
