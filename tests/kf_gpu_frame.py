"""Shared frame of the GPU tests of the Kalman-family banks (test_gpu_{kalman,ukf,ekf,iekf,enkf,kalman_smooth,ukf_smooth}.py).

Every bank of the family (Kalman, unscented, extended, iterated extended, ensemble) runs F filters over T steps behind one handle, and its
GPU tests hold the device to the bank's C twin (tests/kf_host.py) bit for bit.  What the files have in common is here once: the model
lists they run, and the test bodies that differ between two banks only in how a bank is made and which twin it is held to.  A test file
says that with a `Family`; the bodies take every size of their case as an argument, so the file still states the case it runs, and they
end where the files stop agreeing: what a file asserts beyond the common part stays in the file, after the call."""
import ctypes as C
from collections import namedtuple

import numpy as np
import pytest

import llpf_amd
from llpf_amd import _capi, _structs as S
import ekf_common as ec
import kalman_common as kc
from kalman_common import _data, _same
from gpu_common import _Inject
import models as M
import ukf_common as uc

OUTS = _capi.KALMAN_OUTPUTS
SOUTS = ("xT", "RT")


# ------------------------------------------------------------------------------------------------
# the model lists
# ------------------------------------------------------------------------------------------------
def with_id(m, model_id):
    c = S.Model.from_buffer_copy(bytes(m))
    c.model_id = model_id
    return c


def lg_models(rng, F, nx, ny, nu):
    return [kc.random_system(rng, nx, ny, nu, k % 3, D=False)[0] for k in range(F)]


def quadtank_models(F):
    base = M.quadtank_model()
    return [S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, 2,
                                  gamma1=0.2 + 0.001 * (k % 50), a1=0.03 + 0.0001 * (k % 7)) for k in range(F)]


def pendulum_models(n):
    out = []
    for k in range(n):
        m = uc.pendulum_model()
        m.qt[0], m.qt[1] = 9.81 * (1 + 0.002 * k), 0.05 + 0.001 * (k % 10)
        out.append(m)
    return out


def square_models(n):
    return [ec.square_model(1.0 + 0.01 * k, 0.36) for k in range(n)]


def c1_specs(n):
    specs = []
    for k in range(n):
        mt = kc.matrices(M.lg_c1_model(seed=k), np.zeros((2, 2)))
        specs.append((llpf_amd.LinearDynamics(mt["A"], mt["B"]), llpf_amd.LinearMeasurement(mt["C"]), llpf_amd.MvNormal(np.zeros(2), mt["R1"]),
                      llpf_amd.MvNormal(np.zeros(2), mt["R2"]), llpf_amd.MvNormal(mt["x0"], mt["P0"])))
    return specs


def quadtank_specs(n):
    specs = []
    for k in range(n):
        specs.append((llpf_amd.QuadTankDynamics(supersample=2, gamma1=0.2 + 0.01 * k), llpf_amd.QuadTankMeasurement(),
                      llpf_amd.MvNormal(np.zeros(4), np.full(4, 0.1)), llpf_amd.MvNormal(np.zeros(2), np.full(2, 1e-4)),
                      llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1))))
    return specs


# ------------------------------------------------------------------------------------------------
# one bank, as the shared bodies see it
# ------------------------------------------------------------------------------------------------
Family = namedtuple("Family", "name bank host_run models timed host_smooth", defaults=(None,))
Family.__doc__ = """One bank to the shared bodies; a test file builds its own, and another one where a test needs other weights or iterations.
name: "kalman", "ukf", "ekf" or "iekf", also the stem of the fault-injection sites ("error:%s_smooth") and of the C entry points.
bank(models): a fresh handle.  host_run(host, models, U, Y, T, **kw): the twin's (outputs, final state).  models(rng, F, nx, ny, nu): F random
linear-Gaussian filters in the form `bank` and `host_run` take.  timed: whether the bank's C entry points take t_index0.
host_smooth(hsmooth, models, U, forward, T, **kw), in the two smoother files: the twin's smoothed outputs over the forward ones.  The bodies
of a family that has it smooth where the others run, take `host` as the pair (host, hsmooth) and compare xT and RT as well."""


def every_output(fam, b, U, Y, *per_filter, **kw):
    """the family's verb with every forward output: a smooth where the family has a smoother twin, a run elsewhere"""
    if fam.host_smooth is None:
        return b.run(U, Y, *per_filter, outputs=OUTS, **kw)
    return b.smooth(U, Y, *per_filter, forward=OUTS, **kw)


def keys(fam):
    return OUTS + (() if fam.host_smooth is None else SOUTS) + ("ll",)


def twin(fam, host, models, U, Y, T, **kw):
    """every output of the family's verb from the twin, and the final state"""
    if fam.host_smooth is None:
        return fam.host_run(host, models, U, Y, T, **kw)
    h, st = fam.host_run(host[0], models, U, Y, T, **kw)
    h.update(fam.host_smooth(host[1], models, U, h, T, **kw))
    return h, st


# ------------------------------------------------------------------------------------------------
# the shared bodies
# ------------------------------------------------------------------------------------------------
def check_shape(fam, host, rng, *, F, T, nx, ny, nu, missing, what):
    """F random filters of one shape over T steps against the twin.  Returns the bank, the device's and the twin's outputs, the twin's
    final state, U and Y."""
    models = fam.models(rng, F, nx, ny, nu)
    U, Y = _data(rng, T, nu, ny, missing=missing)
    b = fam.bank(models)
    g = every_output(fam, b, U, Y)
    h, st = twin(fam, host, models, U, Y, T)
    _same(g, h, keys(fam), what)
    return b, g, h, st, U, Y


def check_broadcast_inputs(fam, b, g, U, Y, *, F, nu, what):
    """the shared U and Y handed to `b` as per-filter inputs give the bits `g` of the shared run"""
    b.reset()
    gp = every_output(fam, b, np.broadcast_to(U, (F,) + U.shape), np.broadcast_to(Y, (F,) + Y.shape), u_per_filter=nu > 0, y_per_filter=True)
    _same(gp, g, keys(fam), what)


def check_each_output_alone(fam, host, *, seed, F, T, nx, ny, nu):
    """one bank, every output at once (held to the twin), then from a reset one run per output with only that output asked for: its
    columns and ll are the bits of the run with every output.  A smoother family asks for one forward output at a time beside xT and RT,
    then for xT alone and for RT alone."""
    rng = np.random.default_rng(seed)
    models = fam.models(rng, F, nx, ny, nu)
    U, Y = _data(rng, T, nu, ny)
    b = fam.bank(models)
    ref = every_output(fam, b, U, Y)
    _same(ref, twin(fam, host, models, U, Y, T)[0], keys(fam), "every output")
    for key in OUTS:
        b.reset()
        one = b.run(U, Y, outputs=(key,)) if fam.host_smooth is None else b.smooth(U, Y, forward=(key,))
        _same(one, ref, (key, "ll"), "%s alone" % key)
    for key in () if fam.host_smooth is None else SOUTS:
        b.reset()
        _same(b.smooth(U, Y, outputs=(key,)), ref, (key, "ll"), "%s alone" % key)
    b.close()


def check_bank_sizes_and_chunk_edges(fam, host, *, seed, F, nx, ny, nu, missing, Ts):
    """one bank of F filters over the first T of max(Ts) steps for every T of Ts, from a reset: the outputs and the final state"""
    rng = np.random.default_rng(seed)
    models = fam.models(rng, F, nx, ny, nu)
    U, Y = _data(rng, max(Ts), nu, ny, missing=missing)
    b = fam.bank(models)
    for T in Ts:
        b.reset()
        g = every_output(fam, b, U[:T], Y[:T])
        h, st = twin(fam, host, models, U[:T], Y[:T], T)
        _same(g, h, keys(fam), (F, T))
        x, R = b.get_state()
        assert kc.bits_equal(x, st[0]) and kc.bits_equal(R, st[1]), (F, T, "final state")


def check_continuation(fam, host, *, seed, F, T, nx, ny, nu, missing, cut):
    """run(a) then run(b) is run(a + b), cut after `cut` steps; the second half against the twin from the state between; set_state on
    a fresh bank; ll alone.  Returns (rng, b, U, Y) for what the file sets on `b` next."""
    rng = np.random.default_rng(seed)
    models = fam.models(rng, F, nx, ny, nu)
    U, Y = _data(rng, T, nu, ny, missing=missing)
    b = fam.bank(models)
    whole = b.run(U, Y, outputs=OUTS)
    b.reset()
    first = b.run(U[:cut], Y[:cut], outputs=OUTS)
    x, R = b.get_state()
    second = b.run(U[cut:], Y[cut:], outputs=OUTS, t_index0=float(cut))
    for k in OUTS:
        assert kc.bits_equal(np.concatenate([first[k], second[k]]), whole[k]), k
    h2, _ = fam.host_run(host, models, U[cut:], Y[cut:], T - cut, state=(x, R), t_index0=float(cut))
    _same(second, h2, what="second half")
    fresh = fam.bank(models)
    fresh.set_state(x, R)
    xs, Rs = fresh.get_state()
    assert kc.bits_equal(xs, x) and kc.bits_equal(np.tril(Rs), np.tril(R))
    again = fresh.run(U[cut:], Y[cut:], outputs=OUTS, t_index0=float(cut))
    _same(again, second, what="set_state")
    b.reset()
    bare = b.run(U, Y)                                  # ll only: nothing is staged per step
    assert kc.bits_equal(bare["ll"], whole["ll"])
    return rng, b, U, Y


def check_per_filter_inputs_and_a_nan_filter(fam, host, *, seed, F, T, nx, ny, nu, missing, stride, row, nan_filter):
    """per-filter U and Y, the rows `missing` missing for every filter and `row` for every `stride`-th; then filter `nan_filter` from an
    indefinite covariance: NaN in its own outputs, the others' bits unmoved, and the twin's"""
    rng = np.random.default_rng(seed)
    models = fam.models(rng, F, nx, ny, nu)
    U = rng.standard_normal((F, T, nu))
    Y = 2.0 * rng.standard_normal((F, T, ny))
    Y[:, list(missing), 0] = np.nan
    Y[::stride, row, 0] = np.nan
    b = fam.bank(models)
    x, R = b.get_state()
    ok = b.run(U, Y, True, True, outputs=OUTS)
    assert np.all(ok["ll_steps"][list(missing)] == 0.0) and np.all(np.isnan(ok["e"][list(missing)]))
    h, _ = fam.host_run(host, models, U, Y, T, per_filter=3)
    _same(ok, h, what="per-filter inputs")
    R[nan_filter] = -100.0 * np.eye(nx)
    b.set_state(x, R)
    bad = b.run(U, Y, True, True, outputs=OUTS)
    assert np.isnan(bad["ll"][nan_filter]) and np.all(np.isnan(bad["xt"][:, nan_filter])) and np.all(np.isnan(bad["R"][1:, nan_filter]))
    assert np.all(bad["ll_steps"][list(missing), nan_filter] == 0.0)
    keep = [f for f in range(F) if f != nan_filter]
    for k in OUTS:
        assert kc.bits_equal(bad[k][:, keep], ok[k][:, keep]), k
    hb, _ = fam.host_run(host, models, U, Y, T, per_filter=3, state=(x, R))
    _same(bad, hb, what="NaN filter")


def check_throw_and_refused_allocation(fam, *, seed, F, T, nx, ny, nu, short, huge):
    """a smooth that throws (error:<name>_smooth) is a status and leaves the state; a smooth of `huge` steps after a run of `short` is
    refused by the allocation of its stored posterior before any launch, the state and the outputs untouched; the handle smooths on"""
    rng = np.random.default_rng(seed)
    models = fam.models(rng, F, nx, ny, nu)
    U, Y = _data(rng, T, nu, ny)
    b = fam.bank(models)
    ref = b.smooth(None, Y)
    b.reset()
    xi, Ri = b.get_state()
    with _Inject("error:%s_smooth" % fam.name):
        with pytest.raises(_capi.LLPFError) as ei:
            b.smooth(None, Y)
    assert ei.value.code == _capi.ERR_INTERNAL
    x0, R0 = b.get_state()
    assert kc.bits_equal(x0, xi) and kc.bits_equal(R0, Ri)
    again = b.smooth(None, Y)
    _same(again, ref, SOUTS + ("ll",), "after a throw")
    b.reset()
    b.run(None, Y[:short])
    x1, R1 = b.get_state()
    out = S.KalmanSmoothOutputs()
    out.struct_size = C.sizeof(S.KalmanSmoothOutputs)
    xT = np.zeros(4)
    out.xT = _capi.dptr(xT)
    ll = np.zeros(F)
    smooth = getattr(_capi.lib(), "llpf_%s_bank_smooth" % fam.name)
    rc = smooth(b.h, None, _capi.dptr(Y), C.c_int64(huge), 0, *((0.0,) if fam.timed else ()), _capi.dptr(ll), None, C.byref(out))
    assert rc == _capi.ERR_ALLOC, rc
    x2, R2 = b.get_state()
    assert kc.bits_equal(x1, x2) and kc.bits_equal(R1, R2) and np.all(xT == 0.0)
    b.reset()
    _same(b.smooth(None, Y), ref, SOUTS + ("ll",), "after a refused allocation")
