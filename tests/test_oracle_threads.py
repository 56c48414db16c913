"""The device-order oracle gives the same bits at any thread count.

Every GPU parity test holds the engine to the device-order oracle, and the long ones run that oracle on 16 threads to fit their
time.  Its reductions are integer sums and its bins an integer prefix sum (oracle/llpf_oracle.c: dev_exp_sums, dev_bins,
dev_search), so the thread count cannot change a bit; these tests hold it to that, over whole runs, at 1 and 8 threads.
Together with the goldens, the known-answer tests and the independent oracle (which pin the 1-thread bits) they show that the
parallel oracle computes what the serial one did."""
import numpy as np
import pytest

import bench
import models as M
import oracle_binding as ob
import rbfull_models as RM
from llpf_amd import _structs as S

THREADS = (1, 8)


def _lg(N, T, thr, strategy=S.RESAMPLE_SYSTEMATIC):
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, T, seed=1)
    return S.make_config(model, N, S.PARTICLE_FILTER, strategy, thr, 1000, 0), U, Y


def _bench(name, N, T, thr=None):
    model, U, Y, kind, thr0, _ = bench.build_workload(name, N, T)
    return S.make_config(model, N, kind, S.RESAMPLE_SYSTEMATIC, thr0 if thr is None else thr, 1000, 0), U, Y


def _case(name):
    """(config, U, Y, run the auxiliary filter's loglik loop)"""
    if name in ("systematic", "stratified", "residual"):
        strategy = {"systematic": S.RESAMPLE_SYSTEMATIC, "stratified": S.RESAMPLE_STRATIFIED, "residual": S.RESAMPLE_RESIDUAL}[name]
        return _lg(10007, 30, 0.5, strategy) + (False,)
    if name == "outlier":                     # the bound test of dev_norm_bound fails: the exact-max form for that step
        cfg, U, Y = _lg(20011, 24, 0.1)
        Y[12] += 12.0
        return cfg, U, Y, False
    if name == "missing":
        cfg, U, Y = _lg(20011, 24, 0.5)
        Y[[5, 6, 17]] = np.nan
        return cfg, U, Y, False
    if name == "nan_filter":                  # an infinite measurement: every weight -Inf, then NaN from there on
        cfg, U, Y = _lg(5003, 16, 0.5)
        Y[9] = np.inf
        return cfg, U, Y, False
    if name == "aux":
        return _bench("aux", 10007, 25) + (True,)
    if name == "rbpf":
        return _bench("rbpf", 10007, 30) + (False,)
    if name == "rbpf_full":
        return _bench("rbpf_full", 3001, 12) + (False,)
    if name == "quadtank":
        return _bench("quadtank", 100003, 8) + (False,)
    if name == "N1":
        return _lg(1, 20, 1.0) + (False,)         # threshold 1: a lone particle resamples (onto itself) every step
    if name == "large":
        return _lg(200003, 20, 0.1) + (False,)
    raise ValueError(name)


def _same_bits(a, b):
    """bit for bit, except that any NaN equals any NaN: the sign and payload of a NaN are no value (x86 passes on one operand's
    NaN, and the compiler may commute a product, differently in a loop's vector body and its remainder)"""
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    na = np.isnan(a)
    return np.array_equal(na, np.isnan(b)) and a[~na].tobytes() == b[~na].tobytes()


def _run(cfg, U, Y, aux, threads):
    ob.set_threads(threads)
    try:
        o = ob.OracleFilter(cfg, ob.ORDER_DEVICE)
        o.reset()
        r = o.run_aux(U, Y, 1, ll_steps=True) if aux else o.run(U, Y, 1.0, ll_steps=True)
        out = {"ll_steps": r["ll_steps"], "particles": o.particles(), "weights": o.weights(), "expweights": o.expweights(),
               "ancestors": o.ancestors(), "bins": o.bins(),
               "counts": np.array([o.resample_count(), o.exact_steps(), o.index()], dtype=np.int64)}
        if cfg.model.model_id == S.MODEL_RB_BILINEAR:
            out["xl"], out["R"] = o.rb_linear_state()
        return out, o
    finally:
        ob.set_threads(1)


CASES = ["systematic", "stratified", "residual", "outlier", "missing", "nan_filter", "aux", "rbpf", "rbpf_full", "quadtank",
         "N1", "large"]


@pytest.mark.parametrize("name", CASES)
def test_device_order_does_not_depend_on_the_thread_count(name):
    cfg, U, Y, aux = _case(name)
    (a, oa), (b, ob_) = (_run(cfg, U, Y, aux, n) for n in THREADS)
    for key in a:
        assert a[key].dtype == b[key].dtype and a[key].shape == b[key].shape, key
        assert _same_bits(a[key], b[key]), "%s: %s differs between %d and %d threads" % (name, key, *THREADS)
    # the case exercises what it is named for
    ll = a["ll_steps"]
    if name == "nan_filter":
        assert np.all(np.isfinite(ll[:9])) and np.isnan(ll[9])
    else:
        assert np.all(np.isfinite(ll))
    if name == "outlier":
        assert oa.exact_steps() >= 1
    if name in ("systematic", "stratified", "residual", "missing", "large"):
        assert 0 < oa.resample_count() < len(Y)           # resampling and non-resampling steps mixed
    if name == "N1":
        assert oa.resample_count() >= 1


@pytest.mark.parametrize("strategy", [S.RESAMPLE_SYSTEMATIC, S.RESAMPLE_STRATIFIED])
@pytest.mark.parametrize("n,m", [(1, 1), (7, 7), (4097, 300), (300, 4097), (100003, 100003)])
def test_standalone_device_order_resample_does_not_depend_on_the_thread_count(strategy, n, m):
    rng = np.random.default_rng(n + m)
    we = rng.exponential(size=n) ** 3
    we /= we.sum()
    U = ob.resample_uniforms(strategy, m, 77, 3)
    out = []
    for th in THREADS:
        ob.set_threads(th)
        try:
            out.append(ob.resample(strategy, we, U, m, order=ob.ORDER_DEVICE))
        finally:
            ob.set_threads(1)
    (j1, b1), (j8, b8) = out
    assert np.array_equal(j1, j8)
    assert b1.tobytes() == b8.tobytes()
    # the first bin above every threshold (src/resample.jl:23-34 / :49-58), an output with none left as it was (0 here)
    binsN = b1[-1]
    i = np.arange(m, dtype=np.float64)
    thr = U[0] * binsN / n + i * (1.0 / m) if strategy == S.RESAMPLE_SYSTEMATIC else (i + U) / m * binsN
    k = np.searchsorted(b1, thr, side="right")
    assert np.array_equal(j1, np.where(k < n, k, 0))
