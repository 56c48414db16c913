"""Throughput of a bank of extended Kalman filters (llpf_ekf_bank_run): filter-steps per second for F in {1e3, 1e4, 1e5}, T = 1000, on
the linear-Gaussian model at (nx, ny) in {(2, 1), (4, 2)} and on the quad-tank — tools/bench_ukf.py's models and sizes — with ll_total
only and with every per-step output, against the single-thread host build of the same header (tests/ekf_host.c, cc -O2), and beside the
unscented bank (llpf_ukf_bank_run, Merwe (1, 0, 1)) timed in the same process on the same inputs.  End-to-end wall time of the call
around its synchronise (median of --reps after one warm-up, with the spread of the repetitions); the kernels' own times come from a
`rocprofv3 --kernel-trace --stats` run of this script.  Runs whose outputs would exceed --max-out-gb of host memory are skipped.
Prints one JSON line per configuration.
--iterated: the iterated extended Kalman filter (llpf_ekf_bank_set_iterations, maxiters 10, epsilon 1e-8) beside the plain one instead
of the unscented bank — the same bank handle, ll_total only, plain then iterated in the same process — on the same models and sizes and
on a bank of pendulum snippets with per-filter priors (tests/ekf_common.py: PENDULUM_JAC_SRC), the one case whose lanes iterate more
than twice; its mean linearisations per step come from the host build (tests/ekf_host.c) over --host-filters filters.  In a rocprofv3
run the plain kernel is k_ekf<..., EkfArgs> and the iterated one k_ekf<..., IekfArgs>."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import llpf_amd  # noqa: E402,F401
from llpf_amd import _capi, _structs as S  # noqa: E402
import ekf_common as ec  # noqa: E402
import iekf_common as ic  # noqa: E402
import kalman_common as kc  # noqa: E402
import models as M  # noqa: E402
import ukf_common as uc  # noqa: E402

OUTS = _capi.KALMAN_OUTPUTS


def quadtank_models(n):
    base = M.quadtank_model()
    return [S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, 2, gamma1=0.2 + 0.0005 * (k % 100))
            for k in range(n)]


def timed(bank, U, Y, outputs, t_index0, reps):
    ts = []
    for r in range(reps + 1):
        bank.reset()
        t1 = time.perf_counter()
        res = bank.run(U, Y, outputs=outputs, t_index0=t_index0)
        ts.append(time.perf_counter() - t1)
        assert np.all(np.isfinite(res["ll"]))
        del res
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


ITERATIONS = (10, 1e-8)


def iterated(a):
    """plain against iterated, ll only: one JSON line per (case, F)"""
    host = ic.build_host(tempfile.mkdtemp())
    rng = np.random.default_rng(0)
    T = a.T
    for case in a.cases.split(",") + ["pendulum"]:
        kind = None
        if case == "quadtank":
            nx, ny = 4, 2
            base = hbase = quadtank_models(256)
            U, Y = M.quadtank_data(T)
            t_index0 = 1.0
        elif case == "pendulum":
            nx, ny = 2, 1
            hbase, base = ic.pendulum_bank_models(256), ic.pendulum_bank_models(256, _capi.model_compile(ec.PENDULUM_JAC_SRC, 2, 1))
            U, Y = uc.pendulum_data(T)
            t_index0, kind = 0.0, ec.KIND_PENDULUM
        else:
            nx, ny = (int(v) for v in case.split("x"))
            base = hbase = [kc.random_system(rng, nx, ny, 1, k % 3, D=False)[0] for k in range(256)]
            U = rng.standard_normal((T, 1))
            Y = rng.standard_normal((T, ny))
            t_index0 = 0.0
        h, _ = ic.host_run(host, hbase[: a.host_filters], U, Y, T, *ITERATIONS, t_index0=t_index0, kind=kind)
        for F in (int(v) for v in a.F.split(",")):
            be = _capi.EkfBankHandle(0, [base[k % len(base)] for k in range(F)])
            wall, lo, hi = timed(be, U, Y, (), t_index0, a.reps)
            be.set_iterations(*ITERATIONS)
            iwall, ilo, ihi = timed(be, U, Y, (), t_index0, a.reps)
            print(json.dumps(dict(bench="iekf", case=case, nx=nx, ny=ny, F=F, T=T, outputs="ll", maxiters=ITERATIONS[0], epsilon=ITERATIONS[1],
                                  mean_linearisations=float(h["iters"].mean()), max_linearisations=int(h["iters"].max()),
                                  wall_s=wall, wall_min_s=lo, wall_max_s=hi, iterated_wall_s=iwall, iterated_wall_min_s=ilo,
                                  iterated_wall_max_s=ihi, iterated_over_plain=iwall / wall)), flush=True)
            be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", default="1000,10000,100000")
    ap.add_argument("--cases", default="2x1,4x2,quadtank")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-out-gb", type=float, default=6.0)
    ap.add_argument("--host-filters", type=int, default=100)
    ap.add_argument("--iterated", action="store_true")
    a = ap.parse_args()
    if a.iterated:
        return iterated(a)
    host = ec.build_host(tempfile.mkdtemp())
    rng = np.random.default_rng(0)
    T = a.T
    Fs = [int(v) for v in a.F.split(",")]
    for case in a.cases.split(","):
        if case == "quadtank":
            nx, ny = 4, 2
            base = quadtank_models(256)
            U, Y = M.quadtank_data(T)
            t_index0 = 1.0
        else:
            nx, ny = (int(v) for v in case.split("x"))
            base = [kc.random_system(rng, nx, ny, 1, k % 3, D=False)[0] for k in range(256)]
            U = rng.standard_normal((T, 1))
            Y = rng.standard_normal((T, ny))
            t_index0 = 0.0
        t0 = time.perf_counter()
        ec.host_run(host, base[: a.host_filters], U, Y, T, t_index0=t_index0)
        host_rate = a.host_filters * T / (time.perf_counter() - t0)      # (outputs included: the host loop writes them either way)
        w = uc.merwe(nx, 1.0, 0.0, 1.0)
        for F in Fs:
            models = [base[k % len(base)] for k in range(F)]
            be = _capi.EkfBankHandle(0, models)
            bu = _capi.UkfBankHandle(0, models, w)
            per_step = 1 + 2 * nx + 2 * nx * nx + ny
            for outputs in ((), OUTS):
                gb = F * T * per_step * 8 / 2**30 if outputs else 0.0
                rec = dict(bench="ekf", case=case, nx=nx, ny=ny, F=F, T=T, outputs="all" if outputs else "ll", host_steps_per_s=host_rate)
                if gb > a.max_out_gb:
                    rec["skipped"] = "outputs of %.1f GB" % gb
                    print(json.dumps(rec), flush=True)
                    continue
                wall, lo, hi = timed(be, U, Y, outputs, t_index0, a.reps)
                uwall, ulo, uhi = timed(bu, U, Y, outputs, t_index0, a.reps)
                rec.update(wall_s=wall, wall_min_s=lo, wall_max_s=hi, steps_per_s=F * T / wall, speedup_vs_host=F * T / wall / host_rate,
                           ukf_wall_s=uwall, ukf_wall_min_s=ulo, ukf_wall_max_s=uhi, ukf_over_ekf=uwall / wall)
                print(json.dumps(rec), flush=True)
            be.close()
            bu.close()


if __name__ == "__main__":
    main()
