"""Throughput of a bank of unscented Kalman filters (llpf_ukf_bank_run): filter-steps per second for F in {1e3, 1e4, 1e5}, T = 1000, on
the linear-Gaussian model at (nx, ny) in {(2, 1), (4, 2)} and on the quad-tank, with ll_total only and with every per-step output, against
the single-thread host build of the same header (tests/ukf_host.c, cc -O2).  End-to-end wall time of the call around its synchronise
(median of --reps after one warm-up, with the spread of the repetitions); the kernel's own time comes from a
`rocprofv3 --kernel-trace --stats` run of this script.  Runs whose outputs would exceed --max-out-gb of host memory are skipped.
--particles N (default 10000; 0: off): for the quad-tank at the smallest F also the same sweep's FilterBank.loglik with N particles, the
cost the unscented bank replaces.  Prints one JSON line per configuration.

--smooth: the same for llpf_ukf_bank_smooth (forward pass plus the unscented RTS smoother's backward pass) in two forms, ll + xT and
xT + RT; the host baseline is one thread running the header's forward step and its backward step (tests/ukf_host.c)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import llpf_amd  # noqa: E402
from llpf_amd import _capi, _structs as S  # noqa: E402
import kalman_common as kc  # noqa: E402
import models as M  # noqa: E402
import ukf_common as uc  # noqa: E402
import ukf_smooth_common as us  # noqa: E402

OUTS = _capi.KALMAN_OUTPUTS


def quadtank_models(n):
    base = M.quadtank_model()
    return [S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, 2, gamma1=0.2 + 0.0005 * (k % 100))
            for k in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", default="1000,10000,100000")
    ap.add_argument("--cases", default="2x1,4x2,quadtank")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-out-gb", type=float, default=6.0)
    ap.add_argument("--host-filters", type=int, default=100)
    ap.add_argument("--particles", type=int, default=10000)
    ap.add_argument("--smooth", action="store_true", help="measure llpf_ukf_bank_smooth")
    a = ap.parse_args()
    host = uc.build_host(tempfile.mkdtemp())
    hsm = us.build_host_smooth(tempfile.mkdtemp()) if a.smooth else None
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
        w = uc.merwe(nx, 1.0, 0.0, 1.0)
        if a.smooth:
            smooth_case(a, host, hsm, case, nx, ny, base, w, U, Y, t_index0, Fs)
            continue
        t0 = time.perf_counter()
        uc.host_run(host, base[: a.host_filters], w, U, Y, T, t_index0=t_index0)
        host_rate = a.host_filters * T / (time.perf_counter() - t0)      # (outputs included: the host loop writes them either way)
        for F in Fs:
            models = [base[k % len(base)] for k in range(F)]
            b = _capi.UkfBankHandle(0, models, w)
            per_step = 1 + 2 * nx + 2 * nx * nx + ny
            for outputs in ((), OUTS):
                gb = F * T * per_step * 8 / 2**30 if outputs else 0.0
                rec = dict(bench="ukf", case=case, nx=nx, ny=ny, F=F, T=T, outputs="all" if outputs else "ll", host_steps_per_s=host_rate)
                if gb > a.max_out_gb:
                    rec["skipped"] = "outputs of %.1f GB" % gb
                    print(json.dumps(rec), flush=True)
                    continue
                ts = []
                for r in range(a.reps + 1):
                    b.reset()
                    t1 = time.perf_counter()
                    res = b.run(U, Y, outputs=outputs, t_index0=t_index0)
                    ts.append(time.perf_counter() - t1)
                    assert np.all(np.isfinite(res["ll"]))
                    del res
                wall = float(np.median(ts[1:]))
                rec.update(wall_s=wall, wall_min_s=min(ts[1:]), wall_max_s=max(ts[1:]), steps_per_s=F * T / wall,
                           speedup_vs_host=F * T / wall / host_rate)
                print(json.dumps(rec), flush=True)
            b.close()
        if case == "quadtank" and a.particles > 0:        # the particle-filter sweep the unscented bank stands in for
            F = min(Fs)
            specs = [(llpf_amd.QuadTankDynamics(supersample=2, gamma1=0.2 + 0.0005 * (k % 100)), llpf_amd.QuadTankMeasurement(),
                      llpf_amd.MvNormal(np.zeros(4), np.full(4, 0.1)), llpf_amd.MvNormal(np.zeros(2), np.full(2, 1e-4)),
                      llpf_amd.MvNormal(np.array([2.0, 2.0, 3.0, 3.0]), np.full(4, 0.1))) for k in range(F)]
            pf = llpf_amd.FilterBank(a.particles, specs, rng=1)
            ts = []
            for r in range(a.reps + 1):
                t1 = time.perf_counter()
                ll = pf.loglik(U, Y)
                ts.append(time.perf_counter() - t1)
            wall = float(np.median(ts[1:]))
            print(json.dumps(dict(bench="filterbank_loglik", case=case, F=F, T=T, particles=a.particles, wall_s=wall, wall_min_s=min(ts[1:]),
                                  wall_max_s=max(ts[1:]), steps_per_s=F * T / wall, finite=int(np.isfinite(ll).sum()))), flush=True)


def smooth_case(a, host, hsm, case, nx, ny, base, w, U, Y, t_index0, Fs):
    T = a.T
    hb = base[: a.host_filters]
    t0 = time.perf_counter()
    fw, _ = uc.host_run(host, hb, w, U, Y, T, t_index0=t_index0)
    us.host_smooth(hsm, hb, w, U, fw, T, t_index0=t_index0)
    host_rate = len(hb) * T / (time.perf_counter() - t0)     # forward + backward, every output written
    del fw
    for F in Fs:
        models = [base[k % len(base)] for k in range(F)]
        b = _capi.UkfBankHandle(0, models, w)
        for form, outputs in (("ll+xT", ("xT",)), ("xT+RT", ("xT", "RT"))):
            per_step = nx + (nx * nx if "RT" in outputs else 0)
            gb = F * T * per_step * 8 / 2**30
            rec = dict(bench="ukf_smooth", case=case, nx=nx, ny=ny, F=F, T=T, outputs=form, host_steps_per_s=host_rate,
                       posterior_gb=F * T * (nx + nx * (nx + 1) // 2) * 8 / 2**30)
            if gb > a.max_out_gb:
                rec["skipped"] = "outputs of %.1f GB" % gb
                print(json.dumps(rec), flush=True)
                continue
            ts = []
            for r in range(a.reps + 1):
                b.reset()
                t1 = time.perf_counter()
                res = b.smooth(U, Y, outputs=outputs, t_index0=t_index0)
                ts.append(time.perf_counter() - t1)
                assert np.all(np.isfinite(res["ll"])) and np.all(np.isfinite(res["xT"][:, :: max(1, F // 64)]))
                del res
            wall = float(np.median(ts[1:]))
            rec.update(wall_s=wall, wall_min_s=min(ts[1:]), wall_max_s=max(ts[1:]), steps_per_s=F * T / wall,
                       speedup_vs_host=F * T / wall / host_rate)
            print(json.dumps(rec), flush=True)
        b.close()


if __name__ == "__main__":
    main()
