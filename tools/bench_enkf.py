"""Throughput of a bank of ensemble Kalman filters (llpf_enkf_bank_run): member-steps per second for F in {256, 1024, 4096} filters of
N in {64, 256, 1024, 4096} members, T = 1000, on the linear-Gaussian model at (nx, ny) = (2, 1) and on the quad-tank, with ll_total only
and with every per-step output.  In the same process on the same inputs it also times a FilterBank (llpf_bank_run) of the same F x N —
what gave such a model a log-likelihood per parameter set before — and the unscented bank (llpf_ukf_bank_run, Merwe (1, 0, 1)) at the
same F.  End-to-end wall time of the call around its synchronise (median of --reps after one warm-up, with the spread of the
repetitions); the kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (k_enkf<...>).  Prints one JSON
line per configuration."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import llpf_amd  # noqa: E402,F401
from llpf_amd import _capi, _structs as S  # noqa: E402
import models as M  # noqa: E402
import ukf_common as uc  # noqa: E402

OUTS = _capi.KALMAN_OUTPUTS


def quadtank_models(n):
    base = M.quadtank_model()
    return [S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, 2, gamma1=0.2 + 0.0005 * (k % 100))
            for k in range(n)]


def timed(run, reps):
    ts = []
    for r in range(reps + 1):
        t1 = time.perf_counter()
        ll = run()
        ts.append(time.perf_counter() - t1)
        assert np.all(np.isfinite(ll))
    return float(np.median(ts[1:])), min(ts[1:]), max(ts[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", default="256,1024,4096")
    ap.add_argument("--N", default="64,256,1024,4096")
    ap.add_argument("--cases", default="2x1,quadtank")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-particle-bank", action="store_true")
    a = ap.parse_args()
    T = a.T
    for case in a.cases.split(","):
        if case == "quadtank":
            nx, ny = 4, 2
            base = quadtank_models(256)
            U, Y = M.quadtank_data(T)
            t_index0 = 1.0
        else:
            nx, ny = 2, 1
            base = [M.lg_test_model(0.05 + 0.002 * k) for k in range(256)]
            _, U, Y = M.simulate_lg(M.lg_test_model(0.1), T, seed=0)
            t_index0 = 1.0
        for F in (int(v) for v in a.F.split(",")):
            models = [base[k % len(base)] for k in range(F)]
            bu = _capi.UkfBankHandle(0, models, uc.merwe(nx, 1.0, 0.0, 1.0))

            def run_ukf():
                bu.reset()
                return bu.run(U, Y, t_index0=t_index0)["ll"]
            uwall, ulo, uhi = timed(run_ukf, a.reps)
            bu.close()
            for N in (int(v) for v in a.N.split(",")):
                be = _capi.EnkfBankHandle(0, models, N, seed=1)
                rec = dict(bench="enkf", case=case, nx=nx, ny=ny, F=F, N=N, T=T, ukf_wall_s=uwall, ukf_wall_min_s=ulo, ukf_wall_max_s=uhi)
                for outputs in ((), OUTS):
                    def run_enkf():
                        be.seed(1)
                        return be.run(U, Y, outputs=outputs, t_index0=t_index0)["ll"]
                    wall, lo, hi = timed(run_enkf, a.reps)
                    tag = "all" if outputs else "ll"
                    rec.update({tag + "_wall_s": wall, tag + "_wall_min_s": lo, tag + "_wall_max_s": hi, tag + "_member_steps_per_s": F * N * T / wall})
                be.close()
                if not a.no_particle_bank:
                    pf = _capi.BankHandle(S.make_config(models[0], N, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.1, 1, 0), models)

                    def run_pf():
                        pf.reset()
                        return pf.run(U, Y, t_index0=t_index0)["ll"]
                    pwall, plo, phi = timed(run_pf, a.reps)
                    pf.close()
                    rec.update(pf_wall_s=pwall, pf_wall_min_s=plo, pf_wall_max_s=phi, pf_particle_steps_per_s=F * N * T / pwall,
                               pf_over_enkf=pwall / rec["ll_wall_s"])
                print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
