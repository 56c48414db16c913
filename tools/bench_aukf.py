"""Time of a bank of unscented Kalman filters with augmented process noise (llpf_aukf_bank_run) beside the unscented bank
(llpf_ukf_bank_run) in one process over the same descriptors and data: milliseconds per 1000 steps and their ratio, for
  quadtank   F = 10^4 built-in quad-tank filters with per-filter parameters, T = 1000: k_aukf takes the additive path (f at the 9 distinct
             state points, as k_ukf; 17 points in the sums);
  pendulum   F = 10^4 noisy-pendulum snippets (tests/aukf_common.py: dynamics_w at all 9 points) beside the plain pendulum snippet
             (tests/user_models.py) under k_ukf (5 points), T = 1000: the same descriptors, the noise levels read as R1 by either.
Timed the way tools/bench_sqekf.py times: the wall time of the call with ll_total only (shared inputs, nothing staged per step: the call is
its kernel launches, one per chunk of 256 steps, and ends in a device synchronise), the median of --reps after one warm-up, the two banks
alternating; the kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (k_aukf, k_ukf).  Every ll must be
finite; the largest relative difference between the two banks' ll is reported, not asserted (they are different transforms, and on the
pendulum different models).  Prints one JSON line per model."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llpf_amd import _capi  # noqa: E402
import aukf_common as ac  # noqa: E402
import kf_gpu_frame as kg  # noqa: E402
import models as M  # noqa: E402
import ukf_common as uc  # noqa: E402
import user_models as UM  # noqa: E402


def timed(banks, U, Y, reps, t_index0):
    ts = {k: [] for k in banks}
    ll = {}
    for r in range(reps + 1):
        for name, b in banks.items():
            b.reset()
            t0 = time.perf_counter()
            ll[name] = b.run(U, Y, t_index0=t_index0)["ll"]
            ts[name].append(time.perf_counter() - t0)
    return ts, ll


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", type=int, default=10000)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--models", default="quadtank,pendulum")
    a = ap.parse_args()
    F, T = a.F, a.T
    for which in a.models.split(","):
        if which == "quadtank":
            nx, ny = 4, 2
            models = kg.quadtank_models(F)
            U, Y = M.quadtank_data(T)
            pair = ac.merwe_pair(nx, 1.0, 0.0, 1.0)
            banks = {"ukf": _capi.UkfBankHandle(0, models, pair[0]), "aukf": _capi.AukfBankHandle(0, models, pair)}
            t_index0 = 1.0
        else:
            nx, ny = 2, 1
            models = ac.noisy_pendulum_models(F)
            U, Y = uc.pendulum_data(T)
            pair = ac.merwe_pair(nx, 1.0, 0.0, 1.0)
            plain, noisy = _capi.model_compile(UM.PENDULUM_SRC, 2, 1), _capi.model_compile(ac.NOISY_PENDULUM_SRC, 2, 1)
            banks = {"ukf": _capi.UkfBankHandle(0, [kg.with_id(m, plain) for m in models], pair[0]),
                     "aukf": _capi.AukfBankHandle(0, [kg.with_id(m, noisy) for m in models], pair)}
            t_index0 = 0.0
        ts, ll = timed(banks, U, Y, a.reps, t_index0)
        assert np.all(np.isfinite(ll["aukf"])) and np.all(np.isfinite(ll["ukf"]))
        ms = {k: 1e3 * float(np.median(v[1:])) * 1000.0 / T for k, v in ts.items()}
        print(json.dumps(dict(bench="aukf", model=which, nx=nx, ny=ny, F=F, T=T, ukf_ms_per_1000_steps=ms["ukf"],
                              aukf_ms_per_1000_steps=ms["aukf"], ratio=ms["aukf"] / ms["ukf"],
                              ll_max_rel_diff=float(np.max(np.abs(ll["aukf"] - ll["ukf"]) / np.abs(ll["ukf"]))),
                              aukf_spread_ms=[1e3 * min(ts["aukf"][1:]) * 1000.0 / T, 1e3 * max(ts["aukf"][1:]) * 1000.0 / T])), flush=True)
        for b in banks.values():
            b.close()


if __name__ == "__main__":
    main()
