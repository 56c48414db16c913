"""Time of a bank of square-root extended Kalman filters (llpf_sqekf_bank_run) beside the extended bank (llpf_ekf_bank_run) in one
process over the same descriptors and data: milliseconds per 1000 steps at F = 10^4 quad-tank filters with per-filter parameters,
T = 1000, and their ratio.  Timed the way tools/bench_sqkf.py times: the wall time of the call with ll_total only (shared inputs, nothing
staged per step: the call is its kernel launches, one per chunk of 256 steps, and ends in a device synchronise), the median of --reps
after one warm-up, the two banks alternating; the kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script
(k_sqekf, k_ekf).  Before timing, the two banks' ll must agree to 1e-9 relative.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llpf_amd import _capi  # noqa: E402
import kf_gpu_frame as kg  # noqa: E402
import models as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", type=int, default=10000)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    F, T = a.F, a.T
    models = kg.quadtank_models(F)
    U, Y = M.quadtank_data(T)
    banks = {"ekf": _capi.EkfBankHandle(0, models), "sqekf": _capi.SqekfBankHandle(0, models)}
    ts = {k: [] for k in banks}
    ll = {}
    for r in range(a.reps + 1):
        for name, b in banks.items():
            b.reset()
            t0 = time.perf_counter()
            ll[name] = b.run(U, Y, t_index0=1.0)["ll"]
            ts[name].append(time.perf_counter() - t0)
    assert np.all(np.isfinite(ll["sqekf"])) and np.all(np.abs(ll["sqekf"] - ll["ekf"]) <= 1e-9 * np.abs(ll["ekf"]))
    ms = {k: 1e3 * float(np.median(v[1:])) * 1000.0 / T for k, v in ts.items()}
    print(json.dumps(dict(bench="sqekf", model="quadtank", nx=4, ny=2, F=F, T=T, ekf_ms_per_1000_steps=ms["ekf"],
                          sqekf_ms_per_1000_steps=ms["sqekf"], ratio=ms["sqekf"] / ms["ekf"],
                          sqekf_spread_ms=[1e3 * min(ts["sqekf"][1:]) * 1000.0 / T, 1e3 * max(ts["sqekf"][1:]) * 1000.0 / T])), flush=True)
    for b in banks.values():
        b.close()


if __name__ == "__main__":
    main()
