"""Time of a bank of square-root Kalman filters (llpf_sqkf_bank_run) beside the Kalman bank (llpf_kalman_bank_run) in one process on the
same models and data: milliseconds per 1000 steps at F = 10^4 for (nx, ny) in {(2, 1), (4, 2), (8, 4)}, and their ratio.  Timed the way
tools/bench_kalman.py times: the wall time of the call with ll_total only (shared inputs, nothing staged per step: the call is its
kernel launches, one per chunk of 256 steps, and ends in a device synchronise), the median of --reps after one warm-up, the two banks
alternating; the kernels' own times come from a `rocprofv3 --kernel-trace --stats` run of this script (k_sqkf, k_kalman).  Before
timing, the two banks' ll must agree to 1e-9 relative.  Prints one JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llpf_amd import _capi  # noqa: E402
import kalman_common as kc  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", type=int, default=10000)
    ap.add_argument("--shapes", default="2x1,4x2,8x4")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--nu", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    F, T = a.F, a.T
    for shape in a.shapes.split(","):
        nx, ny = (int(v) for v in shape.split("x"))
        base = [kc.random_system(rng, nx, ny, a.nu, k % 3) for k in range(256)]
        systems = [base[k % len(base)] for k in range(F)]
        U = rng.standard_normal((T, a.nu))
        Y = rng.standard_normal((T, ny))
        models, Ds = [m for m, _ in systems], np.stack([D for _, D in systems])
        banks = {"kalman": _capi.KalmanBankHandle(0, models, Ds), "sqkf": _capi.SqkfBankHandle(0, models, Ds)}
        ts = {k: [] for k in banks}
        ll = {}
        for r in range(a.reps + 1):
            for name, b in banks.items():
                b.reset()
                t0 = time.perf_counter()
                ll[name] = b.run(U, Y)["ll"]
                ts[name].append(time.perf_counter() - t0)
        assert np.all(np.isfinite(ll["sqkf"])) and np.all(np.abs(ll["sqkf"] - ll["kalman"]) <= 1e-9 * np.abs(ll["kalman"]))
        ms = {k: 1e3 * float(np.median(v[1:])) * 1000.0 / T for k, v in ts.items()}
        print(json.dumps(dict(bench="sqkf", nx=nx, ny=ny, nu=a.nu, F=F, T=T, kalman_ms_per_1000_steps=ms["kalman"],
                              sqkf_ms_per_1000_steps=ms["sqkf"], ratio=ms["sqkf"] / ms["kalman"],
                              sqkf_spread_ms=[1e3 * min(ts["sqkf"][1:]) * 1000.0 / T, 1e3 * max(ts["sqkf"][1:]) * 1000.0 / T])), flush=True)
        for b in banks.values():
            b.close()


if __name__ == "__main__":
    main()
