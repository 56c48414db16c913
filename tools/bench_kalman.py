"""Throughput of a bank of Kalman filters (llpf_kalman_bank_run): filter-steps per second for F in {1e3, 1e4, 1e5}, T = 1000 and
(nx, ny) in {(2, 1), (4, 2), (8, 4)}, with ll_total only and with every per-step output, against the single-thread host build of the same
header (tests/kalman_host.c).  End-to-end wall time of the call (median of --reps after one warm-up); the kernel's own time comes from a
`rocprofv3 --kernel-trace --stats` run of this script.  Runs whose outputs would exceed --max-out-gb of host memory are skipped.
Prints one JSON line per configuration.

--smooth: the same for llpf_kalman_bank_smooth (forward pass plus the RTS smoother's backward pass) at (nx, ny) in {(4, 2), (8, 4)} by
default, in two forms: ll + xT, and xT + RT; the host baseline is one thread running the header's forward step with the posterior stored
and its backward step (tests/kalman_host.c)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from llpf_amd import _capi  # noqa: E402
import kalman_common as kc  # noqa: E402
import kalman_smooth_common as ks  # noqa: E402

OUTS = _capi.KALMAN_OUTPUTS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", default="1000,10000,100000")
    ap.add_argument("--shapes", default="2x1,4x2,8x4")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--nu", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--max-out-gb", type=float, default=6.0)
    ap.add_argument("--host-filters", type=int, default=200)
    ap.add_argument("--smooth", action="store_true", help="measure llpf_kalman_bank_smooth (default shapes 4x2,8x4)")
    a = ap.parse_args()
    if a.smooth:
        return smooth_main(a)
    host = kc.build_host(tempfile.mkdtemp())
    rng = np.random.default_rng(0)
    T = a.T
    for shape in a.shapes.split(","):
        nx, ny = (int(v) for v in shape.split("x"))
        base = [kc.random_system(rng, nx, ny, a.nu, k % 3) for k in range(256)]
        U = rng.standard_normal((T, a.nu))
        Y = rng.standard_normal((T, ny))
        t0 = time.perf_counter()
        kc.host_run(host, base[: a.host_filters], U, Y, T)
        host_rate = a.host_filters * T / (time.perf_counter() - t0)      # (outputs included: the host loop writes them either way)
        for F in (int(v) for v in a.F.split(",")):
            systems = [base[k % len(base)] for k in range(F)]
            b = _capi.KalmanBankHandle(0, [m for m, _ in systems], np.stack([D for _, D in systems]))
            per_step = 1 + 2 * nx + 2 * nx * nx + ny
            for outputs in ((), OUTS):
                gb = F * T * per_step * 8 / 2**30 if outputs else 0.0
                rec = dict(bench="kalman", nx=nx, ny=ny, nu=a.nu, F=F, T=T, outputs="all" if outputs else "ll", host_steps_per_s=host_rate)
                if gb > a.max_out_gb:
                    rec["skipped"] = "outputs of %.1f GB" % gb
                    print(json.dumps(rec), flush=True)
                    continue
                ts = []
                for r in range(a.reps + 1):
                    b.reset()
                    t1 = time.perf_counter()
                    res = b.run(U, Y, outputs=outputs)
                    ts.append(time.perf_counter() - t1)
                    assert np.all(np.isfinite(res["ll"]))
                    del res
                wall = float(np.median(ts[1:]))
                rec.update(wall_s=wall, steps_per_s=F * T / wall, speedup_vs_host=F * T / wall / host_rate)
                print(json.dumps(rec), flush=True)
            b.close()


def smooth_main(a):
    host = kc.build_host(tempfile.mkdtemp())
    hsm = ks.build_host_smooth(tempfile.mkdtemp())
    rng = np.random.default_rng(0)
    T = a.T
    shapes = "4x2,8x4" if a.shapes == "2x1,4x2,8x4" else a.shapes
    for shape in shapes.split(","):
        nx, ny = (int(v) for v in shape.split("x"))
        base = [kc.random_system(rng, nx, ny, a.nu, k % 3) for k in range(256)]
        U = rng.standard_normal((T, a.nu))
        Y = rng.standard_normal((T, ny))
        hb = base[: a.host_filters]
        t0 = time.perf_counter()
        fw, _ = kc.host_run(host, hb, U, Y, T)
        ks.host_smooth(hsm, hb, U, fw, T)
        host_rate = len(hb) * T / (time.perf_counter() - t0)     # forward + backward, every output written
        del fw
        for F in (int(v) for v in a.F.split(",")):
            systems = [base[k % len(base)] for k in range(F)]
            b = _capi.KalmanBankHandle(0, [m for m, _ in systems], np.stack([D for _, D in systems]))
            for form, outputs in (("ll+xT", ("xT",)), ("xT+RT", ("xT", "RT"))):
                per_step = nx + (nx * nx if "RT" in outputs else 0)
                gb = F * T * per_step * 8 / 2**30
                rec = dict(bench="kalman_smooth", nx=nx, ny=ny, nu=a.nu, F=F, T=T, outputs=form, host_steps_per_s=host_rate,
                           posterior_gb=F * T * (nx + nx * (nx + 1) // 2) * 8 / 2**30)
                if gb > a.max_out_gb:
                    rec["skipped"] = "outputs of %.1f GB" % gb
                    print(json.dumps(rec), flush=True)
                    continue
                ts = []
                for r in range(a.reps + 1):
                    b.reset()
                    t1 = time.perf_counter()
                    res = b.smooth(U, Y, outputs=outputs)
                    ts.append(time.perf_counter() - t1)
                    assert np.all(np.isfinite(res["ll"])) and np.all(np.isfinite(res["xT"][:, :: max(1, F // 64)]))
                    del res
                wall = float(np.median(ts[1:]))
                rec.update(wall_s=wall, steps_per_s=F * T / wall, speedup_vs_host=F * T / wall / host_rate)
                print(json.dumps(rec), flush=True)
            b.close()


if __name__ == "__main__":
    main()
