#!/usr/bin/env python3
"""The headline workload (bench.py's C2: linear-Gaussian, N = 10^6, T = 1000, resample_threshold 1) with the two things the lean run
form excludes: stratified resampling, or weighted means asked for.  Such runs keep the kernel with the run-time tests and must not get
slower.  Timed as bench.py times its workload; one JSON line.
usage: bench_c2_variants.py {stratified|xmean|plain} [--steps K] [--warmup W] [--particles N] [--T T]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variant", choices=["stratified", "xmean", "plain"])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--T", type=int, default=1000)
    args = ap.parse_args()
    import torch
    import bench
    from llpf_amd import _capi, _structs as S
    model, U, Y, kind, thr, _ = bench.build_workload("lg", args.particles, args.T)
    strategy = S.RESAMPLE_STRATIFIED if args.variant == "stratified" else S.RESAMPLE_SYSTEMATIC
    pf = _capi.FilterHandle(S.make_config(model, args.particles, kind, strategy, thr, 1000, 0))
    xm = args.variant == "xmean"

    def one_pass():
        pf.reset()
        return pf.run(U, Y, 1.0, xmean=xm)["ll"]

    for _ in range(2 + args.warmup):      # two set-up passes: the second captures the run's graph (bench.py does the same)
        one_pass()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dev_ms = 0.0
    for _ in range(args.steps):
        ll = one_pass()
        dev_ms += pf.last_run_ms()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    form = pf.last_run_form() if hasattr(_capi.lib(), "llpf_last_run_form") else {}
    print(json.dumps({"variant": args.variant, "particles": args.particles, "timesteps": args.T, "resample_threshold": thr,
                      "ms_per_step": 1e3 * dt / args.steps, "device_ms_per_step": dev_ms / args.steps, "loglik": ll, "form": form}))


if __name__ == "__main__":
    main()
