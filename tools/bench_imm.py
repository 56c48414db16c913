"""The price of the interaction: a bank of F IMM filters of M modes (llpf_imm_bank_run) beside a bank of F * M Kalman filters
(llpf_kalman_bank_run) — the same correct! / predict! work without the exchange between the lanes of a filter — in one process,
alternating, for F = 10^4, M in {2, 3, 4}, (nx, ny) in {(2, 1), (4, 2)}, T = 1000, ll_total only, shared U / Y.

Without arguments: the end-to-end wall time of the two calls (median of --reps after one warm-up each), one JSON line per configuration.
The kernels' own time comes from a run of this script under `rocprofv3 --kernel-trace --output-format csv`, in a run of its own:
`--trace <kernel_trace.csv>` reads that file, assigns its launches to the runs in the order this script makes them (the k_imm of M = 3 and
of M = 4 is the same kernel, G = 4: only the order tells them apart; give the --shapes, --modes, --T and --reps of the traced run) and
prints per configuration the median kernel time of an IMM run, of the Kalman run and their ratio.

--extended: the same question for extended modes.  F quad-tank IMMs of M modes (the built-in model, modes that differ in gamma1 and a1;
k_imm_ekf through llpf_imm_bank_run_at) beside an ExtendedKalmanFilterBank's handle of F * M filters over the same descriptors (k_ekf), in
the same process, alternating; (nx, ny) = (4, 2) and nu = 2 are the model's, --shapes and --nu are ignored.  --trace reads k_imm_ekf and
k_ekf in the place of k_imm and k_kalman.

--unscented: the same for unscented modes.  The same quad-tank IMMs over unscented Kalman filter modes (k_imm_ukf through an
llpf_imm_bank_create_unscented bank, Merwe (1, 0, 1) weights) beside an UnscentedKalmanFilterBank's handle of F * M filters over the same
descriptors and weights (k_ukf), in the same process, alternating.  --trace reads k_imm_ukf and k_ukf."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CHUNK = 256      # host/pipe.hpp: CHUNK_STEPS (shared inputs, no per-step output: a chunk is 256 steps)


def configs(a):
    if a.extended or a.unscented:
        for M in (int(v) for v in a.modes.split(",")):
            yield 4, 2, M
        return
    for shape in a.shapes.split(","):
        nx, ny = (int(v) for v in shape.split("x"))
        for M in (int(v) for v in a.modes.split(",")):
            yield nx, ny, M


def measure(a):
    from llpf_amd import _capi
    import imm_common as ic
    rng = np.random.default_rng(0)
    T, F = a.T, a.F
    for nx, ny, M in configs(a):
        base = [ic.random_imm(rng, M, nx, ny, a.nu, k % 3) for k in range(64)]
        imms = [base[k % len(base)] for k in range(F)]
        U = rng.standard_normal((T, a.nu))
        Y = rng.standard_normal((T, ny))
        bi = ic.bank(imms)
        bk = _capi.KalmanBankHandle(0, [m for imm in imms for m in imm["models"]], np.stack([D for imm in imms for D in imm["D"]]))
        ti, tk = [], []
        for r in range(a.reps + 1):
            for b, ts in ((bi, ti), (bk, tk)):
                b.reset()
                t1 = time.perf_counter()
                res = b.run(U, Y)
                ts.append(time.perf_counter() - t1)
                assert np.all(np.isfinite(res["ll"]))
        wi, wk = float(np.median(ti[1:])), float(np.median(tk[1:]))
        print(json.dumps(dict(bench="imm", nx=nx, ny=ny, nu=a.nu, M=M, F=F, T=T, imm_wall_s=wi, kalman_wall_s=wk, kalman_filters=F * M,
                              wall_ratio=wi / wk, imm_steps_per_s=F * T / wi)), flush=True)
        bi.close()
        bk.close()


def measure_model_driven(a):
    """--extended or --unscented: the quad-tank IMMs beside the bank of F * M single filters of the same kind"""
    from llpf_amd import _capi, _structs as S
    import imm_common as ic
    import models as Mo
    tag = "ukf" if a.unscented else "ekf"
    if a.unscented:
        import imm_ukf_common as iu
        import ukf_common as uc
        w = uc.merwe(4, 1.0, 0.0, 1.0)
    rng = np.random.default_rng(0)
    T, F = a.T, a.F
    base = Mo.quadtank_model()
    U, Y = Mo.quadtank_data(T)
    for nx, ny, M in configs(a):
        modes = [S.make_quadtank_model(base.dynamics_density, base.measurement_density, base.initial_density, 1.0, 2,
                                       gamma1=0.2 + 0.001 * (k % 50) + 0.05 * (k % M), a1=0.03 + 0.0001 * (k % 7) + 0.003 * (k % M)) for k in range(F * M)]
        imms = ic.grouped(modes, rng, F, M)
        bi = iu.bank(imms, w) if a.unscented else ic.bank(imms)
        be = _capi.UkfBankHandle(0, modes, w) if a.unscented else _capi.EkfBankHandle(0, modes)
        ti, te = [], []
        for r in range(a.reps + 1):
            for b, ts in ((bi, ti), (be, te)):
                b.reset()
                t1 = time.perf_counter()
                res = b.run(U, Y, t_index0=1.0)
                ts.append(time.perf_counter() - t1)
                assert np.all(np.isfinite(res["ll"]))
        wi, we = float(np.median(ti[1:])), float(np.median(te[1:]))
        print(json.dumps({"bench": "imm_unscented" if a.unscented else "imm_extended", "model": "quadtank", "nx": nx, "ny": ny, "M": M, "F": F, "T": T,
                          "imm_wall_s": wi, tag + "_wall_s": we, tag + "_filters": F * M, "wall_ratio": wi / we, "imm_steps_per_s": F * T / wi}),
              flush=True)
        bi.close()
        be.close()


def from_trace(a):
    rows = list(csv.DictReader(open(a.trace, newline="")))
    key = {k.lower(): k for k in rows[0]}
    name, t0, t1 = key["kernel_name"], key["start_timestamp"], key["end_timestamp"]
    kerns = ("k_imm_ukf", "k_ukf") if a.unscented else ("k_imm_ekf", "k_ekf") if a.extended else ("k_imm", "k_kalman")
    single = kerns[1][2:]
    mine = lambda kern, r: kern + "<" in r[name] or kern + "I" in r[name]
    rows = sorted((r for r in rows if mine(kerns[0], r) or mine(kerns[1], r)), key=lambda r: int(r[t0]))
    n = (a.T + CHUNK - 1) // CHUNK
    it = iter(rows)
    for nx, ny, M in configs(a):
        sums = {kerns[0]: [], kerns[1]: []}
        for r in range(a.reps + 1):
            for kern in kerns:
                launches = [next(it) for _ in range(n)]
                assert all(mine(kern, l) for l in launches), (nx, ny, M, r, kern, launches[0][name])
                sums[kern].append(sum(int(l[t1]) - int(l[t0]) for l in launches) * 1e-6)
        ki, kk = float(np.median(sums[kerns[0]][1:])), float(np.median(sums[kerns[1]][1:]))
        print(json.dumps({"bench": "imm_unscented_kernels" if a.unscented else "imm_extended_kernels" if a.extended else "imm_kernels", "nx": nx,
                          "ny": ny, "M": M, "F": a.F, "T": a.T, kerns[0] + "_ms": ki, kerns[1] + "_ms": kk, single + "_filters": a.F * M, "ratio": ki / kk,
                          kerns[0] + "_spread_ms": [min(sums[kerns[0]][1:]), max(sums[kerns[0]][1:])],
                          kerns[1] + "_spread_ms": [min(sums[kerns[1]][1:]), max(sums[kerns[1]][1:])]}), flush=True)
    assert next(it, None) is None, "launches left over: the trace is not of a run with these arguments"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--F", type=int, default=10000)
    ap.add_argument("--shapes", default="2x1,4x2")
    ap.add_argument("--modes", default="2,3,4")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--nu", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--extended", action="store_true", help="quad-tank IMMs over extended Kalman filter modes beside an extended Kalman bank")
    ap.add_argument("--unscented", action="store_true", help="quad-tank IMMs over unscented Kalman filter modes beside an unscented Kalman bank")
    ap.add_argument("--trace", help="the kernel trace (csv) of a run of this script under rocprofv3 with the same arguments")
    a = ap.parse_args()
    if a.extended and a.unscented:
        ap.error("--extended and --unscented are two runs")
    return from_trace(a) if a.trace else measure_model_driven(a) if a.extended or a.unscented else measure(a)


if __name__ == "__main__":
    main()
