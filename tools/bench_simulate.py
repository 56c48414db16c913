#!/usr/bin/env python3
"""Device simulation (llpf_simulate: M trajectories of the reference's simulate(pf, T, du), src/filtering.jl:457-477) against the host.

Cases: the linear-Gaussian 2 x 2 system of examples/example_lineargaussian.jl (BASELINE C1 model) with X and Y; the quad-tank with Y only;
a user snippet with a process noise of its own (tests/user_models.py MULT_NOISE_BOX_SRC) with X and Y — each M = 10^6, T = 100 by default.
Per case: the end-to-end time of one call into preallocated (touched) host arrays, trajectory-steps per second, the kernel time apart from
the copies (llpf_set_profiling: LLPF_PROF_PROPAGATE), the bytes the kernels store per kernel second against the 8 TB/s HBM peak, the
normals drawn per kernel second (nx + ny per trajectory-step), and the speedup over api.simulate (one trajectory per call, timed on a few
and scaled to M) and over tools/bench_mc.py's numpy simulate_cell (timed at min(M, 10^5) trajectories and scaled to M).

    python tools/bench_simulate.py [--M 1000000] [--T 100] [--repeat 3]      # one JSON line
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK = 8.0e12


def _objects(model):
    """api.py descriptors of an llpf_model (for the host-side api.simulate)"""
    import llpf_amd
    from llpf_amd import _structs as S
    nx, nu, ny = model.nx, model.nu, model.ny
    g = lambda d: llpf_amd.MvNormal(np.array(S.gaussian_mean(d)), S.gaussian_cov_matrix(d))
    return g(model.dynamics_density), g(model.measurement_density), g(model.initial_density)


def run_case(name, model, M, T, U, states, repeat, host_pf=None, host_cell=None):
    from llpf_amd import _capi, _structs as S
    h = _capi.FilterHandle(S.make_config(model, 1024, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 1, 0))
    flags = _capi.SIM_DYNAMICS_NOISE | _capi.SIM_MEASUREMENT_NOISE | _capi.SIM_SAMPLE_INITIAL
    X = np.ones((T, M, model.nx)) if states else None
    Y = np.ones((T, M, model.ny))
    Uc = np.ascontiguousarray(U, dtype=np.float64)
    L = _capi.lib()

    def call(m=M):
        _capi.check(L.llpf_simulate(h.h, m, T, _capi.dptr(Uc), 0, 0.0, 99, 0, flags, _capi.dptr(X), _capi.dptr(Y)))

    call(1024)                                  # code objects loaded (and a user model's k_simulate compiled) before the timing
    walls, kms = [], []
    for _ in range(repeat):
        h.set_profiling(True)
        t0 = time.perf_counter()
        call()
        walls.append(time.perf_counter() - t0)
        ms, n = h.profile()
        kms.append(float(ms[0]))
        h.set_profiling(False)
    wall, kernel_s = min(walls), min(kms) / 1e3
    steps = float(M) * T
    stored = steps * ((model.nx if states else 0) + model.ny) * 8
    out = dict(case=name, M=M, T=T, outputs="X+Y" if states else "Y", wall_s=round(wall, 4), wall_s_all=[round(w, 4) for w in walls],
               traj_steps_per_s=steps / wall, kernel_ms=round(kernel_s * 1e3, 3), copy_and_host_ms=round((wall - kernel_s) * 1e3, 1),
               bytes_stored=int(stored), store_bytes_per_kernel_s=stored / kernel_s, store_frac_of_8TBps=round(stored / kernel_s / HBM_PEAK, 4),
               normals_per_kernel_s=steps * (model.nx + model.ny) / kernel_s, traj_steps_per_kernel_s=steps / kernel_s)
    if host_pf is not None:
        import llpf_amd
        k = 5
        t0 = time.perf_counter()
        for i in range(k):
            llpf_amd.simulate(host_pf, U, sample_initial=True, rng=np.random.default_rng(i))
        per_traj = (time.perf_counter() - t0) / k
        out["api_simulate_s_per_trajectory"] = per_traj
        out["speedup_vs_api_simulate"] = per_traj * M / wall
    if host_cell is not None:
        out.update(host_cell(M, T, wall))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=1_000_000)
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    import llpf_amd
    from llpf_amd import _capi, _structs as S
    import models as MD
    import user_models as UM
    from bench_mc import simulate_cell
    if _capi.device_count() < 1:
        raise SystemExit("bench_simulate needs a GPU")
    M, T = args.M, args.T
    rng = np.random.default_rng(0)
    res = []

    # linear-Gaussian 2 x 2 (nu = 2): the system of bench_mc.py's simulate_cell
    lg = MD.lg_c1_model()
    A = np.array(lg.A[:4]).reshape(2, 2); B = np.array(lg.B[:4]).reshape(2, 2); Cm = np.array(lg.C[:4]).reshape(2, 2)
    df, dg, d0 = _objects(lg)
    pf = llpf_amd.ParticleFilter(1000, llpf_amd.LinearDynamics(A, B), llpf_amd.LinearMeasurement(Cm), df, dg, d0)

    def cell(M, T, wall):
        m = min(M, 100_000)
        t0 = time.perf_counter()
        simulate_cell(A, B, Cm, np.array(S.gaussian_mean(lg.initial_density)), m, T, np.random.default_rng(1))
        s = (time.perf_counter() - t0) * M / m
        return {"bench_mc_simulate_cell_s_scaled": s, "bench_mc_simulate_cell_measured_at_M": m, "speedup_vs_bench_mc_simulate_cell": s / wall}

    res.append(run_case("lg_2x2", lg, M, T, rng.standard_normal((T, 2)), True, args.repeat, host_pf=pf, host_cell=cell))

    # quad-tank, Y only
    qt = MD.quadtank_model()
    dfq, dgq, d0q = _objects(qt)
    pfq = llpf_amd.ParticleFilter(1000, llpf_amd.QuadTankDynamics(supersample=2), llpf_amd.QuadTankMeasurement(), dfq, dgq, d0q)
    Uq = np.full((T, 2), 0.25)
    res.append(run_case("quadtank", qt, M, T, Uq, False, args.repeat, host_pf=pfq))

    # a user snippet with its own process noise (no host version: api.simulate cannot run it)
    m = S.Model.from_buffer_copy(bytes(MD.lg_test_model()))
    m.model_id = _capi.model_compile(UM.MULT_NOISE_BOX_SRC, m.nx, m.ny)
    for i, v in enumerate([0.1, 0.25, -1.0, 0.5, 3.0, 2.5]):
        m.qt[i] = v
    res.append(run_case("user_noise_hook", m, M, T, rng.standard_normal((T, 1)), True, args.repeat))
    print(json.dumps({"bench": "simulate", "cases": res}))


if __name__ == "__main__":
    main()
