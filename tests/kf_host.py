"""What the Python sides of the host twins share (kalman_common, kalman_smooth_common, ukf_common, ukf_smooth_common, ekf_common,
iekf_common around tests/kalman_host.c, tests/ukf_host.c, tests/ekf_host.c): the one compiler line, the pointer helper, and the arrays
that every twin takes in the layout of tests/kf_host_frame.h."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from llpf_amd import _structs as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "shared")
_dp = C.POINTER(C.c_double)
# the arguments that the model-driven forward entry points have in common, up to the model and from x0 on (ukf_host_run has w between)
MODEL_HEAD = [C.c_int] * 4 + [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(S.Model)]
RUN_TAIL = [_dp] * 4 + [C.c_int64, C.c_int, C.c_double] + [_dp] * 7


def build(outdir, source, signatures):
    """cc -O2 -ffp-contract=off of tests/<source> into outdir; signatures: {entry point: its argtypes} (restype int, or (restype,
    argtypes)).  Returns the loaded library."""
    cc = shutil.which("cc") or shutil.which("gcc")
    so = os.path.join(str(outdir), "lib" + os.path.splitext(source)[0] + ".so")
    subprocess.run([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-I", SHARED, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", source), "-o", so], check=True)
    L = C.CDLL(so)
    for name, sig in signatures.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = sig if isinstance(sig, tuple) else (C.c_int, sig)
    return L


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def inputs(U, nu):
    """U as the twins take it: one zero stands in for the inputs of a model without any"""
    return f64(U) if nu > 0 else np.zeros(1)


def pack_models(models, state=None):
    """R1 [F, nx, nx], R2 [F, ny, ny] of the descriptors and x0 [F, nx], P0 [F, nx, nx]: copies of state = (x0, P0), or the initial
    densities (reset).  The twin overwrites x0, P0 with the final state."""
    R1 = f64(np.stack([S.gaussian_cov_matrix(m.dynamics_density) for m in models]))
    R2 = f64(np.stack([S.gaussian_cov_matrix(m.measurement_density) for m in models]))
    if state is None:
        x0 = f64(np.stack([S.gaussian_mean(m.initial_density) for m in models]))
        P0 = f64(np.stack([S.gaussian_cov_matrix(m.initial_density) for m in models]))
    else:
        x0, P0 = np.array(state[0], dtype=np.float64), np.array(state[1], dtype=np.float64)
    return R1, R2, x0, P0


def outputs(T, F, nx, ny):
    """the outputs of a forward pass in the device's layout, and their pointers in the order of the entry points' last seven arguments"""
    out = dict(ll=np.empty(F), ll_steps=np.empty((T, F)), x=np.empty((T, F, nx)), xt=np.empty((T, F, nx)), R=np.empty((T, F, nx, nx)),
               Rt=np.empty((T, F, nx, nx)), e=np.empty((T, F, ny)))
    return out, [_p(out[k]) for k in ("ll", "ll_steps", "x", "xt", "R", "Rt", "e")]


def smooth_io(fw, T, F, nx):
    """the posterior xt, Rt of the forward outputs fw, the smoother's outputs in the device's layout, and the pointers of all four"""
    xt, Rt = f64(fw["xt"]), f64(fw["Rt"])
    assert xt.shape == (T, F, nx) and Rt.shape == (T, F, nx, nx)
    out = dict(xT=np.empty((T, F, nx)), RT=np.empty((T, F, nx, nx)))
    return out, [_p(xt), _p(Rt), _p(out["xT"]), _p(out["RT"])]
