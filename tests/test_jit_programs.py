"""The run-time compile paths of the engine without a device: every program the library builds with hiprtc — a model's step kernels
(llpf_model_compile), a k_rbfull shape, a model's k_simulate, k_ukf, k_ukf_smooth, k_ekf and the iterated k_ekf — goes through one
compile function (csrc/kernels/jit.hpp: jit_program_compile), and hiprtc cross-compiles for gfx950 when no device is visible.  The
stand-alone program tests/jit_programs_host.cpp links libllpf_hip.so, calls each path, calls it again (the cached entry), asks for
precompiled shapes (nothing to compile), for an id nobody compiled and for a model k_ekf cannot be compiled for (each with its own
message), and prints one line per check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd")
SRC = os.path.join(ROOT, "tests", "jit_programs_host.cpp")


def test_every_compile_path_without_a_device(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    if not os.path.exists(os.path.join(PKG, "libllpf_hip.so")):
        pytest.skip("libllpf_hip.so not built")
    exe = str(tmp_path / "jit_programs_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), SRC, "-L", PKG, "-lllpf_hip", "-Wl,-rpath," + PKG, "-o", exe],
                   check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failed", r.stdout
    assert len([ln for ln in lines if ln.startswith("ok  ")]) == 26 and not [ln for ln in lines if ln.startswith("FAIL")]
