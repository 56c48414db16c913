"""RunForm::lean_run without a device (csrc/host/run_plan.hpp): a run at resample_threshold 1 whose fused launches store neither weights
nor ancestors, which resamples systematically and wants no weighted means, takes the kernel with those facts compiled in.  The
stand-alone program tests/run_plan_lean_host.cpp, built by a host compiler alone with the address and undefined-behaviour sanitizers,
checks the rule over the product of strategy, xmean, threshold, tiles, model, LLPF_SKIP_ANC and LLPF_LEAN, that RunForm stays 17 ints, and
that two plans which differ only in the field are different graph keys; it prints one line per check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "run_plan_lean_host.cpp")


def test_lean_run_without_a_device(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "run_plan_lean_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LLPF_")}      # the program sets the switch it checks itself
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failed", r.stdout
    assert len([ln for ln in lines if ln.startswith("ok  ")]) == 28 and not [ln for ln in lines if ln.startswith("FAIL")]
