"""RunForm::skip_anc_run without a device (csrc/host/run_plan.hpp): a run at resample_threshold 1 whose fused launches store no weights
stores no ancestors between its steps either.  The stand-alone program tests/run_plan_skip_anc_host.cpp, built by a host compiler alone,
checks that the field follows skip_w_run's preconditions, that LLPF_SKIP_ANC=0 clears it, that two plans which differ only in it are
different graph keys, and that the step bookkeeping does not depend on it; it prints one line per check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "run_plan_skip_anc_host.cpp")


def test_skip_anc_run_without_a_device(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "run_plan_skip_anc_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", SRC, "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LLPF_")}      # the program sets the switch it checks itself
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failed", r.stdout
    assert len([ln for ln in lines if ln.startswith("ok  ")]) == 36 and not [ln for ln in lines if ln.startswith("FAIL")]
