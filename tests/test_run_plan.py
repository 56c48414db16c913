"""The form of a run without a device: csrc/host/run_plan.hpp decides, from the facts of a bank, the requested outputs and the
environment, which launches a trajectory loop consists of (fused or balanced, merged or split schedule, lazy quanta, skipped weight
store, source-side dynamics, nontemporal accesses, captured graph), and in which host-side state each timestep runs.  The header makes
no HIP call, so the stand-alone program tests/run_plan_host.cpp is built by a host compiler alone; it checks the plan of every shape at
which a rule changes its answer, every switch both ways, the step bookkeeping of runs of 1 to 9 steps from every entry state, and
that the key of a captured graph tells any two forms apart, and prints one line per check."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "run_plan_host.cpp")


def test_the_form_of_a_run_without_a_device(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "run_plan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", SRC, "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LLPF_")}      # the program sets the switches it checks itself
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == "0 failed", r.stdout
    assert len([ln for ln in lines if ln.startswith("ok  ")]) == 180 and not [ln for ln in lines if ln.startswith("FAIL")]
