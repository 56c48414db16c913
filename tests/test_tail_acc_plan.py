"""Which launches of a run at resample_threshold 1 leave no running maximum, without a device: csrc/host/run_plan.hpp plans
RunKey::skip_max where the run's level is 3 and LLPF_SKIP_MAX is not 0, and launch_level(plan, fast, weight, next_weight) then gives
RUN_NO_MAX (4) to the level-3 launches that another launch with a weighting phase follows.  The stand-alone program
tests/tail_acc_host.cpp is built by a host compiler alone, with the address and undefined-behaviour sanitizers; it checks the plan over
every combination of facts and switches the rule depends on, every (level, skip_max, fast, weight, next_weight) of one launch, the
launches of whole runs of 1 to 6 steps, the environment switch, and that the key of a captured graph differs where skip_max does."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tail_acc_host.cpp")
CHECKS = 21     # the ok lines of the program


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("tail_acc") / "tail_acc_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LLPF_")}      # the program sets the switch it checks itself
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    return r.returncode, r.stdout


def test_the_launches_without_a_maximum_without_a_device(program):
    rc, stdout = program
    lines = stdout.splitlines()
    assert rc == 0 and lines[-1] == "0 failed", stdout
    assert len([ln for ln in lines if ln.startswith("ok  ")]) == CHECKS and not [ln for ln in lines if ln.startswith("FAIL")], stdout
