"""The form of a run without a device: csrc/host/run_plan.hpp decides, from the facts of a bank, the requested outputs and the
environment, which launches a trajectory loop consists of (fused or balanced, merged or split schedule, lazy quanta, what a run at
resample_threshold 1 leaves out — its level —, source-side dynamics, nontemporal accesses, captured graph), and in which host-side state
each timestep runs.  The header makes no HIP call, so the stand-alone program tests/run_plan_host.cpp is built by a host compiler alone,
with the address and undefined-behaviour sanitizers; it checks the plan of every shape at which a rule changes its answer, every switch
both ways, the level over the products of the facts and switches it depends on, the level of every launch of a run, the step
bookkeeping of runs of 1 to 9 steps from every entry state, and that the key of a captured graph tells any two forms apart, and prints
one line per check, in two sections: one test here for each."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "run_plan_host.cpp")
FORM_CHECKS, LEVEL_CHECKS = 190, 48      # the ok lines of the program's two sections


@pytest.fixture(scope="module")
def sections(tmp_path_factory):
    """the program built and run once: its exit status, its whole output and the check lines of each section"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path_factory.mktemp("run_plan") / "run_plan_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("LLPF_")}      # the program sets the switches it checks itself
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
    print(r.stdout)
    out, cur = {}, None
    for ln in r.stdout.splitlines():
        if ln.startswith("# "):
            cur = out.setdefault(ln[2:], [])
        elif cur is not None and ln[:4] in ("ok  ", "FAIL"):
            cur.append(ln)
    return r.returncode, r.stdout, out


def _assert_section(sections, name, count):
    rc, stdout, out = sections
    assert rc == 0 and stdout.splitlines()[-1] == "0 failed", stdout
    assert len([ln for ln in out[name] if ln.startswith("ok  ")]) == count and not [ln for ln in out[name] if ln.startswith("FAIL")], stdout


def test_the_form_of_a_run_without_a_device(sections):
    """the plan of every shape at which a rule changes its answer, the step bookkeeping, the graph key"""
    _assert_section(sections, "form", FORM_CHECKS)


def test_the_level_of_a_run_without_a_device(sections):
    """RunForm::level over its preconditions, the three switches and their environment, launch_level over every (level, fast, weight),
    and that the step bookkeeping does not depend on the level: the checks of the former skip_anc and lean programs, and the new ones"""
    _assert_section(sections, "level", LEVEL_CHECKS)
