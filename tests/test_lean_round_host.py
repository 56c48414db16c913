"""The helpers a round of the level-3 output loop is written in (csrc/kernels/resprop.hpp: LLPF_LR_*) are new functions beside the ones the
oracle and every other kernel keep: llpf_q64_from_fix96 (csrc/shared/llpf_fixed.h) takes the quantum out of the fixed-point exp-weight, and
llpf_u01_open_s53 / llpf_u01_half_x64 with llpf_log_unit_split_s53 / llpf_sincos2pi_split_x64 (llpf_philox.h, llpf_rngmath.h) fold the
uniforms' power-of-two scalings.  The stand-alone program tests/lean_round_host.c (a host compiler alone) holds each against the function
it stands for, bit for bit: every exponent field, both signs, edge and random mantissas and K = 0 .. 62 for the quanta; the all-zero and
all-one words, the words around every power of two and 10^6 random words for the uniforms and what the log and sincos splits make of
them; and the normal draws through both.  It returns the number of parts with a mismatch; the counts it prints are pinned from below."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "shared")
AT_LEAST = {"quanta": 2047 * 2 * 12 * 63, "uniforms": 1000000, "normals": 200000}


def test_helpers_equal_the_functions_they_stand_for(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if not cc:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "lean_round_host")
    # (-ffp-contract=off: the shared math is the IEEE sequence as written, as in every build of it)
    subprocess.run([cc, "-O1", "-Wall", "-ffp-contract=off", "-I", SHARED, os.path.join(ROOT, "tests", "lean_round_host.c"), "-lm", "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    got = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"^(\w+): (\d+) cases, (\d+) mismatches$", r.stdout, re.M)}
    assert set(got) == set(AT_LEAST), r.stdout
    for part, (cases, bad) in got.items():
        assert bad == 0 and cases >= AT_LEAST[part], "%s: %d cases, %d mismatches" % (part, cases, bad)
