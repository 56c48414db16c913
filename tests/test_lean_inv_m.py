"""1 / M of a level-3 launch of the fused kernel comes from the host (csrc/host/run_plan.hpp: lean_inv_M, passed as ResArgs::inv_M) in
place of a division in every wave.  IEEE division is correctly rounded wherever it is evaluated, so the host's double is the one the
kernel, and the oracle, compute as 1.0 / (double)M: the stand-alone program tests/lean_inv_m_host.cpp (a host compiler alone) prints the
bits of both for M in {1, 3, 1025, 70001, 10^6, 2^29 - 1}, and they are compared here once more against numpy's float64 division."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lean_inv_m_host.cpp")
MS = (1, 3, 1025, 70001, 10 ** 6, 2 ** 29 - 1)


def test_the_host_value_equals_the_oracles_expression_bit_for_bit(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no C++ compiler")
    # the expression the program evaluates as the oracle's is the oracle's
    with open(os.path.join(ROOT, "oracle", "llpf_oracle.c")) as fh:
        assert "c.step = 1.0 / (double)m;" in fh.read(), "the oracle forms the thresholds' step in another way"
    exe = str(tmp_path / "lean_inv_m_host")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "0 failed", r.stdout
    rows = [re.match(r"ok   M (\d+) host ([0-9a-f]{16}) oracle ([0-9a-f]{16})$", ln) for ln in r.stdout.splitlines()[:-1]]
    assert all(rows) and tuple(int(m.group(1)) for m in rows) == MS, r.stdout
    for m in rows:
        M, host, orc = int(m.group(1)), int(m.group(2), 16), int(m.group(3), 16)
        want = int((np.float64(1.0) / np.float64(M)).view(np.uint64))
        assert host == orc == want, "M = %d: host %016x, oracle %016x, numpy %016x" % (M, host, orc, want)
