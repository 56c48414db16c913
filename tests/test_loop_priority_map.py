"""The wave priority of a round of the level-3 output loop comes from the rounds the wave still has to do (csrc/shared/llpf_loop_prio.h,
used by kernels/resprop.hpp: LLPF_ROUND_PRIO).  The stand-alone program tests/loop_prio_host.c (a host compiler alone) prints the map for
rounds_left = 0 .. 9; pinned here: map A is min(2, rounds_left - 1), map B min(3, rounds_left - 1), neither below 0, map 0 is 0 throughout.
A wave's last round (rounds_left 1) runs at priority 0 under every map, and priority 3 is reached by map B alone."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHARED = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "shared")
WANT = {
    0: [0, 0, 0, 0, 0, 0, 0, 0, 0, 0],
    1: [0, 0, 1, 2, 2, 2, 2, 2, 2, 2],
    2: [0, 0, 1, 2, 3, 3, 3, 3, 3, 3],
}


def test_both_maps_for_zero_to_nine_rounds_left(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if not cc:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "loop_prio_host")
    subprocess.run([cc, "-O1", "-Wall", "-I", SHARED, os.path.join(ROOT, "tests", "loop_prio_host.c"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    got = {}
    for ln in r.stdout.splitlines():
        head, vals = ln.split(":")
        got[int(head.split()[1])] = [int(v) for v in vals.split()]
    assert got == WANT
    for m, row in WANT.items():
        assert row == [max(0, min((0, 2, 3)[m], r - 1)) for r in range(10)]
