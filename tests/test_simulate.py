"""llpf_simulate / llpf_bank_simulate on a machine without a GPU: declared, exported, bound, guarded, reachable from Julia, and refusing
bad handles with a status (the GPU behaviour is tests/test_gpu_simulate.py)."""
import ctypes as C
import os
import re

import numpy as np

import llpf_amd
from llpf_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("llpf_simulate", "llpf_bank_simulate")


def test_declared_exported_bound_and_guarded():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "llpf.h")).read(), flags=re.S)
    capi = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "capi.hip")).read()
    L = _capi.lib()
    for name in NEW:
        m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, hdr, re.S)
        assert m and len(m.group(1).split(",")) == 11, name
        assert hasattr(L, name) and name in _capi.SYMBOLS and len(_capi.SYMBOLS[name]) == 11
        assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % name, capi, flags=re.M | re.S) and "LLPF_GUARD(%s)" % name in capi
    for flag, bit in (("LLPF_SIM_DYNAMICS_NOISE", 1), ("LLPF_SIM_MEASUREMENT_NOISE", 2), ("LLPF_SIM_SAMPLE_INITIAL", 4)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (flag, bit), hdr)
    assert (_capi.SIM_DYNAMICS_NOISE, _capi.SIM_MEASUREMENT_NOISE, _capi.SIM_SAMPLE_INITIAL) == (1, 2, 4)
    ma, mi = C.c_int32(-1), C.c_int32(-1)
    assert L.llpf_version(C.byref(ma), C.byref(mi)) == 0 and (ma.value, mi.value) == (0, 7)


def test_julia_wrapper_calls_both():
    jl = open(os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "julia", "LLPFAmd.jl")).read()
    for name in NEW:
        assert re.search(r"ccall\(\(:%s, LIB\)" % name, jl), name
    assert re.search(r"^function simulate_batch\(pf::GPF,", jl, re.M) and re.search(r"^function simulate_batch\(b::GPUFilterBank,", jl, re.M)
    assert "simulate_batch" in jl.split("export GPUParticleFilter", 1)[1].split("\n\n", 1)[0]


def test_null_handles_are_a_status_and_nothing_runs_on_the_cpu():
    L = _capi.lib()
    X = np.zeros((4, 8, 2))
    for name in NEW:
        rc = getattr(L, name)(None, 8, 4, None, 0, 0.0, 1, 0, 3, _capi.dptr(X), None)
        assert rc == _capi.ERR_ARG and b"null" in L.llpf_last_error(), name
    assert not X.any()


def test_python_entry_points():
    assert callable(llpf_amd.simulate_batch) and "simulate_batch" in llpf_amd.api.__all__
    assert callable(llpf_amd.FilterBank.simulate) and callable(_capi.FilterHandle.simulate) and callable(_capi.BankHandle.simulate)


def test_host_drawn_inputs_are_those_of_simulate():
    from llpf_amd.api import _sim_inputs
    du = llpf_amd.MvNormal(np.array([0.5, -1.0]), np.array([0.3, 2.0]))
    T, u = _sim_inputs(2, 25, 7, du, False, None)
    rng = np.random.default_rng(0)
    assert T == 25 and np.array_equal(u, np.stack([du.rand(rng) for _ in range(25)]))      # api.simulate's own draw
    T, u = _sim_inputs(2, 40, 5000, du, True, np.random.default_rng(1), lead=(3,))
    assert T == 40 and u.shape == (3, 5000, 40, 2)
    assert np.allclose(u.reshape(-1, 2).mean(0), du.mean, atol=0.05) and np.allclose(u.reshape(-1, 2).var(0), [0.3, 2.0], rtol=0.05)
    T, u = _sim_inputs(0, 9, 4, None, True, None)
    assert T == 9 and u.shape == (4, 9, 0)
    T, u = _sim_inputs(1, np.arange(6.0), 4, None, False, None)
    assert T == 6 and u.shape == (6, 1)
    T, u = _sim_inputs(1, np.zeros((4, 6, 1)), 4, None, True, None)
    assert T == 6 and u.shape == (4, 6, 1)
