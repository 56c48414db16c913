"""include/llpf.h: "no C++ exception crosses the ABI".  Every export of libllpf_hip.so is a function-try-block whose handler
turns std::bad_alloc into LLPF_ERR_ALLOC and anything else into LLPF_ERR_INTERNAL (csrc/capi.hip: LLPF_TRY / LLPF_GUARD); the
host threads of a multi-GPU bank catch inside the thread.  The reference's analogue: a throw inside the likelihood becomes
-Inf, never a dead session (src/smoothing.jl:275-279).

Faults are injected with LLPF_TEST_THROW="<alloc|error|other>:<site>" (capi.hip: test_throw)."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

from llpf_amd import _capi, _structs as S
from gpu_common import _Inject
import models as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPI = os.path.join(ROOT, "lowlevelparticlefilters.jl_amd", "csrc", "capi.hip")


def _declared():
    txt = open(os.path.join(ROOT, "include", "llpf.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(llpf_[a-z0-9_]+)\s*\(", txt)))


def test_every_export_is_guarded():
    src = open(CAPI).read()
    guarded = re.findall(r"LLPF_GUARD\((llpf_[a-z0-9_]+)\)", src)
    assert len(guarded) == len(set(guarded))
    # llpf_last_error returns the message itself (a c_str() of a thread-local: cannot throw) and is the one export without a status
    assert sorted(guarded + ["llpf_last_error"]) == _declared()
    # each guard closes a function-try-block of the export it names
    for name in guarded:
        assert re.search(r"^int %s\([^;{]*\)\s*LLPF_TRY\s*\{" % name, src, flags=re.M | re.S), name
    # no thread body without a handler of its own
    mb = open(os.path.join(os.path.dirname(CAPI), "host", "mbank.hpp")).read()
    assert mb.count("emplace_back([&") == 1 and "noexcept {" in mb and 'guard_catch("shard worker")' in mb


def _struct_span(src, name):
    m = re.search(r"\bstruct %s\b[^;{]*\{" % name, src)
    assert m, name
    depth, i = 1, m.end()
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    return m.start(), i


def test_device_resources_are_owned():
    # device buffers, captured graphs and handles are owned by types (host/bank.hpp: DevBuf, GraphExec; std::unique_ptr for the
    # handles): no hand-written cleanup that an early return or a throw can skip
    d = os.path.dirname(CAPI)
    srcs = {os.path.relpath(p, d): re.sub(r"//[^\n]*", "", open(p).read()) for p in [CAPI] + sorted(glob.glob(os.path.join(d, "host", "*.hpp")))}
    bank = srcs["host/bank.hpp"]
    for owner in ("DevBuf", "GraphExec"):
        a, b = _struct_span(bank, owner)
        assert "hip" in bank[a:b]
        bank = bank[:a] + bank[b:]
    srcs["host/bank.hpp"] = bank
    for name, src in srcs.items():
        for word in ("hipMalloc(", "hipFree(", "hipGraphExecDestroy(", "free_bank", "mbank_free"):
            assert word not in src, (name, word)
        for line in src.splitlines():
            if "new (std::nothrow)" in line:
                assert re.search(r"std::unique_ptr<\w+> \w+\(new \(std::nothrow\)|\w+\.reset\(new \(std::nothrow\)", line), (name, line)
    a, b = _struct_span(bank, "Bank")
    assert not re.search(r"\bcap(_\w+|[A-Z]\w*)\b", bank[a:b])
    # ... and so are the copy stream, the events and the pinned memory of the chunked staging pipeline (host/pipe.hpp: ChunkPipe): outside
    # it nothing creates them; the only other streams are the banks' own (BankStream::stream, created at one site, destroyed by BankStream)
    pipe = srcs["host/pipe.hpp"]
    a, b = _struct_span(pipe, "ChunkPipe")
    assert all(word in pipe[a:b] for word in ("hipHostMalloc(", "hipHostFree(", "hipStreamCreateWithFlags(", "hipEventCreateWithFlags("))
    srcs["host/pipe.hpp"] = pipe[:a] + pipe[b:]
    for name, src in srcs.items():
        for word in ("hipHostMalloc(", "hipHostFree(", "hipEventCreateWithFlags(", "SimPipe"):
            assert word not in src, (name, word)
        for line in src.splitlines():
            if "hipStreamCreateWithFlags(" in line:
                assert name == "host/bank.hpp" and "(&b.stream, hipStreamNonBlocking)" in line, (name, line)
    assert sum(src.count("hipStreamCreateWithFlags(") for src in srcs.values()) == 1      # (open_stream: every kind of bank opens its stream there)


@pytest.mark.parametrize("kind,code,needle", [("alloc", _capi.ERR_ALLOC, b"out of host memory"),
                                              ("error", _capi.ERR_INTERNAL, b"injected at create"),
                                              ("other", _capi.ERR_INTERNAL, b"unknown exception")])
def test_a_throw_in_a_constructor_becomes_a_status(kind, code, needle):
    L = _capi.lib()
    cfg = S.make_config(M.lg_test_model(), 1000)
    h = C.c_void_p()
    with _Inject(kind + ":create"):
        assert L.llpf_create(C.byref(cfg), C.byref(h)) == code
        msg = L.llpf_last_error()
        assert needle in msg and b"llpf_create" in msg
        assert not h.value
        hb = C.c_void_p()
        assert L.llpf_bank_create(C.byref(cfg), None, 4, C.byref(hb)) == code
        assert b"llpf_bank_create" in L.llpf_last_error() and not hb.value
    # and the process, the library and the error slot are alive: the next call behaves as always
    assert L.llpf_reset(None) == _capi.ERR_ARG
    assert b"null handle" in L.llpf_last_error()


@pytest.mark.gpu
def test_a_throw_inside_a_run_leaves_a_usable_handle():
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 12)
    g = _capi.FilterHandle(S.make_config(model, 4096, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 7, 0))
    g.seed(7); g.reset()
    ref = g.run(U, Y, 0.0)["ll"]
    g.reset()
    for kind, code in (("alloc", _capi.ERR_ALLOC), ("error", _capi.ERR_INTERNAL)):
        with _Inject(kind + ":run"):
            with pytest.raises(_capi.LLPFError) as ei:
                g.run(U, Y, 0.0)
            assert ei.value.code == code
    g.seed(7); g.reset()          # (reset! alone keeps drawing fresh noise: the same seed again gives the same run)
    assert g.run(U, Y, 0.0)["ll"] == ref


def _device_free_bytes():
    # hipMemGetInfo of the HIP runtime the library is bound to (the lookup through its handle searches its dependencies)
    free, total = C.c_size_t(), C.c_size_t()
    assert _capi.lib()["hipMemGetInfo"](C.byref(free), C.byref(total)) == 0
    return free.value


@pytest.mark.gpu
def test_a_failed_create_leaks_no_device_memory():
    # a throw right after the pool of a handle is allocated (LLPF_TEST_THROW=alloc:pool): the half-built handle is freed
    L = _capi.lib()
    cfg = S.make_config(M.lg_test_model(), 1 << 24)      # a pool of ~1.3 GB (76 bytes per particle at nx = 2)
    _capi.FilterHandle(cfg).close()                       # (the runtime's own first allocations are not counted)
    free0 = _device_free_bytes()
    with _Inject("alloc:pool"):
        for _ in range(8):
            h = C.c_void_p()
            assert L.llpf_create(C.byref(cfg), C.byref(h)) == _capi.ERR_ALLOC
            assert b"out of host memory" in L.llpf_last_error() and not h.value
            hb = C.c_void_p()
            assert L.llpf_bank_create(C.byref(cfg), None, 1, C.byref(hb)) == _capi.ERR_ALLOC
            assert not hb.value
    assert free0 - _device_free_bytes() < 1 << 30      # less than one pool; sixteen leaked pools would be ~20 GB


@pytest.mark.gpu
def test_a_throw_inside_a_split_schedule_run_leaves_a_usable_handle():
    # N = 2e6 at threshold 0.1: the split schedule with two weight buffers (host/run.hpp).  The first run of its shape is enqueued, and
    # the throw comes after all its steps are (LLPF_TEST_THROW=error:run_loop).  The buffers are back in place there, but the run is still
    # marked as alternating between them (Bank::w_pingpong), and a verb whose fused kernel forms weights (the auxiliary predict!, through
    # BankDev::w_next) would write them to the spare buffer: the run must clear that on every exit.
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 12)
    cfg = S.make_config(model, 2_000_000, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.1, 7, 0)
    g = _capi.FilterHandle(cfg)
    with _Inject("error:run_loop"):
        with pytest.raises(_capi.LLPFError) as ei:
            g.run(U, Y, 0.0)
        assert ei.value.code == _capi.ERR_INTERNAL
    out = []
    for h in (g, _capi.FilterHandle(cfg)):
        h.seed(7); h.reset()
        ll = h.correct(U[0], Y[0], 1.0)
        h.predict(U[0], 1.0)
        single = (h.particles(), h.weights(), h.expweights())
        h.aux_predict(U[1], Y[2], 2.0)
        aux = (h.particles(), h.weights(), h.expweights(), np.array([h.aux_correct()]))
        r = h.run(U[2:], Y[2:], 3.0, ll_steps=True)
        out.append([np.array([ll]), *single, *aux, r["ll_steps"], h.particles(), h.weights(), h.expweights()])
    for a, b in zip(*out):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.gpu
def test_an_absurd_horizon_is_a_status():
    # T = 2^46 timesteps: the staging of the inputs alone is beyond any allocation; must come back as a status
    model = M.lg_test_model()
    g = _capi.FilterHandle(S.make_config(model, 1024, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 7, 0))
    g.reset()
    L = _capi.lib()
    y = np.zeros((4, model.ny))
    u = np.zeros((4, max(model.nu, 1)))
    ll = C.c_double()
    rc = L.llpf_run(g.h, _capi.dptr(u), _capi.dptr(y), C.c_int64(1 << 46), C.c_double(0.0), C.byref(ll), None)
    assert rc == _capi.ERR_ALLOC, rc
    assert L.llpf_last_error()
    # ... and the refused allocation does not poison the handle's next call (the runtime's sticky last-error is cleared)
    _, U, Y = M.simulate_lg(model, 5)
    g.seed(7); g.reset()
    assert np.isfinite(g.run(U, Y, 0.0)["ll"])


@pytest.mark.gpu
@pytest.mark.parametrize("site", ["shard", "thread"])
def test_a_throw_in_a_shard_thread_is_a_status(site):
    # two shards folded onto one GPU: mbank_foreach drives them from two host threads
    model = M.lg_test_model()
    _, U, Y = M.simulate_lg(model, 6)
    cfg = S.make_config(model, 2048, S.PARTICLE_FILTER, S.RESAMPLE_SYSTEMATIC, 0.5, 7, 0)
    mb = _capi.MBankHandle(cfg, None, 4, devices=[0, 0])
    mb.seed(7); mb.reset()
    ref = mb.run(U, Y, 0.0)["ll"]
    for kind, code in (("alloc", _capi.ERR_ALLOC), ("error", _capi.ERR_INTERNAL)):
        with _Inject(kind + ":" + site):
            with pytest.raises(_capi.LLPFError) as ei:
                mb.reset()
            assert ei.value.code == code
    mb.seed(7); mb.reset()
    assert np.array_equal(ref, mb.run(U, Y, 0.0)["ll"])
