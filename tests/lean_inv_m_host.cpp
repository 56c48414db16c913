// The step of the systematic thresholds as a level-3 launch of the fused kernel gets it from the host (csrc/host/run_plan.hpp:
// lean_inv_M -> ResArgs::inv_M), against the oracle's expression for the same number.  No device, no HIP call: a host compiler builds
// this alone (tests/test_lean_inv_m.py).  One line per M: M, the host value's bits, the oracle expression's bits.
#include <inttypes.h>
#include <stdio.h>

#include "../lowlevelparticlefilters.jl_amd/csrc/host/run_plan.hpp"

// oracle/llpf_oracle.c (orc_resample, and the filter's own resampling): `c.step = 1.0 / (double)m;` with an int64_t m — the test holds
// the oracle's source to that text.  volatile: evaluated at run time, by this machine's division, not folded by the compiler.
static double oracle_step(int64_t m_in) {
    volatile int64_t m = m_in;
    return 1.0 / (double)m;
}

static uint64_t bits(double v) { uint64_t u; memcpy(&u, &v, sizeof u); return u; }

int main() {
    const int32_t Ms[] = {1, 3, 1025, 70001, 1000000, (1 << 29) - 1};
    int failed = 0;
    for (int32_t M0 : Ms) {
        volatile int32_t M = M0;
        const uint64_t host = bits(lean_inv_M(M)), orc = bits(oracle_step(M0));
        printf("%s M %" PRId32 " host %016" PRIx64 " oracle %016" PRIx64 "\n", host == orc ? "ok  " : "FAIL", M0, host, orc);
        failed += host != orc;
    }
    printf("%d failed\n", failed);
    return failed ? 1 : 0;
}
