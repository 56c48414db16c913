/* lean_round_host.c — the helpers of the level-3 round (csrc/kernels/resprop.hpp: LLPF_LR_*) against the functions they stand for, bit for bit.
 *   1. llpf_q64_from_fix96(llpf_fix96_unit(e), K) == llpf_q64_unit(e, K) for every exponent field and both signs, mantissa 0, 1, all ones
 *      and random (so NaN, +-Inf, subnormals and e in (1, 2) are among them), K = 0 .. 62; llpf_q64_from_fix96_k33 likewise for K >= 33.
 *   2. llpf_u01_open_s53 / llpf_log_unit_split_s53 against llpf_u01_open / llpf_log_unit_split, and llpf_u01_half_x64 /
 *      llpf_sincos2pi_split_x64 against llpf_u01_half / llpf_sincos2pi_split: the uniforms themselves, and m, dk, f and both table indices,
 *      for the all-zero and all-one words (u = 2^-53 and u = 1 of the open form, 0 and 1 - 2^-53 of the half-open one), the words around
 *      them and 10^6 random words; then the normal pairs of llpf_normal_pair_tab_s against llpf_normal_pair_tab.
 * Prints one line per part and returns the number of parts with a mismatch.
 * Build: cc -O1 -Wall -I <csrc>/shared lean_round_host.c -lm -o lean_round_host   (tests/test_lean_round_host.py) */
#include <stdio.h>
#include <string.h>
#include "llpf_fixed.h"
#include "llpf_philox.h"

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t next64(void) {      /* splitmix64 */
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}
static uint64_t dbits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
static double bitsd(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

static long bad_q = 0, n_q = 0;
static void check_q(uint64_t ebits) {
    const double e = bitsd(ebits);
    const llpf_u128 f = llpf_fix96_unit(e);
    for (int K = 0; K <= 62; ++K) {
        const uint64_t want = llpf_q64_unit(e, K);
        ++n_q;
        if (llpf_q64_from_fix96(f, K) != want || (K >= 33 && llpf_q64_from_fix96_k33(f, K) != want)) {
            if (bad_q++ < 5) printf("quantum: e = %016llx K = %d: %016llx, want %016llx\n", (unsigned long long)ebits, K,
                                    (unsigned long long)llpf_q64_from_fix96(f, K), (unsigned long long)want);
        }
    }
}

static long bad_u = 0, n_u = 0;
static void check_word(uint64_t a) {
    const uint32_t lo = (uint32_t)a, hi = (uint32_t)(a >> 32);
    int bad = 0;
    /* the open uniform and the split of the logarithm */
    const double u1 = llpf_u01_open(lo, hi), us = llpf_u01_open_s53(lo, hi);
    double m0, dk0, m1, dk1;
    const int i0 = llpf_log_unit_split(u1, &m0, &dk0), i1 = llpf_log_unit_split_s53(us, &m1, &dk1);
    bad |= dbits(us * 1.1102230246251565e-16) != dbits(u1);
    bad |= dbits(m0) != dbits(m1) || dbits(dk0) != dbits(dk1) || i0 != i1;
    /* the half-open uniform and the split of the sine and cosine */
    const double u2 = llpf_u01_half(lo, hi), t = llpf_u01_half_x64(lo, hi);
    double f0, f1;
    const int j0 = llpf_sincos2pi_split(u2, &f0), j1 = llpf_sincos2pi_split_x64(t, &f1);
    bad |= dbits(64.0 * u2) != dbits(t);
    bad |= dbits(f0) != dbits(f1) || j0 != j1;
    ++n_u;
    if (bad && bad_u++ < 5) printf("uniforms: word %016llx: u1 %a us %a  m %a %a  dk %g %g  i %d %d | u2 %a t %a  f %a %a  j %d %d\n",
                                   (unsigned long long)a, u1, us, m0, m1, dk0, dk1, i0, i1, u2, t, f0, f1, j0, j1);
}

int main(void) {
    /* 1. quanta */
    for (int sign = 0; sign <= 1; ++sign) {
        for (uint64_t E = 0; E <= 2047; ++E) {
            const uint64_t top = ((uint64_t)sign << 63) | (E << 52);
            check_q(top);
            check_q(top | 1u);
            check_q(top | 0x000fffffffffffffULL);
            check_q(top | 0x0008000000000000ULL);
            for (int r = 0; r < 8; ++r) check_q(top | (next64() >> 12));
        }
    }
    for (int r = 0; r < 20000; ++r) {      /* exp-weights as the kernels form them: (0, 1], and (1, 2) */
        check_q(dbits(bitsd(0x3ff0000000000000ULL | (next64() >> 12)) - 1.0));
        check_q(0x3ff0000000000000ULL | (next64() >> 12));
    }
    check_q(dbits(1.0)); check_q(dbits(0.0)); check_q(dbits(-0.0)); check_q(dbits(2.0));
    printf("quanta: %ld cases, %ld mismatches\n", n_q, bad_q);

    /* 2. uniforms */
    check_word(0); check_word(~(uint64_t)0);
    for (uint64_t d = 1; d <= 4096; d <<= 1) { check_word(d); check_word(d - 1); check_word(~d); check_word(~(d - 1)); }
    for (int s = 11; s < 64; ++s) {        /* every power of two of the 53-bit integer and its neighbours: the big / small mantissa arms, rint's ties */
        const uint64_t p = (uint64_t)1 << s;
        check_word(p); check_word(p - ((uint64_t)1 << 11)); check_word(p + ((uint64_t)1 << 11)); check_word(p | (p >> 1)); check_word((p | (p >> 1)) - ((uint64_t)1 << 11));
    }
    for (int r = 0; r < 1000000; ++r) check_word(next64());
    for (int r = 0; r < 100000; ++r) check_word(next64() >> (r % 53));      /* small integers: large negative dk */
    printf("uniforms: %ld cases, %ld mismatches\n", n_u, bad_u);

    /* the draws themselves, through copies of the tables as a kernel keeps them */
    static double lg[2 * LLPF_RNG_LG_ENTRIES], sc[2 * LLPF_RNG_SC_ENTRIES];
    for (int i = 0; i < LLPF_RNG_LG_ENTRIES; ++i) { lg[2 * i] = LLPF_LOG_INVC[i]; lg[2 * i + 1] = LLPF_LOG_LNC[i]; }
    for (int j = 0; j < LLPF_RNG_SC_ENTRIES; ++j) { sc[2 * j] = LLPF_SIN64[j]; sc[2 * j + 1] = LLPF_COS64[j]; }
    long bad_z = 0, n_z = 0;
    for (int r = 0; r < 200000; ++r) {
        const uint64_t a = next64(), k = next64();
        double x[2], y[2];
        llpf_normals_tab((uint32_t)a, (uint32_t)(a >> 32) & 1023u, LLPF_STREAM_DYNAMICS, (uint32_t)k, (uint32_t)(k >> 32), 2, x, lg, sc);
        llpf_normals_tab_s((uint32_t)a, (uint32_t)(a >> 32) & 1023u, LLPF_STREAM_DYNAMICS, (uint32_t)k, (uint32_t)(k >> 32), 2, y, lg, sc);
        ++n_z;
        if (dbits(x[0]) != dbits(y[0]) || dbits(x[1]) != dbits(y[1])) { if (bad_z++ < 5) printf("normals: idx %u: %a %a, want %a %a\n", (uint32_t)a, y[0], y[1], x[0], x[1]); }
    }
    printf("normals: %ld cases, %ld mismatches\n", n_z, bad_z);
    return (bad_q != 0) + (bad_u != 0) + (bad_z != 0);
}
