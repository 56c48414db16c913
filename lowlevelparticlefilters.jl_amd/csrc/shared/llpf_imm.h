/* llpf_imm.h — the interacting-multiple-model (IMM) filter over Kalman filters with constant matrices or over first-order extended Kalman
 * filters (the reference's IMM(models, P, mu), src/imm.jl), in the one operation order that the device banks (kernels/imm.hpp and
 * kernels/imm_ekf.hpp, one lane per (filter, mode)) and a host build of this file share.  This header IS the device-order definition: the GPU reproduces a host build of it (-ffp-contract=off) bit for bit.
 * The recursion is the textbook one (Blom & Bar-Shalom 1988); it was NOT checked against the reference's source, which was not available
 * when this was written.  No smoother.  The mode's own step is either header's: a Kalman filter of llpf_kalman.h (llpf_kf_correct,
 * llpf_kf_predict), or a first-order extended Kalman filter of llpf_ekf.h (llpf_ekf_correct, llpf_ekf_predict around the model's value
 * and Jacobian) — every mode of an IMM the same kind, and an extended IMM's modes one model type with a descriptor each.  The
 * arithmetic of this file is the same for both: it never looks inside a mode's step.
 *
 * Plain C for host and device, on top of llpf_kalman.h and in its style: explicit llpf_fma, every sum over the mode index in increasing
 * order, llpf_exp / llpf_log of llpf_detmath.h.
 *
 * One IMM: M modes (1 <= M <= LLPF_IMM_MAXM), each with its own A, B, C, D, R1, R2, d0 (nx, ny, nu common), a row-stochastic transition
 * matrix P [M][M] (P_ij: from mode i to mode j), mode probabilities mu [M] and the flag `interact`.  The carried state is the per-mode
 * (x_j, packed R_j), mu and the run's ll_total.  The combined estimate is a pure function of that state:
 *     x = sum_j mu_j x_j,   R = sum_j mu_j (R_j + (x_j - x)(x_j - x)'), lower triangle only.
 *
 * Step t of a run (the frame of llpf_kalman.h's step):
 *   1. the combined prior x[t], R[t] is taken from the state as it stands;
 *   2. every mode runs llpf_kf_correct, giving ll_j;
 *   3. c_j = sum_i P_ij mu_i;  a_j = log c_j + ll_j;  m = max_j a_j;  w_j = exp(a_j - m);  s = sum_j w_j;
 *      ll[t] = m + log s;  mu_j = w_j / s;
 *   4. the combined posterior xt[t], Rt[t] is taken;
 *   5. with `interact`: c_j = sum_i P_ij mu_i (the new mu);  mu_ij = (P_ij mu_i) / c_j;  x_j <- sum_i mu_ij x_i;
 *      R_j <- sum_i mu_ij (R_i + (x_i - x_j)(x_i - x_j)') with the new x_j — every mode from the modes as they were before the mixing;
 *   6. every mode runs llpf_kf_predict.
 * update! is this step; a run's ll_total starts at 0.0 and adds ll[t] in step order.
 * Extended modes: stage 2 is the model's measurement_jac at the mode's prior x_j followed by llpf_ekf_correct; on a missing row
 * (llpf_ekf_missing) the stage is skipped, e is unused and ll_j = 0 — what llpf_kf_correct gives there.  Stage 6 is the model's
 * dynamics_jac at the mode's x_j AFTER the mixing, followed by llpf_ekf_predict.  The model is evaluated at tau = (t_index0 + t) * Ts, as
 * the extended Kalman bank evaluates it.  Stages 1, 3, 4, 5 and every corner rule below are unchanged.
 *
 * Corner rules.
 *   - A missing row (first element NaN): no mode corrects, ll[t] = 0 exactly, mu <- c without normalisation, every ll_j of the step is 0.
 *   - c_j == 0 (a mode without mass): a_j = -inf, w_j = 0 exactly and so mu_j = 0; a term whose weight is exactly 0 enters no sum
 *     (llpf_imm_mean_term, llpf_imm_cov_term return their accumulator), and mode j is not mixed: it keeps its own x_j, R_j.
 *   - A mode whose S loses definiteness has ll_j = NaN: then a_j, s, ll[t] and every mu_j are NaN, and the step sets x_j, R_j of every
 *     mode to NaN (llpf_imm_poison) — the whole IMM is NaN from that step on; a missing row still adds 0 to nothing but NaN.
 *
 * Shape.  A lane of the device holds ONE mode; it cannot loop over arrays of all of them.  The functions here are therefore the scalar
 * steps of the sums over the source mode i; the loop over i and the fetch of mode i's mu_i, a_i, w_i, x_i, R_i belong to the caller (the
 * host twin reads arrays, the kernel reads lane i).  llpf_imm_mean_add / llpf_imm_cov_add are the per-source-mode accumulations over a
 * whole vector / packed triangle, for callers that hold mode i's state in memory. */
#ifndef LLPF_IMM_H
#define LLPF_IMM_H

#include "llpf_kalman.h"

#define LLPF_IMM_MAXM 4

/* c_j = sum_i P_ij mu_i: from acc = 0.0, one call per source mode i in increasing order */
LLPF_HD double llpf_imm_c_add(double Pij, double mu_i, double acc) { return llpf_fma(Pij, mu_i, acc); }

/* a_j = log c_j + ll_j; a mode without mass has -inf (its NaN ll_j still shows) */
LLPF_HD double llpf_imm_loga(double c, double ll) {
    if (c == 0.0) return ll == ll ? -LLPF_INF : ll;
    return llpf_log(c) + ll;
}
/* m = max_i a_i: from m = a_0, one call per further mode (a NaN a_i leaves m; it shows in w_i) */
LLPF_HD double llpf_imm_max(double m, double a) { return a > m ? a : m; }
/* w_j = exp(a_j - m); exactly 0 for a mode without mass (exp of a clamped -inf would be a subnormal) */
LLPF_HD double llpf_imm_w(double c, double a, double m) { return c == 0.0 ? 0.0 : llpf_exp(a - m); }
/* s = sum_i w_i from 0.0 in increasing i (s = s + w_i: an exact 0 changes nothing);  ll = m + log s;  mu_j = w_j / s */
LLPF_HD double llpf_imm_ll(double m, double s) { return m + llpf_log(s); }
/* mu_ij = (P_ij mu_i) / c_j */
LLPF_HD double llpf_imm_mix_w(double Pij, double mu_i, double c) { return (Pij * mu_i) / c; }

/* one term of a weighted mean, acc + w x_i, and of a weighted covariance, acc + w (R_i + d_r d_c) with d = x_i - mean; a weight that
 * is exactly 0 enters no sum */
LLPF_HD double llpf_imm_mean_term(double w, double xi, double acc) { return w == 0.0 ? acc : llpf_fma(w, xi, acc); }
LLPF_HD double llpf_imm_cov_term(double w, double Ri, double dr, double dc, double acc) {
    return w == 0.0 ? acc : llpf_fma(w, llpf_fma(dr, dc, Ri), acc);
}

/* the accumulation steps of source mode i over a whole state: xm += w x_i (xm from zeros), then, with xm complete,
 * Rm += w (R_i + (x_i - xm)(x_i - xm)') on the packed lower triangle (Rm from zeros) */
LLPF_HD void llpf_imm_mean_add(const int nx, double w, const double* xi, double* xm) {
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) xm[r] = llpf_imm_mean_term(w, xi[r], xm[r]);
}
LLPF_HD void llpf_imm_cov_add(const int nx, double w, const double* xi, const double* Ri, const double* xm, double* Rm) {
    double d[LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) d[r] = xi[r] - xm[r];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) Rm[llpf_kf_idx(r, c)] = llpf_imm_cov_term(w, Ri[llpf_kf_idx(r, c)], d[r], d[c], Rm[llpf_kf_idx(r, c)]);
    }
}

/* a step whose ll[t] is NaN: this mode's x_j, R_j are NaN from here on */
LLPF_HD void llpf_imm_poison(const int nx, double ll, double* x, double* R) {
    if (ll == ll) return;
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) x[r] = llpf_kf_nan();
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = llpf_kf_nan();
}

#endif /* LLPF_IMM_H */
