/* llpf_enkf.h — the stochastic (perturbed-observation) ensemble Kalman filter with Gaussian R2, in the one operation order that the
 * device bank (kernels/enkf.hpp, one workgroup per ensemble) and a host build of this file share.  This header IS the device-order
 * definition: the GPU reproduces a host build of it (-ffp-contract=off) bit for bit.
 *
 * UNVERIFIED against the reference: its EnsembleKalmanFilter (enkf.jl) was not available when this was written.  Every choice below —
 * the perturbed-observation form, the N - 1 divisor, the sample covariance without inflation of S, multiplicative inflation after
 * predict!, which random stream perturbs the observation — is this project's.
 *
 * Plain C for host and device, with the conventions of llpf_kalman.h, whose pieces it uses (llpf_kf_idx, LLPF_KF_NP, llpf_kf_chol):
 * packed lower triangles, every accumulation over a dimension index in increasing order with explicit llpf_fma.
 *
 * The filter: N members x_i, i = 0 .. N-1, of nx states.
 *   reset!    x_i is the draw reset! gives particle i of a particle filter with the same key (k_init / k_init_user: LLPF_STREAM_INIT,
 *             and LLPF_STREAM_USER_INIT for a model with `initial`, at counter (i, n_reset)).
 *   correct!(u, y, tau)
 *             Y_i = g(x_i);  xbar = sum x_i / N, ybar = sum Y_i / N;  dX_i = x_i - xbar, dY_i = Y_i - ybar;
 *             Pxy = sum dX_i dY_i' / (N - 1);  S = sum dY_i dY_i' / (N - 1) + R2 (lower triangle);  e = y - ybar;
 *             S = L L' (llpf_kf_chol), W = L^-1 Pxy' (ny x nx), z = L^-1 e,
 *             ll = -(ny/2) log 2 pi - log prod L_ii - z'z / 2     (the arithmetic of llpf_kf_gain_update);
 *             for every member v_i = gauss_sample(measurement density, xi_i), xi_i from LLPF_STREAM_MEASURE at (i, step) — the
 *             measurement noise k_simulate gives trajectory i —, d_i = y - (Y_i + v_i), z_i = L^-1 d_i, x_i += W' z_i.
 *             A row of Y whose first element is NaN is missing: correct! is skipped, e is NaN, ll is 0.  S not positive definite (a
 *             pivot not > 0, or NaN): ll is NaN and every member is NaN from that step on; nothing else is touched.
 *   predict!(u, tau)
 *             x_i = f(x_i) + w_i exactly as k_simulate forms it at Philox step `step` (the Gaussian descriptor with LLPF_STREAM_DYNAMICS,
 *             or the model's own noise(x, fx, xi, uu, out) with the uniforms of LLPF_STREAM_USER); then, only when the inflation rho
 *             is not 1: xbar again and x_i = fma(rho, x_i - xbar, xbar).  The step counter grows by one.
 *   state is xbar, covariance the sample covariance sum dX dX' / (N - 1) (lower triangle).  The per-step outputs x, R are mean and
 *   sample covariance of the prior members, xt, Rt those of the updated members.  No output feeds back.
 *
 * THE SUM OVER THE ENSEMBLE is part of the definition (llpf_enkf_sum): LLPF_ENKF_SLOTS = 256 slots, slot s holds
 * 0.0 + v_s + v_{s+256} + ... in increasing i, and the 256 slots are added in a balanced tree of adjacent pairs: (s0 + s1), (s2 + s3),
 * ..., then those pairwise, up to one value.  A product (dX_a dY_b) is formed per member with one multiplication and then added: no fma
 * across members.  This tree is what a butterfly of DPP moves computes inside a wave of 64 lanes, followed by (w0 + w1) + (w2 + w3) over
 * the four waves of a workgroup; it does not depend on the number of filters, on the grid, or on the chunking of T.  If a cheaper tree
 * is found, it changes here and the kernel follows.
 *
 * Parameters of one filter are entries P[e * ps] (host: ps = 1; device: the SoA [entry][F] with ps = F): R1 packed, then R2 packed —
 * the unscented and the extended bank's block; only R2 is read (the process noise is drawn through the model's descriptor). */
#ifndef LLPF_ENKF_H
#define LLPF_ENKF_H

#include "llpf_kalman.h"

#define LLPF_ENKF_SLOTS 256
#define LLPF_ENKF_MAX_MEMBERS 65536
#define LLPF_ENKF_OFF_R2(nx) LLPF_KF_NP(nx)
/* the phases of a step that a launch runs (EnkfArgs::phases) */
#define LLPF_ENKF_CORRECT 1
#define LLPF_ENKF_PREDICT 2

/* the balanced tree over the 256 slots, in place; returns the total */
LLPF_HD double llpf_enkf_tree(double* slot) {
    for (int n = LLPF_ENKF_SLOTS; n > 1; n /= 2)
        for (int j = 0; j < n / 2; ++j) slot[j] = slot[2 * j] + slot[2 * j + 1];
    return slot[0];
}

/* sum of v[i * stride], i = 0 .. n-1: the definition of every sum over the ensemble */
LLPF_HD double llpf_enkf_sum(const double* v, const int64_t n, const int64_t stride) {
    double slot[LLPF_ENKF_SLOTS];
    for (int s = 0; s < LLPF_ENKF_SLOTS; ++s) {
        double acc = 0.0;
        for (int64_t i = s; i < n; i += LLPF_ENKF_SLOTS) acc = acc + v[i * stride];
        slot[s] = acc;
    }
    return llpf_enkf_tree(slot);
}

/* a mean and a second moment from their sums */
LLPF_HD double llpf_enkf_mean(const double sum, const int n) { return sum / (double)n; }
LLPF_HD double llpf_enkf_cov(const double sum, const int n) { return sum / (double)(n - 1); }

/* From the sums of a correct!: sxy[i * LLPF_KF_MAXX + c] = sum dX_c dY_i (ny x nx), syy = sum dY dY' (packed lower triangle), ybar and y:
 *     S = syy / (N - 1) + R2 = L L',  W = L^-1 (sxy / (N - 1)),  e = y - ybar,  z = L^-1 e.
 * Out: the factor L (packed), inv[i] = 1 / L_ii, W (ny x nx, row stride LLPF_KF_MAXX), e, *ok (0: S is not positive definite); returns
 * ll, NaN when !*ok. */
LLPF_HD double llpf_enkf_gain(const int nx, const int ny, const int n, const double* P, const int64_t ps, const double* sxy, const double* syy,
                              const double* y, const double* ybar, double* L, double* inv, double* W, double* e, int* ok) {
    const int oR2 = LLPF_ENKF_OFF_R2(nx);
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(ny); ++i) L[i] = llpf_enkf_cov(syy[i], n) + P[(int64_t)(oR2 + i) * ps];
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) e[r] = y[r] - ybar[r];
    *ok = llpf_kf_chol(ny, L, inv);
    double z[LLPF_KF_MAXY];
    LLPF_KF_UNROLL
    for (int i = 0; i < ny; ++i) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = llpf_enkf_cov(sxy[i * LLPF_KF_MAXX + c], n);
            LLPF_KF_UNROLL
            for (int q = 0; q < i; ++q) acc = llpf_fma(-L[llpf_kf_idx(i, q)], W[q * LLPF_KF_MAXX + c], acc);
            W[i * LLPF_KF_MAXX + c] = acc * inv[i];
        }
        double acc = e[i];
        LLPF_KF_UNROLL
        for (int q = 0; q < i; ++q) acc = llpf_fma(-L[llpf_kf_idx(i, q)], z[q], acc);
        z[i] = acc * inv[i];
    }
    double quad = z[0] * z[0], det = L[0];
    LLPF_KF_UNROLL
    for (int i = 1; i < ny; ++i) {
        quad = llpf_fma(z[i], z[i], quad);
        det = det * L[llpf_kf_idx(i, i)];
    }
    const double c0 = -((double)ny * llpf_log(6.283185307179586)) / 2.0;
    const double ll = (c0 - llpf_log(det)) - 0.5 * quad;
    return *ok ? ll : llpf_kf_nan();
}

/* The update of one member from its Y = g(x) and its measurement noise v:  d = y - (Y + v),  z = L^-1 d,  x += W' z.
 * !ok: the member is NaN. */
LLPF_HD void llpf_enkf_member_update(const int nx, const int ny, const int ok, const double* L, const double* inv, const double* W,
                                     const double* y, const double* Y, const double* v, double* x) {
    double z[LLPF_KF_MAXY];
    LLPF_KF_UNROLL
    for (int i = 0; i < ny; ++i) {
        double acc = y[i] - (Y[i] + v[i]);
        LLPF_KF_UNROLL
        for (int q = 0; q < i; ++q) acc = llpf_fma(-L[llpf_kf_idx(i, q)], z[q], acc);
        z[i] = acc * inv[i];
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double acc = W[r] * z[0];
        LLPF_KF_UNROLL
        for (int i = 1; i < ny; ++i) acc = llpf_fma(W[i * LLPF_KF_MAXX + r], z[i], acc);
        x[r] = ok ? x[r] + acc : llpf_kf_nan();
    }
}

/* multiplicative inflation of one member about the ensemble mean */
LLPF_HD void llpf_enkf_inflate(const int nx, const double rho, const double* xbar, double* x) {
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) x[r] = llpf_fma(rho, x[r] - xbar[r], xbar[r]);
}

#endif /* LLPF_ENKF_H */
