/* llpf_aukf.h — the unscented Kalman filter with augmented (non-additive) process noise (the reference's UnscentedKalmanFilter with
 * dynamics(x, u, p, t, w)), in the one operation order that the device bank (kernels/aukf.hpp, one filter per thread) and a host build of
 * this file share.  This header IS the device-order definition: the GPU reproduces a host build of it (-ffp-contract=off) bit for bit.
 * It is the textbook augmented form (Julier & Uhlmann; Wan & van der Merwe) and was not checked against the reference's source: there
 * is none here.
 *
 * Plain C for host and device, over llpf_kalman.h and llpf_ukf.h with their conventions: packed lower triangles, every sum over the
 * points in increasing index in one accumulator, explicit llpf_fma.
 *
 * Model: x' = f(x, u, p, tau, w), w in R^nx, w ~ N(0, R1);  y = g(x, u, p, tau) + e, e ~ N(0, R2) (the measurement noise stays additive).
 * Two sets of four weights: the measurement set (gamma, wm0, wc0, wi) for L = nx, llpf_ukf.h's, and the dynamics set
 * (gamma_a, wm0a, wc0a, wia) for L = 2 nx.
 *   correct!:  llpf_ukf_factor / llpf_ukf_point / llpf_ukf_correct_finish with the measurement set, call for call: on the same prior the
 *              unscented bank's bits.
 *   predict!:  N = 4 nx + 1 points of the augmented (x; 0) with the factor blkdiag(Cf, C1), Cf = chol(R) (llpf_ukf_factor), C1 = chol(R1)
 *              (llpf_aukf_noise_factor, once per filter before the time loop):
 *                  point 0                 X = x                         W = 0
 *                  points 1 .. nx          X = x + gamma_a Cf[:, j]      W = 0              (llpf_ukf_point's arithmetic)
 *                  points nx+1 .. 2nx      X = x                         W = +gamma_a C1[:, j], 0.0 above row j
 *                  points 2nx+1 .. 3nx     X = x - gamma_a Cf[:, j]      W = 0
 *                  points 3nx+1 .. 4nx     X = x                         W = -gamma_a C1[:, j], 0.0 above row j
 *              X'_i = f(X_i, W_i) (the model's dynamics_w);  x = sum wm_i X'_i;  R = sum wc_i (X'_i - x)(X'_i - x)', nothing added.
 *              A model without dynamics_w is additive: X'_i = f(X_i) at the points with W = 0, and X'_i[d] = f(x)[d] + W_i[d] at a noise
 *              point, f(x) the centre's value (llpf_aukf_additive).
 * If Cf or C1 does not exist (a pivot not > 0, or NaN), x and R are NaN from that step on and nothing else is touched.  A missing row
 * is llpf_ukf.h's, and so is the parameter block: R1 packed, then R2 packed (LLPF_UKF_OFF_*).
 *
 * The header does not know the model; the caller evaluates it between the stages:
 *     ok1 = llpf_aukf_noise_factor(nx, P, ps, C1)                                   once
 *     ok = llpf_ukf_factor(nx, R, Cf) & ok1
 *     for i in 0 .. 4 nx:  noise = llpf_aukf_point(nx, gamma_a, x, Cf, C1, i, X, W);  Z[i][:] = f(X, W)
 *     llpf_aukf_predict_finish(nx, wm0a, wc0a, wia, ok, Z, zs, x, R)
 * with Z[(i * nx + d) * zs] as llpf_ukf.h keeps its mapped points. */
#ifndef LLPF_AUKF_H
#define LLPF_AUKF_H

#include "llpf_ukf.h"

#define LLPF_AUKF_NPTS(nx) (4 * (nx) + 1)
#define LLPF_AUKF_Z(i, d) (Z[(int64_t)((i) * dim + (d)) * zs])

/* C1 = the lower Cholesky factor of R1 = P[LLPF_UKF_OFF_R1 ...] (packed); returns 1, or 0 when R1 is not positive definite */
LLPF_HD int llpf_aukf_noise_factor(const int nx, const double* P, const int64_t ps, double* C1) {
    double inv[LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) C1[i] = P[(int64_t)(LLPF_UKF_OFF_R1 + i) * ps];
    return llpf_kf_chol(nx, C1, inv);
}

/* 1 when point i (0 .. 4 nx) is a noise point (nx+1 .. 2nx, 3nx+1 .. 4nx), whose state part is x itself */
LLPF_HD int llpf_aukf_is_noise(const int nx, const int i) { return (i > nx && i <= 2 * nx) || i > 3 * nx; }

/* point i of the augmented set: the state part into X, the noise part into W; returns llpf_aukf_is_noise(nx, i) */
LLPF_HD int llpf_aukf_point(const int nx, const double gamma_a, const double* x, const double* Cf, const double* C1, const int i, double* X,
                            double* W) {
    const int noise = llpf_aukf_is_noise(nx, i);
    if (!noise) {
        /* the state points are llpf_ukf_point's 0, 1 .. nx (+) and nx+1 .. 2nx (-) */
        llpf_ukf_point(nx, gamma_a, x, Cf, i <= nx ? i : i - nx, X);
        LLPF_KF_UNROLL
        for (int d = 0; d < nx; ++d) W[d] = 0.0;
    } else {
        const int j = i <= 2 * nx ? i - nx - 1 : i - 3 * nx - 1;
        const double g = i <= 2 * nx ? gamma_a : -gamma_a;
        LLPF_KF_UNROLL
        for (int d = 0; d < nx; ++d) {
            X[d] = x[d];
            W[d] = d >= j ? g * C1[llpf_kf_idx(d, j)] : 0.0;
        }
    }
    return noise;
}

/* the mapped value of a noise point of an additive model: out[d] = fx[d] + W[d], fx = f(x) of the centre */
LLPF_HD void llpf_aukf_additive(const int nx, const double* fx, const double* W, double* out) {
    LLPF_KF_UNROLL
    for (int d = 0; d < nx; ++d) out[d] = fx[d] + W[d];
}

/* the mean of the npts mapped points into mean [dim]; Z becomes the deviations Z_i - mean (llpf_ukf_center's accumulation rule) */
LLPF_HD void llpf_aukf_center(const int npts, const int dim, const double wm0, const double wi, double* Z, const int64_t zs, double* mean) {
    LLPF_KF_UNROLL
    for (int r = 0; r < dim; ++r) {
        double acc = wm0 * LLPF_AUKF_Z(0, r);
        LLPF_KF_UNROLL
        for (int i = 1; i < npts; ++i) acc = llpf_fma(wi, LLPF_AUKF_Z(i, r), acc);
        mean[r] = acc;
    }
    LLPF_KF_UNROLL
    for (int i = 0; i < npts; ++i) {
        LLPF_KF_UNROLL
        for (int r = 0; r < dim; ++r) LLPF_AUKF_Z(i, r) = LLPF_AUKF_Z(i, r) - mean[r];
    }
}

/* out (packed lower triangle, dim x dim) = sum wc_i Z_i Z_i' over the npts deviations, nothing added (llpf_ukf_cov's accumulation rule) */
LLPF_HD void llpf_aukf_cov(const int npts, const int dim, const double wc0, const double wi, const double* Z, const int64_t zs, double* out) {
    LLPF_KF_UNROLL
    for (int r = 0; r < dim; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = (wc0 * LLPF_AUKF_Z(0, r)) * LLPF_AUKF_Z(0, c);
            LLPF_KF_UNROLL
            for (int i = 1; i < npts; ++i) acc = llpf_fma(wi * LLPF_AUKF_Z(i, r), LLPF_AUKF_Z(i, c), acc);
            out[llpf_kf_idx(r, c)] = acc;
        }
    }
}

/* predict!, after the caller has put X'_i of the 4 nx + 1 points into Z.  ok: llpf_ukf_factor's status & llpf_aukf_noise_factor's. */
LLPF_HD void llpf_aukf_predict_finish(const int nx, const double wm0a, const double wc0a, const double wia, const int ok, double* Z,
                                      const int64_t zs, double* x, double* R) {
    llpf_aukf_center(LLPF_AUKF_NPTS(nx), nx, wm0a, wia, Z, zs, x);
    llpf_aukf_cov(LLPF_AUKF_NPTS(nx), nx, wc0a, wia, Z, zs, R);
    if (!ok) {                              /* R or R1 not positive definite: this filter is NaN from here on */
        LLPF_KF_UNROLL
        for (int r = 0; r < nx; ++r) x[r] = llpf_kf_nan();
        LLPF_KF_UNROLL
        for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = llpf_kf_nan();
    }
}

#undef LLPF_AUKF_Z

#endif /* LLPF_AUKF_H */
