/* llpf_ekf.h — the extended Kalman filter with additive noise (the textbook first-order filter, what the reference documents its
 * ExtendedKalmanFilter(dynamics, measurement, R1, R2, d0) to be), in the one operation order that the device bank (kernels/ekf.hpp, one
 * filter per thread) and a host build of this file share.  This header IS the device-order definition: the GPU reproduces a host build of
 * it (-ffp-contract=off) bit for bit.
 *
 * Plain C for host and device, with the conventions of llpf_kalman.h, whose pieces it uses (llpf_kf_idx, LLPF_KF_NP, llpf_kf_gain_update):
 * packed lower triangles, every accumulation over its summation index in increasing order with explicit llpf_fma.
 *
 * Model: x' = f(x, u, p, tau) + w, w ~ N(0, R1);  y = g(x, u, p, tau) + e, e ~ N(0, R2).
 *   correct!:  gx = g(x), C = dg/dx at the prior x;  e = y - gx;  CR = C R;  S = (C R) C' + R2 (lower triangle);  then
 *              llpf_kf_gain_update(nx, ny, 1, L, CR, e, x, R):  S = L L', W = L^-1 CR, z = L^-1 e, x += W' z, R -= W' W,
 *              ll = -(ny/2) log 2 pi - log prod L_ii - z'z / 2
 *   predict!:  fx = f(x), A = df/dx at the posterior x;  x = fx;  R = A R A' + R1 (lower triangle, A R formed one row at a time)
 * The covariance arithmetic is llpf_kf_correct's / llpf_kf_predict's, operation for operation, with C / A read from a local array in the
 * place of the parameter block: on a linear model whose Jacobians are the matrices themselves, R and Rt are the Kalman bank's bits.
 *
 * The header does not know the model: the caller evaluates value and Jacobian (on the device the kernel with Model::measurement_jac /
 * dynamics_jac, on the host a shim with function pointers) and hands over numbers.  A Jacobian is row-major with row stride ld
 * (J[r * ld + c] = d out_r / d x_c); the local matrices of this file have row stride LLPF_KF_MAXX.
 *
 * A filter whose S is not positive definite (a pivot not > 0, or NaN) is NaN from that step on; nothing else is touched.  A row of Y
 * whose first element is NaN is missing: the caller skips correct! (x and R stay, e is NaN, ll is 0) — llpf_ekf_missing.
 *
 * Parameters of one filter are entries P[e * ps] (host: ps = 1; device: the SoA [entry][F] with ps = F): R1 packed, then R2 packed —
 * the unscented bank's block. */
#ifndef LLPF_EKF_H
#define LLPF_EKF_H

#include "llpf_kalman.h"

#define LLPF_EKF_OFF_R1 0
#define LLPF_EKF_OFF_R2(nx) LLPF_KF_NP(nx)
#define LLPF_EKF_NPAR(nx, ny) (LLPF_KF_NP(nx) + LLPF_KF_NP(ny))

#define LLPF_EKF_P(e) (P[(int64_t)(e) * ps])

/* a missing measurement row: its first element is NaN */
LLPF_HD int llpf_ekf_missing(const double* y) { return !(y[0] == y[0]); }

/* correct! from gx = g(x) and C = dg/dx (ny x nx, row stride ld), both at the prior x: e, x and R updated in place; returns
 * logpdf(N(0, S), e) */
LLPF_HD double llpf_ekf_correct(const int nx, const int ny, const double* P, const int64_t ps, const double* y, const double* gx,
                                const double* C, const int ld, double* x, double* R, double* e) {
    const int oR2 = LLPF_EKF_OFF_R2(nx);
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) e[r] = y[r] - gx[r];
    /* CR = C R  (ny x nx) */
    double CR[LLPF_KF_MAXY * LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = C[r * ld] * R[llpf_kf_idx(0, c)];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(C[r * ld + q], R[llpf_kf_idx(q, c)], acc);
            CR[r * LLPF_KF_MAXX + c] = acc;
        }
    }
    /* S = (C R) C' + R2, lower triangle; factored by llpf_kf_gain_update */
    double L[LLPF_KF_NP(LLPF_KF_MAXY)];
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = CR[r * LLPF_KF_MAXX] * C[c * ld];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(CR[r * LLPF_KF_MAXX + q], C[c * ld + q], acc);
            L[llpf_kf_idx(r, c)] = acc + LLPF_EKF_P(oR2 + llpf_kf_idx(r, c));
        }
    }
    return llpf_kf_gain_update(nx, ny, 1, L, CR, e, x, R);
}

/* predict! from fx = f(x) and A = df/dx (nx x nx, row stride ld), both at the posterior x: x = fx, R = A R A' + R1 */
LLPF_HD void llpf_ekf_predict(const int nx, const double* P, const int64_t ps, const double* fx, const double* A, const int ld, double* x,
                              double* R) {
    double Rn[LLPF_KF_NP(LLPF_KF_MAXX)];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double ar[LLPF_KF_MAXX];             /* row r of A R */
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = A[r * ld] * R[llpf_kf_idx(0, c)];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(A[r * ld + q], R[llpf_kf_idx(q, c)], acc);
            ar[c] = acc;
        }
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = ar[0] * A[c * ld];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(ar[q], A[c * ld + q], acc);
            Rn[llpf_kf_idx(r, c)] = acc + LLPF_EKF_P(LLPF_EKF_OFF_R1 + llpf_kf_idx(r, c));
        }
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) x[r] = fx[r];
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = Rn[i];
}
#undef LLPF_EKF_P

#endif /* LLPF_EKF_H */
