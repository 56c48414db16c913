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
 * the unscented bank's block.
 *
 * The iterated extended Kalman filter (llpf_iekf_iterate, llpf_iekf_stop) repeats correct! around a moving linearisation point; its
 * definition stands with the functions below. */
#ifndef LLPF_EKF_H
#define LLPF_EKF_H

#include "llpf_kalman.h"

#define LLPF_EKF_OFF_R1 0
#define LLPF_EKF_OFF_R2(nx) LLPF_KF_NP(nx)
#define LLPF_EKF_NPAR(nx, ny) (LLPF_KF_NP(nx) + LLPF_KF_NP(ny))

#define LLPF_EKF_P(e) (P[(int64_t)(e) * ps])

/* a missing measurement row: its first element is NaN */
LLPF_HD int llpf_ekf_missing(const double* y) { return !(y[0] == y[0]); }

/* CR = C R (ny x nx, row stride LLPF_KF_MAXX) and S = (C R) C' + R2 (packed lower triangle, into L) from C = dg/dx (row stride ld) and
 * the prior covariance R: the cross term and the innovation covariance that llpf_kf_gain_update takes */
LLPF_HD void llpf_ekf_innovation_cov(const int nx, const int ny, const double* P, const int64_t ps, const double* C, const int ld,
                                     const double* R, double* CR, double* L) {
    const int oR2 = LLPF_EKF_OFF_R2(nx);
    /* CR = C R  (ny x nx) */
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
}

/* correct! from gx = g(x) and C = dg/dx (ny x nx, row stride ld), both at the prior x: e, x and R updated in place; returns
 * logpdf(N(0, S), e) */
LLPF_HD double llpf_ekf_correct(const int nx, const int ny, const double* P, const int64_t ps, const double* y, const double* gx,
                                const double* C, const int ld, double* x, double* R, double* e) {
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) e[r] = y[r] - gx[r];
    double CR[LLPF_KF_MAXY * LLPF_KF_MAXX], L[LLPF_KF_NP(LLPF_KF_MAXY)];
    llpf_ekf_innovation_cov(nx, ny, P, ps, C, ld, R, CR, L);
    return llpf_kf_gain_update(nx, ny, 1, L, CR, e, x, R);
}

/* ---- the iterated extended Kalman filter ----
 * The textbook iterated EKF (Bell & Cathey 1993, "The iterated Kalman filter update as a Gauss-Newton method"): correct! repeated with
 * the linearisation point moved from the prior mean to the last iterate, which converges to the mode of p(x | y) for the prior
 * N(xb, Rb) — the full Gauss-Newton step, no step length.  predict! is llpf_ekf_predict.  With x_0 = xb, for i = 0, 1, ...:
 *     gx_i = g(x_i), C_i = dg/dx(x_i)                         (ONE evaluation of the model's measurement_jac, by the caller)
 *     r_i  = (y - gx_i) - C_i (xb - x_i)                      (at i = 0 the second term is not formed: r_0 is llpf_ekf_correct's e)
 *     CR = C_i Rb, S = (C_i Rb) C_i' + R2                     (llpf_ekf_innovation_cov: llpf_ekf_correct's arithmetic)
 *     llpf_kf_gain_update on copies of (xb, Rb) with r_i:     x_{i+1} = xb + K r_i,  R_{i+1} = Rb - W'W,  ll_i = logpdf(N(0, S), r_i)
 *     move = max_d |x_{i+1,d} - x_{i,d}|
 * and the iteration stops when i + 1 == maxiters or !(move > epsilon) (llpf_iekf_stop), so a NaN iterate stops at once.  The outputs of
 * the step are those of the last iteration run: xt = x_{i+1}, Rt = R_{i+1}, ll = ll_i, e = r_i — r_i is the innovation of the model
 * linearised at x_i, taken at the prior mean: the quantity whose density ll is.  maxiters = 1 is llpf_ekf_correct, bit for bit.  The
 * NaN rule and the missing-row rule are the EKF's.
 * The choices of ll, e and Rt are this project's; the reference's IteratedExtendedKalmanFilter (its iekf.jl) was not at hand, and this
 * definition is UNVERIFIED against it, as the EKF above is against ekf.jl.
 *
 * llpf_iekf_iterate is one iteration: xb, Rb the prior (not written); xi holds x_i on entry and x_{i+1} on return; Rn receives R_{i+1},
 * e receives r_i, *move the move; first != 0 at i = 0.  The loop around it and around the model is the caller's (kernels/ekf.hpp, a
 * host shim). */
#define LLPF_IEKF_MAXITERS 100

LLPF_HD double llpf_iekf_iterate(const int nx, const int ny, const double* P, const int64_t ps, const double* y, const double* gx,
                                 const double* C, const int ld, const double* xb, const double* Rb, const int first, double* xi,
                                 double* Rn, double* e, double* move) {
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) e[r] = y[r] - gx[r];
    if (!first) {
        LLPF_KF_UNROLL
        for (int r = 0; r < ny; ++r) {
            double acc = C[r * ld] * (xb[0] - xi[0]);
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(C[r * ld + q], xb[q] - xi[q], acc);
            e[r] = e[r] - acc;
        }
    }
    double CR[LLPF_KF_MAXY * LLPF_KF_MAXX], L[LLPF_KF_NP(LLPF_KF_MAXY)];
    llpf_ekf_innovation_cov(nx, ny, P, ps, C, ld, Rb, CR, L);
    double xn[LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int d = 0; d < nx; ++d) xn[d] = xb[d];
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) Rn[i] = Rb[i];
    const double ll = llpf_kf_gain_update(nx, ny, 1, L, CR, e, xn, Rn);
    double m = 0.0;                         /* max |x_{i+1} - x_i|; a NaN difference makes it NaN and keeps it so */
    LLPF_KF_UNROLL
    for (int d = 0; d < nx; ++d) {
        const double a = llpf_fabs(xn[d] - xi[d]);
        m = ((a > m) | (a != a)) ? a : m;
        xi[d] = xn[d];
    }
    *move = m;
    return ll;
}

/* after iteration i (done = i + 1 iterations run): 1 when the step is over */
LLPF_HD int llpf_iekf_stop(const int done, const int maxiters, const double move, const double epsilon) {
    return (done >= maxiters) | !(move > epsilon);
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
