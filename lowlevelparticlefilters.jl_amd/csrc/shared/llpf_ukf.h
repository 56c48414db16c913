/* llpf_ukf.h — the unscented Kalman filter with additive noise (the reference's UnscentedKalmanFilter(dynamics, measurement, R1, R2, d0),
 * not augmented), in the one operation order that the device bank (kernels/ukf.hpp, one filter per thread) and a host build of this file
 * share.  This header IS the device-order definition: the GPU reproduces a host build of it (-ffp-contract=off) bit for bit.
 *
 * Plain C for host and device, with the conventions of llpf_kalman.h, whose pieces it uses (llpf_kf_idx, LLPF_KF_NP, llpf_kf_chol,
 * llpf_kf_gain_update, llpf_kf_smooth_finish): packed lower triangles, every accumulation over its summation index in increasing order
 * with explicit llpf_fma, sqrt and log those of llpf_detmath.h, triangular solves multiply by 1 / L_ii.
 *
 * Model: x' = f(x, u, p, tau) + w, w ~ N(0, R1);  y = g(x, u, p, tau) + e, e ~ N(0, R2).  With L = nx and N = 2 L + 1 points:
 *   points of (m, R):  R = C C' (lower Cholesky factor),  X_0 = m,  X_i = m + gamma C[:, i],  X_{L+i} = m - gamma C[:, i],  i = 1..L
 *   weights:           four numbers, gamma, wm0, wc0, wi (mean weights wm0, wi, ..., wi; covariance weights wc0, wi, ..., wi)
 *   correct!:          points of the prior (x, R);  Y_i = g(X_i);  yh = sum wm_i Y_i;  S = sum wc_i (Y_i - yh)(Y_i - yh)' + R2;
 *                      Cxy = sum wc_i (X_i - x)(Y_i - yh)';  e = y - yh;  then llpf_kf_gain_update with Cxy' in the place of C R:
 *                      S = L L', W = L^-1 Cxy', z = L^-1 e, x += W' z, R -= W' W, ll = -(ny/2) log 2 pi - log prod L_ii - z'z / 2
 *   predict!:          points of the posterior (x, R), drawn again;  X'_i = f(X_i);  x = sum wm_i X'_i;
 *                      R = sum wc_i (X'_i - x)(X'_i - x)' + R1
 * Every sum over the points runs i = 0, 1, ..., 2 L in that order in one accumulator:  acc = (w_0 a_0) b_0, then
 * acc = fma(w_i a_i, b_i, acc) for a weighted product, acc = w_0 a_0, then acc = fma(w_i, a_i, acc) for a weighted mean.
 *
 * The header does not know the model.  The caller evaluates f / g between its stages — on the device the kernel with Model::dynamics /
 * measurement, on the host a shim with function pointers:
 *     ok = llpf_ukf_factor(nx, R, Cf)                                    the factor of R
 *     for i in 0 .. 2 nx:  llpf_ukf_point(nx, gamma, x, Cf, i, X);  Z[i][:] = g(X)  (or f(X))
 *     ll = llpf_ukf_correct_finish(...)   /   llpf_ukf_predict_finish(...)   /   llpf_ukf_smooth_finish(...)  (f, backward pass)
 * The mapped points are the only per-point storage: Z[(i * dim + d) * zs] (dim = ny or nx; zs = 1 for a local array, the number of
 * lanes for a [point][d][lane] array in LDS).  A sigma point itself is a function of (x, Cf, i) and is formed again where the cross
 * covariance needs it — the same operations on the same numbers, so the same bits — never a second evaluation of f or g.
 *
 * A filter whose R (either factorisation) or S is not positive definite (a pivot not > 0, or NaN) is NaN from that step on; nothing else
 * is touched.  A row of Y whose first element is NaN is missing: the caller skips correct! (x and R stay, e is NaN, ll is 0).
 *
 * Parameters of one filter are entries P[e * ps] (host: ps = 1; device: the SoA [entry][F] with ps = F): R1 packed, then R2 packed. */
#ifndef LLPF_UKF_H
#define LLPF_UKF_H

#include "llpf_kalman.h"

#define LLPF_UKF_NPTS(nx) (2 * (nx) + 1)
#define LLPF_UKF_OFF_R1 0
#define LLPF_UKF_OFF_R2(nx) LLPF_KF_NP(nx)
#define LLPF_UKF_NPAR(nx, ny) (LLPF_KF_NP(nx) + LLPF_KF_NP(ny))

#define LLPF_UKF_P(e) (P[(int64_t)(e) * ps])
#define LLPF_UKF_Z(i, d) (Z[(int64_t)((i) * dim + (d)) * zs])

/* Cf = the lower Cholesky factor of R (both packed); returns 1, or 0 when R is not positive definite */
LLPF_HD int llpf_ukf_factor(const int nx, const double* R, double* Cf) {
    double inv[LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) Cf[i] = R[i];
    return llpf_kf_chol(nx, Cf, inv);
}

/* sigma point i (0 .. 2 nx) of (m, Cf): column j of the factor has no entries above row j, those components are m[d] itself */
LLPF_HD void llpf_ukf_point(const int nx, const double gamma, const double* m, const double* Cf, const int i, double* X) {
    const int j = i <= nx ? i - 1 : i - 1 - nx;
    const double g = i <= nx ? gamma : -gamma;
    LLPF_KF_UNROLL
    for (int d = 0; d < nx; ++d) X[d] = (i >= 1 && d >= j) ? llpf_fma(g, Cf[llpf_kf_idx(d, j)], m[d]) : m[d];
}

/* the mean of the mapped points into mean [dim]; Z becomes the deviations Z_i - mean */
LLPF_HD void llpf_ukf_center(const int nx, const int dim, const double wm0, const double wi, double* Z, const int64_t zs, double* mean) {
    LLPF_KF_UNROLL
    for (int r = 0; r < dim; ++r) {
        double acc = wm0 * LLPF_UKF_Z(0, r);
        LLPF_KF_UNROLL
        for (int i = 1; i < LLPF_UKF_NPTS(nx); ++i) acc = llpf_fma(wi, LLPF_UKF_Z(i, r), acc);
        mean[r] = acc;
    }
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_UKF_NPTS(nx); ++i) {
        LLPF_KF_UNROLL
        for (int r = 0; r < dim; ++r) LLPF_UKF_Z(i, r) = LLPF_UKF_Z(i, r) - mean[r];
    }
}

/* out (packed lower triangle, dim x dim) = sum wc_i Z_i Z_i' + Q, Z the deviations, Q = P[off ...] packed */
LLPF_HD void llpf_ukf_cov(const int nx, const int dim, const double wc0, const double wi, const double* Z, const int64_t zs, const double* P,
                          const int64_t ps, const int off, double* out) {
    LLPF_KF_UNROLL
    for (int r = 0; r < dim; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = (wc0 * LLPF_UKF_Z(0, r)) * LLPF_UKF_Z(0, c);
            LLPF_KF_UNROLL
            for (int i = 1; i < LLPF_UKF_NPTS(nx); ++i) acc = llpf_fma(wi * LLPF_UKF_Z(i, r), LLPF_UKF_Z(i, c), acc);
            out[llpf_kf_idx(r, c)] = acc + LLPF_UKF_P(off + llpf_kf_idx(r, c));
        }
    }
}

/* correct!, after the caller has put Y_i = g(X_i) of the points of (x, Cf) into Z (dim = ny).  ok: what llpf_ukf_factor returned.
 * The innovation into e, x and R updated in place; returns logpdf(N(0, S), e). */
LLPF_HD double llpf_ukf_correct_finish(const int nx, const int ny, const double gamma, const double wm0, const double wc0, const double wi,
                                       const double* P, const int64_t ps, const int ok, const double* Cf, double* Z, const int64_t zs,
                                       const double* y, double* x, double* R, double* e) {
    const int dim = ny;
    double yh[LLPF_KF_MAXY], L[LLPF_KF_NP(LLPF_KF_MAXY)], CR[LLPF_KF_MAXY * LLPF_KF_MAXX];
    llpf_ukf_center(nx, ny, wm0, wi, Z, zs, yh);
    llpf_ukf_cov(nx, ny, wc0, wi, Z, zs, P, ps, LLPF_UKF_OFF_R2(nx), L);
    /* CR = Cxy' (ny x nx) = sum wc_i (Y_i - yh)(X_i - x)' */
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_UKF_NPTS(nx); ++i) {
        double X[LLPF_KF_MAXX];
        llpf_ukf_point(nx, gamma, x, Cf, i, X);
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) X[c] = X[c] - x[c];
        LLPF_KF_UNROLL
        for (int r = 0; r < ny; ++r) {
            const double t = (i == 0 ? wc0 : wi) * LLPF_UKF_Z(i, r);
            LLPF_KF_UNROLL
            for (int c = 0; c < nx; ++c) CR[r * LLPF_KF_MAXX + c] = i == 0 ? t * X[c] : llpf_fma(t, X[c], CR[r * LLPF_KF_MAXX + c]);
        }
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) e[r] = y[r] - yh[r];
    return llpf_kf_gain_update(nx, ny, ok, L, CR, e, x, R);
}

/* predict!, after the caller has put X'_i = f(X_i) of the points of (x, Cf) into Z (dim = nx).  ok: what llpf_ukf_factor returned. */
LLPF_HD void llpf_ukf_predict_finish(const int nx, const double wm0, const double wc0, const double wi, const double* P, const int64_t ps,
                                     const int ok, double* Z, const int64_t zs, double* x, double* R) {
    llpf_ukf_center(nx, nx, wm0, wi, Z, zs, x);
    llpf_ukf_cov(nx, nx, wc0, wi, Z, zs, P, ps, LLPF_UKF_OFF_R1, R);
    if (!ok) {                              /* R not positive definite: this filter is NaN from here on */
        LLPF_KF_UNROLL
        for (int r = 0; r < nx; ++r) x[r] = llpf_kf_nan();
        LLPF_KF_UNROLL
        for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = llpf_kf_nan();
    }
}

/* One backward step of the unscented Rauch-Tung-Striebel smoother (Sarkka 2008, additive noise), after the caller has put
 * X'_i = f(X_i) of the points of the posterior (xt, Cf) of step t into Z (dim = nx).  ok: what llpf_ukf_factor(nx, Rt, Cf) returned.
 * On entry xT, RT are the smoothed estimate of step t + 1 (packed), on return that of step t; xt, Rt must not alias them.  From
 * xT[T] = xt[T], RT[T] = Rt[T], for t = T-1 down to 1 (1-based):
 *     x- = sum wm_i X'_i;  R- = sum wc_i dX'_i dX'_i' + R1;  G = sum wc_i dX'_i (X_i - xt)';
 *     J' = R-^-1 G;  xT[t] = xt[t] + J (xT[t+1] - x-);  RT[t] = Rt[t] + J (RT[t+1] - R-) J'
 * The form computed here:
 *   - x-, R- are llpf_ukf_center and llpf_ukf_cov on the mapped points exactly as llpf_ukf_predict_finish applies them — the same
 *     functions of the same numbers, so the bits of the forward pass's prior x[t+1], R[t+1], which is not stored;
 *   - G (nx x nx, G[r][c] = Cov(x'_r, x_c)) is accumulated as llpf_ukf_correct_finish accumulates Cxy': point i is formed again from
 *     (xt, Cf, i), f is not evaluated a second time;
 *   - the rest is llpf_kf_smooth_finish (llpf_kalman.h) with G in the place of A Rt: the Cholesky of R-, the two triangular solves,
 *     xT and the (J D) J' update in the lower triangle.
 * A filter whose Rt (!ok) or R- is not positive definite gets NaN xT, RT at step t and so at every earlier step; nothing else is
 * touched.  A missing row needs nothing: its posterior is its prior. */
LLPF_HD void llpf_ukf_smooth_finish(const int nx, const double gamma, const double wm0, const double wc0, const double wi, const double* P,
                                    const int64_t ps, const int ok, const double* Cf, double* Z, const int64_t zs, const double* xt,
                                    const double* Rt, double* xT, double* RT) {
    const int dim = nx;
    double xp[LLPF_KF_MAXX], L[LLPF_KF_NP(LLPF_KF_MAXX)], Jt[LLPF_KF_MAXX * LLPF_KF_MAXX];
    llpf_ukf_center(nx, nx, wm0, wi, Z, zs, xp);
    llpf_ukf_cov(nx, nx, wc0, wi, Z, zs, P, ps, LLPF_UKF_OFF_R1, L);
    /* Jt = G = sum wc_i (X'_i - x-)(X_i - xt)' */
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_UKF_NPTS(nx); ++i) {
        double X[LLPF_KF_MAXX];
        llpf_ukf_point(nx, gamma, xt, Cf, i, X);
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) X[c] = X[c] - xt[c];
        LLPF_KF_UNROLL
        for (int r = 0; r < nx; ++r) {
            const double t = (i == 0 ? wc0 : wi) * LLPF_UKF_Z(i, r);
            LLPF_KF_UNROLL
            for (int c = 0; c < nx; ++c) Jt[r * LLPF_KF_MAXX + c] = i == 0 ? t * X[c] : llpf_fma(t, X[c], Jt[r * LLPF_KF_MAXX + c]);
        }
    }
    llpf_kf_smooth_finish(nx, ok, xp, L, Jt, xt, Rt, xT, RT);
}

/* One step t of forward_trajectory: x, R on entry are the prior; correct! (skipped at a missing row) gives ll[t], e[t] and the posterior
 * xt[t], Rt[t]; predict! gives the prior of t + 1.  A run's ll_total starts at 0.0 and adds ll[t] in step order. */
#undef LLPF_UKF_Z
#undef LLPF_UKF_P

#endif /* LLPF_UKF_H */
