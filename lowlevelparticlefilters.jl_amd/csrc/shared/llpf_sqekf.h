/* llpf_sqekf.h — the square-root extended Kalman filter with additive noise: the first-order filter of llpf_ekf.h carrying a factor of its
 * covariance as llpf_sqkf.h does, in the one operation order that the device bank (kernels/sqekf.hpp, one filter per thread) and a host
 * build of this file share.  This header IS the device-order definition: the GPU reproduces a host build of it (-ffp-contract=off) bit
 * for bit.  It is the textbook array form (Kailath, Sayed and Hassibi, Linear Estimation, ch. 12) around a model linearised at the current
 * mean, and is unverified against the reference's source.
 *
 * Plain C for host and device, on the conventions of llpf_sqkf.h and llpf_ekf.h, whose pieces it uses (llpf_sq_lq, llpf_sq_cov,
 * llpf_ekf_missing, the LLPF_EKF_OFF_* layout) and none of whose functions it changes.
 *
 * Model: that of llpf_ekf.h.  The filter carries x [nx] and the packed lower-triangular Lr [np] with R = Lr Lr' and a diagonal >= 0.
 * Parameters: the extended bank's block (LLPF_EKF_OFF_R1, LLPF_EKF_OFF_R2(nx), entries P[e * ps]) with the packed lower Cholesky factors
 * L1, L2 (R1 = L1 L1', R2 = L2 L2', llpf_kf_chol on the host, once) in the places of R1 and R2.
 * The header does not know the model: the caller evaluates value and Jacobian and hands over numbers, as for llpf_ekf_correct and
 * llpf_ekf_predict.  A Jacobian is row-major with row stride ld (J[r * ld + c] = d out_r / d x_c).
 *
 * predict!: fx = f(x), A = df/dx at the posterior x;  x = fx;  the pre-array is [L1 | A Lr] (nx x 2 nx), z = nx, with
 * (A Lr)_rc = sum over q = c .. nx-1 of A_rq Lr_qc (the first product, then llpf_fma in increasing q); llpf_sq_lq makes it [L 0] and
 * Lr becomes L.
 * correct!: gx = g(x), C = dg/dx at the prior x;  e = y - gx;  the pre-array is [[L2, C Lr], [0, Lr]] ((ny + nx) square), z = ny, C Lr
 * formed like A Lr; llpf_sq_lq makes it [[Ls, 0], [Kb, Lt]].  Then z = Ls^-1 e (forward substitution, multiplying by 1 / Ls_ii),
 * x += Kb z (the first product, then llpf_fma in increasing index, then one addition), Lr = Lt and
 * ll = (-(ny/2) log(2 pi) - log(Ls_11 ... Ls_nn)) - z'z / 2 in llpf_sq_correct's expression shape.
 * Both are llpf_sq_predict / llpf_sq_correct operation for operation, with A / C read from a local array in the place of the parameter
 * block: on a linear model whose Jacobians are the matrices themselves, Lr, R = llpf_sq_cov(Lr) and Rt are the square-root Kalman bank's
 * bits — what llpf_ekf.h promises against llpf_kalman.h.
 *
 * A row of Y whose first element is NaN is missing: the caller skips correct! (x and Lr stay, e is NaN, ll is 0) — llpf_ekf_missing.
 * Nothing is subtracted from a covariance, so nothing here makes a finite filter NaN: R2 positive definite keeps every Ls_ii > 0.  A
 * filter is NaN only where its inputs, its model's values or its state are.
 *
 * There is no smoother, no iterated form, and the filter is not a mode of an IMM. */
#ifndef LLPF_SQEKF_H
#define LLPF_SQEKF_H

#include "llpf_sqkf.h"
#include "llpf_ekf.h"

#define LLPF_SQEKF_P(e) (P[(int64_t)(e) * ps])

/* row r of G Lr into out[0 .. nx-1]: G is a local row-major matrix with row stride ld (A or C) */
LLPF_HD void llpf_sqekf_row_times_factor(const int nx, const double* G, const int ld, const int r, const double* Lr, double* out) {
    LLPF_KF_UNROLL
    for (int c = 0; c < nx; ++c) {
        double acc = G[r * ld + c] * Lr[llpf_kf_idx(c, c)];
        LLPF_KF_UNROLL
        for (int q = 0; q < nx; ++q)
            if (q > c) acc = llpf_fma(G[r * ld + q], Lr[llpf_kf_idx(q, c)], acc);
        out[c] = acc;
    }
}

/* correct! from gx = g(x) and C = dg/dx (ny x nx, row stride ld), both at the prior x: e, x and Lr updated in place; returns
 * logpdf(N(0, S), e) */
LLPF_HD double llpf_sqekf_correct(const int nx, const int ny, const double* P, const int64_t ps, const double* y, const double* gx,
                                  const double* C, const int ld, double* x, double* Lr, double* e) {
    const int oL2 = LLPF_EKF_OFF_R2(nx);
    const int n = ny + nx;
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) e[r] = y[r] - gx[r];
    /* M = [[L2, C Lr], [0, Lr]] */
    double M[LLPF_SQ_MAXN * LLPF_SQ_MAXN];
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < ny; ++c) M[r * n + c] = c <= r ? LLPF_SQEKF_P(oL2 + llpf_kf_idx(r, c)) : 0.0;
        llpf_sqekf_row_times_factor(nx, C, ld, r, Lr, M + r * n + ny);
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < ny; ++c) M[(ny + r) * n + c] = 0.0;
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) M[(ny + r) * n + ny + c] = c <= r ? Lr[llpf_kf_idx(r, c)] : 0.0;
    }
    llpf_sq_lq(n, n, ny, M);                /* [[Ls, 0], [Kb, Lt]] */
    /* z = Ls^-1 e */
    double z[LLPF_KF_MAXY];
    LLPF_KF_UNROLL
    for (int i = 0; i < ny; ++i) {
        double acc = e[i];
        LLPF_KF_UNROLL
        for (int q = 0; q < i; ++q) acc = llpf_fma(-M[i * n + q], z[q], acc);
        z[i] = acc * (1.0 / M[i * n + i]);
    }
    /* ll = -(ny/2) log(2 pi) - log(Ls11 ... Lsnn) - z'z / 2 */
    double quad = z[0] * z[0], det = M[0];
    LLPF_KF_UNROLL
    for (int i = 1; i < ny; ++i) {
        quad = llpf_fma(z[i], z[i], quad);
        det = det * M[i * n + i];
    }
    const double c0 = -((double)ny * llpf_log(6.283185307179586)) / 2.0;
    const double ll = (c0 - llpf_log(det)) - 0.5 * quad;
    /* x += Kb z ;  Lr = Lt */
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double acc = M[(ny + r) * n] * z[0];
        LLPF_KF_UNROLL
        for (int i = 1; i < ny; ++i) acc = llpf_fma(M[(ny + r) * n + i], z[i], acc);
        x[r] = x[r] + acc;
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) Lr[llpf_kf_idx(r, c)] = M[(ny + r) * n + ny + c];
    }
    return ll;
}

/* predict! from fx = f(x) and A = df/dx (nx x nx, row stride ld), both at the posterior x: x = fx, Lr = the LQ factor of [L1 | A Lr] */
LLPF_HD void llpf_sqekf_predict(const int nx, const double* P, const int64_t ps, const double* fx, const double* A, const int ld,
                                double* x, double* Lr) {
    const int m = 2 * nx;
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) x[r] = fx[r];
    double M[LLPF_KF_MAXX * 2 * LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) M[r * m + c] = c <= r ? LLPF_SQEKF_P(LLPF_EKF_OFF_R1 + llpf_kf_idx(r, c)) : 0.0;
        llpf_sqekf_row_times_factor(nx, A, ld, r, Lr, M + r * m + nx);
    }
    llpf_sq_lq(nx, m, nx, M);
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) Lr[llpf_kf_idx(r, c)] = M[r * m + c];
    }
}

/* One step t of forward_trajectory is llpf_ekf.h's: llpf_sqekf_correct on the prior gives ll[t], e[t] and the posterior (skipped on a
 * missing row), llpf_sqekf_predict the prior of t + 1; ll_total starts at 0.0 and adds ll[t] in step order. */
#undef LLPF_SQEKF_P

#endif /* LLPF_SQEKF_H */
