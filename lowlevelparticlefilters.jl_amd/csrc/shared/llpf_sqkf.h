/* llpf_sqkf.h — the square-root Kalman filter with constant matrices (the reference's SqKalmanFilter, src/sq_kalman.jl), in the one
 * operation order that the device bank (kernels/sqkf.hpp, one filter per thread) and a host build of this file share.
 * This header IS the device-order definition: the GPU reproduces a host build of it (-ffp-contract=off) bit for bit.
 * The reference's sq_kalman.jl was not at hand when this was written: what follows is the textbook array form (Kailath, Sayed and
 * Hassibi, Linear Estimation, ch. 12) and is unverified against the reference's source.
 *
 * Plain C for host and device, on the conventions of llpf_kalman.h: packed lower triangles through llpf_kf_idx, every accumulation over
 * its summation index in increasing order with explicit llpf_fma, llpf_sqrt and llpf_log of llpf_detmath.h, literal nx, ny on the device
 * (every loop over them unrolls), parameters as P[e * ps].
 *
 * Model: that of llpf_kalman.h.  The filter carries x [nx] and the packed lower-triangular Lr [np] with R = Lr Lr' and a diagonal >= 0.
 * Parameters: the LLPF_KF_OFF_* layout with the packed lower Cholesky factors L1, L2 (R1 = L1 L1', R2 = L2 L2', llpf_kf_chol on the host,
 * once) in the places of R1 and R2.
 *
 * llpf_sq_lq(n, m, z, M) — the core: M (n x m, row-major, row stride m, n <= m) becomes [L 0] with L lower triangular (n x n) and a
 * diagonal >= 0 and L L' = M M', by Householder reflections applied from the right, one per row i = 0 .. n-1 in that order.
 *   - the known zeros: in a row i < z the entries of the columns i+1 .. z-1 are zero on entry and no earlier reflection touches them
 *     (both pre-arrays below start with a lower-triangular block of z columns), so the reflection of row i acts on the column i and the
 *     columns j0 .. m-1 only, j0 = z for i < z and j0 = i + 1 else.  Those columns are the row's "tail".
 *   - tail = sum of M_ij^2 over the tail in increasing j, from 0.0 by llpf_fma(M_ij, M_ij, tail).  A row whose tail is exactly 0.0 (an
 *     empty tail, an all-zero row, a row that is triangular already) gets no reflection.  A NaN tail is not 0.0: NaN goes through.
 *   - else, with a = M_ii: norm = llpf_sqrt(llpf_fma(a, a, tail)); d = a >= 0 ? norm : -norm (the sign against cancellation);
 *     v0 = a + d; the reflection is I - beta v v' with v = (v0, the tail of row i) and beta = 1.0 / (d * v0)  (= 2 / v'v, both factors of
 *     one sign).  Every later row r = i+1 .. n-1, in that order: w = M_ri * v0, then w = llpf_fma(M_rj, M_ij, w) over the tail in
 *     increasing j; w = w * beta; M_ri = llpf_fma(-w, v0, M_ri) and M_rj = llpf_fma(-w, M_ij, M_rj) over the tail.  Row i itself is set,
 *     not computed: M_ii = -d, its tail 0.0.
 *   - at the end every column j < n with M_jj < 0 is negated in the rows j .. n-1.
 * Nothing is scaled: squares of entries must neither overflow nor underflow to zero (|entries| between 1e-150 and 1e150).
 *
 * predict!: x = A x + B u with llpf_kf_predict's accumulation.  The pre-array is [L1 | A Lr] (nx x 2 nx; the columns of the textbook's
 * [A Lr | L1] in the other order, which leaves M M' = A R A' + R1 as it is and puts the triangular block where its zeros are skipped),
 * z = nx; (A Lr)_rc = sum over q = c .. nx-1 of A_rq Lr_qc (Lr's zeros skipped: the first product, then llpf_fma in increasing q).  Lr
 * becomes the triangle L.
 * correct!: e = y - (C x + D u) as llpf_kf_correct; the pre-array is [[L2, C Lr], [0, Lr]] ((ny + nx) square), z = ny, C Lr formed like
 * A Lr; it becomes [[Ls, 0], [Kb, Lt]] with Ls Ls' = S = C R C' + R2, Kb = R C' Ls^-T and Lt Lt' = R - Kb Kb'.  Then z = Ls^-1 e (forward
 * substitution, multiplying by 1 / Ls_ii as llpf_kf_gain_update does), x += Kb z (the first product, then llpf_fma in increasing index,
 * then one addition), Lr = Lt and ll = (-(ny/2) log(2 pi) - log(Ls_11 ... Ls_nn)) - z'z / 2 in llpf_kf_gain_update's expression shape.
 * A missing row (first element NaN) skips correct!: e is NaN, the result 0.
 * Nothing is subtracted from a covariance, so nothing here makes a finite filter NaN: R2 positive definite keeps every Ls_ii > 0.  A
 * filter is NaN only where its inputs or its state are.
 *
 * llpf_sq_cov(nx, Lr, R): the packed lower triangle of R = Lr Lr', R_rc = sum over k = 0 .. c of Lr_rk Lr_ck (c <= r; the first product,
 * then llpf_fma in increasing k).  The dense R mirrors it (kf_store_dense), so it is exactly symmetric.  The kernel's R and Rt outputs
 * and get_state use it. */
#ifndef LLPF_SQKF_H
#define LLPF_SQKF_H

#include "llpf_kalman.h"

#define LLPF_SQ_MAXN (LLPF_KF_MAXY + LLPF_KF_MAXX)                  /* the rows and columns of correct!'s pre-array */
#define LLPF_SQ_P(e) (P[(int64_t)(e) * ps])

/* (every loop below runs over a range that does not depend on an outer loop's index, and tests the index: on the device the loops
 * unroll and the tests fold, which loops with dependent bounds did not do reliably here) */
LLPF_HD void llpf_sq_lq(const int n, const int m, const int z, double* M) {
    LLPF_KF_UNROLL
    for (int i = 0; i < n; ++i) {
        const int j0 = i < z ? z : i + 1;      /* the tail: columns j0 .. m-1 */
        double tail = 0.0;
        LLPF_KF_UNROLL
        for (int j = 0; j < m; ++j)
            if (j >= j0) tail = llpf_fma(M[i * m + j], M[i * m + j], tail);
        if (!(tail == 0.0)) {
            const double a = M[i * m + i];
            const double norm = llpf_sqrt(llpf_fma(a, a, tail));
            const double d = a >= 0.0 ? norm : -norm;
            const double v0 = a + d;
            const double beta = 1.0 / (d * v0);
            LLPF_KF_UNROLL
            for (int r = 0; r < n; ++r) {
                if (r > i) {
                    double w = M[r * m + i] * v0;
                    LLPF_KF_UNROLL
                    for (int j = 0; j < m; ++j)
                        if (j >= j0) w = llpf_fma(M[r * m + j], M[i * m + j], w);
                    w = w * beta;
                    M[r * m + i] = llpf_fma(-w, v0, M[r * m + i]);
                    LLPF_KF_UNROLL
                    for (int j = 0; j < m; ++j)
                        if (j >= j0) M[r * m + j] = llpf_fma(-w, M[i * m + j], M[r * m + j]);
                }
            }
            M[i * m + i] = -d;
            LLPF_KF_UNROLL
            for (int j = 0; j < m; ++j)
                if (j >= j0) M[i * m + j] = 0.0;
        }
    }
    LLPF_KF_UNROLL
    for (int j = 0; j < n; ++j) {
        const int neg = M[j * m + j] < 0.0;
        LLPF_KF_UNROLL
        for (int r = 0; r < n; ++r) {
            if (r >= j) {
                const double v = M[r * m + j];
                M[r * m + j] = neg ? -v : v;
            }
        }
    }
}

/* row r of G Lr into out[0 .. nx-1]: G is the nx-wide row-major parameter matrix at entry og (A or C) */
LLPF_HD void llpf_sq_row_times_factor(const int nx, const double* P, const int64_t ps, const int og, const int r, const double* Lr,
                                      double* out) {
    LLPF_KF_UNROLL
    for (int c = 0; c < nx; ++c) {
        double acc = LLPF_SQ_P(og + r * nx + c) * Lr[llpf_kf_idx(c, c)];
        LLPF_KF_UNROLL
        for (int q = 0; q < nx; ++q)
            if (q > c) acc = llpf_fma(LLPF_SQ_P(og + r * nx + q), Lr[llpf_kf_idx(q, c)], acc);
        out[c] = acc;
    }
}

/* correct!(kf, u, y): the innovation e (ny), x and Lr updated in place; returns logpdf(N(0, S), e).
 * A row whose first element is NaN is missing: x and Lr stay, e is NaN, the result is 0. */
LLPF_HD double llpf_sq_correct(const int nx, const int ny, const int nu, const double* P, const int64_t ps, const double* u,
                               const double* y, double* x, double* Lr, double* e) {
    if (!(y[0] == y[0])) {
        LLPF_KF_UNROLL
        for (int r = 0; r < ny; ++r) e[r] = llpf_kf_nan();
        return 0.0;
    }
    const int oC = LLPF_KF_OFF_C(nx), oL2 = LLPF_KF_OFF_R2(nx, ny), oD = LLPF_KF_OFF_D(nx, ny, nu);
    const int n = ny + nx;
    /* e = y - (C x + D u) */
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        double acc = LLPF_SQ_P(oC + r * nx) * x[0];
        LLPF_KF_UNROLL
        for (int q = 1; q < nx; ++q) acc = llpf_fma(LLPF_SQ_P(oC + r * nx + q), x[q], acc);
        for (int c = 0; c < nu; ++c) acc = llpf_fma(LLPF_SQ_P(oD + r * nu + c), u[c], acc);
        e[r] = y[r] - acc;
    }
    /* M = [[L2, C Lr], [0, Lr]] */
    double M[LLPF_SQ_MAXN * LLPF_SQ_MAXN];
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < ny; ++c) M[r * n + c] = c <= r ? LLPF_SQ_P(oL2 + llpf_kf_idx(r, c)) : 0.0;
        llpf_sq_row_times_factor(nx, P, ps, oC, r, Lr, M + r * n + ny);
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

/* predict!(kf, u): x = A x + B u, Lr = the LQ factor of [L1 | A Lr] */
LLPF_HD void llpf_sq_predict(const int nx, const int ny, const int nu, const double* P, const int64_t ps, const double* u, double* x,
                             double* Lr) {
    const int oL1 = LLPF_KF_OFF_R1(nx, ny), oB = LLPF_KF_OFF_B(nx, ny);
    const int m = 2 * nx;
    double xn[LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double acc = LLPF_SQ_P(r * nx) * x[0];
        LLPF_KF_UNROLL
        for (int q = 1; q < nx; ++q) acc = llpf_fma(LLPF_SQ_P(r * nx + q), x[q], acc);
        for (int c = 0; c < nu; ++c) acc = llpf_fma(LLPF_SQ_P(oB + r * nu + c), u[c], acc);
        xn[r] = acc;
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) x[r] = xn[r];
    double M[LLPF_KF_MAXX * 2 * LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) M[r * m + c] = c <= r ? LLPF_SQ_P(oL1 + llpf_kf_idx(r, c)) : 0.0;
        llpf_sq_row_times_factor(nx, P, ps, LLPF_KF_OFF_A, r, Lr, M + r * m + nx);
    }
    llpf_sq_lq(nx, m, nx, M);
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) Lr[llpf_kf_idx(r, c)] = M[r * m + c];
    }
}

/* the packed lower triangle of R = Lr Lr' */
LLPF_HD void llpf_sq_cov(const int nx, const double* Lr, double* R) {
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = Lr[llpf_kf_idx(r, 0)] * Lr[llpf_kf_idx(c, 0)];
            LLPF_KF_UNROLL
            for (int k = 1; k < nx; ++k)
                if (k <= c) acc = llpf_fma(Lr[llpf_kf_idx(r, k)], Lr[llpf_kf_idx(c, k)], acc);
            R[llpf_kf_idx(r, c)] = acc;
        }
    }
}

/* One step t of forward_trajectory is llpf_kalman.h's: llpf_sq_correct on the prior gives ll[t], e[t] and the posterior, llpf_sq_predict
 * the prior of t + 1; ll_total starts at 0.0 and adds ll[t] in step order. */
#undef LLPF_SQ_P

#endif /* LLPF_SQKF_H */
