/* llpf_kalman.h — the Kalman filter with constant matrices (reference src/kalman.jl, predict! / correct! of src/filtering.jl:52-128),
 * in the one operation order that the device bank (kernels/kalman.hpp, one filter per thread) and a host build of this file share.
 * This header IS the device-order definition: the GPU reproduces a host build of it (-ffp-contract=off) bit for bit.
 *
 * Plain C for host and device.  Every accumulation runs over its summation index in increasing order with explicit llpf_fma; sqrt and
 * log are those of llpf_detmath.h.  On the device the dimensions nx, ny are literal constants at the call site and every loop over them
 * unrolls; nu is a run-time number (loops over the inputs stay loops).
 *
 * Model: x' = A x + B u + w, w ~ N(0, R1);  y = C x + D u + e, e ~ N(0, R2).  alpha = 1, no cross-covariance R12.
 *
 * The form computed here.  With S = C R C' + R2 = L L' (lower Cholesky factor) and W = L^-1 (C R) (ny x nx):
 *     K e            = R C' S^-1 e = W' z,  z = L^-1 e
 *     (I - K C) R    = R - R C' S^-1 C R = R - W' W
 *     logpdf(N(0, S), e) = -(ny/2) log(2 pi) - log(L11 ... Lnn) - z'z / 2
 * — the reference's correct! (K = (R C')/S_chol, x += K e, R = symmetrize((I - K C) R)) term by term, without forming K.
 * Choices of this order:
 *   - R is symmetric by construction and only its lower triangle is formed and stored (packed, entry (r, c), c <= r, at r(r+1)/2 + c):
 *     symmetrize() is then the identity.  The same holds for S (lower triangle of C R C' plus R2) and for A R A' + R1.
 *   - the triangular solves multiply by 1 / L_ii (one division per diagonal entry);
 *   - log det S / 2 is ONE log of the product of L's diagonal (ny <= 4 factors);
 *   - the running sums of a matrix-vector product continue from the C (A) columns into the D (B) columns in one accumulator.
 * A filter whose S is not positive definite (the Cholesky pivot is not > 0, or NaN) returns ll = NaN and NaN x, R: from that step on
 * every result of that filter is NaN, and nothing else is touched.
 *
 * Parameters of one filter are entries P[e * ps] (host: ps = 1 and one filter's entries consecutive; device: the SoA [entry][F] of the
 * bank with ps = F, P pointing at filter f's column), in the order of LLPF_KF_OFF_* below.  The state is x [nx] and the packed R [np]. */
#ifndef LLPF_KALMAN_H
#define LLPF_KALMAN_H

#include "llpf_detmath.h"

#define LLPF_KF_MAXX 8
#define LLPF_KF_MAXY 4
#define LLPF_KF_MAXU 8
#define LLPF_KF_NP(n) ((n) * ((n) + 1) / 2)

/* parameter entries: A [nx][nx], C [ny][nx], R1 packed, R2 packed, B [nx][nu], D [ny][nu] (the inputs last: A .. R2 sit at offsets that
 * do not depend on the run-time nu) */
#define LLPF_KF_OFF_A 0
#define LLPF_KF_OFF_C(nx) ((nx) * (nx))
#define LLPF_KF_OFF_R1(nx, ny) (LLPF_KF_OFF_C(nx) + (ny) * (nx))
#define LLPF_KF_OFF_R2(nx, ny) (LLPF_KF_OFF_R1(nx, ny) + LLPF_KF_NP(nx))
#define LLPF_KF_OFF_B(nx, ny) (LLPF_KF_OFF_R2(nx, ny) + LLPF_KF_NP(ny))
#define LLPF_KF_OFF_D(nx, ny, nu) (LLPF_KF_OFF_B(nx, ny) + (nx) * (nu))
#define LLPF_KF_NPAR(nx, ny, nu) (LLPF_KF_OFF_D(nx, ny, nu) + (ny) * (nu))

#if defined(__HIP_DEVICE_COMPILE__)
#define LLPF_KF_UNROLL _Pragma("unroll")
#else
#define LLPF_KF_UNROLL
#endif

#define LLPF_KF_P(e) (P[(int64_t)(e) * ps])

LLPF_HD int llpf_kf_idx(int r, int c) { return r >= c ? r * (r + 1) / 2 + c : c * (c + 1) / 2 + r; }
LLPF_HD double llpf_kf_nan(void) { return llpf_u2d(0x7ff8000000000000ULL); }

/* L L' = S in place: S is the packed lower triangle (n x n) on entry, its lower Cholesky factor on return; inv[i] = 1 / L_ii.
 * Returns 1 when every pivot is > 0 (a NaN pivot fails the test), else 0 — the factor is then not usable. */
LLPF_HD int llpf_kf_chol(const int n, double* L, double* inv) {
    int ok = 1;
    LLPF_KF_UNROLL
    for (int i = 0; i < n; ++i) {
        LLPF_KF_UNROLL
        for (int j = 0; j <= i; ++j) {
            double acc = L[llpf_kf_idx(i, j)];
            LLPF_KF_UNROLL
            for (int k = 0; k < j; ++k) acc = llpf_fma(-L[llpf_kf_idx(i, k)], L[llpf_kf_idx(j, k)], acc);
            if (i == j) {
                ok = ok & (acc > 0.0);
                const double d = llpf_sqrt(acc);
                L[llpf_kf_idx(i, i)] = d;
                inv[i] = 1.0 / d;
            } else {
                L[llpf_kf_idx(i, j)] = acc * inv[j];
            }
        }
    }
    return ok;
}

/* The measurement update from the innovation covariance S (packed lower triangle in L, factored here), the cross term CR (ny x nx, row
 * stride LLPF_KF_MAXX: C R of the Kalman filter, Cxy' of the unscented one) and the innovation e:
 *     W = L^-1 CR,  z = L^-1 e,  x += W' z,  R -= W' W (lower triangle),  returns -(ny/2) log(2 pi) - log(L11 ... Lnn) - z'z / 2.
 * ok: 0 when something before this call already made the filter invalid.  Not positive definite (or !ok): NaN ll, x, R. */
LLPF_HD double llpf_kf_gain_update(const int nx, const int ny, int ok, double* L, const double* CR, const double* e, double* x, double* R) {
    double inv[LLPF_KF_MAXY];
    ok = ok & llpf_kf_chol(ny, L, inv);
    /* W = L^-1 (C R)  (ny x nx),  z = L^-1 e */
    double W[LLPF_KF_MAXY * LLPF_KF_MAXX], z[LLPF_KF_MAXY];
    LLPF_KF_UNROLL
    for (int i = 0; i < ny; ++i) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = CR[i * LLPF_KF_MAXX + c];
            LLPF_KF_UNROLL
            for (int q = 0; q < i; ++q) acc = llpf_fma(-L[llpf_kf_idx(i, q)], W[q * LLPF_KF_MAXX + c], acc);
            W[i * LLPF_KF_MAXX + c] = acc * inv[i];
        }
        double acc = e[i];
        LLPF_KF_UNROLL
        for (int q = 0; q < i; ++q) acc = llpf_fma(-L[llpf_kf_idx(i, q)], z[q], acc);
        z[i] = acc * inv[i];
    }
    /* ll = -(ny/2) log(2 pi) - log(L11 ... Lnn) - z'z / 2 */
    double quad = z[0] * z[0], det = L[0];
    LLPF_KF_UNROLL
    for (int i = 1; i < ny; ++i) {
        quad = llpf_fma(z[i], z[i], quad);
        det = det * L[llpf_kf_idx(i, i)];
    }
    const double c0 = -((double)ny * llpf_log(6.283185307179586)) / 2.0;
    double ll = (c0 - llpf_log(det)) - 0.5 * quad;
    /* x += W' z ;  R -= W' W  (lower triangle) */
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double acc = W[r] * z[0];
        LLPF_KF_UNROLL
        for (int i = 1; i < ny; ++i) acc = llpf_fma(W[i * LLPF_KF_MAXX + r], z[i], acc);
        x[r] = x[r] + acc;
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = W[r] * W[c];
            LLPF_KF_UNROLL
            for (int i = 1; i < ny; ++i) acc = llpf_fma(W[i * LLPF_KF_MAXX + r], W[i * LLPF_KF_MAXX + c], acc);
            R[llpf_kf_idx(r, c)] = R[llpf_kf_idx(r, c)] - acc;
        }
    }
    if (!ok) {                              /* S not positive definite: this filter is NaN from here on */
        ll = llpf_kf_nan();
        LLPF_KF_UNROLL
        for (int r = 0; r < nx; ++r) x[r] = llpf_kf_nan();
        LLPF_KF_UNROLL
        for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = llpf_kf_nan();
    }
    return ll;
}

/* correct!(kf, u, y): the innovation e (ny), x and R updated in place; returns logpdf(N(0, S), e).
 * A row whose first element is NaN is missing: x and R stay, e is NaN, the result is 0. */
LLPF_HD double llpf_kf_correct(const int nx, const int ny, const int nu, const double* P, const int64_t ps, const double* u,
                               const double* y, double* x, double* R, double* e) {
    if (!(y[0] == y[0])) {
        LLPF_KF_UNROLL
        for (int r = 0; r < ny; ++r) e[r] = llpf_kf_nan();
        return 0.0;
    }
    const int oC = LLPF_KF_OFF_C(nx), oR2 = LLPF_KF_OFF_R2(nx, ny), oD = LLPF_KF_OFF_D(nx, ny, nu);
    /* e = y - (C x + D u) */
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        double acc = LLPF_KF_P(oC + r * nx) * x[0];
        LLPF_KF_UNROLL
        for (int q = 1; q < nx; ++q) acc = llpf_fma(LLPF_KF_P(oC + r * nx + q), x[q], acc);
        for (int c = 0; c < nu; ++c) acc = llpf_fma(LLPF_KF_P(oD + r * nu + c), u[c], acc);
        e[r] = y[r] - acc;
    }
    /* CR = C R  (ny x nx) */
    double CR[LLPF_KF_MAXY * LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = LLPF_KF_P(oC + r * nx) * R[llpf_kf_idx(0, c)];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(LLPF_KF_P(oC + r * nx + q), R[llpf_kf_idx(q, c)], acc);
            CR[r * LLPF_KF_MAXX + c] = acc;
        }
    }
    /* S = (C R) C' + R2, lower triangle, factored in place: L L' = S */
    double L[LLPF_KF_NP(LLPF_KF_MAXY)];
    LLPF_KF_UNROLL
    for (int r = 0; r < ny; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = CR[r * LLPF_KF_MAXX] * LLPF_KF_P(oC + c * nx);
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(CR[r * LLPF_KF_MAXX + q], LLPF_KF_P(oC + c * nx + q), acc);
            L[llpf_kf_idx(r, c)] = acc + LLPF_KF_P(oR2 + llpf_kf_idx(r, c));
        }
    }
    return llpf_kf_gain_update(nx, ny, 1, L, CR, e, x, R);
}

/* predict!(kf, u): x = A x + B u, R = A R A' + R1 (lower triangle; A R formed one row at a time) */
LLPF_HD void llpf_kf_predict(const int nx, const int ny, const int nu, const double* P, const int64_t ps, const double* u, double* x,
                             double* R) {
    const int oR1 = LLPF_KF_OFF_R1(nx, ny), oB = LLPF_KF_OFF_B(nx, ny);
    double xn[LLPF_KF_MAXX], Rn[LLPF_KF_NP(LLPF_KF_MAXX)];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double acc = LLPF_KF_P(r * nx) * x[0];
        LLPF_KF_UNROLL
        for (int q = 1; q < nx; ++q) acc = llpf_fma(LLPF_KF_P(r * nx + q), x[q], acc);
        for (int c = 0; c < nu; ++c) acc = llpf_fma(LLPF_KF_P(oB + r * nu + c), u[c], acc);
        xn[r] = acc;
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double ar[LLPF_KF_MAXX];             /* row r of A R */
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = LLPF_KF_P(r * nx) * R[llpf_kf_idx(0, c)];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(LLPF_KF_P(r * nx + q), R[llpf_kf_idx(q, c)], acc);
            ar[c] = acc;
        }
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = ar[0] * LLPF_KF_P(c * nx);
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(ar[q], LLPF_KF_P(c * nx + q), acc);
            Rn[llpf_kf_idx(r, c)] = acc + LLPF_KF_P(oR1 + llpf_kf_idx(r, c));
        }
    }
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) x[r] = xn[r];
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = Rn[i];
}

/* One step t of forward_trajectory (reference src/filtering.jl:343-365): x, R on entry are the prior x[t], R[t]; correct! gives ll[t],
 * e[t] and the posterior xt[t], Rt[t]; predict! gives the prior of t + 1.  update! is this step.  A run's ll_total starts at 0.0 and
 * adds ll[t] in step order (ll_total = ll_total + ll[t]), a missing row adding 0. */

/* The second half of a backward step, shared by this smoother and the unscented one (llpf_ukf.h: llpf_ukf_smooth_finish), from the prior
 * of step t + 1 (xp, and the packed R[t+1] in L, factored here) and the cross term G = Cov(x[t+1], x[t] | y[1..t]) (nx x nx, row stride
 * LLPF_KF_MAXX, in Jt: A Rt of the Kalman filter, sum wc_i dX'_i dX_i' of the unscented one):
 *     d = xT - xp,  D = RT - R[t+1],  L L' = R[t+1],  J' = L^-T (L^-1 G),  xT = xt + J d,  RT = Rt + (J D) J' (lower triangle).
 * ok: 0 when something before this call already made the filter invalid.  Not positive definite (or !ok): NaN xT, RT. */
LLPF_HD void llpf_kf_smooth_finish(const int nx, int ok, const double* xp, double* L, double* Jt, const double* xt, const double* Rt,
                                   double* xT, double* RT) {
    double d[LLPF_KF_MAXX], Dl[LLPF_KF_NP(LLPF_KF_MAXX)], inv[LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) d[r] = xT[r] - xp[r];
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) Dl[i] = RT[i] - L[i];
    /* L L' = R[t+1], in place */
    ok = ok & llpf_kf_chol(nx, L, inv);
    /* Jt = L^-1 Jt; Jt = L^-T Jt.  Jt[i][c] = J'(i, c) = J(c, i) */
    LLPF_KF_UNROLL
    for (int i = 0; i < nx; ++i) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = Jt[i * LLPF_KF_MAXX + c];
            LLPF_KF_UNROLL
            for (int q = 0; q < i; ++q) acc = llpf_fma(-L[llpf_kf_idx(i, q)], Jt[q * LLPF_KF_MAXX + c], acc);
            Jt[i * LLPF_KF_MAXX + c] = acc * inv[i];
        }
    }
    LLPF_KF_UNROLL
    for (int n = 0; n < nx; ++n) {          /* row i = nx - 1 - n; q = i + 1 + p runs over i + 1 .. nx - 1 (this loop shape unrolls on the device) */
        const int i = nx - 1 - n;
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = Jt[i * LLPF_KF_MAXX + c];
            LLPF_KF_UNROLL
            for (int p = 0; p < n; ++p) acc = llpf_fma(-L[llpf_kf_idx(i + 1 + p, i)], Jt[(i + 1 + p) * LLPF_KF_MAXX + c], acc);
            Jt[i * LLPF_KF_MAXX + c] = acc * inv[i];
        }
    }
    /* xT = xt + J d */
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double acc = Jt[r] * d[0];
        LLPF_KF_UNROLL
        for (int q = 1; q < nx; ++q) acc = llpf_fma(Jt[q * LLPF_KF_MAXX + r], d[q], acc);
        xT[r] = xt[r] + acc;
    }
    /* RT = Rt + (J D) J'  (lower triangle; row r of J D formed once) */
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        double m[LLPF_KF_MAXX];
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = Jt[r] * Dl[llpf_kf_idx(0, c)];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(Jt[q * LLPF_KF_MAXX + r], Dl[llpf_kf_idx(q, c)], acc);
            m[c] = acc;
        }
        LLPF_KF_UNROLL
        for (int c = 0; c <= r; ++c) {
            double acc = m[0] * Jt[c];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(m[q], Jt[q * LLPF_KF_MAXX + c], acc);
            RT[llpf_kf_idx(r, c)] = Rt[llpf_kf_idx(r, c)] + acc;
        }
    }
    if (!ok) {                              /* R[t+1] not positive definite: this filter is NaN from here back */
        LLPF_KF_UNROLL
        for (int r = 0; r < nx; ++r) xT[r] = llpf_kf_nan();
        LLPF_KF_UNROLL
        for (int i = 0; i < LLPF_KF_NP(nx); ++i) RT[i] = llpf_kf_nan();
    }
}

/* One backward step of the Rauch-Tung-Striebel smoother, smooth(sol, kf, u, y) (reference src/smoothing.jl:10-102).  For t = T-1 down
 * to 1 (1-based), from xT[T] = xt[T], RT[T] = Rt[T]:
 *     C = Rt[t] A' / R[t+1];  xT[t] = xt[t] + C (xT[t+1] - x[t+1]);  RT[t] = Rt[t] + symmetrize(C (RT[t+1] - R[t+1]) C')
 * On entry xt, Rt are the posterior of step t (packed), u = u[t], and xT, RT the smoothed estimate of step t + 1 (packed); on return
 * xT, RT hold that of step t.  xt, Rt must not alias xT, RT.
 * The form computed here:
 *   - the prior x[t+1], R[t+1] is not stored by the forward pass: it is llpf_kf_predict applied to (xt, Rt, u) — the same function of
 *     the same numbers, so the bits the forward pass produced;
 *   - R[t+1] = L L', factored exactly as correct! factors S;
 *   - G = A Rt (the rows predict! forms), then J' = L^-T (L^-1 G) = R[t+1]^-1 A Rt: J is the reference's C, renamed (C is the
 *     measurement matrix here).  The forward substitution runs over increasing rows, the back substitution over decreasing rows with its
 *     sum over increasing index; both multiply by 1 / L_ii;
 *   - xT = xt + J d with d = xT[t+1] - x[t+1];
 *   - with D = RT[t+1] - R[t+1] (packed), J D is formed one row at a time and RT = Rt + (J D) J' only in its lower triangle:
 *     symmetrize() is the identity, as in the forward pass.
 * A filter whose R[t+1] is not positive definite (a pivot not > 0, or NaN) gets NaN xT, RT at step t and so at every earlier step;
 * nothing else is touched. */
LLPF_HD void llpf_kf_smooth(const int nx, const int ny, const int nu, const double* P, const int64_t ps, const double* u, const double* xt,
                            const double* Rt, double* xT, double* RT) {
    /* the prior of step t + 1 */
    double xp[LLPF_KF_MAXX], L[LLPF_KF_NP(LLPF_KF_MAXX)];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) xp[r] = xt[r];
    LLPF_KF_UNROLL
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) L[i] = Rt[i];
    llpf_kf_predict(nx, ny, nu, P, ps, u, xp, L);
    /* Jt = G = A Rt */
    double Jt[LLPF_KF_MAXX * LLPF_KF_MAXX];
    LLPF_KF_UNROLL
    for (int r = 0; r < nx; ++r) {
        LLPF_KF_UNROLL
        for (int c = 0; c < nx; ++c) {
            double acc = LLPF_KF_P(r * nx) * Rt[llpf_kf_idx(0, c)];
            LLPF_KF_UNROLL
            for (int q = 1; q < nx; ++q) acc = llpf_fma(LLPF_KF_P(r * nx + q), Rt[llpf_kf_idx(q, c)], acc);
            Jt[r * LLPF_KF_MAXX + c] = acc;
        }
    }
    llpf_kf_smooth_finish(nx, 1, xp, L, Jt, xt, Rt, xT, RT);
}
#undef LLPF_KF_P

#endif /* LLPF_KALMAN_H */
