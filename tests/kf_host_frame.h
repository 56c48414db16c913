/* kf_host_frame.h — the frame that the host twins of the one-thread-per-filter banks share (tests/kalman_host.c, tests/ukf_host.c,
 * tests/ekf_host.c, and the IMM twins tests/imm_host.c, tests/imm_ekf_host.c over the first and the third): what "the device's layout"
 * means, once.  A twin packs its constants and calls csrc/shared/llpf_{kalman,ukf,ekf}.h in its callbacks; everything around those calls
 * is here, the six stages of csrc/shared/llpf_imm.h around the callbacks of M modes among it.
 *
 * Layouts.  Per filter, dense row-major: R1 [F][nx][nx], R2 [F][ny][ny], x0 [F][nx], P0 [F][nx][nx] (the lower triangles are read; x0, P0
 * receive the final state, the prior of step T).  U [T][nu] or [F][T][nu] (per_filter bit 0; a model without inputs gets nu zeros),
 * Y [T][ny] or [F][T][ny] (bit 1); step t runs at tau = (t_index0 + t) * Ts of the filter.  Outputs, each optional, time-major as the
 * device writes them: ll_steps, iters [T][F], x, xt, xT [T][F][nx], R, Rt, RT [T][F][nx][nx], e [T][F][ny]; ll_total [F]. */
#ifndef KF_HOST_FRAME_H
#define KF_HOST_FRAME_H
#include <stdint.h>
#include <string.h>

#include "llpf_kalman.h"
#include "llpf_imm.h"

typedef struct {
    int F, nx, ny, nu;
    int64_t T;
    int per_filter;
    double t_index0;
    const double *U, *Y;
    double *x0, *P0;                                           /* forward: the state, in and out */
    double *ll_total, *ll_steps, *x, *xt, *R, *Rt, *e;         /* forward: the outputs */
    int32_t* iters;                                            /* forward: what `correct` reports in *done */
    const double *post_x, *post_R;                             /* backward: the posterior of every step, xt and Rt of a forward pass */
    double *xT, *RT;                                           /* backward: the outputs */
} kf_host_io;

/* a family's forward step.  begin: filter f starts (pack its constants); returns its Ts.  correct: returns ll and owns the missing row.
 * The backward step: (xs, Rs) of step t + 1 become those of step t, from the posterior (xf, Rf) of step t */
typedef struct {
    double (*begin)(void* ctx, int f);
    double (*correct)(void* ctx, const double* u, const double* y, double tau, double* x, double* R, double* e, int* done);
    void (*predict)(void* ctx, const double* u, double tau, double* x, double* R);
    void (*smooth)(void* ctx, const double* u, double tau, const double* xf, const double* Rf, double* xs, double* Rs);
} kf_host_family;

/* the dense n x n form of a packed triangle, and the packed lower triangle of a dense matrix */
static inline void kf_host_dense(int n, const double* Rp, double* out) {
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) out[r * n + c] = Rp[llpf_kf_idx(r, c)];
}
static inline void kf_host_pack(int n, const double* dense, double* Rp) {
    for (int r = 0; r < n; ++r)
        for (int c = 0; c <= r; ++c) Rp[llpf_kf_idx(r, c)] = dense[r * n + c];
}
/* row t of filter f in a shared [T][n] or per-filter [F][T][n] input */
static inline const double* kf_host_row(const double* a, int per, int f, int64_t T, int64_t t, int n) {
    return a + (per ? ((size_t)f * T + t) : (size_t)t) * n;
}
static inline const double* kf_host_u(const kf_host_io* io, int f, int64_t t) {
    static const double zero_u[LLPF_KF_MAXU] = {0.0};
    return io->nu > 0 ? kf_host_row(io->U, io->per_filter & 1, f, io->T, t, io->nu) : zero_u;
}

static inline void kf_host_forward(const kf_host_io* io, const kf_host_family* fam, void* ctx) {
    const int F = io->F, nx = io->nx, ny = io->ny;
    for (int f = 0; f < F; ++f) {
        const double Ts = fam->begin(ctx, f);
        double x[LLPF_KF_MAXX], R[LLPF_KF_NP(LLPF_KF_MAXX)], e[LLPF_KF_MAXY];
        memcpy(x, io->x0 + (size_t)f * nx, sizeof(double) * nx);
        kf_host_pack(nx, io->P0 + (size_t)f * nx * nx, R);
        double llt = 0.0;
        for (int64_t t = 0; t < io->T; ++t) {
            const size_t tf = (size_t)t * F + f;
            const double* u = kf_host_u(io, f, t);
            const double* y = kf_host_row(io->Y, io->per_filter & 2, f, io->T, t, ny);
            const double tau = (io->t_index0 + (double)t) * Ts;
            if (io->x) memcpy(io->x + tf * nx, x, sizeof(double) * nx);
            if (io->R) kf_host_dense(nx, R, io->R + tf * nx * nx);
            int done = 0;
            const double ll = fam->correct(ctx, u, y, tau, x, R, e, &done);
            llt = llt + ll;
            if (io->iters) io->iters[tf] = done;
            if (io->ll_steps) io->ll_steps[tf] = ll;
            if (io->e) memcpy(io->e + tf * ny, e, sizeof(double) * ny);
            if (io->xt) memcpy(io->xt + tf * nx, x, sizeof(double) * nx);
            if (io->Rt) kf_host_dense(nx, R, io->Rt + tf * nx * nx);
            fam->predict(ctx, u, tau, x, R);
        }
        if (io->ll_total) io->ll_total[f] = llt;
        memcpy(io->x0 + (size_t)f * nx, x, sizeof(double) * nx);
        kf_host_dense(nx, R, io->P0 + (size_t)f * nx * nx);
    }
}

static inline void kf_host_backward(const kf_host_io* io, const kf_host_family* fam, void* ctx) {
    const int F = io->F, nx = io->nx;
    for (int f = 0; f < F; ++f) {
        const double Ts = fam->begin(ctx, f);
        double xs[LLPF_KF_MAXX], Rs[LLPF_KF_NP(LLPF_KF_MAXX)], xf[LLPF_KF_MAXX], Rf[LLPF_KF_NP(LLPF_KF_MAXX)];
        for (int64_t t = io->T - 1; t >= 0; --t) {
            const size_t tf = (size_t)t * F + f;
            memcpy(xf, io->post_x + tf * nx, sizeof(double) * nx);
            kf_host_pack(nx, io->post_R + tf * nx * nx, Rf);
            if (t == io->T - 1) {                               /* xT[T] = xt[T], RT[T] = Rt[T] */
                memcpy(xs, xf, sizeof(double) * nx);
                memcpy(Rs, Rf, sizeof(double) * LLPF_KF_NP(nx));
            } else {
                fam->smooth(ctx, kf_host_u(io, f, t), (io->t_index0 + (double)t) * Ts, xf, Rf, xs, Rs);
            }
            if (io->xT) memcpy(io->xT + tf * nx, xs, sizeof(double) * nx);
            if (io->RT) kf_host_dense(nx, Rs, io->RT + tf * nx * nx);
        }
    }
}

/* ---- the IMM over M modes of one family: the six stages of csrc/shared/llpf_imm.h, once ---- */
#define KF_HOST_NPK LLPF_KF_NP(LLPF_KF_MAXX)

typedef struct {
    int M, interact;
    const double* P;               /* [F][M][M] */
    double Ts;                     /* the bank's: step t runs at tau = (t_index0 + t) * Ts, whatever a mode's begin returns */
    double *mu, *xm, *Rm;          /* the state, in and out: [F][M], [F][M][nx], [F][M][nx][nx] (lower triangles read) */
    double *mu_steps, *ll_modes;   /* the outputs beside io's ll_total, ll_steps, x, xt, R, Rt: [T][F][M] */
} kf_host_imm_io;

/* the combined estimate of the state as it stands: x = sum_j mu_j x_j, R = sum_j mu_j (R_j + (x_j - x)(x_j - x)') */
static inline void imm_combine(int M, int nx, const double* mu, double xs[][LLPF_KF_MAXX], double Rs[][KF_HOST_NPK], double* x, double* R) {
    for (int r = 0; r < nx; ++r) x[r] = 0.0;
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = 0.0;
    for (int i = 0; i < M; ++i) llpf_imm_mean_add(nx, mu[i], xs[i], x);
    for (int i = 0; i < M; ++i) llpf_imm_cov_add(nx, mu[i], xs[i], Rs[i], x, R);
}

/* ctxs: M contexts of the family, ctx_size bytes each; mode j of filter f is the family's filter f * M + j.  Where the device fetches mode
 * i from lane i, the loops here read mode i's arrays. */
static inline void kf_host_imm(const kf_host_io* io, const kf_host_family* fam, void* ctxs, size_t ctx_size, const kf_host_imm_io* imm) {
    const int F = io->F, nx = io->nx, ny = io->ny, M = imm->M, np = LLPF_KF_NP(nx);
    for (int f = 0; f < F; ++f) {
        double xs[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rs[LLPF_IMM_MAXM][KF_HOST_NPK], mu[LLPF_IMM_MAXM];
        const double* Pf = imm->P + (size_t)f * M * M;
        for (int j = 0; j < M; ++j) {
            const size_t fj = (size_t)f * M + j;
            fam->begin((char*)ctxs + j * ctx_size, (int)fj);
            memcpy(xs[j], imm->xm + fj * nx, sizeof(double) * nx);
            kf_host_pack(nx, imm->Rm + fj * nx * nx, Rs[j]);
            mu[j] = imm->mu[fj];
        }
        double llt = 0.0;
        for (int64_t t = 0; t < io->T; ++t) {
            const size_t tf = (size_t)t * F + f;
            const double* u = kf_host_u(io, f, t);
            const double* y = kf_host_row(io->Y, io->per_filter & 2, f, io->T, t, ny);
            const double tau = (io->t_index0 + (double)t) * imm->Ts;
            double xc[LLPF_KF_MAXX], Rc[KF_HOST_NPK], e[LLPF_KF_MAXY];
            /* 1. the combined prior */
            if (io->x || io->R) imm_combine(M, nx, mu, xs, Rs, xc, Rc);
            if (io->x) memcpy(io->x + tf * nx, xc, sizeof(double) * nx);
            if (io->R) kf_host_dense(nx, Rc, io->R + tf * nx * nx);
            /* 2. correct! of every mode at its own prior; the family owns the missing row (ll_j = 0, x_j and R_j as they were) */
            double llj[LLPF_IMM_MAXM], c[LLPF_IMM_MAXM], a[LLPF_IMM_MAXM], w[LLPF_IMM_MAXM];
            for (int j = 0; j < M; ++j) {
                int done = 0;
                llj[j] = fam->correct((char*)ctxs + j * ctx_size, u, y, tau, xs[j], Rs[j], e, &done);
            }
            /* 3. the mode probabilities */
            for (int j = 0; j < M; ++j) {
                c[j] = 0.0;
                for (int i = 0; i < M; ++i) c[j] = llpf_imm_c_add(Pf[i * M + j], mu[i], c[j]);
            }
            double ll = 0.0;
            if (!(y[0] == y[0])) {
                for (int j = 0; j < M; ++j) mu[j] = c[j];
            } else {
                for (int j = 0; j < M; ++j) a[j] = llpf_imm_loga(c[j], llj[j]);
                double m = a[0];
                for (int i = 1; i < M; ++i) m = llpf_imm_max(m, a[i]);
                for (int j = 0; j < M; ++j) w[j] = llpf_imm_w(c[j], a[j], m);
                double s = 0.0;
                for (int i = 0; i < M; ++i) s = s + w[i];
                ll = llpf_imm_ll(m, s);
                for (int j = 0; j < M; ++j) {
                    mu[j] = w[j] / s;
                    llpf_imm_poison(nx, ll, xs[j], Rs[j]);
                }
            }
            llt = llt + ll;
            if (io->ll_steps) io->ll_steps[tf] = ll;
            if (imm->mu_steps) memcpy(imm->mu_steps + tf * M, mu, sizeof(double) * M);
            if (imm->ll_modes) memcpy(imm->ll_modes + tf * M, llj, sizeof(double) * M);
            /* 4. the combined posterior */
            if (io->xt || io->Rt) imm_combine(M, nx, mu, xs, Rs, xc, Rc);
            if (io->xt) memcpy(io->xt + tf * nx, xc, sizeof(double) * nx);
            if (io->Rt) kf_host_dense(nx, Rc, io->Rt + tf * nx * nx);
            /* 5. the mixing: every mode from the modes as they were */
            if (imm->interact) {
                double xn[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rn[LLPF_IMM_MAXM][KF_HOST_NPK];
                for (int j = 0; j < M; ++j) {
                    double cj = 0.0, wm[LLPF_IMM_MAXM];
                    for (int i = 0; i < M; ++i) cj = llpf_imm_c_add(Pf[i * M + j], mu[i], cj);
                    for (int i = 0; i < M; ++i) wm[i] = llpf_imm_mix_w(Pf[i * M + j], mu[i], cj);
                    for (int r = 0; r < nx; ++r) xn[j][r] = 0.0;
                    for (int i = 0; i < np; ++i) Rn[j][i] = 0.0;
                    for (int i = 0; i < M; ++i) llpf_imm_mean_add(nx, wm[i], xs[i], xn[j]);
                    for (int i = 0; i < M; ++i) llpf_imm_cov_add(nx, wm[i], xs[i], Rs[i], xn[j], Rn[j]);
                    if (cj == 0.0) {                    /* a mode without mass is not mixed */
                        memcpy(xn[j], xs[j], sizeof(double) * nx);
                        memcpy(Rn[j], Rs[j], sizeof(double) * np);
                    }
                }
                memcpy(xs, xn, sizeof(xs));
                memcpy(Rs, Rn, sizeof(Rs));
            }
            /* 6. predict! of every mode, at its x after the mixing */
            for (int j = 0; j < M; ++j) fam->predict((char*)ctxs + j * ctx_size, u, tau, xs[j], Rs[j]);
        }
        if (io->ll_total) io->ll_total[f] = llt;
        for (int j = 0; j < M; ++j) {
            const size_t fj = (size_t)f * M + j;
            memcpy(imm->xm + fj * nx, xs[j], sizeof(double) * nx);
            kf_host_dense(nx, Rs[j], imm->Rm + fj * nx * nx);
            imm->mu[fj] = mu[j];
        }
    }
}
#endif
