/* kf_host_frame.h — the frame that the host twins of the one-thread-per-filter banks share (tests/kalman_host.c, tests/ukf_host.c,
 * tests/ekf_host.c): what "the device's layout" means, once.  A twin packs its constants and calls csrc/shared/llpf_{kalman,ukf,ekf}.h
 * in its callbacks; everything around those calls is here.
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
#endif
