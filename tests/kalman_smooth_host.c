/* kalman_smooth_host.c — a host build of llpf_kf_smooth (csrc/shared/llpf_kalman.h, the device order of the Kalman bank's smoother), for
 * the tests and for tools/bench_kalman.py --smooth.  Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared kalman_smooth_host.c
 *
 * kf_host_smooth: the backward pass of F filters over the posterior of a forward pass (tests/kalman_host.c: kf_host_run), exactly as
 * llpf_kalman_bank_smooth runs it on the device.  Matrices per filter, row-major as for kf_host_run.  U [T][nu] or [F][T][nu] (per_filter
 * bit 0).  xt [T][F][nx], Rt [T][F][nx][nx] the posterior of every step (the lower triangle of Rt is read).  Outputs time-major as the
 * device writes them: xT [T][F][nx], RT [T][F][nx][nx]. */
#include <stdint.h>
#include <string.h>

#include "llpf_kalman.h"

int kf_host_smooth(int F, int nx, int ny, int nu, const double* A, const double* B, const double* C, const double* D, const double* R1,
                   const double* R2, const double* U, int64_t T, int per_filter, const double* xt, const double* Rt, double* xTo,
                   double* RTo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU || T < 1) return -1;
    double P[LLPF_KF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY, LLPF_KF_MAXU)];
    for (int f = 0; f < F; ++f) {
        memset(P, 0, sizeof(P));
        for (int i = 0; i < nx * nx; ++i) P[LLPF_KF_OFF_A + i] = A[(size_t)f * nx * nx + i];
        for (int i = 0; i < ny * nx; ++i) P[LLPF_KF_OFF_C(nx) + i] = C[(size_t)f * ny * nx + i];
        for (int r = 0; r < nx; ++r)
            for (int c = 0; c <= r; ++c) P[LLPF_KF_OFF_R1(nx, ny) + llpf_kf_idx(r, c)] = R1[((size_t)f * nx + r) * nx + c];
        for (int r = 0; r < ny; ++r)
            for (int c = 0; c <= r; ++c) P[LLPF_KF_OFF_R2(nx, ny) + llpf_kf_idx(r, c)] = R2[((size_t)f * ny + r) * ny + c];
        for (int i = 0; i < nx * nu; ++i) P[LLPF_KF_OFF_B(nx, ny) + i] = B[(size_t)f * nx * nu + i];
        for (int i = 0; i < ny * nu; ++i) P[LLPF_KF_OFF_D(nx, ny, nu) + i] = D[(size_t)f * ny * nu + i];
        double xs[LLPF_KF_MAXX], Rs[LLPF_KF_NP(LLPF_KF_MAXX)], xf[LLPF_KF_MAXX], Rf[LLPF_KF_NP(LLPF_KF_MAXX)];
        for (int64_t t = T - 1; t >= 0; --t) {
            const size_t tf = (size_t)t * F + f;
            for (int i = 0; i < nx; ++i) xf[i] = xt[tf * nx + i];
            for (int r = 0; r < nx; ++r)
                for (int c = 0; c <= r; ++c) Rf[llpf_kf_idx(r, c)] = Rt[(tf * nx + r) * nx + c];
            if (t == T - 1) {                                   /* xT[T] = xt[T], RT[T] = Rt[T] */
                memcpy(xs, xf, sizeof(double) * nx);
                memcpy(Rs, Rf, sizeof(double) * LLPF_KF_NP(nx));
            } else {
                const double* u = nu > 0 ? U + ((per_filter & 1) ? ((size_t)f * T + t) : (size_t)t) * nu : U;
                llpf_kf_smooth(nx, ny, nu, P, 1, u, xf, Rf, xs, Rs);
            }
            if (xTo) memcpy(xTo + tf * nx, xs, sizeof(double) * nx);
            if (RTo)
                for (int r = 0; r < nx; ++r)
                    for (int c = 0; c < nx; ++c) RTo[(tf * nx + r) * nx + c] = Rs[llpf_kf_idx(r, c)];
        }
    }
    return 0;
}
