/* kalman_host.c — a host build of csrc/shared/llpf_kalman.h (the device order of the Kalman bank), for the tests and for
 * tools/bench_kalman.py.  Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared kalman_host.c -o libkalman_host.so
 *
 * kf_host_run: T steps of F filters from x0, P0 (the lower triangle of P0 is read), exactly as llpf_kalman_bank_run after
 * llpf_kalman_bank_set_state(x0, P0).  Matrices per filter, row-major: A [F][nx][nx], B [F][nx][nu], C [F][ny][nx], D [F][ny][nu],
 * R1 [F][nx][nx], R2 [F][ny][ny].  U [T][nu] or [F][T][nu] (per_filter bit 0), Y [T][ny] or [F][T][ny] (bit 1).  Outputs (each
 * optional) time-major as the device writes them: ll_steps [T][F], x, xt [T][F][nx], R, Rt [T][F][nx][nx], e [T][F][ny]; ll_total [F];
 * x0, P0 receive the final state (the prior of step T). */
#include <stdint.h>
#include <string.h>

#include "llpf_kalman.h"

static void dense(int nx, const double* Rp, double* out) {
    for (int r = 0; r < nx; ++r)
        for (int c = 0; c < nx; ++c) out[r * nx + c] = Rp[llpf_kf_idx(r, c)];
}

int kf_host_run(int F, int nx, int ny, int nu, const double* A, const double* B, const double* C, const double* D, const double* R1,
                const double* R2, double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter,
                double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    const int npar = LLPF_KF_NPAR(nx, ny, nu);
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
        (void)npar;
        double x[LLPF_KF_MAXX], R[LLPF_KF_NP(LLPF_KF_MAXX)], e[LLPF_KF_MAXY];
        for (int i = 0; i < nx; ++i) x[i] = x0[(size_t)f * nx + i];
        for (int r = 0; r < nx; ++r)
            for (int c = 0; c <= r; ++c) R[llpf_kf_idx(r, c)] = P0[((size_t)f * nx + r) * nx + c];
        double llt = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const size_t tf = (size_t)t * F + f;
            const double* u = nu > 0 ? U + ((per_filter & 1) ? ((size_t)f * T + t) : (size_t)t) * nu : U;
            const double* y = Y + ((per_filter & 2) ? ((size_t)f * T + t) : (size_t)t) * ny;
            if (xo) memcpy(xo + tf * nx, x, sizeof(double) * nx);
            if (Ro) dense(nx, R, Ro + tf * nx * nx);
            const double ll = llpf_kf_correct(nx, ny, nu, P, 1, u, y, x, R, e);
            llt = llt + ll;
            if (ll_steps) ll_steps[tf] = ll;
            if (eo) memcpy(eo + tf * ny, e, sizeof(double) * ny);
            if (xto) memcpy(xto + tf * nx, x, sizeof(double) * nx);
            if (Rto) dense(nx, R, Rto + tf * nx * nx);
            llpf_kf_predict(nx, ny, nu, P, 1, u, x, R);
        }
        if (ll_total) ll_total[f] = llt;
        for (int i = 0; i < nx; ++i) x0[(size_t)f * nx + i] = x[i];
        dense(nx, R, P0 + (size_t)f * nx * nx);
    }
    return 0;
}
