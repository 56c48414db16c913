/* iekf_host.c — a host build of the iterated extended Kalman filter of csrc/shared/llpf_ekf.h (llpf_iekf_iterate, llpf_iekf_stop: the
 * device order of an extended Kalman bank after llpf_ekf_bank_set_iterations), for the tests and for tools/bench_ekf.py.  The models and
 * their C twins are those of tests/ekf_host.c, taken by inclusion: the library holds ekf_host_run as well.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include iekf_host.c -o libiekf_host.so
 *
 * iekf_host_run: ekf_host_run's arguments and layouts, then maxiters >= 1, epsilon >= 0 and iters [T][F] (optional): the number of
 * linearisations of the measurement that step t of filter f ran, 0 at a missing row — reported here for the tests only, the C ABI has no
 * such output. */
#include "ekf_host.c"

/* gx = g(x) and C = dg/dx at x, as ekf_host_run evaluates them */
static void measurement_jac(int kind, ekf_fn g, const llpf_model* m, int nx, int ny, const double* x, const double* u, double tau, double* gx,
                            double* J) {
    if (kind == EKF_LG) {
        g(m, x, u, tau, gx);
        for (int i = 0; i < ny * nx; ++i) J[i] = m->C[i];
    } else if (kind == EKF_QUADTANK) {
        gx[0] = x[0]; gx[1] = x[1];
        for (int i = 0; i < 8; ++i) J[i] = 0.0;
        J[0] = 1.0; J[5] = 1.0;
    } else if (kind == EKF_PENDULUM) {
        pendulum_g_jac(x, gx, J);
    } else {
        gx[0] = x[0] * x[0];
        J[0] = x[0] + x[0];
        for (int i = 1; i < nx; ++i) J[i] = 0.0;
    }
}

int iekf_host_run(int F, int nx, int ny, int nu, ekf_fn f, ekf_fn g, int kind, const llpf_model* models, const double* R1, const double* R2,
                  double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0, double* ll_total,
                  double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo, int maxiters, double epsilon,
                  int32_t* iters) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    if (kind == EKF_LG && (!f || !g)) return -2;
    if (kind == EKF_QUADTANK && (nx != 4 || ny != 2 || nu != 2)) return -3;
    if (kind == EKF_PENDULUM && (nx != 2 || ny != 1)) return -3;
    if (kind == EKF_SQUARE && ny != 1) return -3;
    if (maxiters < 1 || maxiters > LLPF_IEKF_MAXITERS || !(epsilon >= 0.0)) return -4;
    const double zero_u[LLPF_KF_MAXU] = {0.0};
    double P[LLPF_EKF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY)];
    for (int k = 0; k < F; ++k) {
        const llpf_model* m = models + k;
        for (int r = 0; r < nx; ++r)
            for (int c = 0; c <= r; ++c) P[LLPF_EKF_OFF_R1 + llpf_kf_idx(r, c)] = R1[((size_t)k * nx + r) * nx + c];
        for (int r = 0; r < ny; ++r)
            for (int c = 0; c <= r; ++c) P[LLPF_EKF_OFF_R2(nx) + llpf_kf_idx(r, c)] = R2[((size_t)k * ny + r) * ny + c];
        double x[LLPF_KF_MAXX], R[LLPF_KF_NP(LLPF_KF_MAXX)], e[LLPF_KF_MAXY];
        double val[LLPF_KF_MAXX], J[LLPF_KF_MAXX * LLPF_KF_MAXX];
        for (int i = 0; i < nx; ++i) x[i] = x0[(size_t)k * nx + i];
        for (int r = 0; r < nx; ++r)
            for (int c = 0; c <= r; ++c) R[llpf_kf_idx(r, c)] = P0[((size_t)k * nx + r) * nx + c];
        double llt = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const size_t tf = (size_t)t * F + k;
            const double* u = nu > 0 ? U + ((per_filter & 1) ? ((size_t)k * T + t) : (size_t)t) * nu : zero_u;
            const double* y = Y + ((per_filter & 2) ? ((size_t)k * T + t) : (size_t)t) * ny;
            const double tau = (t_index0 + (double)t) * m->Ts;
            if (xo) memcpy(xo + tf * nx, x, sizeof(double) * nx);
            if (Ro) dense(nx, R, Ro + tf * nx * nx);
            double ll = 0.0;
            int done = 0;
            if (llpf_ekf_missing(y)) {
                for (int r = 0; r < ny; ++r) e[r] = llpf_kf_nan();
            } else {
                double xi[LLPF_KF_MAXX], Rn[LLPF_KF_NP(LLPF_KF_MAXX)], move;
                for (int i = 0; i < nx; ++i) xi[i] = x[i];
                do {
                    measurement_jac(kind, g, m, nx, ny, xi, u, tau, val, J);
                    ll = llpf_iekf_iterate(nx, ny, P, 1, y, val, J, nx, x, R, done == 0, xi, Rn, e, &move);
                    ++done;
                } while (!llpf_iekf_stop(done, maxiters, move, epsilon));
                for (int i = 0; i < nx; ++i) x[i] = xi[i];
                for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = Rn[i];
            }
            if (iters) iters[tf] = done;
            llt = llt + ll;
            if (ll_steps) ll_steps[tf] = ll;
            if (eo) memcpy(eo + tf * ny, e, sizeof(double) * ny);
            if (xto) memcpy(xto + tf * nx, x, sizeof(double) * nx);
            if (Rto) dense(nx, R, Rto + tf * nx * nx);
            if (kind == EKF_LG) {
                f(m, x, u, tau, val);
                for (int i = 0; i < nx * nx; ++i) J[i] = m->A[i];
            } else if (kind == EKF_QUADTANK) {
                ekf_host_qt_jac(m, u, tau, x, val, J);
            } else if (kind == EKF_PENDULUM) {
                pendulum_f_jac(m, x, u, val, J);
            } else {
                for (int r = 0; r < nx; ++r) {
                    val[r] = x[r];
                    for (int c = 0; c < nx; ++c) J[r * nx + c] = r == c ? 1.0 : 0.0;
                }
            }
            llpf_ekf_predict(nx, P, 1, val, J, nx, x, R);
        }
        if (ll_total) ll_total[k] = llt;
        for (int i = 0; i < nx; ++i) x0[(size_t)k * nx + i] = x[i];
        dense(nx, R, P0 + (size_t)k * nx * nx);
    }
    return 0;
}
