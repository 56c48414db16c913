/* ekf_host.c — a host build of csrc/shared/llpf_ekf.h (the device order of the extended Kalman bank) and of
 * csrc/shared/llpf_quadtank_jac.h, for the tests and for tools/bench_ekf.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include ekf_host.c -o libekf_host.so
 *
 * ekf_host_run: T steps of F filters from x0, P0 (the lower triangle of P0 is read), exactly as llpf_ekf_bank_run after
 * llpf_ekf_bank_set_state(x0, P0).  kind names the model and where value and Jacobian come from:
 *   EKF_LG        the linear-Gaussian model: the value through f / g (model, x, u, tau, out) — the tests pass the oracle's orc_dynamics /
 *                 orc_measurement, the device's LinGauss in the device's order — and the Jacobians are the descriptor's A, C
 *   EKF_QUADTANK  the quad-tank: llpf_qt_dynamics_jac of the shared header (value and Jacobian), the two unit rows for the measurement
 *   EKF_PENDULUM  the C twin of the tests' pendulum snippet with its hand-written members (tests/ekf_common.py: PENDULUM_JAC_SRC)
 *   EKF_SQUARE    f(x) = x, g(x) = x_0^2 (SQUARE_JAC_SRC)
 * models [F] are the llpf_model descriptors; R1 [F][nx][nx], R2 [F][ny][ny] dense row-major (the lower triangles are read).  U [T][nu] or
 * [F][T][nu] (per_filter bit 0), Y [T][ny] or [F][T][ny] (bit 1); step t runs at tau = (t_index0 + t) * models[f].Ts.  Outputs (each
 * optional) time-major as the device writes them: ll_steps [T][F], x, xt [T][F][nx], R, Rt [T][F][nx][nx], e [T][F][ny]; ll_total [F];
 * x0, P0 receive the final state. */
#include <stdint.h>
#include <string.h>

#include "llpf.h"
#include "llpf_ekf.h"
#include "llpf_quadtank_jac.h"

enum { EKF_LG = 0, EKF_QUADTANK = 1, EKF_PENDULUM = 2, EKF_SQUARE = 3 };
typedef void (*ekf_fn)(const llpf_model* m, const double* x, const double* u, double t, double* out);

/* the quad-tank through the shared header: fx [4], J [16] */
void ekf_host_qt_jac(const llpf_model* m, const double* u, double t, const double* x, double* fx, double* J) {
    llpf_qt_coef c;
    llpf_qt_coef_set(m->qt, m->Ts, m->supersample, &c);
    llpf_qt_dynamics_jac(&c, u[0], u[1], t, x, fx, J);
}

/* the pendulum: the expressions of the snippet, through the same llpf_sincos2pi / llpf_rint */
static void pendulum_sincos(const double* x, double* sn, double* cs) {
    const double turns = x[0] * 0.15915494309189535;
    llpf_sincos2pi(turns - llpf_rint(turns) < 0.0 ? turns - llpf_rint(turns) + 1.0 : turns - llpf_rint(turns), sn, cs);
}
static void pendulum_f_jac(const llpf_model* m, const double* x, const double* u, double* fx, double* J) {
    const double g_over_l = m->qt[0], damp = m->qt[1], dt = m->Ts, torque = (m->nu > 0 && u) ? u[0] : 0.0;
    double sn, cs;
    pendulum_sincos(x, &sn, &cs);
    fx[0] = x[0] + dt * x[1];
    fx[1] = x[1] + dt * (torque - g_over_l * sn - damp * x[1] * x[1] * x[1]);
    J[0] = 1.0;
    J[1] = dt;
    J[2] = dt * (-(g_over_l * cs));
    J[3] = 1.0 + dt * (-(3.0 * damp * x[1] * x[1]));
}
static void pendulum_g_jac(const double* x, double* gx, double* J) {
    double sn, cs;
    pendulum_sincos(x, &sn, &cs);
    gx[0] = sn;
    J[0] = cs;
    J[1] = 0.0;
}

static void dense(int nx, const double* Rp, double* out) {
    for (int r = 0; r < nx; ++r)
        for (int c = 0; c < nx; ++c) out[r * nx + c] = Rp[llpf_kf_idx(r, c)];
}

int ekf_host_run(int F, int nx, int ny, int nu, ekf_fn f, ekf_fn g, int kind, const llpf_model* models, const double* R1, const double* R2,
                 double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0, double* ll_total,
                 double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    if (kind == EKF_LG && (!f || !g)) return -2;
    if (kind == EKF_QUADTANK && (nx != 4 || ny != 2 || nu != 2)) return -3;
    if (kind == EKF_PENDULUM && (nx != 2 || ny != 1)) return -3;
    if (kind == EKF_SQUARE && ny != 1) return -3;
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
            if (llpf_ekf_missing(y)) {
                for (int r = 0; r < ny; ++r) e[r] = llpf_kf_nan();
            } else {
                if (kind == EKF_LG) {
                    g(m, x, u, tau, val);
                    for (int i = 0; i < ny * nx; ++i) J[i] = m->C[i];
                } else if (kind == EKF_QUADTANK) {
                    val[0] = x[0]; val[1] = x[1];
                    for (int i = 0; i < 8; ++i) J[i] = 0.0;
                    J[0] = 1.0; J[5] = 1.0;
                } else if (kind == EKF_PENDULUM) {
                    pendulum_g_jac(x, val, J);
                } else {
                    val[0] = x[0] * x[0];
                    J[0] = x[0] + x[0];
                    for (int i = 1; i < nx; ++i) J[i] = 0.0;
                }
                ll = llpf_ekf_correct(nx, ny, P, 1, y, val, J, nx, x, R, e);
            }
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
