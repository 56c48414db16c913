/* ukf_host.c — a host build of csrc/shared/llpf_ukf.h (the device order of the unscented Kalman bank) around model functions given as
 * pointers, for the tests and for tools/bench_ukf.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include ukf_host.c -o libukf_host.so
 *
 * ukf_host_run: T steps of F filters from x0, P0 (the lower triangle of P0 is read), exactly as llpf_ukf_bank_run after
 * llpf_ukf_bank_set_state(x0, P0).  f / g: dynamics and measurement (model, x, u, tau, out) — the tests pass the addresses of the
 * oracle's orc_dynamics / orc_measurement, the device's models in the device's order — or NULL with `twin` naming one of the C twins
 * below of the tests' device snippets.  models [F] are the llpf_model descriptors (the model's own parameters); R1 [F][nx][nx],
 * R2 [F][ny][ny] dense row-major (the lower triangles are read); w = gamma, wm0, wc0, wi.  U [T][nu] or [F][T][nu] (per_filter bit 0),
 * Y [T][ny] or [F][T][ny] (bit 1); step t runs at tau = (t_index0 + t) * models[f].Ts.  Outputs (each optional) time-major as the device
 * writes them: ll_steps [T][F], x, xt [T][F][nx], R, Rt [T][F][nx][nx], e [T][F][ny]; ll_total [F]; x0, P0 receive the final state. */
#include <stdint.h>
#include <string.h>

#include "llpf.h"
#include "llpf_ukf.h"

typedef void (*ukf_fn)(const llpf_model* m, const double* x, const double* u, double t, double* out);

/* twin 1: the pendulum of tests/user_models.py (PENDULUM_SRC): the same expressions through the same llpf_sincos2pi / llpf_rint */
static void pendulum_f(const llpf_model* m, const double* x, const double* u, double t, double* out) {
    (void)t;
    const double g_over_l = m->qt[0], damp = m->qt[1], dt = m->Ts, torque = (m->nu > 0 && u) ? u[0] : 0.0;
    double sn, cs;
    const double turns = x[0] * 0.15915494309189535;
    llpf_sincos2pi(turns - llpf_rint(turns) < 0.0 ? turns - llpf_rint(turns) + 1.0 : turns - llpf_rint(turns), &sn, &cs);
    out[0] = x[0] + dt * x[1];
    out[1] = x[1] + dt * (torque - g_over_l * sn - damp * x[1] * x[1] * x[1]);
}
static void pendulum_g(const llpf_model* m, const double* x, const double* u, double t, double* out) {
    (void)m; (void)u; (void)t;
    double sn, cs;
    const double turns = x[0] * 0.15915494309189535;
    llpf_sincos2pi(turns - llpf_rint(turns) < 0.0 ? turns - llpf_rint(turns) + 1.0 : turns - llpf_rint(turns), &sn, &cs);
    out[0] = sn;
}
/* twin 2: f(x) = x, g(x) = x_0^2 (tests/ukf_common.py: SQUARE_SRC) */
static void square_f(const llpf_model* m, const double* x, const double* u, double t, double* out) {
    (void)u; (void)t;
    for (int d = 0; d < m->nx; ++d) out[d] = x[d];
}
static void square_g(const llpf_model* m, const double* x, const double* u, double t, double* out) {
    (void)m; (void)u; (void)t;
    out[0] = x[0] * x[0];
}

static void dense(int nx, const double* Rp, double* out) {
    for (int r = 0; r < nx; ++r)
        for (int c = 0; c < nx; ++c) out[r * nx + c] = Rp[llpf_kf_idx(r, c)];
}

int ukf_host_run(int F, int nx, int ny, int nu, ukf_fn f, ukf_fn g, int twin, const llpf_model* models, const double* R1, const double* R2,
                 const double* w, double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0,
                 double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    if (twin == 1) { f = pendulum_f; g = pendulum_g; }
    if (twin == 2) { f = square_f; g = square_g; }
    if (!f || !g) return -2;
    const double gamma = w[0], wm0 = w[1], wc0 = w[2], wi = w[3];
    const double zero_u[LLPF_KF_MAXU] = {0.0};
    const int npt = LLPF_UKF_NPTS(nx);
    double P[LLPF_UKF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY)];
    for (int k = 0; k < F; ++k) {
        const llpf_model* m = models + k;
        for (int r = 0; r < nx; ++r)
            for (int c = 0; c <= r; ++c) P[LLPF_UKF_OFF_R1 + llpf_kf_idx(r, c)] = R1[((size_t)k * nx + r) * nx + c];
        for (int r = 0; r < ny; ++r)
            for (int c = 0; c <= r; ++c) P[LLPF_UKF_OFF_R2(nx) + llpf_kf_idx(r, c)] = R2[((size_t)k * ny + r) * ny + c];
        double x[LLPF_KF_MAXX], R[LLPF_KF_NP(LLPF_KF_MAXX)], Cf[LLPF_KF_NP(LLPF_KF_MAXX)], e[LLPF_KF_MAXY];
        double Z[LLPF_UKF_NPTS(LLPF_KF_MAXX) * LLPF_KF_MAXX], X[LLPF_KF_MAXX];
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
            if (!(y[0] == y[0])) {
                for (int r = 0; r < ny; ++r) e[r] = llpf_kf_nan();
            } else {
                const int ok = llpf_ukf_factor(nx, R, Cf);
                for (int i = 0; i < npt; ++i) {
                    llpf_ukf_point(nx, gamma, x, Cf, i, X);
                    g(m, X, u, tau, Z + i * ny);
                }
                ll = llpf_ukf_correct_finish(nx, ny, gamma, wm0, wc0, wi, P, 1, ok, Cf, Z, 1, y, x, R, e);
            }
            llt = llt + ll;
            if (ll_steps) ll_steps[tf] = ll;
            if (eo) memcpy(eo + tf * ny, e, sizeof(double) * ny);
            if (xto) memcpy(xto + tf * nx, x, sizeof(double) * nx);
            if (Rto) dense(nx, R, Rto + tf * nx * nx);
            {
                const int ok = llpf_ukf_factor(nx, R, Cf);
                for (int i = 0; i < npt; ++i) {
                    llpf_ukf_point(nx, gamma, x, Cf, i, X);
                    f(m, X, u, tau, Z + i * nx);
                }
                llpf_ukf_predict_finish(nx, wm0, wc0, wi, P, 1, ok, Z, 1, x, R);
            }
        }
        if (ll_total) ll_total[k] = llt;
        for (int i = 0; i < nx; ++i) x0[(size_t)k * nx + i] = x[i];
        dense(nx, R, P0 + (size_t)k * nx * nx);
    }
    return 0;
}
