/* ukf_smooth_host.c — a host build of llpf_ukf_smooth_finish (csrc/shared/llpf_ukf.h, the device order of the unscented bank's smoother)
 * around a dynamics function given as a pointer, for the tests and for tools/bench_ukf.py --smooth.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include ukf_smooth_host.c -o libukf_smooth_host.so
 *
 * ukf_host_smooth: the backward pass of F filters over the posterior of a forward pass (tests/ukf_host.c: ukf_host_run), exactly as
 * llpf_ukf_bank_smooth runs it on the device.  f: the dynamics (model, x, u, tau, out) — the address of the oracle's orc_dynamics — or
 * NULL with `twin` naming one of the C twins below of the tests' device snippets (the twins of tests/ukf_host.c).  models [F] are the
 * llpf_model descriptors; R1 [F][nx][nx] dense row-major (the lower triangle is read); w = gamma, wm0, wc0, wi.  U [T][nu] or [F][T][nu]
 * (per_filter bit 0); step t runs at tau = (t_index0 + t) * models[f].Ts.  xt [T][F][nx], Rt [T][F][nx][nx] the posterior of every step
 * (the lower triangle of Rt is read).  Outputs time-major as the device writes them: xT [T][F][nx], RT [T][F][nx][nx]. */
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
/* twin 2: f(x) = x (tests/ukf_common.py: SQUARE_SRC) */
static void square_f(const llpf_model* m, const double* x, const double* u, double t, double* out) {
    (void)u; (void)t;
    for (int d = 0; d < m->nx; ++d) out[d] = x[d];
}

int ukf_host_smooth(int F, int nx, int nu, ukf_fn f, int twin, const llpf_model* models, const double* R1, const double* w, const double* U,
                    int64_t T, int per_filter, double t_index0, const double* xt, const double* Rt, double* xTo, double* RTo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || nu < 0 || nu > LLPF_KF_MAXU || T < 1) return -1;
    if (twin == 1) f = pendulum_f;
    if (twin == 2) f = square_f;
    if (!f) return -2;
    const double gamma = w[0], wm0 = w[1], wc0 = w[2], wi = w[3];
    const double zero_u[LLPF_KF_MAXU] = {0.0};
    const int npt = LLPF_UKF_NPTS(nx);
    double P[LLPF_KF_NP(LLPF_KF_MAXX)];
    for (int k = 0; k < F; ++k) {
        const llpf_model* m = models + k;
        for (int r = 0; r < nx; ++r)
            for (int c = 0; c <= r; ++c) P[LLPF_UKF_OFF_R1 + llpf_kf_idx(r, c)] = R1[((size_t)k * nx + r) * nx + c];
        double xs[LLPF_KF_MAXX], Rs[LLPF_KF_NP(LLPF_KF_MAXX)], xf[LLPF_KF_MAXX], Rf[LLPF_KF_NP(LLPF_KF_MAXX)], Cf[LLPF_KF_NP(LLPF_KF_MAXX)];
        double Z[LLPF_UKF_NPTS(LLPF_KF_MAXX) * LLPF_KF_MAXX], X[LLPF_KF_MAXX];
        for (int64_t t = T - 1; t >= 0; --t) {
            const size_t tf = (size_t)t * F + k;
            for (int i = 0; i < nx; ++i) xf[i] = xt[tf * nx + i];
            for (int r = 0; r < nx; ++r)
                for (int c = 0; c <= r; ++c) Rf[llpf_kf_idx(r, c)] = Rt[(tf * nx + r) * nx + c];
            if (t == T - 1) {                                   /* xT[T] = xt[T], RT[T] = Rt[T] */
                memcpy(xs, xf, sizeof(double) * nx);
                memcpy(Rs, Rf, sizeof(double) * LLPF_KF_NP(nx));
            } else {
                const double* u = nu > 0 ? U + ((per_filter & 1) ? ((size_t)k * T + t) : (size_t)t) * nu : zero_u;
                const double tau = (t_index0 + (double)t) * m->Ts;
                const int ok = llpf_ukf_factor(nx, Rf, Cf);
                for (int i = 0; i < npt; ++i) {
                    llpf_ukf_point(nx, gamma, xf, Cf, i, X);
                    f(m, X, u, tau, Z + i * nx);
                }
                llpf_ukf_smooth_finish(nx, gamma, wm0, wc0, wi, P, 1, ok, Cf, Z, 1, xf, Rf, xs, Rs);
            }
            if (xTo) memcpy(xTo + tf * nx, xs, sizeof(double) * nx);
            if (RTo)
                for (int r = 0; r < nx; ++r)
                    for (int c = 0; c < nx; ++c) RTo[(tf * nx + r) * nx + c] = Rs[llpf_kf_idx(r, c)];
        }
    }
    return 0;
}
