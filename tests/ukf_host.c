/* ukf_host.c — a host build of csrc/shared/llpf_ukf.h (the device order of the unscented Kalman bank and of its smoother) around model
 * functions given as pointers, for the tests and for tools/bench_ukf.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include ukf_host.c -o libukf_host.so
 * The loops, the layouts and the optional outputs are those of tests/kf_host_frame.h.
 *
 * ukf_host_run: T steps of F filters from x0, P0, exactly as llpf_ukf_bank_run after llpf_ukf_bank_set_state(x0, P0).  f / g: dynamics
 * and measurement (model, x, u, tau, out) — the tests pass the addresses of the oracle's orc_dynamics / orc_measurement, the device's
 * models in the device's order — or NULL with `twin` naming one of the C twins below of the tests' device snippets.  models [F] are the
 * llpf_model descriptors (the model's own parameters, Ts among them); w = gamma, wm0, wc0, wi.
 * ukf_host_smooth: the backward pass of F filters over the posterior xt, Rt of a forward pass, exactly as llpf_ukf_bank_smooth runs it
 * on the device; of the model it takes the dynamics only. */
#include "llpf.h"
#include "llpf_ukf.h"
#include "kf_host_frame.h"

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

typedef struct {
    int nx, ny;
    ukf_fn f, g;
    const llpf_model *models, *m;      /* m: the filter in hand */
    const double *R1, *R2;             /* R2 null: the smoother's, which reads R1 only */
    double gamma, wm0, wc0, wi;
    double P[LLPF_UKF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY)];
    double Cf[LLPF_KF_NP(LLPF_KF_MAXX)], Z[LLPF_UKF_NPTS(LLPF_KF_MAXX) * LLPF_KF_MAXX], X[LLPF_KF_MAXX];
} ukf_ctx;

/* 0, or the entry point's error; the model functions of a twin replace f / g */
static int ukf_ctx_set(ukf_ctx* k, int nx, int ny, ukf_fn f, ukf_fn g, int twin, const llpf_model* models, const double* R1, const double* R2,
                       const double* w) {
    if (twin == 1) { f = pendulum_f; g = pendulum_g; }
    if (twin == 2) { f = square_f; g = square_g; }
    if (!f || !g) return -2;
    k->nx = nx; k->ny = ny; k->f = f; k->g = g; k->models = models; k->R1 = R1; k->R2 = R2;
    k->gamma = w[0]; k->wm0 = w[1]; k->wc0 = w[2]; k->wi = w[3];
    return 0;
}
static double ukf_begin(void* ctx, int f) {
    ukf_ctx* k = ctx;
    k->m = k->models + f;
    kf_host_pack(k->nx, k->R1 + (size_t)f * k->nx * k->nx, k->P + LLPF_UKF_OFF_R1);
    if (k->R2) kf_host_pack(k->ny, k->R2 + (size_t)f * k->ny * k->ny, k->P + LLPF_UKF_OFF_R2(k->nx));
    return k->m->Ts;
}
/* Z = fn at the sigma points of (x, R), `dim` values each; returns llpf_ukf_factor's status */
static int ukf_propagate(ukf_ctx* k, ukf_fn fn, int dim, const double* u, double tau, const double* x, const double* R) {
    const int ok = llpf_ukf_factor(k->nx, R, k->Cf);
    for (int i = 0; i < LLPF_UKF_NPTS(k->nx); ++i) {
        llpf_ukf_point(k->nx, k->gamma, x, k->Cf, i, k->X);
        fn(k->m, k->X, u, tau, k->Z + i * dim);
    }
    return ok;
}
static double ukf_correct(void* ctx, const double* u, const double* y, double tau, double* x, double* R, double* e, int* done) {
    ukf_ctx* k = ctx;
    (void)done;
    if (!(y[0] == y[0])) {
        for (int r = 0; r < k->ny; ++r) e[r] = llpf_kf_nan();
        return 0.0;
    }
    const int ok = ukf_propagate(k, k->g, k->ny, u, tau, x, R);
    return llpf_ukf_correct_finish(k->nx, k->ny, k->gamma, k->wm0, k->wc0, k->wi, k->P, 1, ok, k->Cf, k->Z, 1, y, x, R, e);
}
static void ukf_predict(void* ctx, const double* u, double tau, double* x, double* R) {
    ukf_ctx* k = ctx;
    const int ok = ukf_propagate(k, k->f, k->nx, u, tau, x, R);
    llpf_ukf_predict_finish(k->nx, k->wm0, k->wc0, k->wi, k->P, 1, ok, k->Z, 1, x, R);
}
static void ukf_smooth(void* ctx, const double* u, double tau, const double* xf, const double* Rf, double* xs, double* Rs) {
    ukf_ctx* k = ctx;
    const int ok = ukf_propagate(k, k->f, k->nx, u, tau, xf, Rf);
    llpf_ukf_smooth_finish(k->nx, k->gamma, k->wm0, k->wc0, k->wi, k->P, 1, ok, k->Cf, k->Z, 1, xf, Rf, xs, Rs);
}
static const kf_host_family ukf_family = {ukf_begin, ukf_correct, ukf_predict, ukf_smooth};

int ukf_host_run(int F, int nx, int ny, int nu, ukf_fn f, ukf_fn g, int twin, const llpf_model* models, const double* R1, const double* R2,
                 const double* w, double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0,
                 double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    ukf_ctx k;
    const int rc = ukf_ctx_set(&k, nx, ny, f, g, twin, models, R1, R2, w);
    if (rc) return rc;
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .Y = Y,
                           .x0 = x0, .P0 = P0, .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto, .e = eo};
    kf_host_forward(&io, &ukf_family, &k);
    return 0;
}

int ukf_host_smooth(int F, int nx, int nu, ukf_fn f, int twin, const llpf_model* models, const double* R1, const double* w, const double* U,
                    int64_t T, int per_filter, double t_index0, const double* xt, const double* Rt, double* xTo, double* RTo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || nu < 0 || nu > LLPF_KF_MAXU || T < 1) return -1;
    ukf_ctx k;
    const int rc = ukf_ctx_set(&k, nx, 0, f, f, twin, models, R1, NULL, w);
    if (rc) return rc;
    const kf_host_io io = {.F = F, .nx = nx, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .post_x = xt,
                           .post_R = Rt, .xT = xTo, .RT = RTo};
    kf_host_backward(&io, &ukf_family, &k);
    return 0;
}
