/* aukf_host.c — a host build of csrc/shared/llpf_aukf.h (the device order of the bank of unscented Kalman filters with augmented process
 * noise) around model functions given as pointers, for the tests and for tools/bench_aukf.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include aukf_host.c -o libaukf_host.so
 * The loops, the layouts and the optional outputs are those of tests/kf_host_frame.h.
 *
 * aukf_host_run: T steps of F filters from x0, P0, exactly as llpf_aukf_bank_run after llpf_aukf_bank_set_state(x0, P0).  f / g: dynamics
 * and measurement (model, x, u, tau, out) without a noise argument — the tests pass the addresses of the oracle's orc_dynamics /
 * orc_measurement — and the filter takes them as additive (the noise points reuse the centre's value, as the device does for a model
 * without dynamics_w); or NULL with `twin` naming one of the C twins below of the tests' device snippets, which form their own noise.
 * models [F] are the llpf_model descriptors; w = the measurement set gamma, wm0, wc0, wi, then the dynamics set. */
#include "llpf.h"
#include "llpf_aukf.h"
#include "kf_host_frame.h"

typedef void (*aukf_fn)(const llpf_model* m, const double* x, const double* u, double t, double* out);
typedef void (*aukf_fw)(const llpf_model* m, const double* x, const double* u, double t, const double* w, double* out);

/* twin 1: the pendulum of tests/ekf_common.py with its torque carrying w[0] and its damping multiplied by (1 + w[1])
 * (tests/aukf_common.py: NOISY_PENDULUM_SRC): the same expressions through the same llpf_sincos2pi / llpf_rint */
static void pendulum_sin(const double* x, double* sn) {
    double cs;
    const double turns = x[0] * 0.15915494309189535;
    llpf_sincos2pi(turns - llpf_rint(turns) < 0.0 ? turns - llpf_rint(turns) + 1.0 : turns - llpf_rint(turns), sn, &cs);
}
static void noisy_pendulum_f(const llpf_model* m, const double* x, const double* u, double t, const double* w, double* out) {
    (void)t;
    const double g_over_l = m->qt[0], damp = m->qt[1], dt = m->Ts, torque = (m->nu > 0 && u) ? u[0] : 0.0;
    double sn;
    pendulum_sin(x, &sn);
    out[0] = x[0] + dt * x[1];
    out[1] = x[1] + dt * ((torque + w[0]) - g_over_l * sn - damp * (1.0 + w[1]) * x[1] * x[1] * x[1]);
}
static void pendulum_g(const llpf_model* m, const double* x, const double* u, double t, double* out) {
    (void)m; (void)u; (void)t;
    pendulum_sin(x, out);
}
/* twin 2: x' = a x (1 + w) + w^2 with a = qt[0], g(x) = x^2 (tests/aukf_common.py: MULT_SRC) */
static void mult_f(const llpf_model* m, const double* x, const double* u, double t, const double* w, double* out) {
    (void)u; (void)t;
    const double a = m->qt[0];
    out[0] = a * x[0] * (1.0 + w[0]) + w[0] * w[0];
}
static void mult_g(const llpf_model* m, const double* x, const double* u, double t, double* out) {
    (void)m; (void)u; (void)t;
    out[0] = x[0] * x[0];
}

/* twins 3 and 4, the known answers of one predict!: x' = x + w^2, and x' = a x (1 + w) */
static void square_noise_f(const llpf_model* m, const double* x, const double* u, double t, const double* w, double* out) {
    (void)m; (void)u; (void)t;
    out[0] = x[0] + w[0] * w[0];
}
static void mult_only_f(const llpf_model* m, const double* x, const double* u, double t, const double* w, double* out) {
    (void)u; (void)t;
    out[0] = m->qt[0] * x[0] * (1.0 + w[0]);
}

typedef struct {
    int nx, ny;
    aukf_fn f, g;                      /* f: an additive model's dynamics (fw null) */
    aukf_fw fw;                        /* a model's dynamics_w */
    const llpf_model *models, *m;      /* m: the filter in hand */
    const double *R1, *R2;
    double gamma, wm0, wc0, wi, gamma_a, wm0a, wc0a, wia;
    int ok1;
    double P[LLPF_UKF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY)];
    double Cf[LLPF_KF_NP(LLPF_KF_MAXX)], C1[LLPF_KF_NP(LLPF_KF_MAXX)], Z[LLPF_AUKF_NPTS(LLPF_KF_MAXX) * LLPF_KF_MAXX];
} aukf_ctx;

static double aukf_begin(void* ctx, int f) {
    aukf_ctx* k = ctx;
    k->m = k->models + f;
    kf_host_pack(k->nx, k->R1 + (size_t)f * k->nx * k->nx, k->P + LLPF_UKF_OFF_R1);
    kf_host_pack(k->ny, k->R2 + (size_t)f * k->ny * k->ny, k->P + LLPF_UKF_OFF_R2(k->nx));
    k->ok1 = llpf_aukf_noise_factor(k->nx, k->P, 1, k->C1);       /* once per filter, before the time loop */
    return k->m->Ts;
}
/* llpf_ukf.h's correct!, call for call, with the measurement set */
static double aukf_correct(void* ctx, const double* u, const double* y, double tau, double* x, double* R, double* e, int* done) {
    aukf_ctx* k = ctx;
    (void)done;
    if (!(y[0] == y[0])) {
        for (int r = 0; r < k->ny; ++r) e[r] = llpf_kf_nan();
        return 0.0;
    }
    double X[LLPF_KF_MAXX];
    const int ok = llpf_ukf_factor(k->nx, R, k->Cf);
    for (int i = 0; i < LLPF_UKF_NPTS(k->nx); ++i) {
        llpf_ukf_point(k->nx, k->gamma, x, k->Cf, i, X);
        k->g(k->m, X, u, tau, k->Z + i * k->ny);
    }
    return llpf_ukf_correct_finish(k->nx, k->ny, k->gamma, k->wm0, k->wc0, k->wi, k->P, 1, ok, k->Cf, k->Z, 1, y, x, R, e);
}
static void aukf_predict(void* ctx, const double* u, double tau, double* x, double* R) {
    aukf_ctx* k = ctx;
    const int nx = k->nx;
    double X[LLPF_KF_MAXX], W[LLPF_KF_MAXX];
    const int ok = llpf_ukf_factor(nx, R, k->Cf) & k->ok1;
    for (int i = 0; i < LLPF_AUKF_NPTS(nx); ++i) {
        const int noise = llpf_aukf_point(nx, k->gamma_a, x, k->Cf, k->C1, i, X, W);
        if (k->fw) k->fw(k->m, X, u, tau, W, k->Z + i * nx);
        else if (noise) llpf_aukf_additive(nx, k->Z, W, k->Z + i * nx);      /* Z[0 ..]: f at the centre, not yet centred */
        else k->f(k->m, X, u, tau, k->Z + i * nx);
    }
    llpf_aukf_predict_finish(nx, k->wm0a, k->wc0a, k->wia, ok, k->Z, 1, x, R);
}
static const kf_host_family aukf_family = {aukf_begin, aukf_correct, aukf_predict, 0};

int aukf_host_run(int F, int nx, int ny, int nu, aukf_fn f, aukf_fn g, int twin, const llpf_model* models, const double* R1, const double* R2,
                  const double* w, double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0,
                  double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    aukf_ctx k;
    k.fw = 0;
    if (twin == 1) { k.fw = noisy_pendulum_f; g = pendulum_g; }
    if (twin == 2) { k.fw = mult_f; g = mult_g; }
    if (twin == 3) { k.fw = square_noise_f; g = mult_g; }
    if (twin == 4) { k.fw = mult_only_f; g = mult_g; }
    if ((!f && !k.fw) || !g) return -2;
    k.nx = nx; k.ny = ny; k.f = f; k.g = g; k.models = models; k.R1 = R1; k.R2 = R2;
    k.gamma = w[0]; k.wm0 = w[1]; k.wc0 = w[2]; k.wi = w[3];
    k.gamma_a = w[4]; k.wm0a = w[5]; k.wc0a = w[6]; k.wia = w[7];
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .Y = Y,
                           .x0 = x0, .P0 = P0, .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto, .e = eo};
    kf_host_forward(&io, &aukf_family, &k);
    return 0;
}
