/* ekf_host.c — a host build of csrc/shared/llpf_ekf.h (the device order of the extended Kalman bank, plain and iterated) and of
 * csrc/shared/llpf_quadtank_jac.h, for the tests and for tools/bench_ekf.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include ekf_host.c -o libekf_host.so
 * The loops, the layouts and the optional outputs are those of tests/kf_host_frame.h.
 *
 * ekf_host_run: T steps of F filters from x0, P0, exactly as llpf_ekf_bank_run after llpf_ekf_bank_set_state(x0, P0).  kind names the
 * model and where value and Jacobian come from:
 *   EKF_LG        the linear-Gaussian model: the value through f / g (model, x, u, tau, out) — the tests pass the oracle's orc_dynamics /
 *                 orc_measurement, the device's LinGauss in the device's order — and the Jacobians are the descriptor's A, C
 *   EKF_QUADTANK  the quad-tank: llpf_qt_dynamics_jac of the shared header (value and Jacobian), the two unit rows for the measurement
 *   EKF_PENDULUM  the C twin of the tests' pendulum snippet with its hand-written members (tests/ekf_common.py: PENDULUM_JAC_SRC)
 *   EKF_SQUARE    f(x) = x, g(x) = x_0^2 (SQUARE_JAC_SRC)
 * models [F] are the llpf_model descriptors (Ts among them).
 * iekf_host_run: the same bank after llpf_ekf_bank_set_iterations (llpf_iekf_iterate, llpf_iekf_stop): ekf_host_run's arguments, then
 * maxiters >= 1, epsilon >= 0 and iters [T][F] (optional): the number of linearisations of the measurement that step t of filter f ran,
 * 0 at a missing row — reported here for the tests only, the C ABI has no such output. */
#include "llpf.h"
#include "llpf_ekf.h"
#include "llpf_quadtank_jac.h"
#include "kf_host_frame.h"

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

typedef struct {
    int nx, ny, kind;
    ekf_fn f, g;
    const llpf_model *models, *m;      /* m: the filter in hand */
    const double *R1, *R2;
    int maxiters;                      /* of the iterated filter */
    double epsilon;
    double P[LLPF_EKF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY)];
    double val[LLPF_KF_MAXX], J[LLPF_KF_MAXX * LLPF_KF_MAXX];
} ekf_ctx;

/* gx = g(x) and J = dg/dx at x */
static void measurement_jac(const ekf_ctx* k, const double* x, const double* u, double tau, double* gx, double* J) {
    const int nx = k->nx, ny = k->ny;
    if (k->kind == EKF_LG) {
        k->g(k->m, x, u, tau, gx);
        for (int i = 0; i < ny * nx; ++i) J[i] = k->m->C[i];
    } else if (k->kind == EKF_QUADTANK) {
        gx[0] = x[0]; gx[1] = x[1];
        for (int i = 0; i < 8; ++i) J[i] = 0.0;
        J[0] = 1.0; J[5] = 1.0;
    } else if (k->kind == EKF_PENDULUM) {
        pendulum_g_jac(x, gx, J);
    } else {
        gx[0] = x[0] * x[0];
        J[0] = x[0] + x[0];
        for (int i = 1; i < nx; ++i) J[i] = 0.0;
    }
}
/* fx = f(x) and J = df/dx at x */
static void dynamics_jac(const ekf_ctx* k, const double* x, const double* u, double tau, double* fx, double* J) {
    const int nx = k->nx;
    if (k->kind == EKF_LG) {
        k->f(k->m, x, u, tau, fx);
        for (int i = 0; i < nx * nx; ++i) J[i] = k->m->A[i];
    } else if (k->kind == EKF_QUADTANK) {
        ekf_host_qt_jac(k->m, u, tau, x, fx, J);
    } else if (k->kind == EKF_PENDULUM) {
        pendulum_f_jac(k->m, x, u, fx, J);
    } else {
        for (int r = 0; r < nx; ++r) {
            fx[r] = x[r];
            for (int c = 0; c < nx; ++c) J[r * nx + c] = r == c ? 1.0 : 0.0;
        }
    }
}

static double ekf_begin(void* ctx, int f) {
    ekf_ctx* k = ctx;
    k->m = k->models + f;
    kf_host_pack(k->nx, k->R1 + (size_t)f * k->nx * k->nx, k->P + LLPF_EKF_OFF_R1);
    kf_host_pack(k->ny, k->R2 + (size_t)f * k->ny * k->ny, k->P + LLPF_EKF_OFF_R2(k->nx));
    return k->m->Ts;
}
static double ekf_correct(void* ctx, const double* u, const double* y, double tau, double* x, double* R, double* e, int* done) {
    ekf_ctx* k = ctx;
    (void)done;
    if (llpf_ekf_missing(y)) {
        for (int r = 0; r < k->ny; ++r) e[r] = llpf_kf_nan();
        return 0.0;
    }
    measurement_jac(k, x, u, tau, k->val, k->J);
    return llpf_ekf_correct(k->nx, k->ny, k->P, 1, y, k->val, k->J, k->nx, x, R, e);
}
static double iekf_correct(void* ctx, const double* u, const double* y, double tau, double* x, double* R, double* e, int* done) {
    ekf_ctx* k = ctx;
    const int nx = k->nx;
    if (llpf_ekf_missing(y)) {
        for (int r = 0; r < k->ny; ++r) e[r] = llpf_kf_nan();
        return 0.0;
    }
    double xi[LLPF_KF_MAXX], Rn[LLPF_KF_NP(LLPF_KF_MAXX)], move, ll;
    for (int i = 0; i < nx; ++i) xi[i] = x[i];
    do {
        measurement_jac(k, xi, u, tau, k->val, k->J);
        ll = llpf_iekf_iterate(nx, k->ny, k->P, 1, y, k->val, k->J, nx, x, R, *done == 0, xi, Rn, e, &move);
        ++*done;
    } while (!llpf_iekf_stop(*done, k->maxiters, move, k->epsilon));
    for (int i = 0; i < nx; ++i) x[i] = xi[i];
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = Rn[i];
    return ll;
}
static void ekf_predict(void* ctx, const double* u, double tau, double* x, double* R) {
    ekf_ctx* k = ctx;
    dynamics_jac(k, x, u, tau, k->val, k->J);
    llpf_ekf_predict(k->nx, k->P, 1, k->val, k->J, k->nx, x, R);
}
static const kf_host_family ekf_family = {ekf_begin, ekf_correct, ekf_predict, NULL};
static const kf_host_family iekf_family = {ekf_begin, iekf_correct, ekf_predict, NULL};

static int ekf_run(const kf_host_family* fam, const kf_host_io* io, ekf_fn f, ekf_fn g, int kind, const llpf_model* models, const double* R1,
                   const double* R2, int maxiters, double epsilon) {
    const int nx = io->nx, ny = io->ny, nu = io->nu;
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    if (kind == EKF_LG && (!f || !g)) return -2;
    if (kind == EKF_QUADTANK && (nx != 4 || ny != 2 || nu != 2)) return -3;
    if (kind == EKF_PENDULUM && (nx != 2 || ny != 1)) return -3;
    if (kind == EKF_SQUARE && ny != 1) return -3;
    if (fam == &iekf_family && (maxiters < 1 || maxiters > LLPF_IEKF_MAXITERS || !(epsilon >= 0.0))) return -4;
    ekf_ctx k = {.nx = nx, .ny = ny, .kind = kind, .f = f, .g = g, .models = models, .R1 = R1, .R2 = R2, .maxiters = maxiters,
                 .epsilon = epsilon};
    kf_host_forward(io, fam, &k);
    return 0;
}

int ekf_host_run(int F, int nx, int ny, int nu, ekf_fn f, ekf_fn g, int kind, const llpf_model* models, const double* R1, const double* R2,
                 double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0, double* ll_total,
                 double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo) {
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .Y = Y,
                           .x0 = x0, .P0 = P0, .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto, .e = eo};
    return ekf_run(&ekf_family, &io, f, g, kind, models, R1, R2, 0, 0.0);
}

int iekf_host_run(int F, int nx, int ny, int nu, ekf_fn f, ekf_fn g, int kind, const llpf_model* models, const double* R1, const double* R2,
                  double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0, double* ll_total,
                  double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo, int maxiters, double epsilon,
                  int32_t* iters) {
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .Y = Y,
                           .x0 = x0, .P0 = P0, .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto, .e = eo,
                           .iters = iters};
    return ekf_run(&iekf_family, &io, f, g, kind, models, R1, R2, maxiters, epsilon);
}
