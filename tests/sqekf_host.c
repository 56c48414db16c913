/* sqekf_host.c — a host build of csrc/shared/llpf_sqekf.h (the device order of the square-root extended Kalman bank), for the tests and
 * for tools/bench_sqekf.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include sqekf_host.c -o libsqekf_host.so
 * The loops, the layouts and the optional outputs are those of tests/kf_host_frame.h; the frame's packed "R" is the factor Lr here, and
 * what the frame stores as R and Rt (the mirrored factor) is replaced by llpf_sq_cov of it afterwards, as tests/sqkf_host.c does.
 * The models — their kinds EKF_LG / EKF_QUADTANK / EKF_PENDULUM / EKF_SQUARE, the context and the two functions that evaluate value and
 * Jacobian — are those of tests/ekf_host.c, included here as it stands (its entry points come along and are not used).
 *
 * sqekf_host_run: T steps of F filters, exactly as llpf_sqekf_bank_run after llpf_sqekf_bank_set_state: ekf_host_run's arguments, then
 * state_is_factor and Rfin.  R1, R2 are the covariances, factored here with llpf_kf_chol as the bank's pack does.  The state: x0 [F][nx]
 * and P0 [F][nx][nx], which is a covariance (factored with llpf_kf_chol, as set_state(x, R) does) or, with state_is_factor, the dense
 * factor whose lower triangle is taken (set_state(x, L)).  On return x0 is the final x, P0 the final dense factor (zeros above the
 * diagonal) and Rfin [F][nx][nx] (optional) llpf_sq_cov of it.  Returns 0, a negative number as ekf_host_run, or 1 + f for the first
 * filter with a factorisation that failed (nothing is run then). */
#include "ekf_host.c"
#include "llpf_sqekf.h"

static int sqekf_fill(ekf_ctx* k, int f) {
    double inv[LLPF_KF_MAXX];
    kf_host_pack(k->nx, k->R1 + (size_t)f * k->nx * k->nx, k->P + LLPF_EKF_OFF_R1);
    kf_host_pack(k->ny, k->R2 + (size_t)f * k->ny * k->ny, k->P + LLPF_EKF_OFF_R2(k->nx));
    int ok = llpf_kf_chol(k->nx, k->P + LLPF_EKF_OFF_R1, inv);
    ok &= llpf_kf_chol(k->ny, k->P + LLPF_EKF_OFF_R2(k->nx), inv);
    return ok;
}
static double sqekf_begin(void* ctx, int f) {
    ekf_ctx* k = ctx;
    k->m = k->models + f;
    sqekf_fill(k, f);
    return k->m->Ts;
}
static double sqekf_correct(void* ctx, const double* u, const double* y, double tau, double* x, double* Lr, double* e, int* done) {
    ekf_ctx* k = ctx;
    (void)done;
    if (llpf_ekf_missing(y)) {
        for (int r = 0; r < k->ny; ++r) e[r] = llpf_kf_nan();
        return 0.0;
    }
    measurement_jac(k, x, u, tau, k->val, k->J);
    return llpf_sqekf_correct(k->nx, k->ny, k->P, 1, y, k->val, k->J, k->nx, x, Lr, e);
}
static void sqekf_predict(void* ctx, const double* u, double tau, double* x, double* Lr) {
    ekf_ctx* k = ctx;
    dynamics_jac(k, x, u, tau, k->val, k->J);
    llpf_sqekf_predict(k->nx, k->P, 1, k->val, k->J, k->nx, x, Lr);
}
static const kf_host_family sqekf_family = {sqekf_begin, sqekf_correct, sqekf_predict, NULL};

/* a dense matrix whose lower triangle is a factor -> the dense covariance, in place */
static void sqekf_cov_dense(int nx, double* dense) {
    double Lr[LLPF_KF_NP(LLPF_KF_MAXX)], R[LLPF_KF_NP(LLPF_KF_MAXX)];
    kf_host_pack(nx, dense, Lr);
    llpf_sq_cov(nx, Lr, R);
    kf_host_dense(nx, R, dense);
}
/* the dense lower Cholesky factor of a dense covariance, in place (llpf_kf_chol; zeros above the diagonal); 1 when positive definite */
static int sqekf_chol_dense(int n, double* R) {
    double Lp[LLPF_KF_NP(LLPF_KF_MAXX)], inv[LLPF_KF_MAXX];
    kf_host_pack(n, R, Lp);
    const int ok = llpf_kf_chol(n, Lp, inv);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) R[r * n + c] = c <= r ? Lp[llpf_kf_idx(r, c)] : 0.0;
    return ok;
}

int sqekf_host_run(int F, int nx, int ny, int nu, ekf_fn f, ekf_fn g, int kind, const llpf_model* models, const double* R1, const double* R2,
                   double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter, double t_index0, double* ll_total,
                   double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo, int state_is_factor, double* Rfin) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU) return -1;
    if (kind == EKF_LG && (!f || !g)) return -2;
    if (kind == EKF_QUADTANK && (nx != 4 || ny != 2 || nu != 2)) return -3;
    if (kind == EKF_PENDULUM && (nx != 2 || ny != 1)) return -3;
    if (kind == EKF_SQUARE && ny != 1) return -3;
    ekf_ctx k = {.nx = nx, .ny = ny, .kind = kind, .f = f, .g = g, .models = models, .R1 = R1, .R2 = R2};
    for (int i = 0; i < F; ++i) {
        if (!sqekf_fill(&k, i)) return 1 + i;
        if (!state_is_factor && !sqekf_chol_dense(nx, P0 + (size_t)i * nx * nx)) return 1 + i;
    }
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .Y = Y,
                           .x0 = x0, .P0 = P0, .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto, .e = eo};
    kf_host_forward(&io, &sqekf_family, &k);
    for (size_t i = 0; i < (size_t)T * F; ++i) {
        if (Ro) sqekf_cov_dense(nx, Ro + i * nx * nx);
        if (Rto) sqekf_cov_dense(nx, Rto + i * nx * nx);
    }
    for (int i = 0; i < F; ++i) {
        double* Lf = P0 + (size_t)i * nx * nx;
        if (Rfin) {
            memcpy(Rfin + (size_t)i * nx * nx, Lf, sizeof(double) * nx * nx);
            sqekf_cov_dense(nx, Rfin + (size_t)i * nx * nx);
        }
        for (int r = 0; r < nx; ++r)
            for (int c = r + 1; c < nx; ++c) Lf[r * nx + c] = 0.0;
    }
    return 0;
}
