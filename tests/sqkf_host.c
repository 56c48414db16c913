/* sqkf_host.c — a host build of csrc/shared/llpf_sqkf.h (the device order of the square-root Kalman bank), for the tests.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared sqkf_host.c -o libsqkf_host.so
 * The loops, the layouts and the optional outputs are those of tests/kf_host_frame.h; the frame's packed "R" is the factor Lr here, and
 * what the frame stores as R and Rt (the mirrored factor) is replaced by llpf_sq_cov of it afterwards.
 *
 * sqkf_host_run: T steps of F filters, exactly as llpf_sqkf_bank_run after llpf_sqkf_bank_set_state.  Matrices per filter as
 * kf_host_run takes them; R1, R2 are the covariances, factored here with llpf_kf_chol as the bank's pack does.  The state: x0 [F][nx] and
 * P0 [F][nx][nx], which is a covariance (factored with llpf_kf_chol, as set_state(x, R) does) or, with state_is_factor, the dense
 * factor whose lower triangle is taken (set_state(x, L)).  On return x0 is the final x, P0 the final dense factor (zeros above the
 * diagonal) and Rfin [F][nx][nx] (optional) llpf_sq_cov of it.  Returns 0, or 1 + f for the first filter with a factorisation that
 * failed (nothing is run then). */
#include "kf_host_frame.h"
#include "llpf_sqkf.h"

typedef struct {
    int nx, ny, nu;
    const double *A, *B, *C, *D, *R1, *R2;
    double P[LLPF_KF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY, LLPF_KF_MAXU)];
} sq_ctx;

static int sq_fill(sq_ctx* k, int f) {
    const int nx = k->nx, ny = k->ny, nu = k->nu;
    double* P = k->P;
    double inv[LLPF_KF_MAXX];
    memset(P, 0, sizeof(k->P));
    for (int i = 0; i < nx * nx; ++i) P[LLPF_KF_OFF_A + i] = k->A[(size_t)f * nx * nx + i];
    for (int i = 0; i < ny * nx; ++i) P[LLPF_KF_OFF_C(nx) + i] = k->C[(size_t)f * ny * nx + i];
    kf_host_pack(nx, k->R1 + (size_t)f * nx * nx, P + LLPF_KF_OFF_R1(nx, ny));
    kf_host_pack(ny, k->R2 + (size_t)f * ny * ny, P + LLPF_KF_OFF_R2(nx, ny));
    int ok = llpf_kf_chol(nx, P + LLPF_KF_OFF_R1(nx, ny), inv);
    ok &= llpf_kf_chol(ny, P + LLPF_KF_OFF_R2(nx, ny), inv);
    for (int i = 0; i < nx * nu; ++i) P[LLPF_KF_OFF_B(nx, ny) + i] = k->B[(size_t)f * nx * nu + i];
    for (int i = 0; i < ny * nu; ++i) P[LLPF_KF_OFF_D(nx, ny, nu) + i] = k->D[(size_t)f * ny * nu + i];
    return ok;
}
static double sq_begin(void* ctx, int f) {
    sq_fill(ctx, f);
    return 0.0;      /* constant matrices: no tau */
}
static double sq_correct(void* ctx, const double* u, const double* y, double tau, double* x, double* Lr, double* e, int* done) {
    const sq_ctx* k = ctx;
    (void)tau; (void)done;
    return llpf_sq_correct(k->nx, k->ny, k->nu, k->P, 1, u, y, x, Lr, e);
}
static void sq_predict(void* ctx, const double* u, double tau, double* x, double* Lr) {
    const sq_ctx* k = ctx;
    (void)tau;
    llpf_sq_predict(k->nx, k->ny, k->nu, k->P, 1, u, x, Lr);
}
static const kf_host_family sq_family = {sq_begin, sq_correct, sq_predict, 0};

/* a dense matrix whose lower triangle is a factor -> the dense covariance, in place */
static void sq_cov_dense(int nx, double* dense) {
    double Lr[LLPF_KF_NP(LLPF_KF_MAXX)], R[LLPF_KF_NP(LLPF_KF_MAXX)];
    kf_host_pack(nx, dense, Lr);
    llpf_sq_cov(nx, Lr, R);
    kf_host_dense(nx, R, dense);
}

/* the dense lower Cholesky factor of the dense covariance R (llpf_kf_chol; zeros above the diagonal); returns 1 when positive definite */
int sqkf_host_chol(int n, const double* R, double* L) {
    double Lp[LLPF_KF_NP(LLPF_KF_MAXX)], inv[LLPF_KF_MAXX];
    if (n < 1 || n > LLPF_KF_MAXX) return -1;
    kf_host_pack(n, R, Lp);
    const int ok = llpf_kf_chol(n, Lp, inv);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) L[r * n + c] = c <= r ? Lp[llpf_kf_idx(r, c)] : 0.0;
    return ok;
}

int sqkf_host_run(int F, int nx, int ny, int nu, const double* A, const double* B, const double* C, const double* D, const double* R1,
                  const double* R2, double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter,
                  int state_is_factor, double* Rfin, double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro, double* Rto,
                  double* eo) {
    if (!(nx >= 1 && nx <= LLPF_KF_MAXX && ny >= 1 && ny <= LLPF_KF_MAXY && nu >= 0 && nu <= LLPF_KF_MAXU)) return -1;
    sq_ctx k = {nx, ny, nu, A, B, C, D, R1, R2, {0.0}};
    for (int f = 0; f < F; ++f) {
        if (!sq_fill(&k, f)) return 1 + f;
        if (!state_is_factor && !sqkf_host_chol(nx, P0 + (size_t)f * nx * nx, P0 + (size_t)f * nx * nx)) return 1 + f;
    }
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .U = U, .Y = Y, .x0 = x0, .P0 = P0,
                           .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto, .e = eo};
    kf_host_forward(&io, &sq_family, &k);
    for (size_t i = 0; i < (size_t)T * F; ++i) {
        if (Ro) sq_cov_dense(nx, Ro + i * nx * nx);
        if (Rto) sq_cov_dense(nx, Rto + i * nx * nx);
    }
    for (int f = 0; f < F; ++f) {
        double* Lf = P0 + (size_t)f * nx * nx;
        if (Rfin) {
            memcpy(Rfin + (size_t)f * nx * nx, Lf, sizeof(double) * nx * nx);
            sq_cov_dense(nx, Rfin + (size_t)f * nx * nx);
        }
        for (int r = 0; r < nx; ++r)
            for (int c = r + 1; c < nx; ++c) Lf[r * nx + c] = 0.0;
    }
    return 0;
}
