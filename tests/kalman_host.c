/* kalman_host.c — a host build of csrc/shared/llpf_kalman.h (the device order of the Kalman bank and of its smoother), for the tests and
 * for tools/bench_kalman.py.  Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared kalman_host.c -o libkalman_host.so
 * The loops, the layouts and the optional outputs are those of tests/kf_host_frame.h.
 *
 * kf_host_run: T steps of F filters from x0, P0, exactly as llpf_kalman_bank_run after llpf_kalman_bank_set_state(x0, P0).  Matrices per
 * filter, row-major: A [F][nx][nx], B [F][nx][nu], C [F][ny][nx], D [F][ny][nu], R1 [F][nx][nx], R2 [F][ny][ny].
 * kf_host_smooth: the backward pass of F filters over the posterior xt, Rt of a forward pass, exactly as llpf_kalman_bank_smooth runs it
 * on the device. */
#include "kf_host_frame.h"

typedef struct {
    int nx, ny, nu;
    const double *A, *B, *C, *D, *R1, *R2;
    double P[LLPF_KF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY, LLPF_KF_MAXU)];
} kf_ctx;

static double kf_begin(void* ctx, int f) {
    kf_ctx* k = ctx;
    const int nx = k->nx, ny = k->ny, nu = k->nu;
    double* P = k->P;
    memset(P, 0, sizeof(k->P));
    for (int i = 0; i < nx * nx; ++i) P[LLPF_KF_OFF_A + i] = k->A[(size_t)f * nx * nx + i];
    for (int i = 0; i < ny * nx; ++i) P[LLPF_KF_OFF_C(nx) + i] = k->C[(size_t)f * ny * nx + i];
    kf_host_pack(nx, k->R1 + (size_t)f * nx * nx, P + LLPF_KF_OFF_R1(nx, ny));
    kf_host_pack(ny, k->R2 + (size_t)f * ny * ny, P + LLPF_KF_OFF_R2(nx, ny));
    for (int i = 0; i < nx * nu; ++i) P[LLPF_KF_OFF_B(nx, ny) + i] = k->B[(size_t)f * nx * nu + i];
    for (int i = 0; i < ny * nu; ++i) P[LLPF_KF_OFF_D(nx, ny, nu) + i] = k->D[(size_t)f * ny * nu + i];
    return 0.0;      /* constant matrices: no tau */
}
static double kf_correct(void* ctx, const double* u, const double* y, double tau, double* x, double* R, double* e, int* done) {
    const kf_ctx* k = ctx;
    (void)tau; (void)done;
    return llpf_kf_correct(k->nx, k->ny, k->nu, k->P, 1, u, y, x, R, e);
}
static void kf_predict(void* ctx, const double* u, double tau, double* x, double* R) {
    const kf_ctx* k = ctx;
    (void)tau;
    llpf_kf_predict(k->nx, k->ny, k->nu, k->P, 1, u, x, R);
}
static void kf_smooth(void* ctx, const double* u, double tau, const double* xf, const double* Rf, double* xs, double* Rs) {
    const kf_ctx* k = ctx;
    (void)tau;
    llpf_kf_smooth(k->nx, k->ny, k->nu, k->P, 1, u, xf, Rf, xs, Rs);
}
static const kf_host_family kf_family = {kf_begin, kf_correct, kf_predict, kf_smooth};

static int kf_dims_ok(int nx, int ny, int nu) {
    return nx >= 1 && nx <= LLPF_KF_MAXX && ny >= 1 && ny <= LLPF_KF_MAXY && nu >= 0 && nu <= LLPF_KF_MAXU;
}

int kf_host_run(int F, int nx, int ny, int nu, const double* A, const double* B, const double* C, const double* D, const double* R1,
                const double* R2, double* x0, double* P0, const double* U, const double* Y, int64_t T, int per_filter,
                double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro, double* Rto, double* eo) {
    if (!kf_dims_ok(nx, ny, nu)) return -1;
    kf_ctx k = {nx, ny, nu, A, B, C, D, R1, R2, {0.0}};
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .U = U, .Y = Y, .x0 = x0, .P0 = P0,
                           .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto, .e = eo};
    kf_host_forward(&io, &kf_family, &k);
    return 0;
}

int kf_host_smooth(int F, int nx, int ny, int nu, const double* A, const double* B, const double* C, const double* D, const double* R1,
                   const double* R2, const double* U, int64_t T, int per_filter, const double* xt, const double* Rt, double* xTo,
                   double* RTo) {
    if (!kf_dims_ok(nx, ny, nu) || T < 1) return -1;
    kf_ctx k = {nx, ny, nu, A, B, C, D, R1, R2, {0.0}};
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .U = U, .post_x = xt, .post_R = Rt,
                           .xT = xTo, .RT = RTo};
    kf_host_backward(&io, &kf_family, &k);
    return 0;
}
