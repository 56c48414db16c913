/* imm_host.c — a host build of csrc/shared/llpf_imm.h (the device order of the IMM bank), for the tests and for tools/bench_imm.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared imm_host.c -o libimm_host.so
 * The six-stage loop, the layouts of inputs and of the per-step outputs are those of tests/kf_host_frame.h (kf_host_imm); the modes are
 * kalman_host.c's family over the flat [F * M] arrays, and that file is part of this one.
 *
 * imm_host_run: T steps of F IMMs of M modes from (mu, xm, Rm), exactly as llpf_imm_bank_run after llpf_imm_bank_set_state.  Matrices per
 * filter and mode, row-major: A [F][M][nx][nx], B [F][M][nx][nu], C [F][M][ny][nx], D [F][M][ny][nu], R1 [F][M][nx][nx],
 * R2 [F][M][ny][ny]; P [F][M][M]; the state mu [F][M], xm [F][M][nx], Rm [F][M][nx][nx] (lower triangles read) is overwritten with the
 * final one.  Outputs, each optional: ll_total [F], ll_steps [T][F], x, xt [T][F][nx], R, Rt [T][F][nx][nx], mu_o, ll_modes [T][F][M]. */
#include "kalman_host.c"

int imm_host_run(int F, int M, int nx, int ny, int nu, int interact, const double* A, const double* B, const double* C, const double* D,
                 const double* R1, const double* R2, const double* P, double* mu0, double* xm0, double* Rm0, const double* U,
                 const double* Y, int64_t T, int per_filter, double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro,
                 double* Rto, double* muo, double* llmo) {
    if (!(kf_dims_ok(nx, ny, nu) && M >= 1 && M <= LLPF_IMM_MAXM)) return -1;
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .U = U, .Y = Y, .ll_total = ll_total,
                           .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto};
    const kf_host_imm_io imm = {.M = M, .interact = interact, .P = P, .mu = mu0, .xm = xm0, .Rm = Rm0, .mu_steps = muo, .ll_modes = llmo};
    kf_ctx k[LLPF_IMM_MAXM];
    for (int j = 0; j < M; ++j) k[j] = (kf_ctx){nx, ny, nu, A, B, C, D, R1, R2, {0.0}};
    kf_host_imm(&io, &kf_family, k, sizeof(kf_ctx), &imm);
    return 0;
}

/* the combined estimate x [F][nx], R [F][nx][nx] of a state (mu, xm, Rm), as llpf_imm_bank_get_state forms it */
int imm_host_combine(int F, int M, int nx, const double* mu, const double* xm, const double* Rm, double* x, double* R) {
    if (!(nx >= 1 && nx <= LLPF_KF_MAXX && M >= 1 && M <= LLPF_IMM_MAXM)) return -1;
    for (int f = 0; f < F; ++f) {
        double xs[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rs[LLPF_IMM_MAXM][KF_HOST_NPK], xc[LLPF_KF_MAXX], Rc[KF_HOST_NPK];
        for (int j = 0; j < M; ++j) {
            memcpy(xs[j], xm + ((size_t)f * M + j) * nx, sizeof(double) * nx);
            kf_host_pack(nx, Rm + ((size_t)f * M + j) * nx * nx, Rs[j]);
        }
        imm_combine(M, nx, mu + (size_t)f * M, xs, Rs, xc, Rc);
        memcpy(x + (size_t)f * nx, xc, sizeof(double) * nx);
        kf_host_dense(nx, Rc, R + (size_t)f * nx * nx);
    }
    return 0;
}
