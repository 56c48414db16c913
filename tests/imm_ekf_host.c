/* imm_ekf_host.c — a host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_ekf.h (the device order of the IMM bank whose modes are
 * first-order extended Kalman filters, kernels/imm_ekf.hpp), for the tests and for tools/bench_imm.py --extended.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include imm_ekf_host.c -o libimm_ekf_host.so
 * The loop is kf_host_imm of tests/kf_host_frame.h, the one imm_host.c runs, over ekf_host.c's family: stage 2 is measurement_jac at the
 * mode's prior followed by llpf_ekf_correct (skipped at a missing row: ll_j = 0), stage 6 is dynamics_jac at the mode's x after the mixing
 * followed by llpf_ekf_predict.  The models are ekf_host.c's kinds (EKF_LG through the caller's f / g with A, C as Jacobians, EKF_QUADTANK
 * through llpf_quadtank_jac.h, the pendulum twin, x0^2): both files are part of this one, so the library also has ekf_host_run,
 * imm_host_run and imm_host_combine, built with the same flags.
 *
 * imm_ekf_host_run: T steps of F IMMs of M modes from (mu, xm, Rm), exactly as llpf_imm_bank_run_at after llpf_imm_bank_set_state.
 * models [F][M] are the llpf_model descriptors of the modes; R1 [F][M][nx][nx], R2 [F][M][ny][ny] dense; P [F][M][M]; the state
 * mu [F][M], xm [F][M][nx], Rm [F][M][nx][nx] (lower triangles read) is overwritten with the final one.  Step t runs at
 * tau = (t_index0 + t) * Ts with Ts that of the first descriptor (the bank's).  Outputs as imm_host_run's. */
#include "ekf_host.c"
#include "imm_host.c"

int imm_ekf_host_run(int F, int M, int nx, int ny, int nu, int interact, ekf_fn fn_f, ekf_fn fn_g, int kind, const llpf_model* models,
                     const double* R1, const double* R2, const double* P, double* mu0, double* xm0, double* Rm0, const double* U,
                     const double* Y, int64_t T, int per_filter, double t_index0, double* ll_total, double* ll_steps, double* xo,
                     double* xto, double* Ro, double* Rto, double* muo, double* llmo) {
    if (!(nx >= 1 && nx <= LLPF_KF_MAXX && ny >= 1 && ny <= LLPF_KF_MAXY && nu >= 0 && nu <= LLPF_KF_MAXU && M >= 1 && M <= LLPF_IMM_MAXM))
        return -1;
    if (kind == EKF_LG && (!fn_f || !fn_g)) return -2;
    if (kind == EKF_QUADTANK && (nx != 4 || ny != 2 || nu != 2)) return -3;
    if (kind == EKF_PENDULUM && (nx != 2 || ny != 1)) return -3;
    if (kind == EKF_SQUARE && ny != 1) return -3;
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .Y = Y,
                           .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto};
    const kf_host_imm_io imm = {.M = M, .interact = interact, .P = P, .Ts = models[0].Ts, .mu = mu0, .xm = xm0, .Rm = Rm0, .mu_steps = muo,
                                .ll_modes = llmo};
    ekf_ctx k[LLPF_IMM_MAXM];
    for (int j = 0; j < M; ++j) k[j] = (ekf_ctx){.nx = nx, .ny = ny, .kind = kind, .f = fn_f, .g = fn_g, .models = models, .R1 = R1, .R2 = R2};
    kf_host_imm(&io, &ekf_family, k, sizeof(ekf_ctx), &imm);
    return 0;
}
