/* imm_ukf_host.c — a host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_ukf.h (the device order of the IMM bank whose modes are
 * unscented Kalman filters, kernels/imm_ukf.hpp), for the tests and for tools/bench_imm.py --unscented.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include imm_ukf_host.c -o libimm_ukf_host.so
 * The loop is kf_host_imm of tests/kf_host_frame.h, the one imm_host.c runs, over ukf_host.c's family: stage 2 maps the sigma points of
 * the mode's prior through the measurement and ends in llpf_ukf_correct_finish (skipped at a missing row: ll_j = 0), stage 6 maps those of
 * the mode's x, R after the mixing through the dynamics and ends in llpf_ukf_predict_finish.  The models are ukf_host.c's: the caller's
 * f / g (the oracle's functions for the built-in models) or one of its twins (the pendulum, x0^2).  Both files are part of this one, so
 * the library also has ukf_host_run, imm_host_run and imm_host_combine, built with the same flags.
 *
 * imm_ukf_host_run: T steps of F IMMs of M modes from (mu, xm, Rm), exactly as llpf_imm_bank_run_at after llpf_imm_bank_set_state on a
 * bank of llpf_imm_bank_create_unscented.  models [F][M] are the llpf_model descriptors of the modes; R1 [F][M][nx][nx],
 * R2 [F][M][ny][ny] dense; w = gamma, wm0, wc0, wi, the bank's; P [F][M][M]; the state mu [F][M], xm [F][M][nx], Rm [F][M][nx][nx]
 * (lower triangles read) is overwritten with the final one.  Step t runs at tau = (t_index0 + t) * Ts with Ts that of the first
 * descriptor (the bank's).  Outputs as imm_host_run's. */
#include "ukf_host.c"
#include "imm_host.c"

int imm_ukf_host_run(int F, int M, int nx, int ny, int nu, int interact, ukf_fn fn_f, ukf_fn fn_g, int twin, const llpf_model* models,
                     const double* R1, const double* R2, const double* w, const double* P, double* mu0, double* xm0, double* Rm0,
                     const double* U, const double* Y, int64_t T, int per_filter, double t_index0, double* ll_total, double* ll_steps,
                     double* xo, double* xto, double* Ro, double* Rto, double* muo, double* llmo) {
    if (!(nx >= 1 && nx <= LLPF_KF_MAXX && ny >= 1 && ny <= LLPF_KF_MAXY && nu >= 0 && nu <= LLPF_KF_MAXU && M >= 1 && M <= LLPF_IMM_MAXM))
        return -1;
    if (twin == 1 && (nx != 2 || ny != 1)) return -3;
    if (twin == 2 && ny != 1) return -3;
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .t_index0 = t_index0, .U = U, .Y = Y,
                           .ll_total = ll_total, .ll_steps = ll_steps, .x = xo, .xt = xto, .R = Ro, .Rt = Rto};
    const kf_host_imm_io imm = {.M = M, .interact = interact, .P = P, .Ts = models[0].Ts, .mu = mu0, .xm = xm0, .Rm = Rm0, .mu_steps = muo,
                                .ll_modes = llmo};
    ukf_ctx ctxs[LLPF_IMM_MAXM];
    for (int j = 0; j < M; ++j) {
        const int rc = ukf_ctx_set(&ctxs[j], nx, ny, fn_f, fn_g, twin, models, R1, R2, w);
        if (rc) return rc;
    }
    kf_host_imm(&io, &ukf_family, ctxs, sizeof(ukf_ctx), &imm);
    return 0;
}
