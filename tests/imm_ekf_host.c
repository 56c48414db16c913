/* imm_ekf_host.c — a host build of csrc/shared/llpf_imm.h over csrc/shared/llpf_ekf.h (the device order of the IMM bank whose modes are
 * first-order extended Kalman filters, kernels/imm_ekf.hpp), for the tests and for tools/bench_imm.py --extended.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include imm_ekf_host.c -o libimm_ekf_host.so
 * The loop is imm_host.c's with two stages replaced: stage 2 is measurement_jac at the mode's prior followed by llpf_ekf_correct (skipped
 * at a missing row: ll_j = 0), stage 6 is dynamics_jac at the mode's x after the mixing followed by llpf_ekf_predict.  The models are
 * ekf_host.c's kinds (EKF_LG through the caller's f / g with A, C as Jacobians, EKF_QUADTANK through llpf_quadtank_jac.h, the pendulum
 * twin, x0^2), through that file's measurement_jac / dynamics_jac: both files are part of this one, so the library also has
 * ekf_host_run, imm_host_run and imm_host_combine, built with the same flags.
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
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .U = U, .Y = Y};
    const int np = LLPF_KF_NP(nx);
    const double Ts = models[0].Ts;
    for (int f = 0; f < F; ++f) {
        ekf_ctx k[LLPF_IMM_MAXM];
        double xs[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rs[LLPF_IMM_MAXM][NPK], mu[LLPF_IMM_MAXM];
        const double* Pf = P + (size_t)f * M * M;
        for (int j = 0; j < M; ++j) {
            const size_t fj = (size_t)f * M + j;
            k[j] = (ekf_ctx){.nx = nx, .ny = ny, .kind = kind, .f = fn_f, .g = fn_g, .models = models, .R1 = R1, .R2 = R2};
            ekf_begin(&k[j], (int)fj);                   /* the mode's descriptor and its packed R1, R2 */
            memcpy(xs[j], xm0 + fj * nx, sizeof(double) * nx);
            kf_host_pack(nx, Rm0 + fj * nx * nx, Rs[j]);
            mu[j] = mu0[fj];
        }
        double llt = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const size_t tf = (size_t)t * F + f;
            const double* u = kf_host_u(&io, f, t);
            const double* y = kf_host_row(Y, per_filter & 2, f, T, t, ny);
            const double tau = (t_index0 + (double)t) * Ts;
            const int missing = llpf_ekf_missing(y);
            double xc[LLPF_KF_MAXX], Rc[NPK], e[LLPF_KF_MAXY];
            /* 1. the combined prior */
            if (xo || Ro) imm_combine(M, nx, mu, xs, Rs, xc, Rc);
            if (xo) memcpy(xo + tf * nx, xc, sizeof(double) * nx);
            if (Ro) kf_host_dense(nx, Rc, Ro + tf * nx * nx);
            /* 2. correct! of every mode: one measurement_jac at the mode's prior */
            double llj[LLPF_IMM_MAXM], c[LLPF_IMM_MAXM], a[LLPF_IMM_MAXM], w[LLPF_IMM_MAXM];
            for (int j = 0; j < M; ++j) {
                llj[j] = 0.0;
                if (missing) continue;
                measurement_jac(&k[j], xs[j], u, tau, k[j].val, k[j].J);
                llj[j] = llpf_ekf_correct(nx, ny, k[j].P, 1, y, k[j].val, k[j].J, nx, xs[j], Rs[j], e);
            }
            /* 3. the mode probabilities */
            for (int j = 0; j < M; ++j) {
                c[j] = 0.0;
                for (int i = 0; i < M; ++i) c[j] = llpf_imm_c_add(Pf[i * M + j], mu[i], c[j]);
            }
            double ll = 0.0;
            if (missing) {
                for (int j = 0; j < M; ++j) mu[j] = c[j];
            } else {
                for (int j = 0; j < M; ++j) a[j] = llpf_imm_loga(c[j], llj[j]);
                double m = a[0];
                for (int i = 1; i < M; ++i) m = llpf_imm_max(m, a[i]);
                for (int j = 0; j < M; ++j) w[j] = llpf_imm_w(c[j], a[j], m);
                double s = 0.0;
                for (int i = 0; i < M; ++i) s = s + w[i];
                ll = llpf_imm_ll(m, s);
                for (int j = 0; j < M; ++j) {
                    mu[j] = w[j] / s;
                    llpf_imm_poison(nx, ll, xs[j], Rs[j]);
                }
            }
            llt = llt + ll;
            if (ll_steps) ll_steps[tf] = ll;
            if (muo) memcpy(muo + tf * M, mu, sizeof(double) * M);
            if (llmo) memcpy(llmo + tf * M, llj, sizeof(double) * M);
            /* 4. the combined posterior */
            if (xto || Rto) imm_combine(M, nx, mu, xs, Rs, xc, Rc);
            if (xto) memcpy(xto + tf * nx, xc, sizeof(double) * nx);
            if (Rto) kf_host_dense(nx, Rc, Rto + tf * nx * nx);
            /* 5. the mixing: every mode from the modes as they were */
            if (interact) {
                double xn[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rn[LLPF_IMM_MAXM][NPK];
                for (int j = 0; j < M; ++j) {
                    double cj = 0.0, wm[LLPF_IMM_MAXM];
                    for (int i = 0; i < M; ++i) cj = llpf_imm_c_add(Pf[i * M + j], mu[i], cj);
                    for (int i = 0; i < M; ++i) wm[i] = llpf_imm_mix_w(Pf[i * M + j], mu[i], cj);
                    for (int r = 0; r < nx; ++r) xn[j][r] = 0.0;
                    for (int i = 0; i < np; ++i) Rn[j][i] = 0.0;
                    for (int i = 0; i < M; ++i) llpf_imm_mean_add(nx, wm[i], xs[i], xn[j]);
                    for (int i = 0; i < M; ++i) llpf_imm_cov_add(nx, wm[i], xs[i], Rs[i], xn[j], Rn[j]);
                    if (cj == 0.0) {                    /* a mode without mass is not mixed */
                        memcpy(xn[j], xs[j], sizeof(double) * nx);
                        memcpy(Rn[j], Rs[j], sizeof(double) * np);
                    }
                }
                memcpy(xs, xn, sizeof(xs));
                memcpy(Rs, Rn, sizeof(Rs));
            }
            /* 6. predict! of every mode: one dynamics_jac at the mode's x after the mixing */
            for (int j = 0; j < M; ++j) {
                dynamics_jac(&k[j], xs[j], u, tau, k[j].val, k[j].J);
                llpf_ekf_predict(nx, k[j].P, 1, k[j].val, k[j].J, nx, xs[j], Rs[j]);
            }
        }
        if (ll_total) ll_total[f] = llt;
        for (int j = 0; j < M; ++j) {
            const size_t fj = (size_t)f * M + j;
            memcpy(xm0 + fj * nx, xs[j], sizeof(double) * nx);
            kf_host_dense(nx, Rs[j], Rm0 + fj * nx * nx);
            mu0[fj] = mu[j];
        }
    }
    return 0;
}
