/* imm_host.c — a host build of csrc/shared/llpf_imm.h (the device order of the IMM bank), for the tests and for tools/bench_imm.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared imm_host.c -o libimm_host.so
 * The layouts of inputs and of the per-step outputs are those of tests/kf_host_frame.h; where the device fetches mode i from lane i, the
 * loops here read mode i's arrays.
 *
 * imm_host_run: T steps of F IMMs of M modes from (mu, xm, Rm), exactly as llpf_imm_bank_run after llpf_imm_bank_set_state.  Matrices per
 * filter and mode, row-major: A [F][M][nx][nx], B [F][M][nx][nu], C [F][M][ny][nx], D [F][M][ny][nu], R1 [F][M][nx][nx],
 * R2 [F][M][ny][ny]; P [F][M][M]; the state mu [F][M], xm [F][M][nx], Rm [F][M][nx][nx] (lower triangles read) is overwritten with the
 * final one.  Outputs, each optional: ll_total [F], ll_steps [T][F], x, xt [T][F][nx], R, Rt [T][F][nx][nx], mu_o, ll_modes [T][F][M]. */
#include "kf_host_frame.h"
#include "llpf_imm.h"

#define NPAR LLPF_KF_NPAR(LLPF_KF_MAXX, LLPF_KF_MAXY, LLPF_KF_MAXU)
#define NPK LLPF_KF_NP(LLPF_KF_MAXX)

/* the combined estimate of the state as it stands: x = sum_j mu_j x_j, R = sum_j mu_j (R_j + (x_j - x)(x_j - x)') */
static void imm_combine(int M, int nx, const double* mu, double xs[][LLPF_KF_MAXX], double Rs[][NPK], double* x, double* R) {
    for (int r = 0; r < nx; ++r) x[r] = 0.0;
    for (int i = 0; i < LLPF_KF_NP(nx); ++i) R[i] = 0.0;
    for (int i = 0; i < M; ++i) llpf_imm_mean_add(nx, mu[i], xs[i], x);
    for (int i = 0; i < M; ++i) llpf_imm_cov_add(nx, mu[i], xs[i], Rs[i], x, R);
}

int imm_host_run(int F, int M, int nx, int ny, int nu, int interact, const double* A, const double* B, const double* C, const double* D,
                 const double* R1, const double* R2, const double* P, double* mu0, double* xm0, double* Rm0, const double* U,
                 const double* Y, int64_t T, int per_filter, double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro,
                 double* Rto, double* muo, double* llmo) {
    if (!(nx >= 1 && nx <= LLPF_KF_MAXX && ny >= 1 && ny <= LLPF_KF_MAXY && nu >= 0 && nu <= LLPF_KF_MAXU && M >= 1 && M <= LLPF_IMM_MAXM))
        return -1;
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .U = U, .Y = Y};
    const int np = LLPF_KF_NP(nx);
    for (int f = 0; f < F; ++f) {
        double par[LLPF_IMM_MAXM][NPAR], xs[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rs[LLPF_IMM_MAXM][NPK], mu[LLPF_IMM_MAXM];
        const double* Pf = P + (size_t)f * M * M;
        for (int j = 0; j < M; ++j) {
            const size_t fj = (size_t)f * M + j;
            double* p = par[j];
            memset(p, 0, sizeof(par[j]));
            for (int i = 0; i < nx * nx; ++i) p[LLPF_KF_OFF_A + i] = A[fj * nx * nx + i];
            for (int i = 0; i < ny * nx; ++i) p[LLPF_KF_OFF_C(nx) + i] = C[fj * ny * nx + i];
            kf_host_pack(nx, R1 + fj * nx * nx, p + LLPF_KF_OFF_R1(nx, ny));
            kf_host_pack(ny, R2 + fj * ny * ny, p + LLPF_KF_OFF_R2(nx, ny));
            for (int i = 0; i < nx * nu; ++i) p[LLPF_KF_OFF_B(nx, ny) + i] = B[fj * nx * nu + i];
            for (int i = 0; i < ny * nu; ++i) p[LLPF_KF_OFF_D(nx, ny, nu) + i] = D[fj * ny * nu + i];
            memcpy(xs[j], xm0 + fj * nx, sizeof(double) * nx);
            kf_host_pack(nx, Rm0 + fj * nx * nx, Rs[j]);
            mu[j] = mu0[fj];
        }
        double llt = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const size_t tf = (size_t)t * F + f;
            const double* u = kf_host_u(&io, f, t);
            const double* y = kf_host_row(Y, per_filter & 2, f, T, t, ny);
            double xc[LLPF_KF_MAXX], Rc[NPK], e[LLPF_KF_MAXY];
            /* 1. the combined prior */
            if (xo || Ro) imm_combine(M, nx, mu, xs, Rs, xc, Rc);
            if (xo) memcpy(xo + tf * nx, xc, sizeof(double) * nx);
            if (Ro) kf_host_dense(nx, Rc, Ro + tf * nx * nx);
            /* 2. correct! of every mode */
            double llj[LLPF_IMM_MAXM], c[LLPF_IMM_MAXM], a[LLPF_IMM_MAXM], w[LLPF_IMM_MAXM];
            for (int j = 0; j < M; ++j) llj[j] = llpf_kf_correct(nx, ny, nu, par[j], 1, u, y, xs[j], Rs[j], e);
            /* 3. the mode probabilities */
            for (int j = 0; j < M; ++j) {
                c[j] = 0.0;
                for (int i = 0; i < M; ++i) c[j] = llpf_imm_c_add(Pf[i * M + j], mu[i], c[j]);
            }
            double ll = 0.0;
            if (!(y[0] == y[0])) {
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
            /* 6. predict! of every mode */
            for (int j = 0; j < M; ++j) llpf_kf_predict(nx, ny, nu, par[j], 1, u, xs[j], Rs[j]);
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

/* the combined estimate x [F][nx], R [F][nx][nx] of a state (mu, xm, Rm), as llpf_imm_bank_get_state forms it */
int imm_host_combine(int F, int M, int nx, const double* mu, const double* xm, const double* Rm, double* x, double* R) {
    if (!(nx >= 1 && nx <= LLPF_KF_MAXX && M >= 1 && M <= LLPF_IMM_MAXM)) return -1;
    for (int f = 0; f < F; ++f) {
        double xs[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rs[LLPF_IMM_MAXM][NPK], xc[LLPF_KF_MAXX], Rc[NPK];
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
