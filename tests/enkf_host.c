/* enkf_host.c — a host build of csrc/shared/llpf_enkf.h (the device order of the ensemble Kalman bank) around llpf_philox.h, for the tests
 * and for tools/bench_enkf.py.
 * Build: cc -O2 -ffp-contract=off -shared -fPIC -I <csrc>/shared -I <root>/include enkf_host.c -o libenkf_host.so
 * Layouts and optional outputs are those of tests/kf_host_frame.h; the ensembles are X [F][N][nx] (llpf_enkf_bank_get_members' layout),
 * in and out.
 *
 * enkf_host_init: the members a reset! draws (counter n_reset) from the Gaussian initial density, exactly as k_enkf_init.
 * enkf_host_run:  T steps of F filters from X, exactly as llpf_enkf_bank_run / _correct / _predict (phases) after
 *                 llpf_enkf_bank_set_members(X) on a bank whose step counter is step0.  kind names the model:
 *   ENKF_ORACLE    f / g (model, x, u, tau, out) are passed in — the tests pass the oracle's orc_dynamics / orc_measurement, the device's
 *                  LinGauss and QuadTank in the device's order
 *   ENKF_PENDULUM  the C twin of the tests' pendulum snippet (tests/user_models.py: PENDULUM_SRC, tests/ekf_common.py: PENDULUM_JAC_SRC)
 *   ENKF_SQUARE    f(x) = x, g(x) = x_0^2
 *   ENKF_LINEAR    g(x) = C x in the order of the tests' linear snippets (tests/user_models.py: _LINEAR_PART), f likewise: for models
 *                  whose process noise is the snippet's own only correct! (phases = 1) is twinned
 * gs (gaussian, xi, out) samples a Gaussian descriptor from standard normals in the device's order: the tests pass orc_gauss_sample.
 * Filter f's key is seed + f.  state_x [F][nx], state_R [F][nx][nx]: mean and sample covariance of the final members. */
#include <stdlib.h>

#include "llpf.h"
#include "llpf_enkf.h"
#include "llpf_philox.h"
#include "kf_host_frame.h"

enum { ENKF_ORACLE = 0, ENKF_PENDULUM = 2, ENKF_SQUARE = 3, ENKF_LINEAR = 4 };
typedef void (*enkf_fn)(const llpf_model* m, const double* x, const double* u, double t, double* out);
typedef void (*enkf_gs)(const llpf_gaussian* g, const double* xi, double* out);

static void pendulum_sincos(const double* x, double* sn, double* cs) {
    const double turns = x[0] * 0.15915494309189535;
    llpf_sincos2pi(turns - llpf_rint(turns) < 0.0 ? turns - llpf_rint(turns) + 1.0 : turns - llpf_rint(turns), sn, cs);
}

typedef struct {
    int nx, ny, kind;
    enkf_fn f, g;
    const llpf_model* m;
} enkf_model;

static void measurement(const enkf_model* k, const double* x, const double* u, double tau, double* out) {
    const llpf_model* m = k->m;
    if (k->kind == ENKF_ORACLE) {
        k->g(m, x, u, tau, out);
    } else if (k->kind == ENKF_PENDULUM) {
        double sn, cs;
        pendulum_sincos(x, &sn, &cs);
        out[0] = sn;
    } else if (k->kind == ENKF_SQUARE) {
        out[0] = x[0] * x[0];
    } else {
        for (int r = 0; r < k->ny; ++r) {
            double cx = m->C[r * k->nx + 0] * x[0];
            for (int c = 1; c < k->nx; ++c) cx = cx + m->C[r * k->nx + c] * x[c];
            out[r] = cx;
        }
    }
}
static void dynamics(const enkf_model* k, const double* x, const double* u, double tau, double* out) {
    const llpf_model* m = k->m;
    if (k->kind == ENKF_ORACLE) {
        k->f(m, x, u, tau, out);
    } else if (k->kind == ENKF_PENDULUM) {
        const double g_over_l = m->qt[0], damp = m->qt[1], dt = m->Ts, torque = (m->nu > 0 && u) ? u[0] : 0.0;
        double sn, cs;
        pendulum_sincos(x, &sn, &cs);
        out[0] = x[0] + dt * x[1];
        out[1] = x[1] + dt * (torque - g_over_l * sn - damp * x[1] * x[1] * x[1]);
    } else if (k->kind == ENKF_SQUARE) {
        for (int r = 0; r < k->nx; ++r) out[r] = x[r];
    } else {
        const int nx = k->nx, nu = m->nu;
        for (int r = 0; r < nx; ++r) {
            double ax = m->A[r * nx + 0] * x[0];
            for (int c = 1; c < nx; ++c) ax = ax + m->A[r * nx + c] * x[c];
            if (nu > 0) {
                double acc = m->B[r * nu + 0] * u[0];
                for (int c = 1; c < nu; ++c) acc = acc + m->B[r * nu + c] * u[c];
                ax = ax + acc;
            }
            out[r] = ax;
        }
    }
}

/* mean [nx] and packed sample covariance [np] (either NULL) of the members X [N][nx]; tmp [N] */
static void moments(int nx, int N, const double* X, double* tmp, double* xbar, double* Rp) {
    double mean[LLPF_KF_MAXX];
    for (int d = 0; d < nx; ++d) mean[d] = llpf_enkf_mean(llpf_enkf_sum(X + d, N, nx), N);
    if (xbar)
        for (int d = 0; d < nx; ++d) xbar[d] = mean[d];
    if (!Rp) return;
    for (int r = 0; r < nx; ++r)
        for (int c = 0; c <= r; ++c) {
            for (int i = 0; i < N; ++i) tmp[i] = (X[(size_t)i * nx + r] - mean[r]) * (X[(size_t)i * nx + c] - mean[c]);
            Rp[llpf_kf_idx(r, c)] = llpf_enkf_cov(llpf_enkf_sum(tmp, N, 1), N);
        }
}

double enkf_host_sum(const double* v, int64_t n) { return llpf_enkf_sum(v, n, 1); }

int enkf_host_init(int F, int nx, int N, enkf_gs gs, const llpf_model* models, uint64_t seed, uint32_t n_reset, double* X) {
    if (nx < 1 || nx > LLPF_KF_MAXX || N < 1 || !gs) return -1;
    for (int f = 0; f < F; ++f) {
        const uint64_t key = seed + (uint64_t)f;
        for (int i = 0; i < N; ++i) {
            double xi[LLPF_KF_MAXX];
            llpf_normals((uint32_t)i, n_reset, LLPF_STREAM_INIT, (uint32_t)key, (uint32_t)(key >> 32), nx, xi);
            gs(&models[f].initial_density, xi, X + ((size_t)f * N + i) * nx);
        }
    }
    return 0;
}

int enkf_host_run(int F, int nx, int ny, int nu, enkf_fn fdyn, enkf_fn gmeas, enkf_gs gs, int kind, const llpf_model* models, const double* R2,
                  double* X, int N, uint64_t seed, uint32_t step0, double rho, int phases, const double* U, const double* Y, int64_t T,
                  int per_filter, double t_index0, double* ll_total, double* ll_steps, double* xo, double* xto, double* Ro, double* Rto,
                  double* eo, double* state_x, double* state_R) {
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU || N < 2 || !gs) return -1;
    if (kind == ENKF_ORACLE && (!fdyn || !gmeas)) return -2;
    if (kind == ENKF_PENDULUM && (nx != 2 || ny != 1)) return -3;
    if (kind == ENKF_SQUARE && ny != 1) return -3;
    const kf_host_io io = {.F = F, .nx = nx, .ny = ny, .nu = nu, .T = T, .per_filter = per_filter, .U = U};
    const int np = LLPF_KF_NP(nx), npy = LLPF_KF_NP(ny);
    double* Yv = malloc(sizeof(double) * (size_t)N * ny);
    double* tmp = malloc(sizeof(double) * (size_t)N);
    if (!Yv || !tmp) { free(Yv); free(tmp); return -5; }
    for (int f = 0; f < F; ++f) {
        enkf_model k = {.nx = nx, .ny = ny, .kind = kind, .f = fdyn, .g = gmeas, .m = models + f};
        const llpf_model* m = k.m;
        const uint64_t key = seed + (uint64_t)f;
        const uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
        double P[LLPF_KF_NP(LLPF_KF_MAXX) + LLPF_KF_NP(LLPF_KF_MAXY)] = {0.0};
        kf_host_pack(ny, R2 + (size_t)f * ny * ny, P + LLPF_ENKF_OFF_R2(nx));
        double* Xf = X + (size_t)f * N * nx;
        double llt = 0.0;
        for (int64_t t = 0; t < T; ++t) {
            const size_t tf = (size_t)t * F + f;
            const double* u = kf_host_u(&io, f, t);
            const double* y = kf_host_row(Y, per_filter & 2, f, T, t, ny);
            const double tau = (t_index0 + (double)t) * m->Ts;
            const uint32_t step = step0 + (uint32_t)t;
            const int missing = !(phases & LLPF_ENKF_CORRECT) || !(y[0] == y[0]);
            double e[LLPF_KF_MAXY], ll = 0.0, Rp[LLPF_KF_NP(LLPF_KF_MAXX)], xbar[LLPF_KF_MAXX];
            if (xo || Ro) {
                moments(nx, N, Xf, tmp, xbar, Ro ? Rp : NULL);
                if (xo) memcpy(xo + tf * nx, xbar, sizeof(double) * nx);
                if (Ro) kf_host_dense(nx, Rp, Ro + tf * nx * nx);
            }
            if (missing) {
                for (int r = 0; r < ny; ++r) e[r] = llpf_kf_nan();
            } else {
                double ybar[LLPF_KF_MAXY], sxy[LLPF_KF_MAXY * LLPF_KF_MAXX], syy[LLPF_KF_NP(LLPF_KF_MAXY)];
                double L[LLPF_KF_NP(LLPF_KF_MAXY)], inv[LLPF_KF_MAXY], W[LLPF_KF_MAXY * LLPF_KF_MAXX];
                int ok = 1;
                for (int i = 0; i < N; ++i) measurement(&k, Xf + (size_t)i * nx, u, tau, Yv + (size_t)i * ny);
                moments(nx, N, Xf, tmp, xbar, NULL);
                for (int r = 0; r < ny; ++r) ybar[r] = llpf_enkf_mean(llpf_enkf_sum(Yv + r, N, ny), N);
                for (int r = 0; r < ny; ++r) {
                    for (int d = 0; d < nx; ++d) {
                        for (int i = 0; i < N; ++i) tmp[i] = (Xf[(size_t)i * nx + d] - xbar[d]) * (Yv[(size_t)i * ny + r] - ybar[r]);
                        sxy[r * LLPF_KF_MAXX + d] = llpf_enkf_sum(tmp, N, 1);
                    }
                    for (int c = 0; c <= r; ++c) {
                        for (int i = 0; i < N; ++i) tmp[i] = (Yv[(size_t)i * ny + r] - ybar[r]) * (Yv[(size_t)i * ny + c] - ybar[c]);
                        syy[llpf_kf_idx(r, c)] = llpf_enkf_sum(tmp, N, 1);
                    }
                }
                (void)npy;
                ll = llpf_enkf_gain(nx, ny, N, P, 1, sxy, syy, y, ybar, L, inv, W, e, &ok);
                for (int i = 0; i < N; ++i) {
                    double xi[LLPF_KF_MAXY], v[LLPF_KF_MAXY];
                    llpf_normals((uint32_t)i, step, LLPF_STREAM_MEASURE, k0, k1, ny, xi);
                    gs(&m->measurement_density, xi, v);
                    llpf_enkf_member_update(nx, ny, ok, L, inv, W, y, Yv + (size_t)i * ny, v, Xf + (size_t)i * nx);
                }
            }
            llt = llt + ll;
            if (ll_steps) ll_steps[tf] = ll;
            if (eo) memcpy(eo + tf * ny, e, sizeof(double) * ny);
            if (xto || Rto) {
                moments(nx, N, Xf, tmp, xbar, Rto ? Rp : NULL);
                if (xto) memcpy(xto + tf * nx, xbar, sizeof(double) * nx);
                if (Rto) kf_host_dense(nx, Rp, Rto + tf * nx * nx);
            }
            if (phases & LLPF_ENKF_PREDICT) {
                for (int i = 0; i < N; ++i) {
                    double fx[LLPF_KF_MAXX], xi[LLPF_KF_MAXX], nz[LLPF_KF_MAXX];
                    double* x = Xf + (size_t)i * nx;
                    dynamics(&k, x, u, tau, fx);
                    llpf_normals((uint32_t)i, step, LLPF_STREAM_DYNAMICS, k0, k1, nx, xi);
                    gs(&m->dynamics_density, xi, nz);
                    for (int d = 0; d < nx; ++d) x[d] = fx[d] + nz[d];
                }
                if (rho != 1.0) {
                    moments(nx, N, Xf, tmp, xbar, NULL);
                    for (int i = 0; i < N; ++i) llpf_enkf_inflate(nx, rho, xbar, Xf + (size_t)i * nx);
                }
            }
        }
        if (ll_total) ll_total[f] = llt;
        {
            double xbar[LLPF_KF_MAXX], Rp[LLPF_KF_NP(LLPF_KF_MAXX)];
            moments(nx, N, Xf, tmp, xbar, Rp);
            if (state_x) memcpy(state_x + (size_t)f * nx, xbar, sizeof(double) * nx);
            if (state_R) kf_host_dense(nx, Rp, state_R + (size_t)f * nx * nx);
        }
        (void)np;
    }
    free(Yv);
    free(tmp);
    return 0;
}

#ifdef ENKF_HOST_MAIN
/* A stand-alone program around the twin for a sanitizer build (cc -fsanitize=address,undefined -DENKF_HOST_MAIN ... enkf_host.c -lm):
 * the square model with scalar covariances, every output, two steps with inflation, at the N given on the command line. */
#include <math.h>
#include <stdio.h>
static void main_gs(const llpf_gaussian* g, const double* xi, double* out) {
    for (int i = 0; i < g->dim; ++i) out[i] = sqrt(g->cov[0]) * xi[i] + g->mu[i];
}
int main(int argc, char** argv) {
    const int N = argc > 1 ? atoi(argv[1]) : 2, T = 3;
    llpf_model m;
    memset(&m, 0, sizeof(m));
    m.nx = 1; m.ny = 1; m.nu = 0; m.Ts = 1.0;
    llpf_gaussian* gd[3] = {&m.dynamics_density, &m.measurement_density, &m.initial_density};
    const double var[3] = {0.1, 0.25, 0.36};
    for (int k = 0; k < 3; ++k) { gd[k]->dim = 1; gd[k]->kind = LLPF_COV_SCAL; gd[k]->cov[0] = var[k]; }
    m.initial_density.mu[0] = 1.0;
    double* X = malloc(sizeof(double) * (size_t)N);
    const double R2 = 0.25, Y[3] = {3.0, llpf_kf_nan(), 2.5};
    double ll, lls[3], x[3], xt[3], R[3], Rt[3], e[3], sx, sR;
    if (!X || enkf_host_init(1, 1, N, main_gs, &m, 7, 0, X) != 0) return 2;
    const int rc = enkf_host_run(1, 1, 1, 0, NULL, NULL, main_gs, ENKF_SQUARE, &m, &R2, X, N, 7, 0, 1.5, LLPF_ENKF_CORRECT | LLPF_ENKF_PREDICT, NULL,
                                 Y, T, 0, 0.0, &ll, lls, x, xt, R, Rt, e, &sx, &sR);
    printf("N=%d rc=%d ll=%.17g mean=%.17g var=%.17g\n", N, rc, ll, sx, sR);
    free(X);
    return rc != 0 || !(ll == ll);
}
#endif
