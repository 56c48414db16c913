// host/imm.hpp — banks of interacting-multiple-model filters over Kalman filters with constant matrices (llpf_imm_bank_*; kernel:
// kernels/imm.hpp, step: shared/llpf_imm.h).  Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank is a KfBank (host/kfbank.hpp) whose columns are lanes: G = 1, 2 or 4 lanes per filter (the smallest G >= M), column f * G + j is
// mode j of filter f, L = F * G columns in all (those of the idle lanes j >= M stay zero).  par is [npar + LLPF_IMM_MAXM][L]: the mode's
// Kalman constants as host/kalman.hpp packs them, then column j of the filter's transition matrix; the state is [nx + np + 2][L]: the
// mode's x, packed R, mu_j and the run's running ll_total (the same number in every lane of a filter).  A run goes through the chunked
// staging pipeline of host/pipe.hpp like kf_forward, with this bank's own outputs.  The combined estimate of get_state is formed on the
// host from the downloaded state, by the functions of shared/llpf_imm.h the kernel forms it with.

namespace llpf {
#include "../kernels/imm_args.hpp"
}

struct llpf_imm_bank : KfBank {
    int M = 0, G = 0, L = 0, interact = 1;
    llpf_imm_bank() : KfBank("imm") {}
};

static int imm_group(int M) { return M <= 1 ? 1 : M == 2 ? 2 : 4; }

// models [F][M] (+ D [F][M][ny][nu] or NULL), P [F][M][M], mu0 [F][M] -> the SoA constants and initial state; every check that needs no device
static int imm_pack(const llpf_model* models, const double* D, const double* P, const double* mu0, int32_t F, int32_t M, int& nx, int& ny,
                    int& nu, std::vector<double>& par, std::vector<double>& init) {
    if (!models) return fail(LLPF_ERR_ARG, "imm: models is null");
    if (!P || !mu0) return fail(LLPF_ERR_ARG, "imm: P and mu0 must both be given");
    if (F < 1) return fail(LLPF_ERR_ARG, "imm: n_filters must be >= 1");
    if (M < 1 || M > LLPF_IMM_MAXM) return fail(LLPF_ERR_ARG, "imm: n_modes must be in 1..4");
    nx = models[0].nx; ny = models[0].ny; nu = models[0].nu;
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU)
        return fail(LLPF_ERR_ARG, "imm: nx must be in 1..8, ny in 1..4 and nu in 0..8");
    const int G = imm_group(M), L = F * G;
    const int np = LLPF_KF_NP(nx), npar = LLPF_KF_NPAR(nx, ny, nu), nstate = nx + np + 2;
    par.assign((size_t)(npar + LLPF_IMM_MAXM) * L, 0.0);
    init.assign((size_t)nstate * L, 0.0);
    for (int f = 0; f < F; ++f) {
        const std::string atf = "imm: filter " + std::to_string(f) + ": ";
        const double* Pf = P + (size_t)f * M * M;
        const double* mf = mu0 + (size_t)f * M;
        double smu = 0.0;
        for (int i = 0; i < M; ++i) {
            double srow = 0.0;
            for (int j = 0; j < M; ++j) {
                if (!(Pf[i * M + j] >= 0.0)) return fail(LLPF_ERR_ARG, atf + "row " + std::to_string(i) + " of P has a negative (or NaN) entry");
                srow += Pf[i * M + j];
            }
            if (!(fabs(srow - 1.0) <= 1e-12)) return fail(LLPF_ERR_ARG, atf + "row " + std::to_string(i) + " of P does not sum to 1");
            if (!(mf[i] >= 0.0)) return fail(LLPF_ERR_ARG, atf + "mu0 of mode " + std::to_string(i) + " is negative (or NaN)");
            smu += mf[i];
        }
        if (!(fabs(smu - 1.0) <= 1e-12)) return fail(LLPF_ERR_ARG, atf + "mu0 does not sum to 1");
        for (int j = 0; j < M; ++j) {
            const llpf_model& m = models[(size_t)f * M + j];
            const std::string at = "imm: filter " + std::to_string(f) + ", mode " + std::to_string(j) + ": ";
            const int col = f * G + j;
            if (m.model_id != LLPF_MODEL_LINEAR_GAUSSIAN) return fail(LLPF_ERR_ARG, at + "model_id must be LLPF_MODEL_LINEAR_GAUSSIAN");
            if (m.nx != nx || m.ny != ny || m.nu != nu) return fail(LLPF_ERR_ARG, at + "dimensions differ from those of filter 0, mode 0");
            CHK(kf_pack_filter(m, at, col, L, nx, ny, LLPF_KF_OFF_R1(nx, ny), LLPF_KF_OFF_R2(nx, ny), par, init));
            GaussD gd;                                // positive definiteness of R2 and P0, as the Kalman bank checks them
            if (gauss_prepare(&m.measurement_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
            if (gauss_prepare(&m.initial_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
            auto put = [&](int e, double v) { par[(size_t)e * L + col] = v; };
            for (int i = 0; i < nx * nx; ++i) put(LLPF_KF_OFF_A + i, m.A[i]);
            for (int i = 0; i < ny * nx; ++i) put(LLPF_KF_OFF_C(nx) + i, m.C[i]);
            for (int i = 0; i < nx * nu; ++i) put(LLPF_KF_OFF_B(nx, ny) + i, m.B[i]);
            for (int i = 0; i < ny * nu; ++i) put(LLPF_KF_OFF_D(nx, ny, nu) + i, D ? D[((size_t)f * M + j) * ny * nu + i] : 0.0);
            for (int i = 0; i < M; ++i) put(npar + i, Pf[i * M + j]);
            init[(size_t)(nx + np) * L + col] = mf[j];
        }
    }
    return LLPF_OK;
}

static int imm_create(int32_t device, const llpf_model* models, const double* D, const double* P, const double* mu0, int32_t F, int32_t M,
                      int32_t flags, llpf_imm_bank& b) {
    if (flags & ~1) return fail(LLPF_ERR_ARG, "imm: flags has bits other than 0");
    std::vector<double> par;
    CHK(imm_pack(models, D, P, mu0, F, M, b.nx, b.ny, b.nu, par, b.h_init));
    CHK(kf_open(b, device, F, LLPF_KF_NPAR(b.nx, b.ny, b.nu), "imm_create"));
    b.M = M; b.G = imm_group(M); b.L = F * b.G;
    b.interact = flags & 1;
    b.nstate = b.nx + b.np + 2;
    CHK(b.d_par.ensure(par.size()));
    CHK(b.d_state.ensure(b.h_init.size()));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int imm_set_models(llpf_imm_bank& b, const llpf_model* models, const double* D, const double* P, const double* mu0) {
    std::vector<double> par, init;
    int nx = 0, ny = 0, nu = 0;
    CHK(imm_pack(models, D, P, mu0, b.F, b.M, nx, ny, nu, par, init));
    if (nx != b.nx || ny != b.ny || nu != b.nu) return fail(LLPF_ERR_ARG, "imm: set_models must keep the dimensions of the bank");
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.h_init.swap(init);
    return LLPF_OK;
}

static int imm_run(llpf_imm_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                   const llpf_imm_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, nullptr));
    if (out && out->struct_size < sizeof(llpf_imm_outputs)) return kf_fail(b.who, "llpf_imm_outputs.struct_size too small (ABI)");
    test_throw("imm_run");
    const int F = b.F, nx = b.nx, ny = b.ny, nu = b.nu, M = b.M;
    const bool upf = nu > 0 && (per_filter & 1), ypf = (per_filter & 2) != 0;
    // the outputs of one step, in staging order: ll, x, xt, R, Rt, mu, ll_modes
    double* dst[7] = {out ? out->ll_steps : nullptr, out ? out->x : nullptr, out ? out->xt : nullptr, out ? out->R : nullptr,
                      out ? out->Rt : nullptr, out ? out->mu : nullptr, out ? out->ll_modes : nullptr};
    const uint64_t width[7] = {1, (uint64_t)nx, (uint64_t)nx, (uint64_t)nx * nx, (uint64_t)nx * nx, (uint64_t)M, (uint64_t)M};
    uint64_t w = 0;
    std::vector<ChunkOut> outs;
    for (int k = 0; k < 7; ++k) {
        if (dst[k]) w += width[k];
        outs.push_back({dst[k], 1, (size_t)F * width[k]});
    }
    const uint64_t in_w = (upf ? (uint64_t)nu : 0) + (ypf ? (uint64_t)ny : 0);
    uint64_t total = 0, in_total = 0;
    if (!doubles_fit({(uint64_t)F, w, (uint64_t)T}, total) || !doubles_fit({(uint64_t)F, in_w, (uint64_t)T}, in_total))
        return kf_fail(b.who, "the size of the outputs or of the inputs overflows");
    std::vector<double> h_ll(ll_total ? (size_t)b.L : 0);
    HIPC(hipSetDevice(b.device));
    ChunkPipe pipe(b.stream);
    CHK(pipe.open(T, (size_t)F * (w + in_w) * sizeof(double), outs,
                  {{nu > 0 ? U : nullptr, upf ? (size_t)F : 0, (size_t)nu, true}, {Y, ypf ? (size_t)F : 0, (size_t)ny, true}}));
    for (int64_t c = 0; c < pipe.nchunk; ++c) {
        CHK(pipe.begin(c, c));
        ImmArgs a{};
        a.par = b.d_par; a.state = b.d_state;
        a.u = pipe.in(0);
        a.y = pipe.in(1);
        double** slot[7] = {&a.ll, &a.x, &a.xt, &a.R, &a.Rt, &a.mu, &a.ll_modes};
        for (int k = 0; k < 7; ++k) *slot[k] = pipe.out(k);
        a.F = F; a.Tc = (int32_t)pipe.tc; a.nu = nu; a.M = M;
        a.u_per = upf ? 1 : 0; a.y_per = ypf ? 1 : 0;
        a.first = c == 0 ? 1 : 0;
        a.interact = b.interact;
        a.par_tstride = 0;
        HIPC(launch_imm(nx, ny, b.G, a, b.stream));
        CHK(pipe.end());
    }
    CHK(pipe.finish());
    if (ll_total) {    // the running sum: row nx + np + 1 of the state, the same in every lane of a filter
        HIPC(hipMemcpyAsync(h_ll.data(), b.d_state.p + (size_t)(nx + b.np + 1) * b.L, sizeof(double) * b.L, hipMemcpyDeviceToHost, b.stream));
        HIPC(hipStreamSynchronize(b.stream));
        for (int f = 0; f < F; ++f) ll_total[f] = h_ll[(size_t)f * b.G];
    }
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// the combined x [F][nx], R [F][nx][nx], and mu [F][M], the modes' xm [F][M][nx], Rm [F][M][nx][nx] of the current state (each may be NULL)
static int imm_get_state(llpf_imm_bank& b, double* x, double* R, double* mu, double* xm, double* Rm) {
    std::vector<double> h((size_t)b.nstate * b.L);
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(h.data(), b.d_state, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    const size_t L = (size_t)b.L;
    const int nx = b.nx, np = b.np, M = b.M;
    for (int f = 0; f < b.F; ++f) {
        double xs[LLPF_IMM_MAXM][LLPF_KF_MAXX], Rs[LLPF_IMM_MAXM][LLPF_KF_NP(LLPF_KF_MAXX)], ms[LLPF_IMM_MAXM];
        for (int j = 0; j < M; ++j) {
            const size_t col = (size_t)f * b.G + j, fj = (size_t)f * M + j;
            for (int i = 0; i < nx; ++i) xs[j][i] = h[i * L + col];
            for (int i = 0; i < np; ++i) Rs[j][i] = h[(nx + i) * L + col];
            ms[j] = h[(size_t)(nx + np) * L + col];
            if (mu) mu[fj] = ms[j];
            if (xm) for (int i = 0; i < nx; ++i) xm[fj * nx + i] = xs[j][i];
            if (Rm) for (int r = 0; r < nx; ++r) for (int c = 0; c < nx; ++c) Rm[(fj * nx + r) * nx + c] = Rs[j][llpf_kf_idx(r, c)];
        }
        if (!x && !R) continue;
        double xc[LLPF_KF_MAXX] = {0.0}, Rc[LLPF_KF_NP(LLPF_KF_MAXX)] = {0.0};
        for (int j = 0; j < M; ++j) llpf_imm_mean_add(nx, ms[j], xs[j], xc);
        for (int j = 0; j < M; ++j) llpf_imm_cov_add(nx, ms[j], xs[j], Rs[j], xc, Rc);
        if (x) for (int i = 0; i < nx; ++i) x[(size_t)f * nx + i] = xc[i];
        if (R) for (int r = 0; r < nx; ++r) for (int c = 0; c < nx; ++c) R[((size_t)f * nx + r) * nx + c] = Rc[llpf_kf_idx(r, c)];
    }
    return LLPF_OK;
}

// mu [F][M], xm [F][M][nx], Rm [F][M][nx][nx] (the lower triangles are taken); the running ll_total is zeroed
static int imm_set_state(llpf_imm_bank& b, const double* mu, const double* xm, const double* Rm) {
    if (!mu || !xm || !Rm) return kf_fail(b.who, "mu, x and R of the modes must all be given");
    std::vector<double> h((size_t)b.nstate * b.L, 0.0);
    const size_t L = (size_t)b.L;
    const int nx = b.nx, np = b.np, M = b.M;
    for (int f = 0; f < b.F; ++f)
        for (int j = 0; j < M; ++j) {
            const size_t col = (size_t)f * b.G + j, fj = (size_t)f * M + j;
            for (int i = 0; i < nx; ++i) h[i * L + col] = xm[fj * nx + i];
            for (int r = 0; r < nx; ++r) for (int c = 0; c <= r; ++c) h[(nx + llpf_kf_idx(r, c)) * L + col] = Rm[(fj * nx + r) * nx + c];
            h[(size_t)(nx + np) * L + col] = mu[fj];
        }
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_state, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}
