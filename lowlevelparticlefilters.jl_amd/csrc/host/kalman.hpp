// host/kalman.hpp — banks of Kalman filters with constant matrices (llpf_kalman_bank_*; kernel: kernels/kalman.hpp, step:
// shared/llpf_kalman.h).  Part of capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank, its state and the drivers of a run and a smooth are host/kfbank.hpp's; here are the constants par [npar][F] (A, C, R1, R2,
// B, D: LLPF_KF_OFF_*) and the launchers of k_kalman and k_kalman_smooth.

struct llpf_kalman_bank : KfBank {
    llpf_kalman_bank() : KfBank("kalman") {}
};

// models (+ D [F][ny][nu] or NULL) -> the SoA constants and initial state; every check that needs no device
static int kalman_pack(const llpf_model* models, const double* D, int32_t F, int& nx, int& ny, int& nu, std::vector<double>& par,
                       std::vector<double>& init) {
    if (!models) return fail(LLPF_ERR_ARG, "kalman: models is null");
    if (F < 1) return fail(LLPF_ERR_ARG, "kalman: n_filters must be >= 1");
    nx = models[0].nx; ny = models[0].ny; nu = models[0].nu;
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU)
        return fail(LLPF_ERR_ARG, "kalman: nx must be in 1..8, ny in 1..4 and nu in 0..8");
    const int np = LLPF_KF_NP(nx), npar = LLPF_KF_NPAR(nx, ny, nu), nstate = nx + np + 1;
    par.assign((size_t)npar * F, 0.0);
    init.assign((size_t)nstate * F, 0.0);
    for (int f = 0; f < F; ++f) {
        const llpf_model& m = models[f];
        const std::string at = "kalman: filter " + std::to_string(f) + ": ";
        if (m.model_id != LLPF_MODEL_LINEAR_GAUSSIAN) return fail(LLPF_ERR_ARG, at + "model_id must be LLPF_MODEL_LINEAR_GAUSSIAN");
        if (m.nx != nx || m.ny != ny || m.nu != nu) return fail(LLPF_ERR_ARG, at + "dimensions differ from filter 0's");
        CHK(kf_pack_filter(m, at, f, F, nx, ny, LLPF_KF_OFF_R1(nx, ny), LLPF_KF_OFF_R2(nx, ny), par, init));
        GaussD gd;                                // positive definiteness of R2 and P0: the host Cholesky of gauss_prepare
        if (gauss_prepare(&m.measurement_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
        if (gauss_prepare(&m.initial_density, &gd) != 0) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
        auto put = [&](int e, double v) { par[(size_t)e * F + f] = v; };
        for (int i = 0; i < nx * nx; ++i) put(LLPF_KF_OFF_A + i, m.A[i]);
        for (int i = 0; i < ny * nx; ++i) put(LLPF_KF_OFF_C(nx) + i, m.C[i]);
        for (int i = 0; i < nx * nu; ++i) put(LLPF_KF_OFF_B(nx, ny) + i, m.B[i]);
        for (int i = 0; i < ny * nu; ++i) put(LLPF_KF_OFF_D(nx, ny, nu) + i, D ? D[(size_t)f * ny * nu + i] : 0.0);
    }
    return LLPF_OK;
}

static int kalman_create(int32_t device, const llpf_model* models, const double* D, int32_t F, llpf_kalman_bank& b) {
    std::vector<double> par;
    CHK(kalman_pack(models, D, F, b.nx, b.ny, b.nu, par, b.h_init));
    CHK(kf_open(b, device, F, LLPF_KF_NPAR(b.nx, b.ny, b.nu), "kalman_create"));
    CHK(b.d_par.ensure(par.size()));
    CHK(b.d_state.ensure(b.h_init.size()));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int kalman_set_models(llpf_kalman_bank& b, const llpf_model* models, const double* D) {
    std::vector<double> par, init;
    int nx = 0, ny = 0, nu = 0;
    CHK(kalman_pack(models, D, b.F, nx, ny, nu, par, init));
    if (nx != b.nx || ny != b.ny || nu != b.nu) return fail(LLPF_ERR_ARG, "kalman: set_models must keep the dimensions of the bank");
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.h_init.swap(init);
    return LLPF_OK;
}

// the forward pass of a run (arguments checked): kf_forward with k_kalman, or k_kalman<..., true> where post is given
static int kalman_forward(llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                          const llpf_kalman_outputs* out, double* post) {
    const int nx = b.nx, ny = b.ny;
    return kf_forward(b, U, Y, T, per_filter, kf_outputs(b, ll_total, out), post, [&](const KfChunk& c) -> int {
        KalmanArgs a{};
        kf_fill_args(a, b, c);
        a.par_tstride = 0;
        a.post = c.post;
        HIPC(launch_kalman(nx, ny, a, b.stream));
        return LLPF_OK;
    });
}

static int kalman_run(llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                      const llpf_kalman_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out));
    test_throw("kalman_run");
    return kalman_forward(b, U, Y, T, per_filter, ll_total, out, nullptr);
}

// smooth(kf, u, y): kf_smooth with kalman_forward and k_kalman_smooth
static int kalman_smooth(llpf_kalman_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double* ll_total,
                         const llpf_kalman_outputs* fwd, const llpf_kalman_smooth_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, fwd));
    const int nx = b.nx;
    return kf_smooth(
        b, U, T, per_filter, out, "kalman_smooth", []() -> int { return LLPF_OK; },
        [&](double* post) { return kalman_forward(b, U, Y, T, per_filter, ll_total, fwd, post); },
        [&](const KfSmoothChunk& c) -> int {
            KalmanSmoothArgs a{};
            kf_fill_smooth_args(a, b, c);
            a.ny = b.ny;
            a.par_tstride = 0;
            HIPC(launch_kalman_smooth(nx, a, b.stream));
            return LLPF_OK;
        });
}
