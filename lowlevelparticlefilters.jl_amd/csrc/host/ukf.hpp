// host/ukf.hpp — banks of unscented Kalman filters (llpf_ukf_bank_*; kernel: kernels/ukf.hpp, step: shared/llpf_ukf.h).  Part of
// capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank, its state and the drivers of a run and a smooth are host/kfbank.hpp's.  Here are the model descriptors ModelD[F] as a bank of
// particle filters keeps them (the model's own parameters), the covariances par [np(nx) + np(ny)][F] (R1, R2 packed, from the llpf_model
// covariances as given — GaussD keeps a factor, not the covariance), the weights, and the launchers of k_ukf and k_ukf_smooth.

struct llpf_ukf_bank : KfBank {
    int model_id = 0;
    double Ts = 1.0;
    llpf_ukf_weights w{};
    DevBuf<ModelD> d_models;
    DevBuf<double> d_zero;
    llpf_ukf_bank() : KfBank("ukf") {}
};

// every check of the weights that needs no device
static int ukf_check_weights(const llpf_ukf_weights* w) {
    if (!w) return fail(LLPF_ERR_ARG, "ukf: weights is null");
    if (w->struct_size < sizeof(llpf_ukf_weights)) return fail(LLPF_ERR_ARG, "ukf: llpf_ukf_weights.struct_size too small (ABI)");
    if (!std::isfinite(w->gamma) || !std::isfinite(w->wm0) || !std::isfinite(w->wc0) || !std::isfinite(w->wi))
        return fail(LLPF_ERR_ARG, "ukf: the weights must be finite");
    if (!(w->gamma > 0.0) || !(w->wi > 0.0)) return fail(LLPF_ERR_ARG, "ukf: gamma and wi must be > 0");
    return LLPF_OK;
}

// models -> the descriptors, the SoA covariances and the initial state; every check that needs no device
static int ukf_pack(const llpf_model* models, int32_t F, int& model_id, int& nx, int& ny, int& nu, std::vector<ModelD>& hm,
                    std::vector<double>& par, std::vector<double>& init) {
    if (!models) return fail(LLPF_ERR_ARG, "ukf: models is null");
    if (F < 1) return fail(LLPF_ERR_ARG, "ukf: n_filters must be >= 1");
    model_id = models[0].model_id; nx = models[0].nx; ny = models[0].ny; nu = models[0].nu;
    if (model_id == LLPF_MODEL_RB_LINEAR || model_id == LLPF_MODEL_RB_BILINEAR)
        return fail(LLPF_ERR_ARG, "ukf: the Rao-Blackwellized models (LLPF_MODEL_RB_LINEAR, LLPF_MODEL_RB_BILINEAR) have no unscented filter");
    if (nx < 1 || nx > LLPF_KF_MAXX || ny < 1 || ny > LLPF_KF_MAXY || nu < 0 || nu > LLPF_KF_MAXU)
        return fail(LLPF_ERR_ARG, "ukf: nx must be in 1..8, ny in 1..4 and nu in 0..8");
    if (model_id == LLPF_MODEL_QUADTANK_RK4) {
        if (nx != 4 || ny != 2 || nu != 2) return fail(LLPF_ERR_ARG, "ukf: the quad-tank has 4 states, 2 outputs and 2 inputs");
    } else if (model_id >= LLPF_MODEL_USER_BASE) {
        std::string src;
        int sx = 0, sy = 0;
        if (!jit_model_source(model_id, src, sx, sy)) return fail(LLPF_ERR_ARG, "ukf: unknown model id " + std::to_string(model_id));
        if (sx != nx || sy != ny) return fail(LLPF_ERR_ARG, "ukf: nx, ny differ from the dimensions the model was compiled for");
        const int traits = jit_model_traits(model_id);
        if (traits & LLPF_TRAIT_LOGLIK) return fail(LLPF_ERR_ARG, "ukf: the model has a likelihood of its own (loglik): there is no Gaussian R2");
        if (traits & LLPF_TRAIT_NOISE) return fail(LLPF_ERR_ARG, "ukf: the model forms its own noise (noise): only additive noise is supported");
        if (traits & LLPF_TRAIT_INITIAL) return fail(LLPF_ERR_ARG, "ukf: the model has an initial density of its own (initial): d0 must be Gaussian");
    } else if (model_id != LLPF_MODEL_LINEAR_GAUSSIAN) {
        return fail(LLPF_ERR_ARG, "ukf: unknown model id " + std::to_string(model_id));
    }
    const int np = LLPF_KF_NP(nx), npar = LLPF_UKF_NPAR(nx, ny), nstate = nx + np + 1;
    hm.resize((size_t)F);
    par.assign((size_t)npar * F, 0.0);
    init.assign((size_t)nstate * F, 0.0);
    for (int f = 0; f < F; ++f) {
        const llpf_model& m = models[f];
        const std::string at = "ukf: filter " + std::to_string(f) + ": ";
        if (m.model_id != model_id || m.nx != nx || m.ny != ny || m.nu != nu) return fail(LLPF_ERR_ARG, at + "model id or dimensions differ from filter 0's");
        CHK(kf_pack_filter(m, at, f, F, nx, ny, LLPF_UKF_OFF_R1, LLPF_UKF_OFF_R2(nx), par, init));
        const int rc = model_prepare(&m, &hm[(size_t)f]);      // the descriptor the model's own methods read; positive definiteness of R1, R2, cov(d0)
        if (rc == -1) return fail(LLPF_ERR_ARG, at + "R1 (dynamics_density) is not positive definite");
        if (rc == -2) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
        if (rc == -3) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
        if (rc) return fail(LLPF_ERR_ARG, at + "invalid model descriptor, code " + std::to_string(rc));
    }
    return LLPF_OK;
}

static int ukf_create(int32_t device, const llpf_model* models, int32_t F, const llpf_ukf_weights* w, llpf_ukf_bank& b) {
    std::vector<ModelD> hm;
    std::vector<double> par;
    CHK(ukf_check_weights(w));
    CHK(ukf_pack(models, F, b.model_id, b.nx, b.ny, b.nu, hm, par, b.h_init));
    CHK(kf_open(b, device, F, LLPF_UKF_NPAR(b.nx, b.ny), "ukf_create"));
    b.Ts = models[0].Ts;
    b.w = *w;
    {
        std::string err;      // a run-time compiled model's k_ukf, on the first bank of that model
        if (ukf_prepare(b.model_id, b.nx, b.ny, err) != 0) return fail(LLPF_ERR_HIP, "ukf: " + err);
    }
    CHK(b.d_models.ensure(hm.size()));
    CHK(b.d_par.ensure(par.size()));
    CHK(b.d_state.ensure(b.h_init.size()));
    CHK(b.d_zero.ensure(MAXU));
    HIPC(hipMemsetAsync(b.d_zero, 0, sizeof(double) * MAXU, b.stream));
    HIPC(hipMemcpyAsync(b.d_models, hm.data(), sizeof(ModelD) * hm.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_state, b.h_init.data(), sizeof(double) * b.h_init.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

static int ukf_set_models(llpf_ukf_bank& b, const llpf_model* models) {
    std::vector<ModelD> hm;
    std::vector<double> par, init;
    int id = 0, nx = 0, ny = 0, nu = 0;
    CHK(ukf_pack(models, b.F, id, nx, ny, nu, hm, par, init));
    if (id != b.model_id || nx != b.nx || ny != b.ny || nu != b.nu) return fail(LLPF_ERR_ARG, "ukf: set_models must keep the model id and the dimensions of the bank");
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_models, hm.data(), sizeof(ModelD) * hm.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.h_init.swap(init);
    b.Ts = models[0].Ts;
    return LLPF_OK;
}

static int ukf_set_weights(llpf_ukf_bank& b, const llpf_ukf_weights* w) {
    CHK(ukf_check_weights(w));
    b.w = *w;          // the weights ride in launch arguments
    return LLPF_OK;
}

// the checks of a run's arguments that need no device (llpf_ukf_bank_run and _smooth)
static int ukf_check_run(const llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0,
                         const llpf_kalman_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out));
    if (!std::isfinite(t_index0)) return fail(LLPF_ERR_ARG, "ukf: t_index0 must be finite");
    return LLPF_OK;
}

// the forward pass of a run (arguments checked): kf_forward with k_ukf, or k_ukf<..., true> where post is given
static int ukf_forward(llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                       const llpf_kalman_outputs* out, double* post) {
    const int nx = b.nx, ny = b.ny;
    return kf_forward(b, U, Y, T, per_filter, ll_total, out, post, [&](const KfChunk& c) -> int {
        UkfArgs a{};
        a.par = b.d_par; a.state = b.d_state; a.zero_u = b.d_zero;
        a.u = c.u;
        a.y = c.y;
        double** slot[6] = {&a.ll, &a.x, &a.xt, &a.R, &a.Rt, &a.e};
        for (int k = 0; k < 6; ++k) *slot[k] = c.out[k];
        a.F = b.F; a.t0 = c.t0; a.Tc = c.tc; a.nu = b.nu;
        a.u_per = c.upf; a.y_per = c.ypf;
        a.first = c.first;
        a.t_index0 = t_index0; a.Ts = b.Ts;
        a.gamma = b.w.gamma; a.wm0 = b.w.wm0; a.wc0 = b.w.wc0; a.wi = b.w.wi;
        a.post = c.post;
        HIPC(launch_ukf(b.model_id, nx, ny, b.d_models, a, b.stream));
        return LLPF_OK;
    });
}

// T steps of every filter from the current state
static int ukf_run(llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                   const llpf_kalman_outputs* out) {
    CHK(ukf_check_run(b, U, Y, T, per_filter, t_index0, out));
    test_throw("ukf_run");
    return ukf_forward(b, U, Y, T, per_filter, t_index0, ll_total, out, nullptr);
}

// smooth(ukf, u, y): kf_smooth with ukf_forward and k_ukf_smooth — kalman_smooth, with the model's dynamics in the place of A.  A run-time
// compiled model's k_ukf_smooth and k_ukf<..., true> are compiled on the first smooth of that model, before anything is allocated.
static int ukf_smooth(llpf_ukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                      const llpf_kalman_outputs* fwd, const llpf_kalman_smooth_outputs* out) {
    CHK(ukf_check_run(b, U, Y, T, per_filter, t_index0, fwd));
    const int nx = b.nx, ny = b.ny;
    return kf_smooth(
        b, U, T, per_filter, out, "ukf_smooth",
        [&]() -> int {
            std::string err;
            if (ukf_smooth_prepare(b.model_id, nx, ny, err) != 0) return fail(LLPF_ERR_HIP, "ukf: " + err);
            return LLPF_OK;
        },
        [&](double* post) { return ukf_forward(b, U, Y, T, per_filter, t_index0, ll_total, fwd, post); },
        [&](const KfSmoothChunk& c) -> int {
            UkfSmoothArgs a{};
            a.par = b.d_par;
            a.post = c.post;
            a.carry = c.carry;
            a.u = c.u;
            a.zero_u = b.d_zero;
            a.xT = c.xT;
            a.RT = c.RT;
            a.F = b.F; a.t0 = c.t0; a.Tc = c.tc; a.nu = b.nu;
            a.u_per = c.upf;
            a.init = c.init;
            a.t_index0 = t_index0; a.Ts = b.Ts;
            a.gamma = b.w.gamma; a.wm0 = b.w.wm0; a.wc0 = b.w.wc0; a.wi = b.w.wi;
            HIPC(launch_ukf_smooth(b.model_id, nx, ny, b.d_models, a, b.stream));
            return LLPF_OK;
        });
}
