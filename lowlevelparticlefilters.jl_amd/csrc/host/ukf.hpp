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

// models -> the descriptors, the SoA covariances and the initial state; every check that needs no device (kf_pack_models)
static int ukf_pack(const llpf_model* models, int32_t F, int& model_id, int& nx, int& ny, int& nu, std::vector<ModelD>& hm,
                    std::vector<double>& par, std::vector<double>& init) {
    return kf_pack_models("ukf", "unscented filter", 0, models, F, model_id, nx, ny, nu, hm, par, init);
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
