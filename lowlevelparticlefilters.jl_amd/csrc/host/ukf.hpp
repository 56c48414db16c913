// host/ukf.hpp — banks of unscented Kalman filters (llpf_ukf_bank_*; kernel: kernels/ukf.hpp, step: shared/llpf_ukf.h).  Part of
// capi.hip (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank, its models, its state and the drivers of a run and a smooth are host/kfbank.hpp's (KfModelBank).  Here are the weights and
// the launchers of k_ukf and k_ukf_smooth.

struct llpf_ukf_bank : KfModelBank {
    llpf_ukf_weights w{};
    llpf_ukf_bank() : KfModelBank("ukf", "unscented filter", 0) {}
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

static int ukf_create(int32_t device, const llpf_model* models, int32_t F, const llpf_ukf_weights* w, llpf_ukf_bank& b) {
    CHK(ukf_check_weights(w));
    b.w = *w;
    return kf_model_create(b, device, models, F, "ukf_create", ukf_prepare);
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
    return kf_forward(b, U, Y, T, per_filter, kf_outputs(b, ll_total, out), post, [&](const KfChunk& c) -> int {
        UkfArgs a{kf_model_args(b, c, t_index0)};
        a.gamma = b.w.gamma; a.wm0 = b.w.wm0; a.wc0 = b.w.wc0; a.wi = b.w.wi;
        a.post = c.post;
        HIPC(launch_ukf(b.model_id, b.nx, b.ny, b.d_models, a, b.stream));
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
    return kf_smooth(
        b, U, T, per_filter, out, "ukf_smooth",
        [&]() -> int {
            std::string err;
            if (ukf_smooth_prepare(b.model_id, b.nx, b.ny, err) != 0) return fail(LLPF_ERR_HIP, "ukf: " + err);
            return LLPF_OK;
        },
        [&](double* post) { return ukf_forward(b, U, Y, T, per_filter, t_index0, ll_total, fwd, post); },
        [&](const KfSmoothChunk& c) -> int {
            UkfSmoothArgs a{};
            kf_fill_smooth_args(a, b, c);
            a.zero_u = b.d_zero;
            a.t0 = c.t0;
            a.t_index0 = t_index0; a.Ts = b.Ts;
            a.gamma = b.w.gamma; a.wm0 = b.w.wm0; a.wc0 = b.w.wc0; a.wi = b.w.wi;
            HIPC(launch_ukf_smooth(b.model_id, b.nx, b.ny, b.d_models, a, b.stream));
            return LLPF_OK;
        });
}
