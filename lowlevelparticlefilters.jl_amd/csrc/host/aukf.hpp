// host/aukf.hpp — banks of unscented Kalman filters with augmented (non-additive) process noise (llpf_aukf_bank_*; kernel:
// kernels/aukf.hpp, step: shared/llpf_aukf.h).  Part of capi.hip (one translation unit), after host/ukf.hpp.
// ------------------------------------------------------------------------------------------------
// The bank, its models, its state and the driver of a run are host/kfbank.hpp's (KfModelBank, the unscented bank's pack and refusals: no
// Jacobians needed, no loglik, noise or initial member admitted; a model's dynamics_w is used where it has one).  Here are the two weight
// sets and the launcher of k_aukf.  There is no smoother.

struct llpf_aukf_bank : KfModelBank {
    llpf_ukf_weights wm{}, wd{};      // the measurement set (L = nx) and the dynamics set (L = 2 nx)
    llpf_aukf_bank() : KfModelBank("aukf", "unscented filter", 0) {}
};

// both sets by ukf_check_weights
static int aukf_set_weights(llpf_aukf_bank& b, const llpf_ukf_weights* w_measurement, const llpf_ukf_weights* w_dynamics) {
    CHK(ukf_check_weights(w_measurement));
    CHK(ukf_check_weights(w_dynamics));
    b.wm = *w_measurement;            // the weights ride in launch arguments
    b.wd = *w_dynamics;
    return LLPF_OK;
}

static int aukf_create(int32_t device, const llpf_model* models, int32_t F, const llpf_ukf_weights* w_measurement,
                       const llpf_ukf_weights* w_dynamics, llpf_aukf_bank& b) {
    CHK(aukf_set_weights(b, w_measurement, w_dynamics));
    return kf_model_create(b, device, models, F, "aukf_create", aukf_prepare);
}

// T steps of every filter from the current state: kf_forward with k_aukf
static int aukf_run(llpf_aukf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                    const llpf_kalman_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out));
    if (!std::isfinite(t_index0)) return fail(LLPF_ERR_ARG, "aukf: t_index0 must be finite");
    test_throw("aukf_run");
    return kf_forward(b, U, Y, T, per_filter, kf_outputs(b, ll_total, out), nullptr, [&](const KfChunk& c) -> int {
        AukfArgs a{kf_model_args(b, c, t_index0)};
        a.gamma = b.wm.gamma; a.wm0 = b.wm.wm0; a.wc0 = b.wm.wc0; a.wi = b.wm.wi;
        a.gamma_a = b.wd.gamma; a.wm0a = b.wd.wm0; a.wc0a = b.wd.wc0; a.wia = b.wd.wi;
        HIPC(launch_aukf(b.model_id, b.nx, b.ny, b.d_models, a, b.stream));
        return LLPF_OK;
    });
}
