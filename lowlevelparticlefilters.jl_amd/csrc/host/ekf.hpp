// host/ekf.hpp — banks of extended Kalman filters (llpf_ekf_bank_*; kernel: kernels/ekf.hpp, step: shared/llpf_ekf.h).  Part of capi.hip
// (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank, its models, its state and the driver of a run are host/kfbank.hpp's (KfModelBank: the unscented bank's block, without its
// weights; a compiled model must define both Jacobian members; created and given new models by kf_model_create / kf_model_set_models).
// Here are the iteration settings and the launcher of k_ekf.

struct llpf_ekf_bank : KfModelBank {
    int32_t maxiters = 1;      // llpf_ekf_bank_set_iterations: 1 is the plain filter (k_ekf), above it the iterated one (k_ekf<..., IekfArgs>)
    double epsilon = 0.0;
    llpf_ekf_bank() : KfModelBank("ekf", "extended Kalman filter", LLPF_TRAIT_DYNAMICS_JAC | LLPF_TRAIT_MEASUREMENT_JAC) {}
};

// The iteration of correct! (shared/llpf_ekf.h): it rides in the launch arguments of every later run; set_models, set_state and reset
// keep it.  The check of the two numbers needs no bank (the C ABI makes it before it looks at the handle).
static int ekf_check_iterations(int32_t maxiters, double epsilon) {
    if (maxiters < 1 || maxiters > LLPF_IEKF_MAXITERS)
        return fail(LLPF_ERR_ARG, "ekf: maxiters must be in 1.." + std::to_string(LLPF_IEKF_MAXITERS) + " (LLPF_IEKF_MAXITERS)");
    if (!std::isfinite(epsilon) || epsilon < 0.0) return fail(LLPF_ERR_ARG, "ekf: epsilon must be finite and >= 0");
    return LLPF_OK;
}

// The first iterated use of a run-time compiled model compiles its iterated kernel; a refused or failed call leaves the setting as it was.
static int ekf_set_iterations(llpf_ekf_bank& b, int32_t maxiters, double epsilon) {
    CHK(ekf_check_iterations(maxiters, epsilon));
    if (maxiters > 1) {
        HIPC(hipSetDevice(b.device));
        std::string err;
        if (iekf_prepare(b.model_id, b.nx, b.ny, err) != 0) return fail(LLPF_ERR_HIP, "ekf: " + err);
    }
    b.maxiters = maxiters;
    b.epsilon = epsilon;
    return LLPF_OK;
}

// T steps of every filter from the current state: kf_forward with k_ekf, in its iterated form when the bank iterates
static int ekf_run(llpf_ekf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                   const llpf_kalman_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out));
    if (!std::isfinite(t_index0)) return fail(LLPF_ERR_ARG, "ekf: t_index0 must be finite");
    test_throw("ekf_run");
    return kf_forward(b, U, Y, T, per_filter, kf_outputs(b, ll_total, out), nullptr, [&](const KfChunk& c) -> int {
        const EkfArgs a{kf_model_args(b, c, t_index0)};
        if (b.maxiters > 1)
            HIPC(launch_iekf(b.model_id, b.nx, b.ny, b.d_models, a, b.maxiters, b.epsilon, b.stream));
        else
            HIPC(launch_ekf(b.model_id, b.nx, b.ny, b.d_models, a, b.stream));
        return LLPF_OK;
    });
}
