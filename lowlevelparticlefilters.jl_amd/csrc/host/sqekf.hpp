// host/sqekf.hpp — banks of square-root extended Kalman filters (llpf_sqekf_bank_*; kernel: kernels/sqekf.hpp, step:
// shared/llpf_sqekf.h).  Part of capi.hip (one translation unit), after host/sqkf.hpp and host/ekf.hpp.
// ------------------------------------------------------------------------------------------------
// The bank, its models, its state rows and the driver of a run are host/kfbank.hpp's (KfModelBank, as the extended bank's: a compiled
// model must define both Jacobian members); the pack is kf_pack_models with the three covariances factored (sqkf_factor: llpf_kf_chol,
// once, here): par holds the packed factors L1, L2 where the extended bank holds R1, R2, and the state rows nx .. nx + np - 1 hold the
// packed factor Lr of R.  There is no smoother and no iterated form, and the filter is not a mode of an IMM bank.

struct llpf_sqekf_bank : KfModelBank {
    llpf_sqekf_bank() : KfModelBank("sqekf", "square-root extended Kalman filter", LLPF_TRAIT_DYNAMICS_JAC | LLPF_TRAIT_MEASUREMENT_JAC) {}
};

// kf_pack_models (every refusal of it unchanged), then R1, R2 and cov(d0) of every filter factored
static int sqekf_pack(const KfModelBank& b, const llpf_model* models, int32_t F, int& model_id, int& nx, int& ny, int& nu,
                      std::vector<ModelD>& hm, std::vector<double>& par, std::vector<double>& init) {
    CHK(kf_pack_models(b.who, b.filter_name, b.need_traits, b.allow_traits, models, F, model_id, nx, ny, nu, hm, par, init));
    for (int f = 0; f < F; ++f) {
        const std::string at = "sqekf: filter " + std::to_string(f) + ": ";
        if (!sqkf_factor(par, LLPF_EKF_OFF_R1, nx, f, F)) return fail(LLPF_ERR_ARG, at + "R1 (dynamics_density) is not positive definite");
        if (!sqkf_factor(par, LLPF_EKF_OFF_R2(nx), ny, f, F)) return fail(LLPF_ERR_ARG, at + "R2 (measurement_density) is not positive definite");
        if (!sqkf_factor(init, nx, nx, f, F)) return fail(LLPF_ERR_ARG, at + "cov(d0) (initial_density) is not positive definite");
    }
    return LLPF_OK;
}

// kf_model_create's steps around the factoring pack
static int sqekf_create(llpf_sqekf_bank& b, int32_t device, const llpf_model* models, int32_t F) {
    std::vector<ModelD> hm;
    std::vector<double> par;
    CHK(sqekf_pack(b, models, F, b.model_id, b.nx, b.ny, b.nu, hm, par, b.h_init));
    CHK(kf_open(b, device, F, LLPF_EKF_NPAR(b.nx, b.ny), "sqekf_create"));
    b.Ts = models[0].Ts;
    {
        std::string err;
        if (sqekf_prepare(b.model_id, b.nx, b.ny, err) != 0) return fail(LLPF_ERR_HIP, std::string(b.who) + ": " + err);
    }
    return kf_upload(b, b.d_models, b.d_zero, hm, par, true);
}

// ... and kf_model_set_models's
static int sqekf_set_models(llpf_sqekf_bank& b, const llpf_model* models) {
    std::vector<ModelD> hm;
    std::vector<double> par, init;
    int id = 0, nx = 0, ny = 0, nu = 0;
    CHK(sqekf_pack(b, models, b.F, id, nx, ny, nu, hm, par, init));
    if (id != b.model_id || nx != b.nx || ny != b.ny || nu != b.nu) return kf_fail(b.who, "set_models must keep the model id and the dimensions of the bank");
    CHK(kf_upload(b, b.d_models, b.d_zero, hm, par, false));
    b.h_init.swap(init);
    b.Ts = models[0].Ts;
    return LLPF_OK;
}

// T steps of every filter from the current state: kf_forward with k_sqekf
static int sqekf_run(llpf_sqekf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                     const llpf_kalman_outputs* out) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out));
    if (!std::isfinite(t_index0)) return fail(LLPF_ERR_ARG, "sqekf: t_index0 must be finite");
    test_throw("sqekf_run");
    return kf_forward(b, U, Y, T, per_filter, kf_outputs(b, ll_total, out), nullptr, [&](const KfChunk& c) -> int {
        HIPC(launch_sqekf(b.model_id, b.nx, b.ny, b.d_models, kf_model_args(b, c, t_index0), b.stream));
        return LLPF_OK;
    });
}
