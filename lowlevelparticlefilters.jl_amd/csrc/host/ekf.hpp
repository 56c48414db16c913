// host/ekf.hpp — banks of extended Kalman filters (llpf_ekf_bank_*; kernel: kernels/ekf.hpp, step: shared/llpf_ekf.h).  Part of capi.hip
// (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank, its state and the driver of a run are host/kfbank.hpp's.  Here are the model descriptors ModelD[F] as a bank of particle
// filters keeps them (the model's own parameters), the covariances par [np(nx) + np(ny)][F] (R1, R2 packed, from the llpf_model
// covariances as given — the unscented bank's block, without its weights) and the launcher of k_ekf.

struct llpf_ekf_bank : KfBank {
    int model_id = 0;
    double Ts = 1.0;
    int32_t maxiters = 1;      // llpf_ekf_bank_set_iterations: 1 is the plain filter (k_ekf), above it the iterated one (k_ekf<..., IekfArgs>)
    double epsilon = 0.0;
    DevBuf<ModelD> d_models;
    DevBuf<double> d_zero;
    llpf_ekf_bank() : KfBank("ekf") {}
};

// models -> the descriptors, the SoA covariances and the initial state; every check that needs no device: the unscented bank's, and
// a compiled model must define both Jacobian members (kf_pack_models)
static int ekf_pack(const llpf_model* models, int32_t F, int& model_id, int& nx, int& ny, int& nu, std::vector<ModelD>& hm,
                    std::vector<double>& par, std::vector<double>& init) {
    return kf_pack_models("ekf", "extended Kalman filter", LLPF_TRAIT_DYNAMICS_JAC | LLPF_TRAIT_MEASUREMENT_JAC, models, F, model_id, nx, ny, nu,
                          hm, par, init);
}

static int ekf_create(int32_t device, const llpf_model* models, int32_t F, llpf_ekf_bank& b) {
    std::vector<ModelD> hm;
    std::vector<double> par;
    CHK(ekf_pack(models, F, b.model_id, b.nx, b.ny, b.nu, hm, par, b.h_init));
    CHK(kf_open(b, device, F, LLPF_EKF_NPAR(b.nx, b.ny), "ekf_create"));
    b.Ts = models[0].Ts;
    {
        std::string err;      // a run-time compiled model's k_ekf, on the first bank of that model
        if (ekf_prepare(b.model_id, b.nx, b.ny, err) != 0) return fail(LLPF_ERR_HIP, "ekf: " + err);
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

static int ekf_set_models(llpf_ekf_bank& b, const llpf_model* models) {
    std::vector<ModelD> hm;
    std::vector<double> par, init;
    int id = 0, nx = 0, ny = 0, nu = 0;
    CHK(ekf_pack(models, b.F, id, nx, ny, nu, hm, par, init));
    if (id != b.model_id || nx != b.nx || ny != b.ny || nu != b.nu) return fail(LLPF_ERR_ARG, "ekf: set_models must keep the model id and the dimensions of the bank");
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_models, hm.data(), sizeof(ModelD) * hm.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipMemcpyAsync(b.d_par, par.data(), sizeof(double) * par.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.h_init.swap(init);
    b.Ts = models[0].Ts;
    return LLPF_OK;
}

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
    const int nx = b.nx, ny = b.ny;
    return kf_forward(b, U, Y, T, per_filter, ll_total, out, nullptr, [&](const KfChunk& c) -> int {
        EkfArgs a{};
        a.par = b.d_par; a.state = b.d_state; a.zero_u = b.d_zero;
        a.u = c.u;
        a.y = c.y;
        double** slot[6] = {&a.ll, &a.x, &a.xt, &a.R, &a.Rt, &a.e};
        for (int k = 0; k < 6; ++k) *slot[k] = c.out[k];
        a.F = b.F; a.t0 = c.t0; a.Tc = c.tc; a.nu = b.nu;
        a.u_per = c.upf; a.y_per = c.ypf;
        a.first = c.first;
        a.t_index0 = t_index0; a.Ts = b.Ts;
        if (b.maxiters > 1)
            HIPC(launch_iekf(b.model_id, nx, ny, b.d_models, a, b.maxiters, b.epsilon, b.stream));
        else
            HIPC(launch_ekf(b.model_id, nx, ny, b.d_models, a, b.stream));
        return LLPF_OK;
    });
}
