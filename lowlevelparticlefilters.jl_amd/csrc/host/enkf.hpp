// host/enkf.hpp — banks of ensemble Kalman filters (llpf_enkf_bank_*; kernel: kernels/enkf.hpp, step: shared/llpf_enkf.h).  Part of capi.hip
// (one translation unit).
// ------------------------------------------------------------------------------------------------
// The bank, its models, its state [nx + np + 1][F] and the driver of a run are host/kfbank.hpp's (KfModelBank: the extended bank's block,
// with `noise` and `initial` members of a compiled model admitted).  Here are the ensembles — one more device buffer [F][nx][N] —, the
// counters of the generator and the launcher of k_enkf.  The counters are the particle bank's (host/bank.hpp): n_reset grows with every
// reset, the step counter with every predict, and only seed zeroes them; filter f's key is seed + f, so a filter's bits do not depend
// on the bank it sits in.  The kernel leaves mean, packed sample covariance and the running ll in d_state at the end of a chunk, where
// kf_get_state and kf_forward read them; reset and set_members put the moments there with k_enkf_moments.

struct llpf_enkf_bank : KfModelBank {
    int32_t N = 0;
    uint64_t seed = 0;
    uint32_t n_reset = 0, step = 0;
    double rho = 1.0;
    DevBuf<double> d_members;     // [F][nx][N]
    llpf_enkf_bank() : KfModelBank("enkf", "ensemble Kalman filter", 0) { allow_traits = LLPF_TRAIT_NOISE | LLPF_TRAIT_INITIAL; }
};

static int enkf_check_inflation(double rho) {
    if (!std::isfinite(rho) || rho < 1.0) return fail(LLPF_ERR_ARG, "enkf: the inflation must be finite and >= 1");
    return LLPF_OK;
}

// reset!: the next draw of every ensemble, its moments into the state, the running ll to 0
static int enkf_reset(llpf_enkf_bank& b) {
    HIPC(hipSetDevice(b.device));
    EnkfInitArgs a{};
    a.members = b.d_members; a.zero_u = b.d_zero; a.key0 = b.seed; a.N = b.N; a.n_reset = b.n_reset;
    HIPC(launch_enkf_init(b.model_id, b.nx, b.ny, b.d_models, b.F, a, b.stream));
    HIPC(launch_enkf_moments(b.nx, b.d_members, b.d_state, b.F, b.N, 1, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    b.n_reset++;
    return LLPF_OK;
}

// the counters restart and the first ensemble of the new seed is drawn: the bank is what create(seed) gives
static int enkf_seed(llpf_enkf_bank& b, uint64_t seed) {
    b.seed = seed;
    b.n_reset = 0;
    b.step = 0;
    return enkf_reset(b);
}

static int enkf_create(llpf_enkf_bank& b, int32_t device, const llpf_model* models, int32_t F, int32_t N, uint64_t seed) {
    if (N < 2) return fail(LLPF_ERR_ARG, "enkf: n_members must be >= 2");
    if (N > LLPF_ENKF_MAX_MEMBERS)
        return fail(LLPF_ERR_ARG, "enkf: n_members must be <= " + std::to_string(LLPF_ENKF_MAX_MEMBERS) + " (LLPF_ENKF_MAX_MEMBERS)");
    CHK(kf_model_create(b, device, models, F, "enkf_create", enkf_prepare));
    uint64_t nm = 0;
    if (!doubles_fit({(uint64_t)F, (uint64_t)b.nx, (uint64_t)N}, nm)) return fail(LLPF_ERR_ARG, "enkf: the size of the ensembles overflows");
    b.N = N;
    CHK(b.d_members.ensure((size_t)nm));
    return enkf_seed(b, seed);
}

// X [F][N][nx] <-> the device's [F][nx][N]
static int enkf_get_members(llpf_enkf_bank& b, double* X) {
    if (!X) return fail(LLPF_ERR_ARG, "enkf: X is null");
    const size_t F = (size_t)b.F, N = (size_t)b.N, nx = (size_t)b.nx;
    std::vector<double> h(F * nx * N);
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(h.data(), b.d_members, sizeof(double) * h.size(), hipMemcpyDeviceToHost, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    for (size_t f = 0; f < F; ++f)
        for (size_t d = 0; d < nx; ++d)
            for (size_t i = 0; i < N; ++i) X[(f * N + i) * nx + d] = h[(f * nx + d) * N + i];
    return LLPF_OK;
}
static int enkf_set_members(llpf_enkf_bank& b, const double* X) {
    if (!X) return fail(LLPF_ERR_ARG, "enkf: X is null");
    const size_t F = (size_t)b.F, N = (size_t)b.N, nx = (size_t)b.nx;
    std::vector<double> h(F * nx * N);
    for (size_t f = 0; f < F; ++f)
        for (size_t d = 0; d < nx; ++d)
            for (size_t i = 0; i < N; ++i) h[(f * nx + d) * N + i] = X[(f * N + i) * nx + d];
    HIPC(hipSetDevice(b.device));
    HIPC(hipMemcpyAsync(b.d_members, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, b.stream));
    HIPC(launch_enkf_moments(b.nx, b.d_members, b.d_state, b.F, b.N, 0, b.stream));
    HIPC(hipStreamSynchronize(b.stream));
    return LLPF_OK;
}

// T steps (phases: LLPF_ENKF_CORRECT | LLPF_ENKF_PREDICT) of every filter from the current ensembles: kf_forward with k_enkf.  Everything
// is allocated before the first launch: a refused allocation leaves members and state as they were.
static int enkf_forward(llpf_enkf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                        const llpf_kalman_outputs* out, int32_t phases) {
    CHK(kf_check_run(b, U, Y, T, per_filter, out));
    if (!std::isfinite(t_index0)) return fail(LLPF_ERR_ARG, "enkf: t_index0 must be finite");
    test_throw("enkf_run");
    const uint32_t step0 = b.step;
    CHK(kf_forward(b, U, Y, T, per_filter, kf_outputs(b, ll_total, out), nullptr, [&](const KfChunk& c) -> int {
        EnkfArgs a{};
        static_cast<KfModelArgs&>(a) = kf_model_args(b, c, t_index0);
        a.members = b.d_members; a.key0 = b.seed; a.rho = b.rho; a.N = b.N; a.step0 = step0; a.phases = phases;
        HIPC(launch_enkf(b.model_id, b.nx, b.ny, b.d_models, a, b.stream));
        return LLPF_OK;
    }));
    if (phases & LLPF_ENKF_PREDICT) b.step += (uint32_t)T;
    return LLPF_OK;
}

static int enkf_run(llpf_enkf_bank& b, const double* U, const double* Y, int64_t T, int32_t per_filter, double t_index0, double* ll_total,
                    const llpf_kalman_outputs* out) {
    return enkf_forward(b, U, Y, T, per_filter, t_index0, ll_total, out, LLPF_ENKF_CORRECT | LLPF_ENKF_PREDICT);
}

// correct!(u, y) of every filter at time t_index * Ts: ll [F] and, optionally, e [F][ny]; u [nu] or [F][nu], y [ny] or [F][ny] (per_filter)
static int enkf_correct(llpf_enkf_bank& b, const double* u, const double* y, int32_t per_filter, double t_index, double* ll, double* e) {
    llpf_kalman_outputs o{};
    o.struct_size = sizeof(o);
    o.e = e;
    return enkf_forward(b, u, y, 1, per_filter, t_index, ll, e ? &o : nullptr, LLPF_ENKF_CORRECT);
}

// predict!(u) of every filter at time t_index * Ts; the step counter grows by one
static int enkf_predict(llpf_enkf_bank& b, const double* u, int32_t per_filter, double t_index) {
    double y[LLPF_KF_MAXY];
    for (int r = 0; r < LLPF_KF_MAXY; ++r) y[r] = llpf_kf_nan();
    return enkf_forward(b, u, y, 1, per_filter & 1, t_index, nullptr, nullptr, LLPF_ENKF_PREDICT);
}
